"""Host side of the training switch for the recording column-split forward
(DLASSO_unfolded.train_split, train_unfolded.py --train-split): a plain opt-in attribute that
changes nothing about the module's state or its CPU path. No GPU."""
import argparse

import numpy as np
import torch

import oracle as O


def _args(K, mode="diff"):
    return argparse.Namespace(GHN_iter_num=K, DADMM_mode=mode, alpha_max=0.1, tau_max=0.99, rho_max=0.99,
                              eta_max=0.99, max_penalty_threshold=0.8, penalty_reduction_factor=0.95)


def _module(K=6, P=4, m=10, n=16, B=3):
    import unfolded_DLASSO as U
    A, b, x = O.make_problem(P, m, n, B, seed=5)
    mod = U.DLASSO_unfolded(torch.from_numpy(A)[None], _args(K))
    with torch.no_grad():
        mod.seq_hyp.param.copy_(0.3 * torch.randn(mod.seq_hyp.param.shape,
                                                  generator=torch.Generator().manual_seed(1)))
    return mod, b, x


def test_train_split_defaults_to_false():
    mod, _, _ = _module()
    assert mod.train_split is False


def test_train_split_is_not_module_state():
    mod, _, _ = _module()
    keys = list(mod.state_dict().keys())
    mod.train_split = True
    assert list(mod.state_dict().keys()) == keys == ["seq_hyp.param"]
    assert [k for k, _ in mod.named_buffers()] == []
    assert [k for k, _ in mod.named_parameters()] == ["seq_hyp.param"]


def test_cpu_training_step_ignores_train_split():
    """CPU tensors run dadmm_cpu whatever the switch says: forward and gradient bit-for-bit."""
    import gnn_dlasso_utils
    K, P, m, n, B = 6, 4, 10, 16, 3
    mod, b, x = _module(K, P, m, n, B)
    mod.train()
    graphs = [O.connected_er_graph(P, 0.5, seed=10 + s) for s in range(B)]
    g = torch.Generator().manual_seed(2)
    inits = tuple(1e-2 * torch.randn(B, P, n, 1, generator=g) for _ in range(3))
    out = []
    for flag in (False, True):
        mod.train_split = flag
        mod.zero_grad(set_to_none=True)
        Y, _ = mod(torch.from_numpy(b)[..., None], graphs, inits=inits)
        assert Y.device.type == "cpu"
        _, loss_final = gnn_dlasso_utils.compute_loss(Y, torch.from_numpy(x)[..., None])
        loss_final.backward()
        out.append((Y.detach().clone(), mod.seq_hyp.param.grad.detach().clone()))
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])
    assert np.isfinite(out[0][1].numpy()).all() and float(out[0][1].abs().max()) > 0.0


def test_driver_parser_accepts_train_split():
    import train_unfolded
    ap = train_unfolded.build_parser()
    assert ap.parse_args([]).train_split is False
    assert ap.parse_args(["--train-split"]).train_split is True
