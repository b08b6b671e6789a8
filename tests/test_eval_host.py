"""The evaluation forward's host side (no GPU): the served-shape query of the C ABI, the module's
``evaluate`` on CPU tensors (forward + compute_loss + layer_losses), its no-grad contract, the
driver's --fused-eval flag, and the two new symbols in the header and the binding."""
import argparse
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(K, mode="diff"):
    return argparse.Namespace(GHN_iter_num=K, DADMM_mode=mode, alpha_max=0.1, tau_max=0.99, rho_max=0.99,
                              eta_max=0.99, max_penalty_threshold=0.8, penalty_reduction_factor=0.95)


def _dims(P, m, n, shared=1, B=37, K=4):
    from dadmm_hip import _lib
    return _lib.Dims(B=B, P=P, m=m, n=n, K=K, variant=0, hyp_rows=1, graph_shared=shared)


def _bytes(d):
    from dadmm_hip import _lib
    return int(_lib.load().dadmm_forward_eval_scratch_bytes(ctypes.byref(d)))


def test_scratch_bytes_nonzero_exactly_on_served_shapes():
    """Non-zero (and at least the K x 4 ceil(B / 16) partial sums) for P 1..5 x n_pad 256, m <= 64,
    a shared graph; zero for P 6, n 128, m 65 and per-sample graphs."""
    for P in range(1, 6):
        for n in range(196, 257, 4):            # the stored row lengths of n = 193..256
            for m in (1, 50, 64):
                got = _bytes(_dims(P, m, n))
                assert got >= 4 * 4 * 4 * 3 and got % 256 == 0, (P, m, n, got)
    assert _bytes(_dims(5, 64, 256, B=4096, K=25)) >= 25 * 4 * 256 * 4
    assert _bytes(_dims(6, 64, 256)) == 0
    assert _bytes(_dims(5, 64, 128)) == 0
    assert _bytes(_dims(5, 65, 256)) == 0
    assert _bytes(_dims(5, 64, 256, shared=0)) == 0


def test_eval_served_follows_the_query():
    """eval_served pads n to the stored row length (n = 193..256 all serve) and refuses per-sample
    graphs; it needs no GPU."""
    from dadmm_hip.graph import ingest
    from dadmm_hip.ops import eval_served
    cpu = torch.device("cpu")
    for P in range(1, 6):
        for n in range(193, 257):
            assert eval_served(_dims(P, 64, n), 16, 3), (P, n)
    assert not eval_served(_dims(6, 64, 256), 16, 3)
    assert not eval_served(_dims(5, 64, 128), 16, 3)
    assert not eval_served(_dims(5, 65, 256), 16, 3)
    shared = ingest([O.er_graph(5, 0.5, seed=1)] * 16, 5, 16, cpu)
    per_sample = ingest([O.er_graph(5, 0.5, seed=s) for s in range(16)], 5, 16, cpu)
    assert eval_served(_dims(5, 64, 256), 16, 3, shared)
    assert not eval_served(_dims(5, 64, 256), 16, 3, per_sample)


def _cpu_module(P, m, n, B, K, mode="diff"):
    import unfolded_DLASSO as U
    A, b, _ = O.make_problem(P, m, n, B, seed=5)
    mod = U.DLASSO_unfolded(torch.from_numpy(A)[None], _args(K, mode))
    with torch.no_grad():
        mod.seq_hyp.param.copy_(0.3 * torch.randn(mod.seq_hyp.param.shape,
                                                  generator=torch.Generator().manual_seed(1)))
    g = torch.Generator().manual_seed(3)
    inits = tuple(1e-2 * torch.randn((B, P, n, 1), generator=g) for _ in range(3))
    label = torch.randn((B, n, 1), generator=g)
    return mod, torch.from_numpy(b)[..., None], inits, label


@pytest.mark.parametrize("mode", ["diff", "same"])
def test_evaluate_on_cpu_is_forward_plus_losses(mode):
    import gnn_dlasso_utils
    P, m, n, B, K = 4, 8, 16, 6, 5
    mod, b, inits, label = _cpu_module(P, m, n, B, K, mode)
    graphs = [O.er_graph(P, 0.6, seed=2)] * B
    mod.requires_grad_(False)
    ev = mod.evaluate(b, graphs, label, K=3, inits=inits)
    assert ev.status is mod.last_status and int(ev.status.item()) == 0
    with torch.no_grad():
        Y, hyp = mod(b, graphs, K=3, inits=inits)
        lm, lf = gnn_dlasso_utils.compute_loss(Y, label)
        losses = gnn_dlasso_utils.layer_losses(Y, label)
    assert type(ev).__name__ == "Evaluation"
    assert ev._fields == ("losses", "loss_mean", "loss_final", "y_final", "hyp", "status")
    assert ev.losses.shape == (3,) and ev.y_final.shape == (B, P, n, 1) and ev.hyp.shape == hyp.shape
    assert torch.equal(ev.losses, losses) and torch.equal(ev.loss_mean, lm) and torch.equal(ev.loss_final, lf)
    assert torch.equal(ev.y_final, Y[-1]) and torch.equal(ev.hyp, hyp)
    # under no_grad a trainable table is fine too
    mod.requires_grad_(True)
    with torch.no_grad():
        ev2 = mod.evaluate(b, graphs, label, K=3, inits=inits, on_guard="flag")
    assert torch.equal(ev2.losses, losses) and torch.equal(ev2.y_final, Y[-1])


def test_evaluate_refuses_to_run_under_autograd():
    P, m, n, B, K = 4, 8, 16, 4, 3
    mod, b, inits, label = _cpu_module(P, m, n, B, K)
    graphs = [O.er_graph(P, 0.6, seed=2)] * B
    assert mod.seq_hyp.param.requires_grad and torch.is_grad_enabled()
    with pytest.raises(RuntimeError, match="forward"):
        mod.evaluate(b, graphs, label, inits=inits)
    with pytest.raises(ValueError, match="on_guard"):
        with torch.no_grad():
            mod.evaluate(b, graphs, label, inits=inits, on_guard="ignore")


def test_driver_fused_eval_prints_the_same_validation_loss(tmp_path, monkeypatch, capsys):
    """train_unfolded.py --device cpu: one epoch with and without --fused-eval, same seeds, prints
    the same epoch line up to its wall-clock field and returns the same losses."""
    monkeypatch.chdir(tmp_path)
    mod = importlib.import_module("train_unfolded")
    args = ["--device", "cpu", "--P", "4", "--m", "8", "--n", "16", "--GHN_iter_num", "3",
            "--batch_size", "8", "--train_size", "16", "--test_size", "8", "--num_epochs", "1", "--seed", "2"]
    runs = []
    for extra in ([], ["--fused-eval"]):
        tr, va = mod.main(args + ["--out", str(tmp_path / ("b" if extra else "a"))] + extra)
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("epoch 1/1")]
        assert len(line) == 1
        runs.append((tr, va, re.sub(r" \([0-9.]+ s\)$", "", line[0])))
    assert runs[0] == runs[1]
    assert "valid" in runs[0][2] and np.isfinite(runs[0][1][0])
    assert mod.build_parser().parse_args([]).fused_eval is False


def test_header_and_binding_declare_the_new_symbols():
    from dadmm_hip import _lib
    header = open(os.path.join(ROOT, "include", "dadmm.h")).read()
    for sym in ("dadmm_forward_eval_scratch_bytes", "dadmm_forward_eval"):
        assert re.search(r"\b%s\(" % sym, header), sym
        assert sym in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), sym)
    assert _lib.ABI_VERSION >= 22
