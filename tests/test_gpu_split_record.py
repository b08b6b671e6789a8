"""GPU parity of the RECORDING column-split forward (csrc/dadmm_split.hip compiled with
DADMM_SPLIT_REC, dadmm_forward_split_record): the training forward for small batches.

The oracle restates the split GEMM1 order (oracle.forward_f32(..., split_cols=64)) but has no
split-order recording, so the trajectory's targets are built from what it exports:
  * Urec[k], k >= 1, is the U_K of the split-order run truncated to the first k rows of the table
    (the per-iteration clamps depend on k only); Urec[0] is U0;
  * Grec[k] is pinned by re-applying the primal update to it in numpy float32:
    clip(y_k - alpha_k * clip(Grec[k], +-gclip_k), +-vclip_k) == Y[k] (two roundings, y_k = y0 or
    Y[k-1]); a wrong pre-clamp gradient inside the clamp band changes Y[k];
  * on inputs whose fp32 sums are exact the split and the fused order coincide, and Grec / Urec
    must equal oracle.forward_f32_rec's bit-for-bit.
Everything is np.array_equal. The adjoint consumes the split trajectory unchanged (its own bound,
test_gpu_adjoint.ADJ_RTOL, along its own trajectory). The default recording path (no opt-in) keeps
the fused order.
"""
import argparse
import os

import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TRAINED = np.load(os.path.join(GOLD, "fixture_25_iter_general_learning_seq_hyp_param.npy"))
MAXP = [0.1, 0.99, 0.99, 0.99]
ADJ_RTOL = 1e-5     # tests/test_gpu_adjoint.py


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _inits(B, P, n, seed=99):
    rng = np.random.default_rng(seed)
    return (1e-2 * rng.standard_normal((3, B, P, n))).astype(np.float32)


def _hyp(K, P, seed=3, same=False):
    rng = np.random.default_rng(seed)
    param = (0.3 * rng.standard_normal((K, 1 if same else P, 4))).astype(np.float32)
    return O.hyp_table(param, MAXP)


def _graphs(P, B, kind):
    """As tests/test_gpu_split.py builds them."""
    if kind == "shared":
        return [O.er_graph(P, 0.5, seed=7)] * B
    graphs = [O.connected_er_graph(P, 0.5, seed=200 + s) for s in range(B)]
    if kind == "ordered":
        import networkx as nx
        rng = np.random.default_rng(5)
        out = []
        for g0 in graphs:       # same edges, adjacency lists inserted in a shuffled order
            g1 = nx.Graph()
            g1.add_nodes_from(range(P))
            edges = list(g0.edges())
            rng.shuffle(edges)
            g1.add_edges_from((v, u) if rng.random() < 0.5 else (u, v) for u, v in edges)
            out.append(g1)
        graphs = out
    return graphs


def _clips(variant, k):
    """iter_clips (unfolded_DLASSO.py:80, :92; gnn_dlasso_models_progressive.py:212, :224)."""
    if variant == 0:
        return np.float32(max(1.0, 30.0 - k)), np.float32(max(10.0, 200.0 - 3 * k))
    return np.float32(10.0), np.float32(100.0)


class _Run:
    pass


def _record(dev, A, b, graphs, hyp, y0, U0, d0, variant=0, path="split", train_split=False):
    from dadmm_hip import PreparedOperator, forward_raw, ingest
    from dadmm_hip.ops import split_cols
    B, P = y0.shape[:2]
    n = A.shape[-1]
    opt_in = {"train_split": True} if train_split else {}    # the keyword only where it is tested
    r = _Run()
    r.op = PreparedOperator(_t(A, dev))
    r.g = ingest(graphs, P, B, dev)
    Y, U, st, traj = forward_raw(r.op, _t(b, dev), r.g, _t(hyp, dev), _t(y0, dev), _t(U0, dev),
                                 _t(d0, dev), variant=variant, want_U=True, path=path, record=True,
                                 **opt_in)
    torch.cuda.synchronize()
    r.traj = traj
    r.fused = traj.fused
    r.Y, r.U, r.st = Y.cpu().numpy(), U.cpu().numpy(), int(st.item())
    r.Grec = traj.Grec[..., :n].cpu().numpy()
    r.Urec = traj.Urec[..., :n].cpu().numpy()
    r.sc = split_cols(r.op, B, hyp.shape[0], r.g, hyp_rows=hyp.shape[1], record=True,
                      **opt_in)
    r.sc_default = split_cols(r.op, B, hyp.shape[0], r.g, hyp_rows=hyp.shape[1], record=True)
    return r


def _assert_eq(got, want, what):
    assert np.array_equal(got, want), (f"{what}: {np.sum(got != want)} of {got.size} differ, first "
                                       f"at {np.argwhere(got != want)[:3].tolist()}")


def _check_reapplication(r, hyp, y0, variant, ks=None):
    """clip(y_k - alpha_k clip(Grec[k])) == Y[k] in float32, two roundings."""
    K = hyp.shape[0]
    for k in (range(K) if ks is None else ks):
        gclip, vclip = _clips(variant, k)
        yk = y0 if k == 0 else r.Y[k - 1]
        al = hyp[k, :, 0].astype(np.float32)[None, :, None]
        g = np.clip(r.Grec[k], -gclip, gclip)
        prod = (al * g).astype(np.float32)
        yn = np.clip((yk - prod).astype(np.float32), -vclip, vclip)
        _assert_eq(yn, r.Y[k], f"re-application of Grec[{k}]")


def _check_urec(r, A, b, graphs, hyp, y0, U0, d0, variant, ks):
    _assert_eq(r.Urec[0], U0, "Urec[0]")
    for k in ks:
        Uk = O.forward_f32(A, b, graphs, hyp[:k], y0, U0, d0, variant=variant, split_cols=64)[1]
        _assert_eq(r.Urec[k], Uk, f"Urec[{k}]")


CASES = [
    # P, m,  n,  B,  K, graph,  variant, same
    (5, 64, 256, 40, 8, "shared", 0, False),
    (5, 64, 256, 48, 6, "ordered", 1, False),
    (6, 64, 256, 17, 5, "shared", 0, True),
    (3, 50, 200, 20, 7, "lane", 0, False),
    (2, 64, 100, 16, 5, "lane", 1, False),
    (1, 32, 256, 24, 4, "shared", 0, False),
]


@pytest.mark.parametrize("P,m,n,B,K,graph,variant,same", CASES)
def test_split_record_bit_exact(cuda, P, m, n, B, K, graph, variant, same):
    A, b, _ = O.make_problem(P, m, n, B, seed=11 + P + n)
    graphs = _graphs(P, B, graph)
    y0, U0, d0 = _inits(B, P, n)
    hyp = _hyp(K, P, same=same)
    r = _record(cuda, A, b, graphs, hyp, y0, U0, d0, variant, path="split")
    assert r.st == 0 and r.fused
    Yo, Uo, sto = O.forward_f32(A, b, graphs, hyp, y0, U0, d0, variant=variant, split_cols=64)
    assert sto == 0
    _assert_eq(r.Y, Yo, "Y")
    _assert_eq(r.U, Uo, "U_K")
    _check_urec(r, A, b, graphs, hyp, y0, U0, d0, variant, range(1, K))
    _check_reapplication(r, hyp, y0, variant)
    assert np.isfinite(r.Grec).all() and np.isfinite(r.Urec).all()


@pytest.mark.parametrize("P,m,n,B", [(5, 64, 256, 40), (4, 64, 128, 20)])
def test_split_record_grec_exact_on_order_independent_inputs(cuda, P, m, n, B):
    """Dyadic inputs whose fp32 sums are exact for two iterations: every summation order gives the
    same bits, so the split recording must equal the fused-order oracle's Grec / Urec."""
    K = 2
    rng = np.random.default_rng(0)
    A = (rng.integers(-1, 2, (P, m, n)) * (rng.random((P, m, n)) < 0.25) * 2.0 ** -3).astype(np.float32)
    b = (rng.integers(-8, 9, (B, P, m)) * 2.0 ** -3).astype(np.float32)
    y0, U0, d0 = ((rng.integers(-4, 5, (B, P, n)) * 2.0 ** -6).astype(np.float32) for _ in range(3))
    hyp = np.tile(np.array([2.0 ** -4, 2.0 ** -2, 2.0 ** -1, 2.0 ** -1], np.float32), (K, P, 1))
    graphs = [O.er_graph(P, 0.5, seed=7)] * B
    Yo, Uo, sto, Go, Uro = O.forward_f32_rec(A, b, graphs, hyp, y0, U0, d0)
    Ys = O.forward_f32(A, b, graphs, hyp, y0, U0, d0, split_cols=64)[0]
    assert sto == 0 and np.array_equal(Ys, Yo), "precondition: the two orders must coincide"
    r = _record(cuda, A, b, graphs, hyp, y0, U0, d0, path="split")
    assert r.st == 0
    _assert_eq(r.Y, Yo, "Y")
    _assert_eq(r.U, Uo, "U_K")
    _assert_eq(r.Grec, Go, "Grec")
    _assert_eq(r.Urec, Uro, "Urec")


def test_split_record_several_tiles_per_group(cuda):
    """B = 2048 at n_pad 256: 128 tiles over 64 workgroup groups (each walks two tiles), through
    the "auto" path with train_split."""
    P, m, n, B, K = 5, 64, 256, 2048, 3
    A, b, _ = O.make_problem(P, m, n, B, seed=77)
    graphs = [O.connected_er_graph(P, 0.5, seed=900 + s % 97) for s in range(B)]
    y0, U0, d0 = _inits(B, P, n, seed=8)
    hyp = _hyp(K, P)
    r = _record(cuda, A, b, graphs, hyp, y0, U0, d0, path="auto", train_split=True)
    assert r.sc == 64 and r.sc_default == 0 and r.st == 0
    Yo, Uo, _ = O.forward_f32(A, b, graphs, hyp, y0, U0, d0, split_cols=64)
    _assert_eq(r.Y, Yo, "Y")
    _assert_eq(r.U, Uo, "U_K")
    _check_urec(r, A, b, graphs, hyp, y0, U0, d0, 0, range(1, K))
    _check_reapplication(r, hyp, y0, 0)


def _close(got, want, rtol=ADJ_RTOL):
    """tests/test_gpu_adjoint.py's bound."""
    err = np.abs(got - want)
    bound = rtol * np.abs(want).max() + rtol * np.abs(want)
    assert (err <= bound).all(), (f"max err {err.max():.3e} (rel to max "
                                  f"{err.max() / np.abs(want).max():.3e})")


@pytest.mark.parametrize("P,m,n,B,K,graph,variant", [
    (5, 64, 256, 40, 25, "shared", 0),     # trained table
    (3, 50, 200, 20, 7, "lane", 1),
])
def test_adjoint_on_split_trajectory(cuda, P, m, n, B, K, graph, variant):
    """dadmm_backward reads only Y / Grec / Urec / y0 / d0: along the split trajectory it meets
    the fp64 oracle adjoint (fed the same arrays) at the project's adjoint bound."""
    from dadmm_hip.ops import backward_raw
    A, b, _ = O.make_problem(P, m, n, B, seed=P * 10 + n)
    graphs = _graphs(P, B, graph)
    y0, U0, d0 = _inits(B, P, n, seed=B)
    hyp = O.hyp_table(TRAINED, MAXP) if K == 25 else _hyp(K, P, seed=K)
    r = _record(cuda, A, b, graphs, hyp, y0, U0, d0, variant, path="split")
    assert r.st == 0 and r.fused
    _assert_eq(r.Y, O.forward_f32(A, b, graphs, hyp, y0, U0, d0, variant=variant, split_cols=64)[0], "Y")
    rng = np.random.default_rng(7)
    gY = rng.standard_normal((K, B, P, n)).astype(np.float32)
    gY[: K // 2] *= 0.1
    dh = backward_raw(r.op, r.g, r.traj, _t(gY, cuda))
    torch.cuda.synchronize()
    want = O.backward_np64(A, graphs, hyp, y0, d0, r.Y, r.Grec, r.Urec, gY, variant=variant)
    _close(dh.cpu().numpy().astype(np.float64), want)


def test_default_record_path_unchanged(cuda):
    """Without the opt-in a recording forward keeps the fused order at a batch the inference path
    splits (and that order is not the split one: the test discriminates)."""
    P, m, n, B, K = 5, 64, 256, 40, 25
    A, b, _ = O.make_problem(P, m, n, B, seed=1234)
    graphs = [O.er_graph(P, 0.5, seed=7)] * B
    y0, U0, d0 = _inits(B, P, n)
    hyp = O.hyp_table(TRAINED, MAXP)
    r = _record(cuda, A, b, graphs, hyp, y0, U0, d0, path="auto")
    assert r.st == 0 and r.sc == 0 and r.sc_default == 0
    Yo, _, _, Go, Uro = O.forward_f32_rec(A, b, graphs, hyp, y0, U0, d0)
    _assert_eq(r.Y, Yo, "Y")
    _assert_eq(r.Grec, Go, "Grec")
    _assert_eq(r.Urec, Uro, "Urec")
    Ys = O.forward_f32(A, b, graphs, hyp, y0, U0, d0, split_cols=64)[0]
    assert not np.array_equal(r.Y, Ys)


def test_split_record_guards_recompute(cuda):
    """A NaN in y0 (reference guard :55-57): the split recording launch flags the batch and the
    gated stepwise launch re-records it with the guards applied (the stepwise order)."""
    P, m, n, B, K = 5, 64, 256, 40, 6
    A, b, _ = O.make_problem(P, m, n, B, seed=3)
    graphs = [O.er_graph(P, 0.5, seed=7)] * B
    y0, U0, d0 = _inits(B, P, n)
    y0[3, 2, 17] = np.nan
    hyp = _hyp(K, P)
    r = _record(cuda, A, b, graphs, hyp, y0, U0, d0, path="auto", train_split=True)
    Yo, Uo, sto = O.forward_f32(A, b, graphs, hyp, y0, U0, d0)
    assert r.sc == 64 and r.st == sto and sto & 1
    _assert_eq(r.Y, Yo, "Y")
    _assert_eq(r.U, Uo, "U_K")


def _args(K, mode="diff"):
    return argparse.Namespace(GHN_iter_num=K, DADMM_mode=mode, alpha_max=0.1, tau_max=0.99,
                              rho_max=0.99, eta_max=0.99, max_penalty_threshold=0.8,
                              penalty_reduction_factor=0.95)


def test_module_train_split(cuda):
    """DLASSO_unfolded.train_split: a training forward follows the split order, loss.backward()
    gives the oracle chain's gradient along that trajectory (built as
    test_gpu_adjoint.test_module_backward_matches_oracle_chain builds it), and the switch off
    gives the fused order."""
    import gnn_dlasso_utils
    import unfolded_DLASSO
    P, m, n, B, K = 5, 64, 256, 32, 25
    A, b, x = O.make_problem(P, m, n, B, seed=21)
    model = unfolded_DLASSO.DLASSO_unfolded(_t(A, cuda)[None], _args(K)).to(cuda)
    with torch.no_grad():
        model.seq_hyp.param.copy_(torch.from_numpy(TRAINED))
    model.train()
    assert model.train_split is False
    graphs = [O.er_graph(P, 0.5, seed=7)] * B
    y0, U0, d0 = _inits(B, P, n)
    inits = tuple(_t(v, cuda) for v in (y0, U0, d0))
    table_cpu = model.seq_hyp.table(K).detach().cpu().numpy()

    Yf, _ = model(_t(b, cuda)[..., None], graphs, inits=inits)
    _assert_eq(Yf[..., 0].detach().cpu().numpy(),
               O.forward_f32_rec(A, b, graphs, table_cpu, y0, U0, d0)[0], "fused-order Y")

    model.train_split = True
    Y, _ = model(_t(b, cuda)[..., None], graphs, inits=inits)
    assert int(model.last_status.item()) == 0
    Yo = O.forward_f32(A, b, graphs, table_cpu, y0, U0, d0, split_cols=64)[0]
    Yh = Y[..., 0].detach().cpu().numpy()
    _assert_eq(Yh, Yo, "split-order Y")
    assert not np.array_equal(Yh, Yf[..., 0].detach().cpu().numpy())

    label = _t(x, cuda)[..., None]
    _, loss_final = gnn_dlasso_utils.compute_loss(Y, label)
    loss_final.backward()
    got = model.seq_hyp.param.grad.cpu().numpy()

    # the oracle chain along the split trajectory: Y and Urec from the oracle's split-order runs,
    # Grec from a raw recording of the same batch (the oracle exports no split-order Grec; the
    # re-application identity pins it to the oracle's Y), the adjoint in fp64, then autograd
    # through the table on the CPU
    r = _record(cuda, A, b, graphs, table_cpu, y0, U0, d0, path="split")
    _assert_eq(r.Y, Yo, "raw split-order Y")
    _check_reapplication(r, table_cpu, y0, 0)
    Uro = np.stack([U0] + [O.forward_f32(A, b, graphs, table_cpu[:k], y0, U0, d0, split_cols=64)[1]
                           for k in range(1, K)])
    _assert_eq(r.Urec, Uro, "Urec")
    gY = np.zeros((K, B, P, n))
    gY[-1] = 2.0 * (Yo[-1].astype(np.float64) - x[:, None, :]) / (B * n * P)
    dtab = O.backward_np64(A, graphs, table_cpu, y0, d0, Yo, r.Grec, Uro, gY)
    p = torch.tensor(TRAINED, dtype=torch.float64, requires_grad=True)
    seq = unfolded_DLASSO.seq_hyperparam([K, P, 4], torch.tensor(MAXP, dtype=torch.float64), _args(K))
    seq.param = torch.nn.Parameter(p)
    seq.train()
    want, = torch.autograd.grad(seq.table(K), seq.param, grad_outputs=torch.from_numpy(dtab))
    _close(got.astype(np.float64), want.numpy(), rtol=1e-4)
