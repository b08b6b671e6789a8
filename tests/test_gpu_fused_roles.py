"""The role-split form of the fused forward (csrc/dadmm_fused_roles.hip, DADMM_FUSED_FORM=roles:
waves 0-3 issue the MFMAs, waves 4-7 the element updates) against the CPU oracle, against the
row-split form (dadmm_fused.hip, DADMM_FUSED_FORM=rows) and against itself: every iterate, U_K and
the status word bit for bit. It serves shared graphs at n_pad = 256, P = 1..5, m <= 64; the cases
cover one full tile, a ragged batch with n < n_pad and m < 64, every agent count's GEMM1 pairing,
K = 1, the empty and the complete graph, the 'same' table and the GNN variant's clamps, the trained
25-row table (the clip schedule's late iterations) and the guards."""
import os

import networkx as nx
import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
MAXP = [0.1, 0.99, 0.99, 0.99]


def _inits(B, P, n, seed=99):
    rng = np.random.default_rng(seed)
    return (1e-2 * rng.standard_normal((3, B, P, n))).astype(np.float32)


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _hyp(K, H, seed):
    rng = np.random.default_rng(seed)
    return O.hyp_table((0.5 * rng.standard_normal((K, H, 4))).astype(np.float32), MAXP)


def _run(dev, monkeypatch, form, A, b, graphs, hyp, y0, U0, d0, variant=0, path="fused"):
    """(Y, U_K, status) of one forward under DADMM_FUSED_FORM=form."""
    from dadmm_hip import PreparedOperator, forward_raw, ingest
    monkeypatch.setenv("DADMM_FUSED_FORM", form)
    B = y0.shape[0]
    op = PreparedOperator(_t(A, dev))
    g = ingest(graphs, A.shape[0], B, dev)
    assert g.shared
    Y, U, st = forward_raw(op, _t(b, dev), g, _t(hyp, dev), _t(y0, dev), _t(U0, dev), _t(d0, dev),
                           variant=variant, want_U=True, path=path)
    torch.cuda.synchronize()
    return Y.cpu().numpy(), U.cpu().numpy(), int(st.item())


def _check(dev, monkeypatch, A, b, graphs, hyp, y0, U0, d0, variant=0):
    """roles == oracle == rows == roles again, on Y, U_K and the status word."""
    args = (A, b, graphs, hyp, y0, U0, d0)
    Y, U, st = _run(dev, monkeypatch, "roles", *args, variant=variant)
    Yo, Uo, sto = O.forward_f32(*args, variant=variant)
    assert st == sto == 0
    assert np.array_equal(Y, Yo), f"vs oracle: max |diff| {np.abs(Y - Yo).max()} at {np.argwhere(Y != Yo)[:3]}"
    assert np.array_equal(U, Uo), f"U_K vs oracle: max |diff| {np.abs(U - Uo).max()}"
    Yr, Ur, str_ = _run(dev, monkeypatch, "rows", *args, variant=variant)
    assert str_ == st and np.array_equal(Y, Yr) and np.array_equal(U, Ur)
    Y2, U2, st2 = _run(dev, monkeypatch, "roles", *args, variant=variant)
    assert st2 == st and np.array_equal(Y, Y2) and np.array_equal(U, U2)


def test_one_full_tile(cuda, monkeypatch):
    P, m, n, B, K = 5, 64, 256, 16, 3
    A, b, _ = O.make_problem(P, m, n, B, seed=41)
    y0, U0, d0 = _inits(B, P, n, seed=1)
    _check(cuda, monkeypatch, A, b, [O.er_graph(P, 0.5, seed=7)] * B, _hyp(K, P, 2), y0, U0, d0)


def test_ragged_batch_and_range_checked_rows(cuda, monkeypatch):
    """Three tiles, five live samples in the last; n < n_pad and m < 64."""
    P, m, n, B, K = 3, 50, 200, 37, 4
    A, b, _ = O.make_problem(P, m, n, B, seed=42)
    y0, U0, d0 = _inits(B, P, n, seed=2)
    _check(cuda, monkeypatch, A, b, [O.er_graph(P, 0.6, seed=3)] * B, _hyp(K, P, 3), y0, U0, d0)


@pytest.mark.parametrize("P", [1, 2, 4])
def test_agent_counts(cuda, monkeypatch, P):
    """A lone GEMM1 chain (P = 1), one pair (P = 2), a single agent beside a group of three (P = 4)."""
    m, n, B, K = 64, 256, 16, 2
    A, b, _ = O.make_problem(P, m, n, B, seed=50 + P)
    y0, U0, d0 = _inits(B, P, n, seed=P)
    _check(cuda, monkeypatch, A, b, [O.er_graph(P, 0.7, seed=P)] * B, _hyp(K, P, 4), y0, U0, d0)


def test_single_iteration(cuda, monkeypatch):
    """K = 1: the only dual update is the final one."""
    P, m, n, B, K = 5, 64, 256, 16, 1
    A, b, _ = O.make_problem(P, m, n, B, seed=43)
    y0, U0, d0 = _inits(B, P, n, seed=3)
    _check(cuda, monkeypatch, A, b, [O.er_graph(P, 0.5, seed=9)] * B, _hyp(K, P, 5), y0, U0, d0)


@pytest.mark.parametrize("kind", ["empty", "complete"])
def test_extreme_graphs(cuda, monkeypatch, kind):
    P, m, n, B, K = 5, 64, 256, 16, 3
    G = nx.empty_graph(P) if kind == "empty" else nx.complete_graph(P)
    A, b, _ = O.make_problem(P, m, n, B, seed=44)
    y0, U0, d0 = _inits(B, P, n, seed=4)
    _check(cuda, monkeypatch, A, b, [G] * B, _hyp(K, P, 6), y0, U0, d0)


@pytest.mark.parametrize("H,variant", [(1, 0), (5, 1), (1, 1)])
def test_same_mode_and_gnn_variant(cuda, monkeypatch, H, variant):
    """One table row per iteration ('same' mode) and the GNN variant's +-20 delta clamp and fixed clips."""
    P, m, n, B, K = 5, 64, 256, 16, 3
    A, b, _ = O.make_problem(P, m, n, B, seed=45)
    y0, U0, d0 = _inits(B, P, n, seed=5)
    rng = np.random.default_rng(7)
    hyp = O.hyp_table(rng.standard_normal((K, H, 4)).astype(np.float32), [0.3, 0.99, 0.99, 0.99])
    _check(cuda, monkeypatch, A, b, [O.er_graph(P, 0.5, seed=2)] * B, hyp, y0, U0, d0, variant=variant)


def test_trained_table_full_depth(cuda, monkeypatch):
    """The trained 25-row table, K = 25: the clip schedule runs through its late iterations."""
    P, m, n, B, K = 5, 64, 256, 32, 25
    trained = np.load(os.path.join(GOLD, "fixture_25_iter_general_learning_seq_hyp_param.npy"))
    A, b, _ = O.make_problem(P, m, n, B, seed=1234)
    y0, U0, d0 = _inits(B, P, n)
    _check(cuda, monkeypatch, A, b, [O.er_graph(P, 0.5, seed=7)] * B, O.hyp_table(trained, MAXP), y0, U0, d0)


def _guard_cases(P, m, n, B, K, seed):
    """(name, bit, A, b, graphs, hyp, y0, U0, d0): inputs drawn as test_gpu_parity's _guard_cases."""
    A, b, _ = O.make_problem(P, m, n, B, seed=seed)
    y0, U0, d0 = _inits(B, P, n, seed=seed)
    hyp = _hyp(K, P, seed)
    G = O.er_graph(P, 0.6, seed=2)
    y2 = y0.copy(); y2[B - 1, P - 1, n - 1] = np.nan
    U2 = U0.copy(); U2[0, 1 % P, 5] = np.inf
    h2 = hyp.copy(); h2[min(2, K - 1), P - 1, 0] = np.nan
    D = nx.DiGraph()
    D.add_nodes_from(range(P))
    D.add_edges_from([(0, 1), (1, 0), (1, 2), (2, 3), (3, 2), (3, 4), (4, 0), (0, 3)])
    return [("y0_nan", 1, A, b, [G] * B, hyp, y2, U0, d0),
            ("U0_inf", 2, A, b, [G] * B, hyp, y0, U2, d0),
            ("table_nan", 8, A, b, [G] * B, h2, y0, U0, d0),
            ("asymmetric_adjacency", 16, A, b, [D] * B, hyp, y0, U0, d0)]


def _auto_split_cols(dev, monkeypatch, A, b, graphs, hyp, y0, U0, d0):
    """The GEMM1 order of path "auto" for this batch, as test_gpu_parity's _run_hip finds it: the
    column-split forward's where it serves the batch and raises no bit on it (a raised bit sends
    the batch through the gated recomputation, whose order is the fused one)."""
    from dadmm_hip import PreparedOperator, ingest
    from dadmm_hip.ops import split_cols
    B = y0.shape[0]
    g = ingest(graphs, A.shape[0], B, dev)
    sc = split_cols(PreparedOperator(_t(A, dev)), B, hyp.shape[0], g, hyp_rows=hyp.shape[1])
    if sc and _run(dev, monkeypatch, "roles", A, b, graphs, hyp, y0, U0, d0, path="split")[2] != 0:
        sc = 0
    return sc


def test_guards(cuda, monkeypatch):
    """Each guard raises the same status bits as the row-split form; through path "auto" the gated
    recomputation then returns the oracle's guarded result."""
    P, m, n, B, K = 5, 64, 256, 16, 3
    for name, bit, *args in _guard_cases(P, m, n, B, K, seed=11):
        st = _run(cuda, monkeypatch, "roles", *args)[2]
        st_rows = _run(cuda, monkeypatch, "rows", *args)[2]
        assert st & bit, (name, st)
        assert st == st_rows, (name, st, st_rows)
        Y, U, sta = _run(cuda, monkeypatch, "roles", *args, path="auto")
        Yo, Uo, sto = O.forward_f32(*args, split_cols=_auto_split_cols(cuda, monkeypatch, *args))
        assert (sta & ~16) == sto, (name, sta, sto)
        np.testing.assert_array_equal(Y, Yo, err_msg=name)
        np.testing.assert_array_equal(U, Uo, err_msg=name)
