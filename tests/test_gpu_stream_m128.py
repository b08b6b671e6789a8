"""GPU parity of the streamed single launch with two 64-row groups per agent
(csrc/dadmm_stream.hip, stream_kernel<8, 1, ., 2>): 64 < m <= 128 at P <= 8, which holds the
reference's default shape P = 5, m = 100, n = 500 (configurations.py:6-9).

Bar: bit-exact (np.array_equal on every iterate, on U_K and on the recorded trajectory) against
oracle.forward_f32 / forward_f32_rec, and bit-identical to the per-iteration launches
(DADMM_TILED_STREAM=0) and to the stepwise recording. Reference: unfolded_DLASSO.py:53-107,
:127-140 and the GNN variant's clamps (gnn_dlasso_models_progressive.py:205-232)."""
import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

MAXP = [0.1, 0.99, 0.99, 0.99]


def _inits(B, P, n, seed=99):
    rng = np.random.default_rng(seed)
    return (1e-2 * rng.standard_normal((3, B, P, n))).astype(np.float32)


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _run(dev, A, b, graphs, hyp, y0, U0, d0, variant=0, want_U=True):
    from dadmm_hip import PreparedOperator, forward_raw, ingest
    B = y0.shape[0]
    op = PreparedOperator(_t(A, dev))
    g = ingest(graphs, A.shape[0], B, dev)
    Y, U, st = forward_raw(op, _t(b, dev), g, _t(hyp, dev), _t(y0, dev), _t(U0, dev),
                           _t(d0, dev), variant=variant, want_U=want_U, path="tiled")
    torch.cuda.synchronize()
    return Y.cpu().numpy(), (U.cpu().numpy() if U is not None else None), int(st.item())


# (P, m, n, B, K, graph prob, per-sample graphs, variant, hyp rows)
SHAPES = [
    (5, 100, 500, 20, 4, 0.5, False, 0, 5),   # the reference's defaults: ragged m, n and last tile
    (8, 128, 128, 16, 3, 0.6, True, 1, 1),    # full m_pad, every wave an agent, 4 blocks, GNN, 'same'
    (1, 65, 192, 5, 4, 0.5, False, 0, 1),     # one row in the second group, no consensus
    (3, 96, 256, 33, 1, 0.5, True, 0, 3),     # K = 1: no GEMM1 beyond R_0
    (8, 100, 160, 17, 2, 1.0, False, 1, 8),   # complete graph: the longest visit rows
    (5, 100, 500, 37, 5, 0.5, True, 1, 5),    # per-sample graphs at the default shape
]

_cache = {}


def _problem(P, m, n, B, K, prob, per_sample, variant, H):
    """Inputs and the oracle's recording for a shape, computed once and shared (never modified)."""
    key = (P, m, n, B, K, prob, per_sample, variant, H)
    if key not in _cache:
        A, b, _ = O.make_problem(P, m, n, B, seed=31 * P + n)
        graphs = ([O.connected_er_graph(P, prob, seed=500 + s) for s in range(B)] if per_sample
                  else [O.er_graph(P, prob, seed=7)] * B)
        y0, U0, d0 = _inits(B, P, n, seed=B + K)
        rng = np.random.default_rng(P + K)
        hyp = O.hyp_table((0.5 * rng.standard_normal((K, H, 4))).astype(np.float32), MAXP)
        ref = O.forward_f32_rec(A, b, graphs, hyp, y0, U0, d0, variant=variant)
        _cache[key] = (A, b, graphs, hyp, y0, U0, d0, ref)
    return _cache[key]


@pytest.mark.parametrize("form", ["stream", "launches"])
@pytest.mark.parametrize("P,m,n,B,K,prob,per_sample,variant,H", SHAPES)
def test_forms_bit_exact(cuda, monkeypatch, form, P, m, n, B, K, prob, per_sample, variant, H):
    from dadmm_hip import tiled_form
    monkeypatch.setenv("DADMM_TILED_STREAM", "1" if form == "stream" else "0")
    if form == "stream":   # a silent fall-back to the launches must not pass
        assert tiled_form((P, m, n)) == 1
    A, b, graphs, hyp, y0, U0, d0, (Yo, Uo, sto, _, _) = _problem(P, m, n, B, K, prob, per_sample, variant, H)
    Y, U, st = _run(cuda, A, b, graphs, hyp, y0, U0, d0, variant=variant)
    assert st == sto == 0
    assert np.array_equal(Y, Yo), f"max |diff| {np.abs(Y - Yo).max()}"
    assert np.array_equal(U, Uo), f"U_K max |diff| {np.abs(U - Uo).max()}"


@pytest.mark.parametrize("P,m,n,B,K,prob,per_sample,variant,H", [SHAPES[0], SHAPES[1], SHAPES[-1]])
def test_recording_bit_exact(cuda, P, m, n, B, K, prob, per_sample, variant, H):
    """record=True on the streamed launch (dadmm_forward_tiled_record) and on the stepwise
    kernels: Y, U_K, Grec and Urec bit-exact against oracle.forward_f32_rec on both, and the
    general adjoint gives the same bits on the two trajectories."""
    from dadmm_hip import PreparedOperator, forward_raw, ingest, tiled_form
    from dadmm_hip.ops import backward_raw
    assert tiled_form((P, m, n), record=True) == 1
    A, b, graphs, hyp, y0, U0, d0, (Yo, Uo, sto, Go, Uro) = _problem(P, m, n, B, K, prob, per_sample, variant, H)
    op = PreparedOperator(_t(A, cuda))
    g = ingest(graphs, P, B, cuda)
    outs = {}
    for path in ("tiled", "stepwise"):
        Y, U, st, traj = forward_raw(op, _t(b, cuda), g, _t(hyp, cuda), _t(y0, cuda), _t(U0, cuda),
                                     _t(d0, cuda), variant=variant, want_U=True, path=path,
                                     record=True)
        torch.cuda.synchronize()
        outs[path] = (Y, U, int(st.item()), traj)
    for path, (Y, U, st, traj) in outs.items():
        assert st == sto == 0, path
        assert np.array_equal(Y.cpu().numpy(), Yo), path
        assert np.array_equal(U.cpu().numpy(), Uo), path
        assert np.array_equal(traj.Grec[..., :n].cpu().numpy(), Go), path
        assert np.array_equal(traj.Urec[..., :n].cpu().numpy(), Uro), path
    gY = np.random.default_rng(3).standard_normal((K, B, P, n)).astype(np.float32)
    dh = [backward_raw(op, g, outs[p][3], _t(gY, cuda)).cpu().numpy() for p in ("tiled", "stepwise")]
    assert np.array_equal(dh[0], dh[1])


def test_without_U_out(cuda, monkeypatch):
    """want_U = False: the launch skips the final dual-update phase; Y is unchanged."""
    monkeypatch.setenv("DADMM_TILED_STREAM", "1")
    A, b, graphs, hyp, y0, U0, d0, (Yo, _, _, _, _) = _problem(*SHAPES[0])
    Y, U, st = _run(cuda, A, b, graphs, hyp, y0, U0, d0, want_U=False)
    assert U is None and st == 0
    assert np.array_equal(Y, Yo)


def test_flags_in_the_second_m_group(cuda, monkeypatch):
    """The streamed launch flags every case where one of the reference's batch-global guards
    fires (unfolded_DLASSO.py:55-61, 84-86, 102-104), also from a row of b in the second m-group
    (its first, row 64, and the last real one, row 99); path='tiled' has no recompute behind it."""
    from dadmm_hip import tiled_form
    monkeypatch.setenv("DADMM_TILED_STREAM", "1")
    P, m, n, B, K = 5, 100, 128, 19, 3
    assert tiled_form((P, m, n)) == 1
    A, b, _ = O.make_problem(P, m, n, B, seed=1)
    G = O.er_graph(P, 0.5, seed=1)
    y0, U0, d0 = _inits(B, P, n)
    hyp = O.hyp_table(np.zeros((K, P, 4), np.float32), MAXP)
    run = lambda *a: _run(cuda, A, *a)[2]   # noqa: E731
    b2 = b.copy(); b2[3, 1, 99] = np.nan
    assert run(b2, [G] * B, hyp, y0, U0, d0) & 4
    b3 = b.copy(); b3[3, 1, 64] = np.nan
    assert run(b3, [G] * B, hyp, y0, U0, d0) & 4
    y2 = y0.copy(); y2[18, 4, 127] = np.inf
    assert run(b, [G] * B, hyp, y2, U0, d0) & 1
    U2 = U0.copy(); U2[7, 2, 63] = -np.inf
    assert run(b, [G] * B, hyp, y0, U2, d0) & 2
    h2 = hyp.copy(); h2[1, 4, 0] = np.nan
    assert run(b, [G] * B, h2, y0, U0, d0) & 8
    assert run(b, [G] * B, hyp, y0, U0, d0) == 0


@pytest.mark.parametrize("case", ["b_nan"])
def test_recording_guard_fired_matches_stepwise(cuda, monkeypatch, case):
    """A training forward at the default shape (record=True, path='auto': the streamed recording
    launch) whose b has a NaN in row 99 is redone by the gated stepwise recomputation, which
    re-records Grec / Urec: status, Y, U_K, Grec, Urec and the adjoint are bit-identical to the
    stepwise recording and to oracle.forward_f32_rec (unfolded_DLASSO.py:55-61, 84-86, 102-104).
    (On 'auto' the streamed recording starts at a batch size where it is the faster one; the test
    lowers that threshold so that its 21 samples take it.)"""
    from dadmm_hip import PreparedOperator, forward_raw, ingest, ops, tiled_form
    from dadmm_hip.ops import backward_raw
    P, m, n, B, K = 5, 100, 500, 21, 4
    assert tiled_form((P, m, n), record=True) == 1
    monkeypatch.setattr(ops, "STREAM_RECORD_M128_MIN_B", 0)
    d = ops._lib.Dims(B=B, P=P, m=m, n=n, K=K, variant=0, hyp_rows=P, graph_shared=0)
    assert "tiled_record" in ops.plan_forward(d, True, record=True).candidates
    A, b, _ = O.make_problem(P, m, n, B, seed=44)
    graphs = [O.connected_er_graph(P, 0.5, seed=1300 + s) for s in range(B)]
    y0, U0, d0 = _inits(B, P, n, seed=45)
    rng = np.random.default_rng(46)
    hyp = O.hyp_table((0.5 * rng.standard_normal((K, P, 4))).astype(np.float32), MAXP)
    b = b.copy(); b[5, 3, 99] = np.nan
    op = PreparedOperator(_t(A, cuda))
    g = ingest(graphs, P, B, cuda)
    outs = {}
    for path in ("auto", "stepwise"):
        Y, U, st, traj = forward_raw(op, _t(b, cuda), g, _t(hyp, cuda), _t(y0, cuda), _t(U0, cuda),
                                     _t(d0, cuda), want_U=True, path=path, record=True)
        torch.cuda.synchronize()
        outs[path] = (Y.cpu().numpy(), U.cpu().numpy(), int(st.item()),
                      traj.Grec[..., :n].cpu().numpy(), traj.Urec[..., :n].cpu().numpy(), traj)
    Yo, Uo, sto, Go, Uro = O.forward_f32_rec(A, b, graphs, hyp, y0, U0, d0)
    assert sto != 0
    for path, (Y, U, st, Gr, Ur, _) in outs.items():
        assert st == sto, (path, st, sto)
        assert np.array_equal(Y, Yo, equal_nan=True), path
        assert np.array_equal(U, Uo, equal_nan=True), path
        assert np.array_equal(Gr, Go, equal_nan=True), path
        assert np.array_equal(Ur, Uro, equal_nan=True), path
    gY = np.random.default_rng(47).standard_normal((K, B, P, n)).astype(np.float32)
    dh = [backward_raw(op, g, outs[p][5], _t(gY, cuda)).cpu().numpy() for p in ("auto", "stepwise")]
    assert np.array_equal(dh[0], dh[1], equal_nan=True)


def test_more_than_eight_agents_keep_their_path(cuda, monkeypatch):
    """P > 8 at m > 64 has no streamed build (its registers do not fit): DADMM_TILED_STREAM=1
    still runs the per-iteration launches, and a recording goes through the stepwise kernels."""
    from dadmm_hip import PreparedOperator, forward_raw, ingest, tiled_form
    monkeypatch.setenv("DADMM_TILED_STREAM", "1")
    P, m, n, B, K = 16, 100, 256, 18, 3
    assert tiled_form((P, m, n)) == 0
    A, b, graphs, hyp, y0, U0, d0, (Yo, Uo, sto, Go, Uro) = _problem(P, m, n, B, K, 0.5, True, 0, P)
    Y, U, st = _run(cuda, A, b, graphs, hyp, y0, U0, d0)
    assert st == sto == 0
    assert np.array_equal(Y, Yo) and np.array_equal(U, Uo)
    op = PreparedOperator(_t(A, cuda))
    g = ingest(graphs, P, B, cuda)
    Y, U, st, traj = forward_raw(op, _t(b, cuda), g, _t(hyp, cuda), _t(y0, cuda), _t(U0, cuda),
                                 _t(d0, cuda), want_U=True, path="auto", record=True)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    assert np.array_equal(Y.cpu().numpy(), Yo) and np.array_equal(U.cpu().numpy(), Uo)
    assert np.array_equal(traj.Grec[..., :n].cpu().numpy(), Go)
    assert np.array_equal(traj.Urec[..., :n].cpu().numpy(), Uro)
