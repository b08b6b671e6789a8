"""The role-split forward with one agent's GEMM1 operand resident in registers
(csrc/dadmm_fused_roles.hip, DADMM_FUSED_FORM=roles) against the same kernel with every fragment
streamed (roles-stream), the row-split form (rows) and the CPU oracle: every iterate, U_K and the
status word bit for bit. The cases sit where the shortened fragment stream can go wrong: the ring
wrapping across one and two iteration boundaries, K = 1 (the block read by GEMM1(0) only), every
agent count (P = 1 streams no GEMM1 fragment, P = 2 has an empty first group, at P = 3 and 4 the
first group is the resident agent alone), resident rows past m and columns past n in a ragged batch, the operator replaced between
launches (a block kept across launches would show), and one guard."""
import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

MAXP = [0.1, 0.99, 0.99, 0.99]
FORMS = ("roles", "roles-stream", "rows")


def _inits(B, P, n, seed):
    rng = np.random.default_rng(seed)
    return (1e-2 * rng.standard_normal((3, B, P, n))).astype(np.float32)


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _hyp(K, H, seed):
    rng = np.random.default_rng(seed)
    return O.hyp_table((0.5 * rng.standard_normal((K, H, 4))).astype(np.float32), MAXP)


def _launch(dev, monkeypatch, form, op, P, b, graphs, hyp, y0, U0, d0):
    """(Y, U_K, status) of one forward of the prepared operator op under DADMM_FUSED_FORM=form."""
    from dadmm_hip import forward_raw, ingest
    monkeypatch.setenv("DADMM_FUSED_FORM", form)
    g = ingest(graphs, P, y0.shape[0], dev)
    assert g.shared
    Y, U, st = forward_raw(op, _t(b, dev), g, _t(hyp, dev), _t(y0, dev), _t(U0, dev), _t(d0, dev),
                           want_U=True, path="fused")
    torch.cuda.synchronize()
    return Y.cpu().numpy(), U.cpu().numpy(), int(st.item())


def _run(dev, monkeypatch, form, A, b, graphs, hyp, y0, U0, d0):
    from dadmm_hip import PreparedOperator
    return _launch(dev, monkeypatch, form, PreparedOperator(_t(A, dev)), A.shape[0], b, graphs, hyp, y0, U0, d0)


def _check(dev, monkeypatch, A, b, graphs, hyp, y0, U0, d0):
    """roles == roles-stream == rows == oracle, on Y, U_K and the status word."""
    args = (A, b, graphs, hyp, y0, U0, d0)
    Yo, Uo, sto = O.forward_f32(*args)
    assert sto == 0
    for form in FORMS:
        Y, U, st = _run(dev, monkeypatch, form, *args)
        assert st == 0, (form, st)
        assert np.array_equal(Y, Yo), \
            f"{form} vs oracle: max |diff| {np.abs(Y - Yo).max()} at {np.argwhere(Y != Yo)[:3]}"
        assert np.array_equal(U, Uo), f"{form}: U_K vs oracle: max |diff| {np.abs(U - Uo).max()}"


@pytest.mark.parametrize("K", [1, 2, 3])
def test_ring_wraps_with_the_shortened_stream(cuda, monkeypatch, K):
    """P = 5, one full tile. K = 1: the resident block is read by GEMM1(0) only; K = 2: the ring
    wraps once into the next iteration; K = 3: across two iteration boundaries."""
    P, m, n, B = 5, 64, 256, 16
    A, b, _ = O.make_problem(P, m, n, B, seed=60 + K)
    y0, U0, d0 = _inits(B, P, n, seed=K)
    _check(cuda, monkeypatch, A, b, [O.er_graph(P, 0.5, seed=7)] * B, _hyp(K, P, 2), y0, U0, d0)


@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_agent_counts(cuda, monkeypatch, P):
    """P = 1: no GEMM1 fragment is streamed, the ring's prefill is the head of GEMM2; P = 2: the
    first GEMM1 group is empty and the resident agent 0 leads the second; P = 3 and 4: the first
    group is the resident agent alone, so stage P streams nothing."""
    m, n, B, K = 64, 256, 16, 2
    A, b, _ = O.make_problem(P, m, n, B, seed=70 + P)
    y0, U0, d0 = _inits(B, P, n, seed=10 + P)
    _check(cuda, monkeypatch, A, b, [O.er_graph(P, 0.7, seed=P)] * B, _hyp(K, P, 4), y0, U0, d0)


def test_ragged_tile_and_resident_rows_past_m(cuda, monkeypatch):
    """Three tiles with five live samples in the last; m = 50: wave 3's resident rows 50..63 are
    padding; n = 200: the resident block's columns 200..255 are."""
    P, m, n, B, K = 3, 50, 200, 37, 4
    A, b, _ = O.make_problem(P, m, n, B, seed=81)
    y0, U0, d0 = _inits(B, P, n, seed=21)
    _check(cuda, monkeypatch, A, b, [O.er_graph(P, 0.6, seed=3)] * B, _hyp(K, P, 3), y0, U0, d0)


def test_operator_changed_between_launches(cuda, monkeypatch):
    """A1, then A2 through a fresh PreparedOperator, then A2 and A1 again copied in place into the
    first operator's workspace (the same device address), in one process: every result is the
    oracle's for the operator that launch was given."""
    from dadmm_hip import PreparedOperator
    P, m, n, B, K = 5, 64, 256, 16, 2
    A1, b, _ = O.make_problem(P, m, n, B, seed=91)
    A2, _, _ = O.make_problem(P, m, n, B, seed=92)
    assert not np.array_equal(A1, A2)
    y0, U0, d0 = _inits(B, P, n, seed=31)
    graphs, hyp = [O.er_graph(P, 0.5, seed=5)] * B, _hyp(K, P, 6)
    want = {}
    for name, A in (("A1", A1), ("A2", A2)):
        want[name] = O.forward_f32(A, b, graphs, hyp, y0, U0, d0)
        assert want[name][2] == 0
    assert not np.array_equal(want["A1"][0], want["A2"][0])

    def check(op, name, step):
        Y, U, st = _launch(cuda, monkeypatch, "roles", op, P, b, graphs, hyp, y0, U0, d0)
        Yo, Uo, _ = want[name]
        assert st == 0, step
        assert np.array_equal(Y, Yo), f"{step}: max |diff| {np.abs(Y - Yo).max()}"
        assert np.array_equal(U, Uo), step

    op1 = PreparedOperator(_t(A1, cuda))
    check(op1, "A1", "first operator")
    op2 = PreparedOperator(_t(A2, cuda))
    check(op2, "A2", "fresh PreparedOperator")
    check(op1, "A1", "first operator again")
    ptr = op1.workspace.data_ptr()
    op1.workspace.copy_(op2.workspace)
    assert op1.workspace.data_ptr() == ptr
    check(op1, "A2", "A2 copied in place")
    op1.workspace.copy_(PreparedOperator(_t(A1, cuda)).workspace)
    assert op1.workspace.data_ptr() == ptr
    check(op1, "A1", "A1 copied back in place")


def test_guard_y0_nan(cuda, monkeypatch):
    """A NaN in y0 raises the same status bits in all three forms."""
    P, m, n, B, K = 5, 64, 256, 16, 3
    A, b, _ = O.make_problem(P, m, n, B, seed=95)
    y0, U0, d0 = _inits(B, P, n, seed=41)
    y0 = y0.copy()
    y0[B - 1, P - 1, n - 1] = np.nan
    args = (A, b, [O.er_graph(P, 0.6, seed=2)] * B, _hyp(K, P, 8), y0, U0, d0)
    st = {form: _run(cuda, monkeypatch, form, *args)[2] for form in FORMS}
    assert st["rows"] & 1, st
    assert st["roles"] == st["rows"] == st["roles-stream"], st
