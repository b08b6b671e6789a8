"""CPU side of the saturating regime (tests/saturation.py): under saturation the oracle is the
referee for vclip, the delta clamp and sign(0), so it is pinned there first (its two fp64
restatements, the fp32 recording, the CPU module path), and a test of the tests shows that the
ladder inputs see every clamp defect listed in ``DEFECTS`` while the suite's usual 1e-2 * randn
inputs see none of them.
"""
import argparse

import numpy as np
import pytest
import torch

import oracle as O
import saturation as S
from oracle import ref_torch as RT

# ---- the ladder itself --------------------------------------------------------------------------
def test_ladder_inits_shape_scales_and_zeros():
    B, P, n, top = 10, 3, 400, 150.0
    y0, U0, d0 = S.ladder_inits(B, P, n, 0, top)
    assert y0.dtype == U0.dtype == d0.dtype == np.float32 and y0.shape == (B, P, n)
    sc = S.ladder_scales(top)
    for s in range(B):
        assert 0.8 * sc[s % 5] <= U0[s].std() <= 1.2 * sc[s % 5]
        assert 0.8 * 0.2 * sc[s % 5] <= d0[s].std() <= 1.2 * 0.2 * sc[s % 5]
    zero = y0 == 0
    neg = zero & np.signbit(y0)
    assert abs(neg.mean() - 0.125) < 0.01 and abs((zero & ~neg).mean() - 0.125) < 0.01
    again = S.ladder_inits(B, P, n, 0, top)
    assert all(np.array_equal(a, b) for a, b in zip((y0, U0, d0), again))


@pytest.mark.parametrize("name", list(S.CASES))
def test_cases_engage_every_clamp(name):
    """The precondition of every GPU case holds on the oracle (adjoint margins included)."""
    S.case(name).engaged(adjoint=True)


def test_assert_engaged_rejects_the_usual_inputs():
    """The suite's 1e-2 * randn regime fails the precondition (only the gradient clamp is active)."""
    P, m, n, B, K = 5, 64, 256, 16, 4
    A, b, _ = O.make_problem(P, m, n, B, seed=1)
    graphs = [O.er_graph(P, 0.5, seed=3)] * B
    y0, U0, d0 = (1e-2 * np.random.default_rng(0).standard_normal((3, B, P, n))).astype(np.float32)
    for variant in (0, 1):
        hyp = S.ladder_hyp(K, P, 0)
        Y, U, st, G, Ur = O.forward_f32_rec(A, b, graphs, hyp, y0, U0, d0, variant=variant)
        with pytest.raises(AssertionError, match="inputs unsuitable"):
            S.assert_engaged(variant, hyp, y0, Y, U, G, Ur, graphs)


# ---- the oracle under saturation ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["lanes_v0", "lanes_v1", "fused_v0", "fused_v1_same", "general_same"])
def test_two_fp64_restatements_agree_on_ladder_inputs(name):
    """forward_f64 (C, the reference's loop form) == forward_np64 (vectorised, Laplacian matrix) at
    test_oracle.test_two_fp64_restatements_agree's bar, where vclip, the delta clamp and sign(0) act."""
    c = S.case(name)
    c.engaged()
    Yc, Uc, st = O.forward_f64(*c.args, variant=c.variant)
    Yn, Un = O.forward_np64(*c.args, variant=c.variant)
    assert st == 0
    np.testing.assert_allclose(Yc, Yn, rtol=0, atol=1e-8)
    np.testing.assert_allclose(Uc, Un, rtol=0, atol=1e-8)


@pytest.mark.parametrize("name,split", [("fused_v0", 0), ("fused_v1", 0), ("lanes_v1", 0), ("tiled_v0", 0),
                                        ("fused_v0", 64), ("fused_v1", 64)])
def test_forward_f32_rec_reapplication_on_ladder_inputs(name, split):
    """As test_oracle.test_forward_f32_rec_records_the_trajectory: Y and U_K are forward_f32's,
    Urec[k] is the truncated run's U, and clip(y_k - alpha_k clip(Grec[k])) == Y[k] bit for bit."""
    c = S.case(name, split_cols=split)
    c.engaged()
    Y, U, st = O.forward_f32(*c.args, variant=c.variant, split_cols=split)
    assert st == c.st == 0
    assert np.array_equal(Y, c.Y) and np.array_equal(U, c.U)
    assert np.array_equal(c.Urec[0], c.U0)
    for k in range(c.K):
        if k:
            Uk = O.forward_f32(c.A, c.b, c.graphs, c.hyp[:k], c.y0, c.U0, c.d0, variant=c.variant,
                               split_cols=split)[1]
            assert np.array_equal(c.Urec[k], Uk)
        gc, vc = (np.float32(v) for v in S.clips(c.variant, k))
        yk = c.y0 if k == 0 else c.Y[k - 1]
        al = np.broadcast_to(c.hyp[k][:, 0], (c.dims[0],))[None, :, None]
        g = np.clip(c.Grec[k], -gc, gc)
        assert np.array_equal(np.clip(yk - al * g, -vc, vc), c.Y[k])


def _args(K, mode="diff"):
    return argparse.Namespace(GHN_iter_num=K, DADMM_mode=mode, alpha_max=0.1, tau_max=0.99, rho_max=0.99,
                              eta_max=0.99, max_penalty_threshold=0.8, penalty_reduction_factor=0.95,
                              GHyp_hidden=8)


@pytest.mark.parametrize("P,m,n,B,K,mode,top", [(5, 20, 32, 10, 4, "diff", 150.0), (4, 10, 16, 10, 4, "same", 150.0)])
def test_cpu_module_forward_on_ladder_inits(P, m, n, B, K, mode, top):
    """dadmm_cpu's module forward against the literal fp32 replay and the fp64 restatement, at
    test_cpu_path.test_unfolded_cpu_matches_reference_ops's bars."""
    import unfolded_DLASSO as U
    from test_cpu_path import _close
    A, b, _ = O.make_problem(P, m, n, B, seed=P + K)
    graphs = [O.connected_er_graph(P, 0.5, seed=10 + s) for s in range(B)]
    mod = U.DLASSO_unfolded(torch.from_numpy(A)[None], _args(K, mode)).eval()
    with torch.no_grad():
        mod.seq_hyp.param.copy_(0.3 * torch.randn(mod.seq_hyp.param.shape, generator=torch.Generator().manual_seed(1)))
        mod.seq_hyp.param[0, :, 0] += 1.5
        mod.seq_hyp.param[0, :, 3] += 1.5
    y0, U0, d0 = S.ladder_inits(B, P, n, 3, top)
    with torch.no_grad():
        Y, _ = mod(torch.from_numpy(b)[..., None], graphs, inits=tuple(torch.from_numpy(v)[..., None] for v in (y0, U0, d0)))
    tab = mod.seq_hyp.table(K).detach().numpy()
    Yo, Uo, st, G, Ur = O.forward_f32_rec(A, b, graphs, tab, y0, U0, d0)
    rows, zeros, lanes = S.activity(0, y0, Yo, Uo, G, Ur, graphs)
    assert zeros >= S.MIN_ZEROS and all(min(r["y"]) > 0 and min(r["U"]) > 0 for r in rows), "inputs unsuitable"
    ref = RT.forward(A, b, graphs, tab, y0, U0, d0)
    _close(Y[..., 0].numpy(), ref)
    Y64, _ = O.forward_np64(A, b, graphs, tab, y0, U0, d0)
    for want in (ref[-1], Y64[-1]):
        assert float(np.mean((Y[-1, ..., 0].numpy() - want) ** 2)) <= 1e-5
    assert int(mod.last_status[0]) == 0


# ---- a test of the tests ------------------------------------------------------------------------
FORWARD_DEFECTS = {
    "vclip_k_for_vclip_prev": (0,),      # a deferred dual update clamping with the next iteration's bound
    "no_dlim": (1,),                     # the GNN variant's delta clamp missing
    "copysign_for_sign": (0, 1),         # sign(+-0) = +-1
    "no_U_clamp": (0, 1),
}
ADJOINT_DEFECTS = {
    "no_w_mask": (0, 1),                 # [|U + delta eta| <= vclip]
    "no_z_mask": (0, 1),                 # [|y - alpha g| <= vclip]
    "no_dlim_mask": (1,),                # [|2Ly| <= 20]
}
DEFECTS = {**FORWARD_DEFECTS, **ADJOINT_DEFECTS}


def _np_run(A, b, graphs, hyp, y0, U0, d0, gY, variant, defect=None):
    """The recurrence and its reverse mode in plain numpy float64 (the ops of
    unfolded_DLASSO.py:53-107 / gnn_dlasso_models_progressive.py:205-237), with one switchable
    defect. Returns (Y, U_K, dhyp [K,P,4])."""
    A = np.asarray(A, np.float64)
    P = A.shape[0]
    K = hyp.shape[0]
    AtA = np.einsum("pri,prj->pij", A, A)
    Atb = np.einsum("pri,bpr->bpi", A, np.asarray(b, np.float64))
    cnt = S.visit_counts(graphs, P)
    L2 = cnt.sum(-1)[:, :, None] * np.eye(P)[None] - cnt                   # 2 L
    deg = np.array([[len(list(G.neighbors(p))) for p in range(P)] for G in graphs], np.float64)[:, :, None]
    cons = lambda v: np.einsum("bpq,bqi->bpi", L2, v)                       # noqa: E731
    h = np.broadcast_to(np.asarray(hyp, np.float64), (K, P, 4))
    y, U, d = (np.asarray(v, np.float64) for v in (y0, U0, d0))
    tape, Y = [], []
    for k in range(K):
        al, ta, rh, et = (h[k][:, c][None, :, None] for c in range(4))
        gclip, vclip = S.clips(variant, k)
        uclip = S.clips(variant, k + 1)[1] if defect == "vclip_k_for_vclip_prev" else vclip
        sg = np.copysign(1.0, y) if defect == "copysign_for_sign" else np.sign(y)
        gr = np.einsum("pij,bpj->bpi", AtA, y) - Atb + sg * ta + U * deg + d * rh
        g = np.clip(gr, -gclip, gclip)
        z = y - al * g
        yn = np.clip(z, -vclip, vclip)
        draw = cons(yn)
        dn = np.clip(draw, -S.DLIM, S.DLIM) if variant != 0 and defect != "no_dlim" else draw
        w = U + dn * et
        Un = w if defect == "no_U_clamp" else np.clip(w, -uclip, uclip)
        tape.append((y, d, gr, g, z, draw, dn, w, sg, gclip, vclip))
        y, U, d = yn, Un, dn
        Y.append(y)
    dh = np.zeros((K, P, 4))
    yb, Ub, db = (np.zeros_like(y) for _ in range(3))
    for k in reversed(range(K)):
        al, ta, rh, et = (h[k][:, c][None, :, None] for c in range(4))
        yk, dk, gr, g, z, draw, dn, w, sg, gclip, vclip = tape[k]
        yb = yb + np.asarray(gY[k], np.float64)
        wb = Ub if defect == "no_w_mask" else Ub * (np.abs(w) <= vclip)
        dh[k, :, 3] = (wb * dn).sum(axis=(0, 2))
        dnb = db + wb * et
        if variant != 0 and defect != "no_dlim_mask":
            dnb = dnb * (np.abs(draw) <= S.DLIM)
        yb = yb + cons(dnb)                                                  # 2 L is symmetric
        zb = yb if defect == "no_z_mask" else yb * (np.abs(z) <= vclip)
        dh[k, :, 0] = (-zb * g).sum(axis=(0, 2))
        grb = -al * zb * (np.abs(gr) <= gclip)
        dh[k, :, 1] = (grb * sg).sum(axis=(0, 2))
        dh[k, :, 2] = (grb * dk).sum(axis=(0, 2))
        Ub = wb + grb * deg
        db = grb * rh
        yb = zb + np.einsum("pij,bpj->bpi", AtA, grb)
    return np.stack(Y), U, dh


def _gY(shape):
    return np.random.default_rng(7).standard_normal(shape)


def test_defect_free_numpy_step_is_the_oracle():
    """With no defect the numpy step is forward_np64 and backward_np64 (H = P and H = 1)."""
    for name in ("lanes_v0", "lanes_v1", "fused_v1_same"):
        c = S.case(name)
        P, m, n, B = c.dims
        gY = _gY((c.K, B, P, n))
        Y, U, dh = _np_run(*c.args, gY, c.variant)
        Yn, Un = O.forward_np64(*c.args, variant=c.variant)
        np.testing.assert_allclose(Y, Yn, rtol=0, atol=1e-9)
        np.testing.assert_allclose(U, Un, rtol=0, atol=1e-9)
        Y64, G64, U64, _ = RT.forward_autograd(c.A.copy(), c.b.copy(), c.graphs,
                                               torch.tensor(c.hyp, dtype=torch.float64),
                                               c.y0.copy(), c.U0.copy(), c.d0.copy(), variant=c.variant)
        want = O.backward_np64(c.A, c.graphs, c.hyp, c.y0, c.d0, Y64.numpy(), G64.numpy(), U64.numpy(), gY,
                               variant=c.variant)
        got = dh.sum(axis=1, keepdims=True) if c.H == 1 else dh
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())


# Measured, and asserted below: the usual inputs are blind to every defect at the fused / split
# shapes (P <= 5) and at 9 agents on a sparse graph, but with 8 and more agents their consensus
# term does cross 20 on a few lanes (tiled_v1: 3 of 16384 lanes at one iteration; general_m130:
# 6-7 of 8064; wide_v1, P = 80: 0.03-1.8 %), and at P = 8 their U reaches the shrinking bound in
# the last iterations of K = 25 (deep_stream). None of them reaches vclip on y, sign(0), or an
# adjoint mask other than the delta clamp's at P = 80.
SEEN_ON_USUAL = {"tiled_v1": {"no_dlim"}, "general_m130": {"no_dlim"},
                 "wide_v1": {"no_dlim", "no_dlim_mask"},
                 "deep_stream": {"vclip_k_for_vclip_prev", "no_U_clamp"}}


def _changed(clean, bad, defect):
    (Y, U, dh), (Yd, Ud, dhd) = clean, bad
    if defect in FORWARD_DEFECTS:
        return not (np.array_equal(Y, Yd) and np.array_equal(U, Ud))
    assert np.array_equal(Y, Yd)
    return not np.array_equal(dh, dhd)


@pytest.mark.parametrize("name", list(S.CASES))
def test_defect_table(name):
    """The gap this regime closes: each defect changes the result on the ladder inputs of every
    GPU case it applies to (a variant-0-only or GNN-only defect on that variant's cases), and on
    the suite's 1e-2 * randn inputs at the same shape not one of them changes a bit of the result,
    except the few SEEN_ON_USUAL lists (many agents)."""
    c = S.case(name)
    P, m, n, B = c.dims
    usual = (1e-2 * np.random.default_rng(99).standard_normal((3, B, P, n))).astype(np.float32)
    rng = np.random.default_rng(c.K)
    usual_hyp = O.hyp_table((0.5 * rng.standard_normal((c.K, c.H, 4))).astype(np.float32), S.MAXP)
    A, b, _ = O.make_problem(P, m, n, B, seed=P * 10 + n)
    gY = _gY((c.K, B, P, n))
    inputs = {"ladder": c.args, "usual": (A, b, c.graphs, usual_hyp, *usual)}
    clean = {k: _np_run(*v, gY, c.variant) for k, v in inputs.items()}
    for defect, variants in DEFECTS.items():
        if c.variant not in variants:
            continue
        seen = {k: _changed(clean[k], _np_run(*v, gY, c.variant, defect), defect) for k, v in inputs.items()}
        assert seen["ladder"], f"{defect} not seen on ladder inputs ({name})"
        assert seen["usual"] == (defect in SEEN_ON_USUAL.get(name, ())), \
            f"{defect} on the usual inputs ({name}): seen = {seen['usual']}"
