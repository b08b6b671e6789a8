"""Every D-ADMM kernel where its value, dual and delta clamps bind.

The rest of the GPU suite draws y0, U0, d0 = 1e-2 * randn: there only the gradient clamp is ever
active at the fused and split kernels' shapes (vclip on y and on U, the GNN variant's +-20 clamp
on delta and sign(+-0) on 0.0000 % of the lanes; with 8 and more agents delta crosses 20 on a few
lanes, tests/test_saturation_host.py::test_defect_table), so a kernel that took vclip_k for vclip_{k-1} in a deferred dual update, dropped the
delta clamp in one form, swapped a med3's bounds, gave sign(+-0) = +-tau, or an adjoint that left
out one of the [|w| <= vclip], [|z| <= vclip], [|2Ly| <= 20] masks, passed everything. Here the
inputs are tests/saturation.py's ladder; every test first asserts, on the CPU oracle's trajectory,
that each clamp has lanes below, inside and above its bound at every iteration
(saturation.assert_engaged: a precondition), and only then looks at the kernel.

Bars: forward paths bit for bit (np.array_equal on Y, U_K, status, and Grec / Urec where recorded)
against oracle.forward_f32[_rec] in the path's GEMM1 order; adjoints against oracle.backward_np64
in fp64 along the kernel's own recorded trajectory at test_gpu_adjoint's bound with
rtol = max(ADJ_RTOL, 4 x the case's fp32 rounding scale), the scale being the distance of
backward_np64(dtype=float32) from the fp64 result on that trajectory (numpy's pairwise float32
sums; the kernels sum per-workgroup partials and then reduce, hence the factor 4). The adjoint
cases also require that no lane of the oracle trajectory lies within fp32 rounding of a bound the
adjoints re-derive (saturation.near_bound_lanes), so a mask disagreement is a defect, not rounding.

Measured on the CPU oracle (per cent of the lanes, minimum-maximum over the iterations; g = the
pre-clamp gradient inside gclip, y / U = lanes ON the value bound per side, d = 2Ly beyond 20 per
side), and the fp32 rounding scale of the adjoint (max |f32 - f64| / max |f64|, gY as _gY draws
it; on the split trajectory in brackets). Every scale is below ADJ_RTOL / 4, so every adjoint
case is held to ADJ_RTOL itself:

  case            top   g inside    y per side   U per side    d per side    adjoint scale
  fused_v0        150   5.7-20.9    1.1-1.4      9.5-17.9      -             2.3e-7 (1.6e-7)
  fused_v1        80    7.7-10.6    0.2-1.5      1.9-3.6       20.6-21.7     4.9e-7 (4.8e-7 .. 7.7e-7)
  fused_v1_same   80    7.6-8.0     0.2-1.6      1.9-3.5       20.3-21.8     3.5e-7
  lanes_v0        150   10.7-28.1   1.3-1.5      8.8-18.9      -
  lanes_v1        250   7.7-10.9    1.5-7.8      6.3-10.8      26.1-26.4     2.8e-7
  tiled_v0        150   4.2-17.4    1.2-1.3      13.1-20.8     -
  tiled_v1        150   6.2-8.6     0.3-4.3      4.0-5.8       25.5-25.9
  wide_v1         80    3.4-8.1     0.3-1.7      2.1-3.0       27.1-30.0
  general_m130    400   3.9-8.7     0.6-7.7      5.4-9.9       21.0-22.0     0.9e-7 .. 1.5e-7
  general_same    80    8.8-10.7    0.2-1.2      1.5-3.7       19.5-21.1     1.1e-7 .. 2.0e-7
  deep_fused      150   5.8-21.4    1.2-2.4      9.8-19.4      -             (K = 25)
  deep_stream     150   4.3-18.2    1.2-2.2      12.7-20.7     -             (K = 25)
  module (K = 25) 150   8.5-24.5    2.3-4.2      9.5-24.1      -
(general_m130, m > n: y leaves its bound after one iteration unless the minimiser lies beyond it,
so the top rung's b is scaled by 100. Scale ranges: numpy builds differ in their float32 sums.)
The GNN step adjoint's scales (float32 torch restatement vs float64, per output, relative to the
output's largest entry): gy 6.5e-8 .. 9.3e-8, gU 4.5e-8 .. 1.0e-7, gd 7.9e-8 .. 1.2e-7,
gA 6.9e-8 .. 1.0e-7, ghyp 5.4e-8 .. 1.2e-7; the kernel came within 1.5e-7 on every output.
"""
import argparse

import numpy as np
import pytest
import torch

import oracle as O
import saturation as S

pytestmark = pytest.mark.gpu

ADJ_RTOL = 1e-5     # tests/test_gpu_adjoint.py
MODULE_SEED = 31


def _t(x, dev):
    return torch.from_numpy(np.array(x)).to(dev)      # a copy: the cases' arrays are read-only


def _eq(got, want, what):
    assert np.array_equal(got, want), (f"{what}: {np.sum(got != want)} of {got.size} differ, first at "
                                       f"{np.argwhere(got != want)[:3].tolist()}, max |diff| "
                                       f"{np.nanmax(np.abs(got - want))}")


class _Run:
    pass


def _forward(dev, c, path, record=False):
    """One forward of case ``c`` through ``path``; host copies of everything it returned."""
    from dadmm_hip import PreparedOperator, forward_raw, ingest
    P, m, n, B = c.dims
    r = _Run()
    r.op = PreparedOperator(_t(c.A, dev))
    r.g = ingest(c.graphs, P, B, dev)
    out = forward_raw(r.op, _t(c.b, dev), r.g, _t(c.hyp, dev), _t(c.y0, dev), _t(c.U0, dev),
                      _t(c.d0, dev), variant=c.variant, want_U=True, path=path, record=record)
    torch.cuda.synchronize()
    r.Y, r.U, r.st = out[0].cpu().numpy(), out[1].cpu().numpy(), int(out[2].item())
    if record:
        r.traj = out[3]
        r.Grec = r.traj.Grec[..., :n].cpu().numpy()
        r.Urec = r.traj.Urec[..., :n].cpu().numpy()
    return r


def _check_forward(r, c, record):
    assert r.st == c.st == 0
    _eq(r.Y, c.Y, "Y")
    _eq(r.U, c.U, "U_K")
    if record:
        _eq(r.Grec, c.Grec, "Grec")
        _eq(r.Urec, c.Urec, "Urec")


def _auto_split(dev, c):
    from dadmm_hip import PreparedOperator, ingest
    from dadmm_hip.ops import split_cols
    P, m, n, B = c.dims
    return split_cols(PreparedOperator(_t(c.A, dev)), B, c.K, ingest(c.graphs, P, B, dev), hyp_rows=c.H)


# ---- forward paths ------------------------------------------------------------------------------
# (the recording fused forward and per-sample graphs have the row-split form only)
FUSED = [(name, form, False) for name in ("fused_v0", "fused_v1", "fused_v1_same") for form in ("rows", "roles")]
FUSED += [("fused_v0", "rows", True), ("fused_v1", "rows", True), ("fused_v1_same", "rows", True),
          ("lanes_v1", "rows", False)]


@pytest.mark.parametrize("name,form,record", FUSED)
def test_fused_forms(cuda, monkeypatch, name, form, record):
    """dadmm_fused.hip / dadmm_fused_roles.hip (mclamp): shared graph, both variants, H = 1, plain
    and recording; and per-sample graphs (lanes_v1)."""
    c = S.case(name)
    c.engaged()
    monkeypatch.setenv("DADMM_FUSED_FORM", form)
    _check_forward(_forward(cuda, c, "fused", record), c, record)


@pytest.mark.parametrize("record", [False, True])
@pytest.mark.parametrize("name", ["fused_v0", "fused_v1"])
def test_split(cuda, name, record):
    """dadmm_split.hip, its deferred dual update included, in the split GEMM1 order."""
    sc = _auto_split(cuda, S.case(name))
    assert sc == 64
    c = S.case(name, split_cols=sc)
    c.engaged()
    _check_forward(_forward(cuda, c, "split", record), c, record)


@pytest.mark.parametrize("stream,record", [("1", False), ("1", True), ("0", False)])
@pytest.mark.parametrize("name", ["tiled_v0", "tiled_v1"])
def test_tiled_forms(cuda, monkeypatch, name, stream, record):
    """dadmm_stream.hip (DADMM_TILED_STREAM=1) and dadmm_tiled.hip's per-iteration launches (tclamp)."""
    c = S.case(name)
    c.engaged()
    monkeypatch.setenv("DADMM_TILED_STREAM", stream)
    _check_forward(_forward(cuda, c, "tiled", record), c, record)


def test_tiled_wide(cuda):
    """P = 80 agents, K = 3, a shared graph, GNN variant."""
    c = S.case("wide_v1")
    c.engaged()
    _check_forward(_forward(cuda, c, "tiled"), c, False)


@pytest.mark.parametrize("name", ["lanes_v0", "lanes_v1"])
def test_stepwise(cuda, name):
    """dadmm_stepwise.hip (clamp_t), recording."""
    c = S.case(name)
    c.engaged()
    _check_forward(_forward(cuda, c, "stepwise", True), c, True)


def test_auto_equals_the_forced_path(cuda):
    c0 = S.case("fused_v0")
    sc = _auto_split(cuda, c0)
    c = S.case("fused_v0", split_cols=sc)
    c.engaged()
    auto = _forward(cuda, c, "auto")
    forced = _forward(cuda, c, "split" if sc else "fused")
    _check_forward(auto, c, False)
    assert auto.st == forced.st
    _eq(auto.Y, forced.Y, "Y auto vs forced")
    _eq(auto.U, forced.U, "U_K auto vs forced")


# ---- the clip schedule over K = 25: U saturated at every k --------------------------------------
@pytest.mark.parametrize("path,form", [("fused", "rows"), ("fused", "roles"), ("split", "roles")])
def test_clip_schedule_fused_and_split(cuda, monkeypatch, path, form):
    """vclip_k = 200 - 3k moves every iteration: vclip_k for vclip_{k-1} in a deferred dual update
    is off by exactly 3 on every saturated lane of U, at every k."""
    sc = _auto_split(cuda, S.case("deep_fused")) if path == "split" else 0
    assert path != "split" or sc == 64
    c = S.case("deep_fused", split_cols=sc)
    c.engaged()
    monkeypatch.setenv("DADMM_FUSED_FORM", form)
    _check_forward(_forward(cuda, c, path), c, False)


def test_clip_schedule_stream(cuda, monkeypatch):
    c = S.case("deep_stream")
    c.engaged()
    monkeypatch.setenv("DADMM_TILED_STREAM", "1")
    _check_forward(_forward(cuda, c, "tiled"), c, False)


# ---- adjoints -----------------------------------------------------------------------------------
def _gY(K, B, P, n):
    rng = np.random.default_rng(7)
    gY = rng.standard_normal((K, B, P, n)).astype(np.float32)
    gY[: K // 2] *= 0.1
    return gY


def _adjoint_bar(c, Y, Grec, Urec, gY):
    """(want fp64, rtol): rtol = max(ADJ_RTOL, 4 x the fp32 rounding scale of this trajectory)."""
    args = (c.A, c.graphs, c.hyp, c.y0, c.d0, Y, Grec, Urec, gY)
    want = O.backward_np64(*args, variant=c.variant)
    w32 = O.backward_np64(*args, variant=c.variant, dtype=np.float32).astype(np.float64)
    scale = float(np.abs(w32 - want).max() / np.abs(want).max())
    print(f"{c.name} split={c.split_cols}: fp32 rounding scale of the adjoint {scale:.3e}")
    return want, max(ADJ_RTOL, 4.0 * scale)


ADJOINT_CASES = [("fused_v0", "fused"), ("fused_v1", "fused"), ("fused_v1_same", "fused"),
                 ("lanes_v1", "fused"), ("fused_v0", "split"), ("fused_v1", "split"),
                 ("general_m130", "auto"), ("general_same", "auto")]


@pytest.mark.parametrize("name,fpath", ADJOINT_CASES)
def test_adjoints(cuda, name, fpath):
    """dadmm_backward.hip (path "auto" on a fused / split trajectory) and dadmm_adjoint.hip (path
    "general", every trajectory) against the fp64 oracle adjoint along the kernel's own recording."""
    from dadmm_hip.ops import backward_raw
    from test_gpu_adjoint import _close
    sc = _auto_split(cuda, S.case(name)) if fpath == "split" else 0
    c = S.case(name, split_cols=sc)
    c.engaged(adjoint=True)
    r = _forward(cuda, c, fpath, record=True)
    _check_forward(r, c, True)
    P, m, n, B = c.dims
    gY = _gY(c.K, B, P, n)
    want, rtol = _adjoint_bar(c, r.Y, r.Grec, r.Urec, gY)
    assert (np.abs(want).max(axis=(0, 1)) > 0).all(), "inputs unsuitable: a hyper-parameter's gradient vanishes"
    paths = ("general",) if fpath == "auto" else ("auto", "general")
    for path in paths:
        assert path != "auto" or r.traj.fused
        dh = backward_raw(r.op, r.g, r.traj, _t(gY, cuda), path=path)
        torch.cuda.synchronize()
        _close(dh.cpu().numpy().astype(np.float64), want, rtol=rtol)


def _args(K, mode="diff"):
    return argparse.Namespace(GHN_iter_num=K, DADMM_mode=mode, alpha_max=0.1, tau_max=0.99,
                              rho_max=0.99, eta_max=0.99, max_penalty_threshold=0.8,
                              penalty_reduction_factor=0.95)


def test_module_backward_on_ladder_inits(cuda):
    """DLASSO_unfolded in train mode with its trained K = 25 table on ladder inits:
    seq_hyp.param.grad equals the oracle chain (as
    test_gpu_adjoint.test_module_backward_matches_oracle_chain builds it)."""
    import gnn_dlasso_utils
    import unfolded_DLASSO
    from test_gpu_adjoint import MAXP, TRAINED, _close
    P, m, n, B, K = 5, 64, 256, 16, 25
    A, b, x = O.make_problem(P, m, n, B, seed=21)
    model = unfolded_DLASSO.DLASSO_unfolded(_t(A, cuda)[None], _args(K)).to(cuda)
    with torch.no_grad():
        model.seq_hyp.param.copy_(torch.from_numpy(TRAINED))
    model.train()
    graphs = [O.er_graph(P, 0.5, seed=7)] * B
    y0, U0, d0 = S.ladder_inits(B, P, n, MODULE_SEED, 150.0)
    table_cpu = model.seq_hyp.table(K).detach().cpu().numpy()
    Yo, Uo, sto, Go, Uro = O.forward_f32_rec(A, b, graphs, table_cpu, y0, U0, d0)
    assert sto == 0
    S.assert_engaged(0, table_cpu, y0, Yo, Uo, Go, Uro, graphs, adjoint=True)
    Y, _ = model(_t(b, cuda)[..., None], graphs, inits=tuple(_t(v, cuda) for v in (y0, U0, d0)))
    label = _t(x, cuda)[..., None]
    _, loss_final = gnn_dlasso_utils.compute_loss(Y, label)
    loss_final.backward()
    got = model.seq_hyp.param.grad.cpu().numpy()
    _eq(Y[..., 0].detach().cpu().numpy(), Yo, "Y")
    gY = np.zeros((K, B, P, n))
    gY[-1] = 2.0 * (Yo[-1].astype(np.float64) - x[:, None, :]) / (B * n * P)
    dtab = O.backward_np64(A, graphs, table_cpu, y0, d0, Yo, Go, Uro, gY)
    p = torch.tensor(TRAINED, dtype=torch.float64, requires_grad=True)
    seq = unfolded_DLASSO.seq_hyperparam([K, P, 4], torch.tensor(MAXP, dtype=torch.float64), _args(K))
    seq.param = torch.nn.Parameter(p)
    seq.train()
    want, = torch.autograd.grad(seq.table(K), seq.param, grad_outputs=torch.from_numpy(dtab))
    _close(got.astype(np.float64), want.numpy(), rtol=1e-4)



# ---- the GNN model: its recurrence, and one step's adjoint in isolation --------------------------
def _gram_trajectory(A, b, graphs, table, y0, U0, d0, Yo):
    """(Grec, Urec) of the GNN recurrence for the precondition only: Urec[k] is U_k of the oracle
    run truncated to k rows, Grec[k] the pre-clamp gradient restated in fp64 from the oracle's
    iterates (gnn_dlasso_models_progressive.py:205-209)."""
    K, B, P = table.shape[0], y0.shape[0], y0.shape[1]
    A64 = A.astype(np.float64)
    AtA = np.einsum("pri,prj->pij", A64, A64)
    Atb = np.einsum("pri,bpr->bpi", A64, b.astype(np.float64))
    cnt = S.visit_counts(graphs, P)
    deg = np.array([[len(list(G.neighbors(p))) for p in range(P)] for G in graphs], np.float64)[:, :, None]
    U = [U0] + [O.forward_f32_gram(A, b, graphs, table[:k], y0, U0, d0, variant=1, hyp_mode=1)[1]
                for k in range(1, K)]
    G = []
    for k in range(K):
        yk = (y0 if k == 0 else Yo[k - 1]).astype(np.float64)
        dk = d0.astype(np.float64) if k == 0 else np.clip(S.delta64(cnt, yk)[0], -S.DLIM, S.DLIM)
        h = table[k].astype(np.float64)
        ta, rh = (np.broadcast_to(h[:, c, :], (B, P))[:, :, None] for c in (1, 2))
        G.append(np.einsum("pij,bpj->bpi", AtA, yk) - Atb + np.sign(yk) * ta + U[k] * deg + dk * rh)
    return np.stack(G), np.stack(U)


@pytest.mark.parametrize("mode,per_sample", [("diff", True), ("same", False)])
def test_gnn_model_recurrence(cuda, mode, per_sample):
    """DLASSO_GNNHyp3_Progressive (dadmm_gnn.hip's step) on ladder inits: Y bit-exact against
    oracle.forward_f32_gram given the recorded hypernetwork outputs; the precondition is evaluated
    on that oracle output. Measured on the CPU path's hypernetwork: g inside 8-24 %, y on its bound
    0.8-7.1 % per side, U 4.7-9.2 %, delta beyond 20 25-27 % per side."""
    from test_gpu_gnn import _hyp_table, _recording, _setup
    P, m, n, B, K = 5, 32, 64, 24, 6
    model, A, b, x, graphs, _ = _setup(cuda, P, m, n, B, K, mode, per_sample)
    inits = S.ladder_inits(B, P, n, 1, 250.0)
    model.eval()
    rec = _recording(model)
    with torch.no_grad():
        Y, _ = model(_t(b, cuda)[..., None], graphs, inits=tuple(_t(v, cuda) for v in inits))
    st = int(model.last_status.item())
    H = 1 if mode == "same" else P
    table = _hyp_table(rec, B, H)
    Yo, Uo, sto = O.forward_f32_gram(A, b, graphs, table, *inits, variant=1, hyp_mode=1)
    assert sto == 0
    Gq, Uq = _gram_trajectory(A, b, graphs, table, *inits, Yo)
    S.assert_engaged(1, table, inits[0], Yo, Uo, Gq, Uq, graphs, hyp_mode=1)
    assert st == 0
    _eq(Y[..., 0].cpu().numpy(), Yo, "Y")


def _step_ref(graphs, deg, y, U, D, AtAy, Atb, hyp, gy1, gU1, gd1, dtype):
    """The literal step ops (gnn_dlasso_models_progressive.py:205-237, as
    oracle/ref_torch.gnn_forward_autograd restates them) under torch autograd in ``dtype``, on the
    given inputs. Returns the gradients (gy, gU, gd, gA, ghyp [B,4,H]) and the step's
    intermediates (pre-clamp gradient, z, 2Ly, w) for the precondition."""
    from oracle import ref_torch
    B, P, n = y.shape
    leaf = lambda v: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True)   # noqa: E731
    const = lambda v: torch.tensor(np.asarray(v), dtype=dtype)                      # noqa: E731
    y, U, D, AtAy, hyp = (leaf(v) for v in (y, U, D, AtAy, hyp))
    al, ta, rh, et = (hyp[:, c, :].expand(B, P)[:, :, None] for c in range(4))
    gr = AtAy - const(Atb) + y.sign() * ta + U * const(deg)[:, :, None] + D * rh
    g = torch.clamp(gr, -10.0, 10.0)
    z = y - al * g
    yn = torch.clamp(z, -100.0, 100.0)
    d_raw = ref_torch._delta_autograd(graphs, yn, P)
    d = torch.clamp(d_raw, -20.0, 20.0)
    w = U + d * et
    U1 = torch.clamp(w, -100.0, 100.0)
    loss = (yn * const(gy1)).sum() + (U1 * const(gU1)).sum() + (d * const(gd1)).sum()
    grads = torch.autograd.grad(loss, (y, U, D, AtAy, hyp))
    return ([v.numpy() for v in grads],
            {k: v.detach().numpy() for k, v in (("g", gr), ("z", z), ("d", d_raw), ("w", w), ("y1", yn))})


def _step_inputs(B, P, n, H, seed, top=250.0):
    """Ladder-scaled y_k, U, D, AtAy; hyp_k in the head's ranges (clamp(sigmoid, 1e-4, 0.9999) x
    (0.1, 0.99, 0.99, 0.99)); random output gradients."""
    rng = np.random.default_rng(seed)
    y, U, D = S.ladder_inits(B, P, n, seed, top)
    sc = S.ladder_scales(top)[np.arange(B) % 5][:, None, None]
    AtAy = (sc * rng.standard_normal((B, P, n))).astype(np.float32)
    mx = np.array([0.1, 0.99, 0.99, 0.99])[None, :, None]
    hyp = (np.clip(rng.random((B, 4, H)), 1e-4, 0.9999) * mx).astype(np.float32)
    gy1, gU1, gd1 = rng.standard_normal((3, B, P, n)).astype(np.float32)
    return y, U, D, AtAy, hyp, gy1, gU1, gd1


def _step_precondition(graphs, P, mid, y, U):
    """Every clamp of the step has at least 32 lanes below, inside and above its bound, at least
    64 lanes of y are exactly zero, and no lane lies within fp32 rounding of a bound: the gradient
    (6 roundings of its terms' sum), z = y - alpha g and w = U + delta eta (4 ulp of 100), 2Ly
    ((visits + 2) 2^-23 x the sum of |y_p| + |y_q| over its terms, y_{k+1} itself being rounded)."""
    cnt = S.visit_counts(graphs, P)
    for name, bound in (("g", 10.0), ("z", 100.0), ("d", S.DLIM), ("w", 100.0)):
        v = mid[name]
        cls = (int((v < -bound).sum()), int((np.abs(v) <= bound).sum()), int((v > bound).sum()))
        assert min(cls) >= S.MIN_LANES, f"inputs unsuitable: step clamp '{name}' (below, inside, above) = {cls}"
    assert int((y == 0).sum()) >= S.MIN_ZEROS, "inputs unsuitable: too few exactly-zero lanes of y"
    ulp100 = 4.0 * np.spacing(np.float32(100.0))
    a1 = np.abs(mid["y1"])
    mag = cnt.sum(-1)[:, :, None] * a1 + np.einsum("bpq,bqi->bpi", cnt, a1)
    near = {"g": np.abs(np.abs(mid["g"]) - 10.0) <= 6.0 * 2.0 ** -23 * (np.abs(mid["g"]) + 4.0 * 250.0),
            "z": np.abs(np.abs(mid["z"]) - 100.0) <= ulp100,
            "w": np.abs(np.abs(mid["w"]) - 100.0) <= ulp100,
            "d": np.abs(np.abs(mid["d"]) - S.DLIM) <= (cnt.sum(-1)[:, :, None] + 2.0) * 2.0 ** -23 * mag}
    bad = {k: int(v.sum()) for k, v in near.items()}
    assert not any(bad.values()), f"inputs unsuitable: lanes within fp32 rounding of a bound: {bad}"


STEP_SEED = 1


# (P = 9: the loop form of the step adjoint, past the 8 agents its register form holds)
@pytest.mark.parametrize("P,n,H", [(4, 32, 4), (4, 32, 1), (4, 36, 4), (9, 32, 9)])
def test_gnn_step_adjoint(cuda, P, n, H):
    """dadmm_gnn_step then dadmm_gnn_step_backward on ladder-scaled inputs, one step in isolation
    (no trajectory drift), against fp64 torch autograd of the literal step ops on the same fp32
    inputs. Bound per output: max(2^-23, 4 x the float32-vs-float64 distance of the torch
    restatement itself) relative to the output's largest entry (2^-23: the results are float32)."""
    from dadmm_hip import _lib
    from dadmm_hip.gnn_ops import GnnRun
    from dadmm_hip.graph import ingest
    from test_gpu_gnn import _setup
    m, B = 16, 8
    model, A, b, x, graphs, _ = _setup(cuda, P, m, n, B, 1, "diff" if H == P else "same", True)
    y, U, D, AtAy, hyp, gy1, gU1, gd1 = _step_inputs(B, P, n, H, STEP_SEED)
    run = GnnRun(model.operator(), _t(b, cuda), ingest(graphs, P, B, cuda), 1, H, _lib.VARIANT_GNN,
                 _t(y, cuda), _t(U, cuda), _t(D, cuda), False)
    ns = run.op.n_store
    pad = lambda v: torch.nn.functional.pad(_t(v, cuda), (0, ns - n)).contiguous()   # noqa: E731
    Atb = run.Atb[..., :n].cpu().numpy()
    deg = np.array([[len(list(G.neighbors(p))) for p in range(P)] for G in graphs], np.float32)
    ref = (graphs, deg, y, U, D, AtAy, Atb, hyp, gy1, gU1, gd1)
    want, mid = _step_ref(*ref, torch.float64)
    _step_precondition(graphs, P, mid, y, U)
    w32, _ = _step_ref(*ref, torch.float32)

    hk, Ud, Dd, Ad = _t(hyp, cuda), pad(U), pad(D), pad(AtAy)
    y1, U1, D1 = run.step(0, Ad, hk, Ud, Dd)
    got = run.step_backward(0, run.y0, Ad, hk, Ud, Dd, pad(gy1), pad(gU1), pad(gd1))
    st = int(run.finish().item())
    torch.cuda.synchronize()
    assert st == 0
    # the step itself, against the fp32 torch ops: clamps are exact, the sums differ by rounding
    on_bound = lambda v: (np.abs(v) == 100.0).astype(np.float32)   # noqa: E731
    _eq(on_bound(y1[..., :n].cpu().numpy()), on_bound(mid["y1"]), "y_{k+1} on its bound")
    np.testing.assert_allclose(y1[..., :n].cpu().numpy(), mid["y1"], rtol=0, atol=1e-4)
    for name, g, w, w3 in zip(("gy", "gU", "gd", "gA", "ghyp"), got, want, w32):
        g = g.cpu().numpy().astype(np.float64)
        g = g[..., :n] if name != "ghyp" else g
        top = np.abs(w).max()
        scale = float(np.abs(w3.astype(np.float64) - w).max() / top)
        rtol = max(2.0 ** -23, 4.0 * scale)
        err = np.abs(g - w)
        print(f"step adjoint P={P} n={n} H={H} {name}: fp32 scale {scale:.3e}, kernel max err / max {err.max() / top:.3e}")
        assert top > 0
        assert (err <= rtol * top + rtol * np.abs(w)).all(), (name, float(err.max() / top), rtol)
