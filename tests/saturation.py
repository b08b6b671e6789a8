"""Inputs that drive the D-ADMM recurrence into every one of its clamps, and the precondition that
proves they do (a helper module of tests/test_gpu_saturation.py and tests/test_saturation_host.py).

The suite's usual draws (y0, U0, d0 = 1e-2 * randn, b = A x) only ever reach the gradient clamp:
|y| stays below 10 and |U| near 100 against value bounds of 200 (unfolded variant) / 100 (GNN
variant), and the GNN variant's +-20 clamp on delta never binds. ``ladder_inits`` draws the samples
of one batch at five scales, from the usual 1e-2 up to ``top`` (about the value bound), so that in
the same launch some lanes sit below, some inside and some above every bound, and plants exact
+0.0 / -0.0 lanes for sign(0). (Uniformly large inputs saturate the gradient clamp on every lane
and the adjoint's tau / rho / Gram terms vanish; hence the ladder.)

``assert_engaged`` is a PRECONDITION on the oracle's trajectory, not a measurement: a test calls
it before it looks at the kernel's output, and it fails with "inputs unsuitable" when a clamp is
not exercised on both sides and inside at some iteration.
"""
import numpy as np

import oracle as O

MAXP = [0.1, 0.99, 0.99, 0.99]
DLIM = 20.0                      # the GNN variant's clamp on delta (gnn_dlasso_models_progressive.py:229)
MIN_SHARE, MIN_LANES, MIN_ZEROS = 1e-3, 32, 64


def clips(variant, k):
    """(gclip_k, vclip_k): unfolded_DLASSO.py:80, :92; gnn_dlasso_models_progressive.py:212, :224."""
    if variant == 0:
        return max(1.0, 30.0 - k), max(10.0, 200.0 - 3 * k)
    return 10.0, 100.0


def ladder_scales(top):
    return np.array([1e-2, 1.0, 0.1 * top, 0.4 * top, top])


def ladder_inits(B, P, n, seed, top):
    """y0, U0, d0 [B,P,n] float32: sample s is scale[s % 5] * randn, d0 at 0.2 of that scale; one
    eighth of the y0 lanes is exactly +0.0 and another eighth exactly -0.0."""
    rng = np.random.default_rng(seed)
    sc = ladder_scales(top)[np.arange(B) % 5][None, :, None, None]
    y0, U0, d0 = (sc * rng.standard_normal((3, B, P, n))).astype(np.float32)
    d0 = (np.float32(0.2) * d0).astype(np.float32)
    pick = rng.random((B, P, n))
    y0[pick < 0.125] = np.float32(0.0)
    y0[(pick >= 0.125) & (pick < 0.25)] = np.float32(-0.0)
    return y0, U0, d0


def ladder_hyp(K, H, seed):
    """The table as the suite builds it (O.hyp_table(0.5 * randn)), with +1.5 on row 0's alpha and
    eta: the rows are cumulative sums, so both sit near their maxima at every iteration."""
    rng = np.random.default_rng(seed)
    param = (0.5 * rng.standard_normal((K, H, 4))).astype(np.float32)
    param[0, :, 0] += np.float32(1.5)
    param[0, :, 3] += np.float32(1.5)
    return O.hyp_table(param, MAXP)


def visit_counts(graphs, P):
    """cnt [B,P,P]: how many terms +-(y_p - y_q) compute_delta (unfolded_DLASSO.py:127-140) adds
    into delta[p] for the pair (p, q); 2 L = diag(cnt.sum(-1)) - cnt (oracle.laplacians)."""
    cache, out = {}, np.zeros((len(graphs), P, P))
    for s, G in enumerate(graphs):
        if id(G) not in cache:
            c = np.zeros((P, P))
            for p in range(P):
                for q in G.neighbors(p):
                    if q != p:
                        c[p, q] += 1.0
                        c[q, p] += 1.0
            cache[id(G)] = c
        out[s] = cache[id(G)]
    return out


def delta64(cnt, y):
    """compute_delta(y) = 2 L y in float64, and the sum of its terms' magnitudes."""
    y = np.asarray(y, np.float64)
    d = cnt.sum(-1)[:, :, None] * y - np.einsum("bpq,bqi->bpi", cnt, y)
    mag = np.einsum("bpq,bpqi->bpi", cnt, np.abs(y[:, :, None, :] - y[:, None, :, :]))
    return d, mag


def _eta(hyp, k, hyp_mode, P):
    """eta of iteration k broadcast to [B or 1, P, 1] (table [K,H,4] or per-sample [K,B,4,H])."""
    if hyp_mode == 0:
        return np.broadcast_to(hyp[k][:, 3].astype(np.float64), (P,))[None, :, None]
    e = hyp[k][:, 3, :].astype(np.float64)
    return np.broadcast_to(e, (e.shape[0], P))[:, :, None]


def shares(x, bound):
    """(below, strictly inside, above) lane counts of x against +-bound; a clamped value that sits
    on its bound counts as below / above."""
    x = np.asarray(x)
    lo, hi = int((x <= -bound).sum()), int((x >= bound).sum())
    return lo, x.size - lo - hi, hi


def activity(variant, y0, Y, U_K, Grec, Urec, graphs):
    """Per iteration, the (below, inside, above) lane counts of Grec[k] against gclip_k (strict:
    a pre-clamp value), Y[k] and U_{k+1} against vclip_k and, in the GNN variant, 2 L Y[k] against
    20 (strict); plus the number of exactly-zero lanes of y0 and the lane count."""
    K, B, P, n = Y.shape
    cnt = visit_counts(graphs, P)
    rows = []
    for k in range(K):
        gclip, vclip = clips(variant, k)
        g = np.asarray(Grec[k])
        r = {"g": (int((g < -gclip).sum()), int((np.abs(g) <= gclip).sum()), int((g > gclip).sum())),
             "y": shares(Y[k], vclip),
             "U": shares(Urec[k + 1] if k + 1 < K else U_K, vclip)}
        if variant != 0:
            d, _ = delta64(cnt, Y[k])
            r["d"] = (int((d < -DLIM).sum()), int((np.abs(d) <= DLIM).sum()), int((d > DLIM).sum()))
        rows.append(r)
    return rows, int((np.asarray(y0) == 0).sum()), B * P * n


def near_bound_lanes(variant, hyp, Y, Urec, graphs, hyp_mode=0):
    """Lanes of the trajectory whose adjoint mask fp32 rounding may flip: the adjoints recompute
    w = U_k + delta eta and delta = 2 L y. |w| within 4 ulp of vclip; |2 L y| within
    (visits of the agent + 2) 2^-23 sum|terms| of 20. Returns per-iteration (w, delta) counts.
    A lane whose delta terms are all exactly zero (every neighbour bit-equal: zero lanes of y0 that
    moved by the same alpha * gclip, or neighbours on the same bound) is exempt: its differences
    are exact in any precision, delta = 0 and w = U_k bit for bit, so no rounding can flip it; such
    lanes with U_k ON its bound are kept on purpose (the mask there is <=, not <)."""
    K, B, P, n = Y.shape
    cnt = visit_counts(graphs, P)
    visits = cnt.sum(-1)[:, :, None]
    out = []
    for k in range(K):
        _, vclip = clips(variant, k)
        d, mag = delta64(cnt, Y[k])
        nd = 0
        if variant != 0:
            nd = int((np.abs(np.abs(d) - DLIM) <= (visits + 2.0) * 2.0 ** -23 * mag).sum())
            d = np.clip(d, -DLIM, DLIM)
        w = np.asarray(Urec[k], np.float64) + d * _eta(hyp, k, hyp_mode, P)
        nw = int(((np.abs(np.abs(w) - vclip) <= 4.0 * np.spacing(np.float32(vclip))) & (mag > 0)).sum())
        out.append((nw, nd))
    return out


def assert_engaged(variant, hyp, y0, Y, U_K, Grec, Urec, graphs, adjoint=False, hyp_mode=0):
    """Every clamp has at least 0.1 % of the lanes and at least 32 lanes below, strictly inside and
    above its bound at EVERY iteration, and y0 has at least 64 exactly-zero lanes; with
    ``adjoint``, no lane lies within fp32 rounding of a bound the adjoints re-derive."""
    assert np.isfinite(Y).all() and np.isfinite(U_K).all(), "inputs unsuitable: non-finite trajectory"
    rows, zeros, lanes = activity(variant, y0, Y, U_K, Grec, Urec, graphs)
    need = max(MIN_LANES, int(np.ceil(MIN_SHARE * lanes)))
    assert zeros >= MIN_ZEROS, f"inputs unsuitable: {zeros} exactly-zero lanes of y0 (< {MIN_ZEROS})"
    for k, r in enumerate(rows):
        for name, cls in r.items():
            assert min(cls) >= need, (f"inputs unsuitable: clamp '{name}' at k = {k} has (below, inside, "
                                      f"above) = {cls} of {lanes} lanes; each needs {need}")
    if adjoint:
        for k, (nw, nd) in enumerate(near_bound_lanes(variant, hyp, Y, Urec, graphs, hyp_mode)):
            assert nw == 0 and nd == 0, (f"inputs unsuitable: at k = {k}, {nw} lanes of U + delta eta "
                                         f"and {nd} of 2 L y lie within fp32 rounding of their bound")


def report(variant, y0, Y, U_K, Grec, Urec, graphs):
    """The activity as percentages (minimum .. maximum over the iterations), for docstrings."""
    rows, zeros, lanes = activity(variant, y0, Y, U_K, Grec, Urec, graphs)
    out = []
    for name in rows[0]:
        a = np.array([r[name] for r in rows], np.float64) * 100.0 / lanes
        out.append(f"{name} below {a[:, 0].min():.1f}-{a[:, 0].max():.1f} inside "
                   f"{a[:, 1].min():.1f}-{a[:, 1].max():.1f} above {a[:, 2].min():.1f}-{a[:, 2].max():.1f}")
    return "; ".join(out) + f"; y0 zeros {zeros}"


# ---- the cases both test modules share ----------------------------------------------------------
#        name        P   m    n    B   K  variant H  per-sample prob  seed  top  [b scale of the top rung]
CASES = {
    "fused_v0":     (5,  64,  256, 16, 4,  0,     5,  False,    0.5,  1,    150.0),
    "fused_v1":     (5,  64,  256, 16, 4,  1,     5,  False,    0.5,  2,    80.0),
    "fused_v1_same": (5, 64,  256, 16, 4,  1,     1,  False,    0.5,  3,    80.0),
    "lanes_v0":     (3,  16,  64,  20, 4,  0,     3,  True,     0.9,  4,    150.0),
    "lanes_v1":     (3,  16,  64,  20, 4,  1,     3,  True,     0.9,  15,   250.0),
    "tiled_v0":     (8,  64,  128, 16, 4,  0,     8,  True,     0.6,  6,    150.0),
    "tiled_v1":     (8,  64,  128, 16, 4,  1,     8,  True,     0.6,  5,    150.0),
    "wide_v1":      (80, 24,  128, 5,  3,  1,     80, False,    0.1,  8,    80.0),
    "general_m130": (12, 130, 96,  7,  4,  1,     12, True,     0.6,  9,    400.0, 100.0),
    "general_same": (9,  40,  320, 14, 4,  1,     1,  False,    0.4,  10,   80.0),
    "deep_fused":   (5,  64,  256, 16, 25, 0,     5,  False,    0.5,  11,   150.0),
    "deep_stream":  (8,  64,  128, 16, 25, 0,     8,  True,     0.6,  12,   150.0),
}
_CACHE = {}


class Case:
    """One case's inputs and its oracle trajectory (computed once, shared, read-only)."""

    def __init__(self, name, split_cols=0):
        P, m, n, B, K, variant, H, per_sample, prob, seed, top, *bx = CASES[name]
        self.name, self.dims, self.K, self.variant, self.H = name, (P, m, n, B), K, variant, H
        self.A, self.b, self.x = O.make_problem(P, m, n, B, seed=P * 10 + n)
        if bx:      # the top rung's b = A x* scaled: its minimiser then lies beyond the value bound
            self.b[4::5] *= np.float32(bx[0])
            self.x[4::5] *= np.float32(bx[0])
        if per_sample:
            self.graphs = [O.connected_er_graph(P, prob, seed=1000 + s) for s in range(B)]
        else:
            self.graphs = [O.er_graph(P, prob, seed=3)] * B
        self.y0, self.U0, self.d0 = ladder_inits(B, P, n, seed, top)
        self.hyp = ladder_hyp(K, H, seed)
        self.split_cols = split_cols
        self.Y, self.U, self.st, self.Grec, self.Urec = O.forward_f32_rec(
            self.A, self.b, self.graphs, self.hyp, self.y0, self.U0, self.d0, variant=variant,
            split_cols=split_cols)
        for v in (self.A, self.b, self.y0, self.U0, self.d0, self.hyp, self.Y, self.U, self.Grec, self.Urec):
            v.setflags(write=False)

    @property
    def args(self):
        return self.A, self.b, self.graphs, self.hyp, self.y0, self.U0, self.d0

    def engaged(self, adjoint=False):
        assert self.st == 0, f"inputs unsuitable: the oracle's guards fired (status {self.st})"
        assert_engaged(self.variant, self.hyp, self.y0, self.Y, self.U, self.Grec, self.Urec,
                       self.graphs, adjoint=adjoint)

    def report(self):
        return report(self.variant, self.y0, self.Y, self.U, self.Grec, self.Urec, self.graphs)


def case(name, split_cols=0):
    key = (name, split_cols)
    if key not in _CACHE:
        _CACHE[key] = Case(name, split_cols)
    return _CACHE[key]
