"""CPU: the oracle against known-answer tests derived from the reference source (SURVEY.md §8c
items 1-10), the committed golden vectors, and the reference's shipped data fixtures.

The reference's own repository has no tests or vectors for this path and could not be run here,
so these KATs are what pins the restatement (oracle/dadmm_oracle.c header: "parity unpinned" by
reference outputs).
"""
import glob
import os

import networkx as nx
import numpy as np
import pytest

import oracle as O
from oracle import ref_torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
TRAINED = np.load(os.path.join(GOLD, "fixture_25_iter_general_learning_seq_hyp_param.npy"))
MAXP = [0.1, 0.99, 0.99, 0.99]


def _inits(B, P, n, seed=0, scale=1e-2):
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal((3, B, P, n))).astype(np.float32)


def _lap(G, P):
    Adj = nx.to_numpy_array(G, nodelist=range(P))
    return np.diag(Adj.sum(1)) - Adj


# ---- KAT 3, 4: the hyper-parameter table (unfolded_DLASSO.py:156-168) ----------------------
def test_kat_hyp_table_zero_param():
    h = O.hyp_table(np.zeros((25, 5, 4), np.float32), MAXP)
    np.testing.assert_allclose(h[..., 0], 0.05, rtol=1e-6)
    np.testing.assert_allclose(h[..., 1:], 0.495, rtol=1e-6)


def test_kat_penalty_never_fires_at_default_maxima():
    big = np.full((10, 5, 4), 50.0, np.float32)    # sigmoid -> 1
    ev = O.hyp_table(big, MAXP, training=False)
    tr = O.hyp_table(big, MAXP, training=True)
    assert np.array_equal(ev, tr)                    # mean <= (0.1 + 3*0.99)/4 = 0.7675 < 0.8


def test_kat_penalty_fires_when_all_maxima_099():
    big = np.full((4, 5, 4), 50.0, np.float32)
    tr = O.hyp_table(big, [0.99] * 4, training=True)
    np.testing.assert_allclose(tr, 0.99 * 0.95, rtol=1e-6)   # 0.9405, below the 0.99 clamp
    ev = O.hyp_table(big, [0.99] * 4, training=False)
    np.testing.assert_allclose(ev, 0.99, rtol=1e-7)


# ---- KAT 1, 2: consensus and degrees ---------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_kat_delta_is_twice_laplacian(seed):
    """With U0 = 0, eta = 1/2 and no clamp active, U_1 = delta_1 / 2 and delta_1 = 2 L y_1."""
    P, m, n, B = 6, 8, 16, 3
    G = nx.erdos_renyi_graph(P, 0.5, seed=seed)
    A, b, _ = O.make_problem(P, m, n, B, seed=seed)
    y0, _, d0 = _inits(B, P, n, seed)
    U0 = np.zeros_like(y0)
    hyp = np.tile(np.array([0.01, 0.1, 0.1, 0.5], np.float32), (1, P, 1))
    Y, U, st = O.forward_f64(A, b, [G] * B, hyp, y0, U0, d0)
    L = _lap(G, P)
    np.testing.assert_allclose(2 * U, 2 * np.einsum("pq,bqi->bpi", L, Y[0]), rtol=1e-12, atol=1e-14)


def test_kat_degrees_are_row_sums():
    P = 7
    G = nx.erdos_renyi_graph(P, 0.4, seed=3)
    _, _, deg = O.graph_arrays([G, G], P)
    np.testing.assert_array_equal(deg[0], nx.to_numpy_array(G, nodelist=range(P)).sum(1))


# ---- KAT 5: one iteration in closed form, clamp bounds ---------------------------------------
def test_kat_one_iteration_closed_form():
    P, m, n, B = 4, 8, 12, 2
    A, b, _ = O.make_problem(P, m, n, B, seed=4)
    G = nx.erdos_renyi_graph(P, 0.6, seed=2)
    y0, U0, d0 = _inits(B, P, n, 1, scale=0.5)
    hyp = np.array([[[0.03, 0.4, 0.3, 0.2]] * P], np.float32)
    Y, U, _ = O.forward_f64(A, b, [G] * B, hyp, y0, U0, d0)
    A64 = A.astype(np.float64)
    AtA = np.einsum("pri,prj->pij", A64, A64)
    Atb = np.einsum("pri,bpr->bpi", A64, b.astype(np.float64))
    deg = nx.to_numpy_array(G, nodelist=range(P)).sum(1)[None, :, None]
    g = np.einsum("pij,bpj->bpi", AtA, y0) - Atb + np.sign(y0) * 0.4 + U0 * deg + d0 * 0.3
    g = np.clip(g, -30, 30)
    y1 = np.clip(y0 - np.float64(np.float32(0.03)) * g, -200, 200)
    np.testing.assert_allclose(Y[0], y1, rtol=1e-6, atol=1e-6)
    d1 = 2 * np.einsum("pq,bqi->bpi", _lap(G, P), y1)
    np.testing.assert_allclose(U, np.clip(U0 + d1 * np.float64(np.float32(0.2)), -200, 200),
                               rtol=1e-6, atol=1e-6)


def test_kat_value_clip_schedule():
    """y far above every bound: Y[k] == max(10, 200 - 3k) exactly (unfolded_DLASSO.py:92)."""
    P, m, n, B, K = 2, 4, 4, 1, 70
    A = np.zeros((P, m, n), np.float32)
    b = np.zeros((B, P, m), np.float32)
    G = nx.empty_graph(P)
    y0 = np.full((B, P, n), 1e6, np.float32)
    z = np.zeros_like(y0)
    hyp = np.tile(np.array([1e-4, 1e-4, 1e-4, 1e-4], np.float32), (K, P, 1))
    Y, _, _ = O.forward_f32(A, b, [G] * B, hyp, y0, z, z)
    want = np.array([max(10.0, 200.0 - 3 * k) for k in range(K)], np.float32)
    np.testing.assert_array_equal(Y[:, 0, 0, 0], want)


def test_kat_grad_clip_schedule():
    """A saturated gradient moves y by exactly alpha * max(1, 30 - k) (unfolded_DLASSO.py:80)."""
    P, m, n, B, K = 1, 4, 4, 1, 35
    A = np.zeros((P, m, n), np.float32)
    b = np.zeros((B, P, m), np.float32)
    G = nx.empty_graph(P)
    y0 = np.zeros((B, P, n), np.float32)
    z = np.zeros_like(y0)
    d0 = np.full_like(y0, 1e6)                                  # delta_0 * rho >> any clip
    alpha = 0.5
    hyp = np.tile(np.array([alpha, 0.0, 1.0, 0.0], np.float32), (K, P, 1))
    Y, _, _ = O.forward_f64(A, b, [G] * B, hyp, y0, z, d0)
    assert Y[0, 0, 0, 0] == -alpha * 30.0                       # k = 0: clip 30
    # afterwards delta = 0 (single agent) and sign(y) * tau = 0: y stays
    assert np.all(Y[1:, 0, 0, 0] == Y[0, 0, 0, 0])
    # with tau >> clip, sign(y) = -1 drives y up by exactly alpha * max(1, 30 - k) per step
    # (K = 30 keeps y negative and inside the value clip through k = 29, where the clip hits 1)
    K2, alpha2 = 30, 0.125
    hyp2 = np.tile(np.array([alpha2, 100.0, 0.0, 0.0], np.float32), (K2, P, 1))
    Y2, _, _ = O.forward_f64(A, b, [G] * B, hyp2, np.full_like(y0, -150.0), z, z)
    steps = np.diff(np.concatenate([[-150.0], Y2[:, 0, 0, 0]]))
    want = np.array([alpha2 * max(1.0, 30.0 - k) for k in range(K2)])
    np.testing.assert_array_equal(steps, want)


# ---- KAT 6, 7: edgeless graph, K prefix --------------------------------------------------------
def test_kat_edgeless_agents_are_independent():
    P, m, n, B, K = 3, 8, 16, 2, 6
    A, b, _ = O.make_problem(P, m, n, B, seed=8)
    y0, U0, d0 = _inits(B, P, n, 3)
    hyp = O.hyp_table(np.random.default_rng(0).standard_normal((K, P, 4)).astype(np.float32), MAXP)
    Y, _, _ = O.forward_f32(A, b, [nx.empty_graph(P)] * B, hyp, y0, U0, d0)
    for p in range(P):
        Yp, _, _ = O.forward_f32(A[p:p + 1], b[:, p:p + 1], [nx.empty_graph(1)] * B,
                                 hyp[:, p:p + 1], y0[:, p:p + 1], U0[:, p:p + 1], d0[:, p:p + 1])
        np.testing.assert_array_equal(Y[:, :, p], Yp[:, :, 0])


def test_kat_k_prefix():
    P, m, n, B, K = 5, 16, 32, 3, 12
    A, b, _ = O.make_problem(P, m, n, B, seed=2)
    G = nx.erdos_renyi_graph(P, 0.5, seed=1)
    y0, U0, d0 = _inits(B, P, n, 5)
    hyp = O.hyp_table(TRAINED[:K], MAXP)
    Y, _, _ = O.forward_f32(A, b, [G] * B, hyp, y0, U0, d0)
    Y7, _, _ = O.forward_f32(A, b, [G] * B, hyp[:7], y0, U0, d0)
    np.testing.assert_array_equal(Y[:7], Y7)


# ---- KAT 8: compute_loss ----------------------------------------------------------------------
def test_kat_compute_loss_constant():
    K, B, P, n = 4, 3, 2, 5
    Y = np.full((K, B, P, n), 2.0)
    label = np.full((B, n), 0.5)
    mean, final = O.compute_loss(Y, label)
    assert mean == pytest.approx(2.25 + 1e-8) and final == pytest.approx(2.25 + 1e-8)
    Y[1, 0, 0, 0] = np.nan
    assert O.compute_loss(Y, label) == (1.0, 1.0)


# ---- KAT 9: Gram vs factored in fp64 -----------------------------------------------------------
def test_kat_gram_equals_factored_fp64():
    P, m, n, B = 5, 32, 64, 4
    A, b, _ = O.make_problem(P, m, n, B, seed=6)
    y = np.random.default_rng(1).standard_normal((B, P, n))
    A64 = A.astype(np.float64)
    gram = np.einsum("pij,bpj->bpi", np.einsum("pri,prj->pij", A64, A64), y) - \
        np.einsum("pri,bpr->bpi", A64, b.astype(np.float64))
    fact = np.einsum("pri,bpr->bpi", A64, np.einsum("prj,bpj->bpr", A64, y) - b)
    np.testing.assert_allclose(gram, fact, rtol=0, atol=1e-12 * np.abs(gram).max())


# ---- the two fp64 restatements agree; fp32 noise band -----------------------------------------
def test_two_fp64_restatements_agree():
    P, m, n, B, K = 5, 32, 64, 6, 25
    A, b, _ = O.make_problem(P, m, n, B, seed=10)
    graphs = [O.connected_er_graph(P, 0.5, seed=s) for s in range(B)]
    y0, U0, d0 = _inits(B, P, n, 2)
    hyp = O.hyp_table(TRAINED, MAXP)
    Yc, Uc, _ = O.forward_f64(A, b, graphs, hyp, y0, U0, d0)
    Yn, Un = O.forward_np64(A, b, graphs, hyp, y0, U0, d0)
    np.testing.assert_allclose(Yc, Yn, rtol=0, atol=1e-8)


def test_fp32_noise_band():
    """KAT 10: fp32 vs fp64 at the headline shape with the trained fixture. Both fp32 forms —
    the kernel-order restatement and the literal torch replay of the reference's own ops — drift
    from fp64 by the same order (mean final-iterate MSE ~1e-6 over problems, single problems up
    to ~1e-5): this sets the tolerance used by the GPU tests."""
    P, m, n, B, K = 5, 64, 256, 16, 25
    hyp = O.hyp_table(TRAINED, MAXP)
    a, r = [], []
    for seed in range(4):
        A, b, _ = O.make_problem(P, m, n, B, seed=100 + seed)
        G = O.er_graph(P, 0.5, seed=seed)
        y0, U0, d0 = _inits(B, P, n, seed)
        Y32, _, _ = O.forward_f32(A, b, [G] * B, hyp, y0, U0, d0)
        Y64, _, _ = O.forward_f64(A, b, [G] * B, hyp, y0, U0, d0)
        Yr = ref_torch.forward(A, b, [G] * B, hyp, y0, U0, d0)
        a.append(((Y32[-1] - Y64[-1]) ** 2).mean())
        r.append(((Yr[-1] - Y64[-1]) ** 2).mean())
    assert np.mean(a) <= 1e-5 and np.mean(r) <= 1e-5, (a, r)


def test_ref_torch_replay_matches_fp64_form():
    """The torch replay of the reference and the C fp64 oracle implement the same recurrence
    (fp64 torch replay == C fp64 up to summation order)."""
    import torch
    P, m, n, B, K = 4, 16, 32, 3, 8
    A, b, _ = O.make_problem(P, m, n, B, seed=12)
    graphs = [O.connected_er_graph(P, 0.5, seed=s) for s in range(B)]
    y0, U0, d0 = _inits(B, P, n, 9)
    hyp = O.hyp_table(np.random.default_rng(1).standard_normal((K, P, 4)).astype(np.float32), MAXP)
    for variant in (0, 1):
        Yr = ref_torch.forward(A, b, graphs, hyp, y0, U0, d0, variant=variant, dtype=torch.float64)
        Yc, _, _ = O.forward_f64(A, b, graphs, hyp, y0, U0, d0, variant=variant)
        np.testing.assert_allclose(Yr, Yc, rtol=0, atol=1e-9)


# ---- guards (unfolded_DLASSO.py:55-61, 84-86, 102-104) -----------------------------------------
def test_guards_reset_batch_globally():
    P, m, n, B, K = 3, 8, 16, 4, 3
    A, b, _ = O.make_problem(P, m, n, B, seed=3)
    G = O.er_graph(P, 0.7, seed=1)
    y0, U0, d0 = _inits(B, P, n, 4)
    hyp = O.hyp_table(np.zeros((K, P, 4), np.float32), MAXP)
    y2 = y0.copy(); y2[1, 2, 3] = np.nan
    Y, _, st = O.forward_f32(A, b, [G] * B, hyp, y2, U0, d0)
    Yz, _, _ = O.forward_f32(A, b, [G] * B, hyp, np.zeros_like(y0), U0, d0)
    assert st & 1 and np.array_equal(Y, Yz)          # y reset to 0 for the WHOLE batch
    b2 = b.copy(); b2[0, 0, 0] = np.nan                # NaN gradient -> zeroed for all samples
    Y, _, st = O.forward_f32(A, b2, [G] * B, hyp, y0, U0, d0)
    assert st & 4
    assert np.isfinite(Y).all()
    for variant in (0, 1):
        Y64, _, st64 = O.forward_f64(A, b2, [G] * B, hyp, y0, U0, d0, variant=variant)
        Yr = ref_torch.forward(A, b2, [G] * B, hyp, y0, U0, d0, variant=variant)
        assert st64 & 4 and np.isfinite(Yr).all()
        np.testing.assert_allclose(Y64, Yr, rtol=1e-4, atol=1e-4)


# ---- goldens ------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "golden_*.npz"))),
                         ids=lambda p: os.path.basename(p))
def test_oracle_reproduces_goldens(path):
    g = np.load(path)
    csr = (g["nbr_ptr"], g["nbr_idx"], g["deg"])
    v = int(g["variant"])
    Y32, U32, _ = O.forward_f32(g["A"], g["b"], csr, g["hyp"], g["y0"], g["U0"], g["d0"], variant=v)
    np.testing.assert_array_equal(Y32, g["Y32"])
    np.testing.assert_array_equal(U32, g["U32"])
    Y64, U64, _ = O.forward_f64(g["A"], g["b"], csr, g["hyp"], g["y0"], g["U0"], g["d0"], variant=v)
    np.testing.assert_allclose(Y64[g["k64"]], g["Y64"], rtol=0, atol=1e-12)


# ---- the reference's shipped data fixtures (stored as data under tests/golden/) ----------------
def test_fixture_A_singular_values_saturate():
    """results/25_iter_general_learning/A.pt (stored by tests/golden/make_fixtures.py): every
    sigma(A_p) == 10 (set_A's clamp, gnn_dlasso_utils.py:14; m=100 < n=500 puts all singular
    values above 10)."""
    A = np.load(os.path.join(GOLD, "fixture_25_iter_general_learning_A.npy"))
    assert A.dtype == np.float32
    A = A.reshape(5, 100, 500)
    s = np.linalg.svd(A.astype(np.float64), compute_uv=False)
    np.testing.assert_allclose(s, 10.0, rtol=1e-5)


def test_fixture_trained_hyp_ranges():
    h = O.hyp_table(TRAINED, MAXP)
    assert 0.0175 <= h[..., 0].min() and h[..., 0].max() <= 0.0502
    assert 0.494 <= h[..., 1].min() and h[..., 1].max() <= 0.923


# ---- the adjoint (§8(f) row 1): reverse mode of the forward w.r.t. the hyper-parameter table ---
def _digraph(P, seed):
    """A random directed graph (successor lists, a self-loop included): compute_delta's map is
    still symmetric (oracle.laplacians)."""
    rng = np.random.default_rng(seed)
    G = nx.DiGraph()
    G.add_nodes_from(range(P))
    G.add_edges_from((p, q) for p in range(P) for q in range(P) if p != q and rng.random() < 0.4)
    G.add_edge(2, 2)
    return G


_ADJ = [(0, 5, False, False), (0, 1, False, False), (1, 5, True, False), (1, 1, True, False),
        (0, 5, False, True), (1, 5, True, True)]
# ladder inputs (tests/saturation.py: vclip on y and U, the delta clamp and sign(0) all active);
# the last entry is the ladder's top
_ADJ_LADDER = [(0, 5, False, False, 150.0), (0, 1, True, False, 150.0), (1, 5, True, False, 400.0),
               (1, 1, False, False, 400.0)]


@pytest.mark.parametrize("variant,H,per_sample,directed,ladder", [
    *(pytest.param(*c, 0, id="-".join(str(v) for v in c)) for c in _ADJ),
    *(pytest.param(*c, id="-".join(str(v) for v in c[:4]) + "-ladder") for c in _ADJ_LADDER)])
def test_adjoint_matches_torch_autograd_of_the_reference_ops(variant, H, per_sample, directed, ladder):
    """backward_np64 == torch.autograd.grad through the reference's op sequence (fp64 replay,
    unfolded_DLASSO.py:53-107 + compute_delta's edge loop), on the same trajectory; directed
    graphs (successor lists) too; and on ladder inputs, where every clamp's mask is mixed."""
    import torch
    P, m, n, B, K = (5, 16, 48, 3, 12) if not ladder else (5, 16, 48, 10, 4)
    A, b, _ = O.make_problem(P, m, n, B, seed=31)
    if directed:
        graphs = ([_digraph(P, 60 + s) for s in range(B)] if per_sample else [_digraph(P, 7)] * B)
    elif per_sample:
        graphs = [O.connected_er_graph(P, 0.5, seed=60 + s) for s in range(B)]
    else:
        graphs = [O.er_graph(P, 0.5, seed=7)] * B
    y0, U0, d0 = _inits(B, P, n, seed=5)
    param = TRAINED[:K, :P] if H == P else TRAINED[:K, :1]
    hyp = O.hyp_table(param, MAXP)
    if ladder:
        import saturation
        y0, U0, d0 = saturation.ladder_inits(B, P, n, 5, ladder)
        hyp = saturation.ladder_hyp(K, H, 5)
    ht = torch.tensor(hyp, dtype=torch.float64, requires_grad=True)
    Y, Gr, Ur, U_K = ref_torch.forward_autograd(A, b, graphs, ht, y0, U0, d0, variant=variant)
    if ladder:
        saturation.assert_engaged(variant, hyp, y0, Y.detach().numpy(), U_K.numpy(), Gr.numpy(),
                                  Ur.numpy(), graphs)
    gY = torch.randn(Y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    want, = torch.autograd.grad((Y * gY).sum(), ht)
    got = O.backward_np64(A, graphs, hyp, y0, d0, Y.detach().numpy(), Gr.numpy(), Ur.numpy(),
                          gY.numpy(), variant=variant)
    assert got.shape == (K, H, 4)
    np.testing.assert_allclose(got, want.numpy(), rtol=1e-9, atol=1e-9 * np.abs(want.numpy()).max())
    # the gradient clamp really is active in this regime (the Gram path is cut on most lanes)
    gclip = np.array([max(1.0, 30.0 - k) if variant == 0 else 10.0 for k in range(K)])
    assert (np.abs(Gr.numpy()) > gclip[:, None, None, None]).mean() > 0.1


def test_forward_f32_rec_records_the_trajectory():
    """Grec/Urec of the order-matched fp32 oracle: Y unchanged, and every y_{k+1} follows from the
    recorded (y_k, Grec[k]) by the reference's clamp/update (:80-93) bit-for-bit."""
    P, m, n, B, K = 5, 16, 64, 4, 10
    A, b, _ = O.make_problem(P, m, n, B, seed=8)
    graphs = [O.er_graph(P, 0.5, seed=7)] * B
    y0, U0, d0 = _inits(B, P, n, seed=2)
    hyp = O.hyp_table(TRAINED[:K, :P], MAXP)
    Y, U, st = O.forward_f32(A, b, graphs, hyp, y0, U0, d0)
    Yr, Ur_, st2, G, Urec = O.forward_f32_rec(A, b, graphs, hyp, y0, U0, d0)
    assert st == st2 == 0
    assert np.array_equal(Y, Yr) and np.array_equal(U, Ur_)
    assert np.array_equal(Urec[0], U0)
    for k in range(K):
        yk = y0 if k == 0 else Y[k - 1]
        gc, vc = np.float32(max(1.0, 30.0 - k)), np.float32(max(10.0, 200.0 - 3 * k))
        g = np.clip(G[k], -gc, gc)
        al = hyp[k][:, 0][None, :, None]
        assert np.array_equal(np.clip(yk - al * g, -vc, vc), Y[k])


def test_adjoint_sensitivity_fp32_vs_fp64_trajectory():
    """The adjoint inherits the forward's sensitivity: an fp32 and an fp64 trajectory of the same
    problem drift apart (clamp masks flip where a lane sits near a bound), and the
    adjoints along them differ by up to a few percent of the largest entry. That is why the GPU
    tests check the HIP adjoint along the kernel's OWN recorded trajectory (tight tolerance), and
    only this loose band against the fp64 trajectory."""
    import torch
    P, m, n, B, K = 5, 32, 128, 4, 25
    A, b, _ = O.make_problem(P, m, n, B, seed=9)
    graphs = [O.er_graph(P, 0.5, seed=7)] * B
    y0, U0, d0 = _inits(B, P, n, seed=4)
    hyp = O.hyp_table(TRAINED[:K, :P], MAXP)
    rng = np.random.default_rng(0)
    gY = np.zeros((K, B, P, n))
    gY[-1] = rng.standard_normal((B, P, n))
    ht = torch.tensor(hyp, dtype=torch.float64)
    Y64, G64, U64, _ = ref_torch.forward_autograd(A, b, graphs, ht, y0, U0, d0)
    d64 = O.backward_np64(A, graphs, hyp, y0, d0, Y64.numpy(), G64.numpy(), U64.numpy(), gY)
    Y32, _, _, G32, U32 = O.forward_f32_rec(A, b, graphs, hyp, y0, U0, d0)
    d32 = O.backward_np64(A, graphs, hyp, y0, d0, Y32, G32, U32, gY)
    assert np.abs(d32 - d64).max() <= 0.1 * np.abs(d64).max()


def test_split_order_restatement():
    """oracle_forward_f32_split (the column-split forward's GEMM1 order, dadmm_split.hip): one
    slice covering every column is the unsplit chain exactly; 64-column slices give a different
    fp32 evaluation of the same recurrence (not bit-equal at a 256-column shape), as close to the
    fp64 restatement as the unsplit order is."""
    P, m, n, B, K = 3, 16, 200, 4, 6
    A, b, _ = O.make_problem(P, m, n, B, seed=5)
    G = O.er_graph(P, 0.6, seed=2)
    rng = np.random.default_rng(0)
    y0, U0, d0 = (1e-2 * rng.standard_normal((3, B, P, n))).astype(np.float32)
    hyp = O.hyp_table(0.3 * rng.standard_normal((K, P, 4)), [0.1, 0.99, 0.99, 0.99])
    Y, U, _ = O.forward_f32(A, b, [G] * B, hyp, y0, U0, d0)
    Y1, U1, _ = O.forward_f32(A, b, [G] * B, hyp, y0, U0, d0, split_cols=256)
    assert np.array_equal(Y, Y1) and np.array_equal(U, U1)
    Ys, _, _ = O.forward_f32(A, b, [G] * B, hyp, y0, U0, d0, split_cols=64)
    assert not np.array_equal(Y, Ys)
    Y64, _, _ = O.forward_f64(A, b, [G] * B, hyp, y0, U0, d0)
    e_split = float(((Ys[-1] - Y64[-1]) ** 2).mean())
    e_fused = float(((Y[-1] - Y64[-1]) ** 2).mean())
    assert e_split <= 1e-8 and e_fused <= 1e-8, (e_split, e_fused)
    with pytest.raises(RuntimeError):
        O.forward_f32(A, b, [G] * B, hyp, y0, U0, d0, split_cols=40)   # not a multiple of 16
