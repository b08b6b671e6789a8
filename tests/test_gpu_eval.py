"""The evaluation forward (csrc/dadmm_fused_roles.hip built with DADMM_ROLES_EVAL, C ABI
dadmm_forward_eval, ops.forward_eval_raw, DLASSO_unfolded.evaluate): the role-split forward that
sums every iterate's squared error against the label in its update role and stores only the last
iterate.

Against the CPU oracle: y_final and U_K bit for bit, status 0, every losses[k] within the derived
bound of the fp64 loss over the oracle's fp32 iterate, `out` recomputed from the returned losses in
the finish kernel's arithmetic, and a second run bit for bit. The bound, relative because every term
is non-negative: a lane adds 16 P terms in one fp32 chain, the wave sum adds 6 levels, each term
takes three roundings (the difference, the square, its addition), and the finish (in double) ends in
one cast and one `+ 1e-8f`: (16 P + 16) * 2^-24, the 16 standing for everything but the lane chain.

Then the guards: a non-finite label, a NaN in y0 (both on_guard policies of the module), a directed
shared graph, drawn inits, and a shape the kernel does not serve."""
import argparse

import networkx as nx
import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

MAXP = [0.1, 0.99, 0.99, 0.99]


def _inits(B, P, n, seed=99):
    rng = np.random.default_rng(seed)
    return (1e-2 * rng.standard_normal((3, B, P, n))).astype(np.float32)


def _label(B, n, seed):
    return np.random.default_rng(seed).standard_normal((B, n)).astype(np.float32)


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _hyp(K, H, seed):
    rng = np.random.default_rng(seed)
    return O.hyp_table((0.5 * rng.standard_normal((K, H, 4))).astype(np.float32), MAXP)


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.int32)


def _run(dev, A, b, graphs, hyp, y0, U0, d0, label, variant=0):
    """(losses, out, y_final, U_K, status, loss_flags) of one forward_eval_raw call, as numpy."""
    from dadmm_hip import PreparedOperator, forward_eval_raw, ingest
    B = y0.shape[0]
    op = PreparedOperator(_t(A, dev))
    g = ingest(graphs, A.shape[0], B, dev)
    assert g.shared
    losses, out, yf, U, st, fl, used = forward_eval_raw(
        op, _t(b, dev), g, _t(hyp, dev), _t(label, dev), _t(y0, dev), _t(U0, dev), _t(d0, dev),
        variant=variant, want_U=True)
    torch.cuda.synchronize()
    for u, x in zip(used, (y0, U0, d0)):        # the inits as used: the caller's, bit for bit
        assert np.array_equal(_bits(u), np.ascontiguousarray(x).view(np.int32))
    return (losses.cpu().numpy(), out.cpu().numpy(), yf.cpu().numpy(), U.cpu().numpy(), int(st.item()),
            fl.cpu().numpy())


def _finish(losses):
    """(loss_mean, loss_final) from the fp32 losses as finish_kernel computes them: the mean summed in
    double in order, cast, then + 1e-8 in fp32."""
    mean = 0.0
    for v in losses:
        mean += float(v)
    return np.array([np.float32(mean / len(losses)) + np.float32(1e-8), losses[-1] + np.float32(1e-8)],
                    dtype=np.float32)


def _check(dev, A, b, graphs, hyp, y0, U0, d0, label, variant=0):
    args = (A, b, graphs, hyp, y0, U0, d0)
    P, K = A.shape[0], hyp.shape[0]
    losses, out, yf, U, st, fl = _run(dev, *args, label, variant=variant)
    Yo, Uo, sto = O.forward_f32(*args, variant=variant)
    assert st == sto == 0
    assert yf.shape == Yo[-1].shape and losses.shape == (K,) and out.shape == (2,)
    assert np.array_equal(yf, Yo[-1]), f"y_final vs oracle: max |diff| {np.abs(yf - Yo[-1]).max()}"
    assert np.array_equal(U, Uo), f"U_K vs oracle: max |diff| {np.abs(U - Uo).max()}"
    bound = (16 * P + 16) * 2.0 ** -24
    for k in range(K):
        ref = np.mean((Yo[k].astype(np.float64) - label.astype(np.float64)[:, None, :]) ** 2)
        rel = abs(float(losses[k]) - ref) / ref
        print(f"losses[{k}] = {losses[k]!r}, fp64 {ref!r}, relative error {rel:.3e} (bound {bound:.3e})")
        assert rel <= bound, (k, losses[k], ref, rel, bound)
    assert np.array_equal(out, _finish(losses)), (out, _finish(losses))
    assert fl.tolist() == [0, 0]
    again = _run(dev, *args, label, variant=variant)
    for x, y in zip((losses, out, yf, U, fl), (again[0], again[1], again[2], again[3], again[5])):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    assert again[4] == st


def test_one_full_tile(cuda):
    P, m, n, B, K = 5, 64, 256, 16, 3
    A, b, _ = O.make_problem(P, m, n, B, seed=41)
    _check(cuda, A, b, [O.er_graph(P, 0.5, seed=7)] * B, _hyp(K, P, 2), *_inits(B, P, n, seed=1), _label(B, n, 1))


def test_ragged_batch_and_padded_columns(cuda):
    """Three tiles, five live samples in the last; n = 198 is stored in rows of 200: the rows past n,
    the padded label columns and the samples past B must add exactly 0 (the denominator is B P n)."""
    P, m, n, B, K = 3, 50, 198, 37, 4
    A, b, _ = O.make_problem(P, m, n, B, seed=42)
    _check(cuda, A, b, [O.er_graph(P, 0.6, seed=3)] * B, _hyp(K, P, 3), *_inits(B, P, n, seed=2), _label(B, n, 2))


@pytest.mark.parametrize("P", [1, 2, 4])
def test_agent_counts(cuda, P):
    m, n, B, K = 64, 256, 16, 2
    A, b, _ = O.make_problem(P, m, n, B, seed=50 + P)
    _check(cuda, A, b, [O.er_graph(P, 0.7, seed=P)] * B, _hyp(K, P, 4), *_inits(B, P, n, seed=P), _label(B, n, P))


def test_single_iteration(cuda):
    """K = 1: the final store is the only iterate."""
    P, m, n, B, K = 5, 64, 256, 16, 1
    A, b, _ = O.make_problem(P, m, n, B, seed=43)
    _check(cuda, A, b, [O.er_graph(P, 0.5, seed=9)] * B, _hyp(K, P, 5), *_inits(B, P, n, seed=3), _label(B, n, 3))


@pytest.mark.parametrize("H,variant", [(1, 0), (5, 1)])
def test_same_mode_and_gnn_variant(cuda, H, variant):
    P, m, n, B, K = 5, 64, 256, 16, 3
    A, b, _ = O.make_problem(P, m, n, B, seed=45)
    rng = np.random.default_rng(7)
    hyp = O.hyp_table(rng.standard_normal((K, H, 4)).astype(np.float32), [0.3, 0.99, 0.99, 0.99])
    _check(cuda, A, b, [O.er_graph(P, 0.5, seed=2)] * B, hyp, *_inits(B, P, n, seed=5), _label(B, n, 5),
           variant=variant)


def test_zero_label(cuda):
    """label = 0: the losses are mean(y^2)."""
    P, m, n, B, K = 2, 64, 256, 16, 2
    A, b, _ = O.make_problem(P, m, n, B, seed=46)
    _check(cuda, A, b, [O.er_graph(P, 0.7, seed=2)] * B, _hyp(K, P, 6), *_inits(B, P, n, seed=6),
           np.zeros((B, n), np.float32))


def test_nonfinite_label_takes_the_fallback(cuda):
    """One inf in the label: (1, 1) as compute_loss returns it; the forward itself is untouched."""
    P, m, n, B, K = 5, 64, 256, 16, 3
    A, b, _ = O.make_problem(P, m, n, B, seed=41)
    args = (A, b, [O.er_graph(P, 0.5, seed=7)] * B, _hyp(K, P, 2), *_inits(B, P, n, seed=1))
    label = _label(B, n, 1)
    label[B - 1, n - 1] = np.inf
    losses, out, yf, U, st, fl = _run(cuda, *args, label)
    Yo, Uo, sto = O.forward_f32(*args)
    assert st == sto == 0
    assert out.tolist() == [1.0, 1.0] and fl.tolist() == [1, 1]
    assert np.array_equal(yf, Yo[-1]) and np.array_equal(U, Uo)


# ---- the module ------------------------------------------------------------------------------------
def _module(dev, A, K, mode="diff"):
    import unfolded_DLASSO as U
    args = argparse.Namespace(GHN_iter_num=K, DADMM_mode=mode, alpha_max=0.1, tau_max=0.99, rho_max=0.99,
                              eta_max=0.99, max_penalty_threshold=0.8, penalty_reduction_factor=0.95)
    mod = U.DLASSO_unfolded(_t(A, dev)[None], args).to(dev)
    with torch.no_grad():
        mod.seq_hyp.param.copy_(0.3 * torch.randn(mod.seq_hyp.param.shape,
                                                  generator=torch.Generator().manual_seed(1)))
    return mod.eval().requires_grad_(False)


def _ordinary(mod, b, graphs, label, inits=None):
    """forward + compute_loss + layer_losses, today's validation step."""
    import gnn_dlasso_utils
    with torch.no_grad():
        Y, hyp = mod(b, graphs, inits=inits)
        lm, lf = gnn_dlasso_utils.compute_loss(Y, label)
        losses = gnn_dlasso_utils.layer_losses(Y, label)
    return Y, hyp, lm, lf, losses


def _problem(dev, P, m, n, B, seed):
    A, b, _ = O.make_problem(P, m, n, B, seed=seed)
    y0, U0, d0 = _inits(B, P, n, seed=seed)
    return A, _t(b, dev)[..., None], [y0, U0, d0], _t(_label(B, n, seed), dev)[..., None]


def test_y0_nan_raw_status_and_both_guard_policies(cuda):
    from dadmm_hip import _lib
    P, m, n, B, K = 5, 64, 256, 16, 3
    A, b, ini, label = _problem(cuda, P, m, n, B, seed=11)
    ini[0][B - 1, P - 1, n - 1] = np.nan
    graphs = [O.er_graph(P, 0.6, seed=2)] * B
    st = _run(cuda, A, b[..., 0].cpu().numpy(), graphs, _hyp(K, P, 11), *ini, label[..., 0].cpu().numpy())[4]
    assert st & _lib.STATUS_Y_NONFINITE, st

    mod = _module(cuda, A, K)
    inits = tuple(_t(x, cuda)[..., None] for x in ini)
    Y, hyp, lm, lf, _ = _ordinary(mod, b, graphs, label, inits)
    ev = mod.evaluate(b, graphs, label, inits=inits)                 # on_guard="recompute"
    assert np.array_equal(_bits(ev.loss_mean), _bits(lm)) and np.array_equal(_bits(ev.loss_final), _bits(lf))
    assert np.array_equal(_bits(ev.y_final), _bits(Y[-1])) and torch.equal(ev.hyp, hyp)
    assert torch.isfinite(ev.y_final).all()

    ev = mod.evaluate(b, graphs, label, inits=inits, on_guard="flag")
    assert int(ev.status.item()) & _lib.STATUS_Y_NONFINITE and ev.status is mod.last_status
    assert torch.isnan(ev.losses).all() and torch.isnan(ev.loss_mean) and torch.isnan(ev.loss_final)
    assert torch.isnan(ev.y_final).all()
    assert ev.loss_final._dadmm_status is ev.status


def test_directed_shared_graph_is_recomputed(cuda):
    """An asymmetric shared adjacency raises DADMM_STATUS_RECOMPUTE in the kernel; "recompute" then
    returns the ordinary path's result."""
    P, m, n, B, K = 5, 64, 256, 16, 3
    A, b, ini, label = _problem(cuda, P, m, n, B, seed=12)
    D = nx.DiGraph()
    D.add_nodes_from(range(P))
    D.add_edges_from([(0, 1), (1, 0), (1, 2), (2, 3), (3, 2), (3, 4), (4, 0), (0, 3)])
    graphs = [D] * B
    st = _run(cuda, A, b[..., 0].cpu().numpy(), graphs, _hyp(K, P, 12), *ini, label[..., 0].cpu().numpy())[4]
    assert st & 16, st
    mod = _module(cuda, A, K)
    inits = tuple(_t(x, cuda)[..., None] for x in ini)
    Y, hyp, lm, lf, losses = _ordinary(mod, b, graphs, label, inits)
    ev = mod.evaluate(b, graphs, label, inits=inits)
    assert np.array_equal(_bits(ev.loss_mean), _bits(lm)) and np.array_equal(_bits(ev.loss_final), _bits(lf))
    assert np.array_equal(_bits(ev.y_final), _bits(Y[-1])) and np.array_equal(_bits(ev.losses), _bits(losses))


def test_module_drawn_inits_follow_the_forward(cuda):
    """evaluate and a forward after re-seeding draw the same inits and leave the generator at the same
    offset; the losses agree with the fp64 loss over forward's iterates within the derived bound. The
    batch is just past the size up to which the ordinary forward takes the column-split kernel, whose
    GEMM1 order (and so its bits) is another."""
    from dadmm_hip.ops import split_cols
    P, m, n, K = 2, 64, 256, 2
    B = 16 * (torch.cuda.get_device_properties(cuda).multi_processor_count // 2 + 1)
    A, b, _, label = _problem(cuda, P, m, n, B, seed=13)
    graphs = [O.er_graph(P, 0.5, seed=7)] * B
    mod = _module(cuda, A, K, mode="same")
    assert split_cols(mod.operator(), B, K) == 0
    gen = torch.cuda.default_generators[cuda.index]
    torch.manual_seed(1234)
    ev = mod.evaluate(b, graphs, label)
    off_eval = gen.get_offset()
    torch.manual_seed(1234)
    Y, hyp, lm, lf, losses = _ordinary(mod, b, graphs, label)
    assert gen.get_offset() == off_eval
    assert int(ev.status.item()) == 0
    assert np.array_equal(_bits(ev.y_final), _bits(Y[-1])) and torch.equal(ev.hyp, hyp)
    assert ev.y_final.shape == (B, P, n, 1) and ev.losses.shape == (K,)
    ref = ((Y[..., 0].double() - label[..., 0].double()[None, :, None, :]) ** 2).mean(dim=(1, 2, 3))
    bound = (16 * P + 16) * 2.0 ** -24
    assert ((ev.losses.double() - ref).abs() <= bound * ref).all()
    assert np.array_equal(ev.loss_final.cpu().numpy(), _finish(ev.losses.cpu().numpy())[1])
    assert np.array_equal(ev.loss_mean.cpu().numpy(), _finish(ev.losses.cpu().numpy())[0])


@pytest.mark.parametrize("case", ["per_sample_graphs", "n128"])
def test_module_on_an_unserved_shape(cuda, case):
    """Per-sample graphs, or n = 128: the same tuple, from forward + compute_loss + layer_losses."""
    P, m, n, B, K = (5, 64, 256, 16, 3) if case == "per_sample_graphs" else (4, 32, 128, 16, 3)
    A, b, ini, label = _problem(cuda, P, m, n, B, seed=14)
    graphs = ([O.er_graph(P, 0.5, seed=s) for s in range(B)] if case == "per_sample_graphs"
              else [O.er_graph(P, 0.5, seed=3)] * B)
    mod = _module(cuda, A, K)
    inits = tuple(_t(x, cuda)[..., None] for x in ini)
    Y, hyp, lm, lf, losses = _ordinary(mod, b, graphs, label, inits)
    ev = mod.evaluate(b, graphs, label, inits=inits)
    assert type(ev).__name__ == "Evaluation" and int(ev.status.item()) == 0
    assert np.array_equal(_bits(ev.losses), _bits(losses))
    assert np.array_equal(_bits(ev.loss_mean), _bits(lm)) and np.array_equal(_bits(ev.loss_final), _bits(lf))
    assert np.array_equal(_bits(ev.y_final), _bits(Y[-1])) and torch.equal(ev.hyp, hyp)


def test_raw_call_refuses_an_unserved_shape(cuda):
    from dadmm_hip import PreparedOperator, forward_eval_raw, ingest
    P, m, n, B, K = 4, 32, 128, 16, 2
    A, b, _ = O.make_problem(P, m, n, B, seed=15)
    g = ingest([O.er_graph(P, 0.5, seed=3)] * B, P, B, cuda)
    with pytest.raises(ValueError, match="does not serve"):
        forward_eval_raw(PreparedOperator(_t(A, cuda)), _t(b, cuda), g, _t(_hyp(K, P, 1), cuda),
                         _t(_label(B, n, 1), cuda), *(_t(x, cuda) for x in _inits(B, P, n)))
