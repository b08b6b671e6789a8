"""The streamed evaluation forward (csrc/dadmm_stream.hip built with DADMM_STREAM_EVAL, C ABI
dadmm_forward_eval_stream, ops.forward_eval_stream_raw, DLASSO_unfolded.evaluate): the streamed
single-launch forward with two iterates of state that take turns instead of K, which sums every
iterate's squared error against the label where it holds the iterate in registers.

Every case compares with the CPU oracle (all iterates, the same inits): y_final and U_K bit for bit,
status 0, every losses[k] within the derived bound of the fp64 loss over the oracle's fp32 iterate,
`out` recomputed from the returned losses in the finish kernel's arithmetic.

The bound, relative because every term is non-negative: a lane adds L = n_pad PW / 4 terms in one
fp32 chain (n_pad / 32 steps, PW agents per wave, 2 tiles, 4 columns), the wave sum adds 6 levels,
each term takes three roundings (the difference, the square, its addition), and the finish (in
double) ends in one cast and one `+ 1e-8f`: (L + 16) * 2^-24, the 16 standing for everything but the
lane chain. Largest relative error observed over the 31 losses of this file on an MI355X: 6.2e-8
(DESIGN.md §4.11b).

Shapes: the smallest that reach each kernel form (<8,1>: P <= 8, m <= 64; <8,2>: P 9..16; <8,1,.,2>:
64 < m <= 128) and each mask (an absent agent, a ragged last tile, a column cut inside a 32-column
block, n_true below the stored row length, both parities of the buffer the last iterate lands in)."""
import argparse

import numpy as np
import pytest
import torch

import oracle as O
from test_gpu_eval import _finish

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


def _graphs(P, B, per_sample, seed=3):
    prob = 0.5 if P <= 8 else 0.3
    if per_sample:
        return [O.er_graph(P, prob, seed=seed + s) for s in range(B)]
    return [O.er_graph(P, prob, seed=seed)] * B


def _run(dev, A, b, graphs, hyp, y0, U0, d0, label, variant=0):
    """(losses, out, y_final, U_K, status, loss_flags) of one forward_eval_stream_raw call, as numpy."""
    from dadmm_hip import PreparedOperator, forward_eval_stream_raw, ingest
    B = y0.shape[0]
    op = PreparedOperator(_t(A, dev))
    g = ingest(graphs, A.shape[0], B, dev)
    losses, out, yf, U, st, fl, used = forward_eval_stream_raw(
        op, _t(b, dev), g, _t(hyp, dev), _t(label, dev), _t(y0, dev), _t(U0, dev), _t(d0, dev),
        variant=variant, want_U=True)
    torch.cuda.synchronize()
    for u, x in zip(used, (y0, U0, d0)):        # the inits as used: the caller's, bit for bit
        assert np.array_equal(_bits(u), np.ascontiguousarray(x).view(np.int32))
    return (losses.cpu().numpy(), out.cpu().numpy(), yf.cpu().numpy(), U.cpu().numpy(), int(st.item()),
            fl.cpu().numpy())


def _bound(P, n):
    nt = -(-n // 64)
    n_pad = 64 * (4 if nt == 3 else nt)               # the prepared operator's row length
    return (n_pad * (2 if P > 8 else 1) // 4 + 16) * 2.0 ** -24


def _check(dev, A, b, graphs, hyp, y0, U0, d0, label, variant=0):
    args = (A, b, graphs, hyp, y0, U0, d0)
    P, K, n = A.shape[0], hyp.shape[0], A.shape[2]
    losses, out, yf, U, st, fl = _run(dev, *args, label, variant=variant)
    Yo, Uo, sto = O.forward_f32(*args, variant=variant)
    assert st == sto == 0
    assert yf.shape == Yo[-1].shape and losses.shape == (K,) and out.shape == (2,)
    assert np.array_equal(yf, Yo[-1]), f"y_final vs oracle: max |diff| {np.abs(yf - Yo[-1]).max()}"
    assert np.array_equal(U, Uo), f"U_K vs oracle: max |diff| {np.abs(U - Uo).max()}"
    bound = _bound(P, n)
    for k in range(K):
        ref = np.mean((Yo[k].astype(np.float64) - label.astype(np.float64)[:, None, :]) ** 2)
        rel = abs(float(losses[k]) - ref) / ref
        print(f"losses[{k}] = {losses[k]!r}, fp64 {ref!r}, relative error {rel:.3e} (bound {bound:.3e})")
        assert rel <= bound, (k, losses[k], ref, rel, bound)
    assert np.array_equal(out, _finish(losses)), (out, _finish(losses))
    assert fl.tolist() == [0, 0]


def _case(dev, P, m, n, B, K, seed, per_sample=False, H=None, variant=0, label=None):
    A, b, _ = O.make_problem(P, m, n, B, seed=seed)
    H = P if H is None else H
    _check(dev, A, b, _graphs(P, B, per_sample, seed), _hyp(K, H, seed), *_inits(B, P, n, seed=seed),
           _label(B, n, seed) if label is None else label, variant=variant)


def test_bound_helper_knows_the_padding():
    assert _bound(7, 198) == (256 // 4 + 16) * 2.0 ** -24 and _bound(16, 512) == (512 * 2 // 4 + 16) * 2.0 ** -24
    assert _bound(5, 500) == (512 // 4 + 16) * 2.0 ** -24 and _bound(8, 128) == (128 // 4 + 16) * 2.0 ** -24


def test_one_agent_per_wave_ragged_everything(cuda):
    """<8,1>: an absent agent on wave 7, five live samples in the last of three tiles, n = 198 stored
    in rows of 200 (a column cut inside a 32-column block, n_true < stored n, n_pad = 256)."""
    _case(cuda, 7, 50, 198, 37, 4, seed=61)


@pytest.mark.parametrize("K", [1, 2, 3])
def test_four_blocks_both_parities_of_the_last_buffer(cuda, K):
    """<8,1> at the minimum of four column blocks; K = 1 never touches the second iterate."""
    _case(cuda, 8, 64, 128, 16, K, seed=62)


def test_two_agents_per_wave_second_absent(cuda):
    """<8,2> at P = 9: the second agent is absent on waves 1..7, whose lanes still hold a real label."""
    _case(cuda, 9, 64, 128, 16, 3, seed=63)


def test_configs2_shape_per_sample_graphs(cuda):
    """<8,2> at BASELINE configs[2]'s shape, one sample past a full tile, a graph per sample."""
    _case(cuda, 16, 64, 512, 17, 3, seed=64, per_sample=True)


@pytest.mark.parametrize("P,m,n,B,K", [(5, 100, 500, 20, 3), (8, 65, 128, 16, 2), (1, 100, 128, 16, 2)])
def test_two_m_groups(cuda, P, m, n, B, K):
    """<8,1,.,2>: the reference's default shape, the first m past one group, one edgeless agent."""
    _case(cuda, P, m, n, B, K, seed=65 + P)


@pytest.mark.parametrize("H,variant", [(1, 0), (9, 1)])
def test_same_mode_and_gnn_variant(cuda, H, variant):
    P, m, n, B, K = 9, 64, 128, 16, 3
    A, b, _ = O.make_problem(P, m, n, B, seed=45)
    rng = np.random.default_rng(7)
    hyp = O.hyp_table(rng.standard_normal((K, H, 4)).astype(np.float32), [0.3, 0.99, 0.99, 0.99])
    _check(cuda, A, b, _graphs(P, B, False, 2), hyp, *_inits(B, P, n, seed=5), _label(B, n, 5), variant=variant)


def test_zero_label(cuda):
    """label = 0: the losses are mean(y^2)."""
    _case(cuda, 7, 64, 128, 16, 2, seed=46, label=np.zeros((16, 128), np.float32))


def test_nonfinite_label_takes_the_fallback(cuda):
    """One inf in the label: (1, 1) as compute_loss returns it; the forward itself is untouched."""
    P, m, n, B, K = 7, 64, 128, 16, 3
    A, b, _ = O.make_problem(P, m, n, B, seed=41)
    args = (A, b, _graphs(P, B, False, 7), _hyp(K, P, 2), *_inits(B, P, n, seed=1))
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
    """forward + compute_loss + layer_losses, the validation step without evaluate."""
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
    P, m, n, B, K = 7, 64, 128, 16, 3
    A, b, ini, label = _problem(cuda, P, m, n, B, seed=11)
    ini[0][B - 1, P - 1, n - 1] = np.nan
    graphs = _graphs(P, B, False, 2)
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


def test_module_routes_to_the_streamed_evaluation(cuda, monkeypatch):
    """evaluate at a streamed shape calls forward_eval_stream_raw (and not forward); at m > 64 only
    from the batch threshold on."""
    from dadmm_hip import ops
    calls = []
    real = ops.forward_eval_stream_raw
    monkeypatch.setattr(ops, "forward_eval_stream_raw", lambda *a, **k: calls.append(1) or real(*a, **k))
    for (P, m, n, B), min_b, want in (((7, 64, 128, 16), None, 1), ((5, 100, 128, 16), 16, 1),
                                      ((5, 100, 128, 16), 17, 0)):
        if min_b is not None:
            monkeypatch.setattr(ops, "STREAM_EVAL_M128_MIN_B", min_b)
        A, b, ini, label = _problem(cuda, P, m, n, B, seed=21)
        mod = _module(cuda, A, 2)
        inits = tuple(_t(x, cuda)[..., None] for x in ini)
        graphs = _graphs(P, B, False, 5)
        del calls[:]
        ev = mod.evaluate(b, graphs, label, inits=inits)
        assert len(calls) == want, (P, m, min_b)
        Y = _ordinary(mod, b, graphs, label, inits)[0]
        assert int(ev.status.item()) == 0 and np.array_equal(_bits(ev.y_final), _bits(Y[-1]))


def test_module_drawn_inits_follow_the_forward(cuda):
    """evaluate and a forward after re-seeding draw the same inits and leave the generator at the same
    offset; per-sample graphs."""
    P, m, n, B, K = 7, 64, 128, 16, 2
    A, b, _, label = _problem(cuda, P, m, n, B, seed=13)
    graphs = _graphs(P, B, True, 7)
    mod = _module(cuda, A, K, mode="same")
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
    assert ((ev.losses.double() - ref).abs() <= _bound(P, n) * ref).all()
    assert np.array_equal(ev.loss_final.cpu().numpy(), _finish(ev.losses.cpu().numpy())[1])
    assert np.array_equal(ev.loss_mean.cpu().numpy(), _finish(ev.losses.cpu().numpy())[0])


def test_memory_is_a_few_states_not_K(cuda):
    """P 16, n 512, B 32, K 12: one evaluate(on_guard="flag") grows the peak by fewer than 8 states of
    B P n_store 4 bytes (three draws, y_final and its flagged copy, two scratch states, label and
    partial sums); Y alone would be 12."""
    from dadmm_hip import ingest
    P, m, n, B, K = 16, 64, 512, 32, 12
    A, b, _, label = _problem(cuda, P, m, n, B, seed=14)
    g = ingest(_graphs(P, B, False, 3), P, B, cuda)
    mod = _module(cuda, A, K)
    mod.evaluate(b, g, label, on_guard="flag")            # the operator, the table, the code objects
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(cuda)
    before = torch.cuda.memory_allocated(cuda)
    ev = mod.evaluate(b, g, label, on_guard="flag")
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated(cuda) - before
    state = B * P * n * 4
    print(f"peak growth {growth} bytes = {growth / state:.2f} states")
    assert growth < 8 * state, (growth, state)
    assert int(ev.status.item()) == 0 and torch.isfinite(ev.losses).all()


def test_raw_call_refuses_a_fused_shape(cuda):
    from dadmm_hip import PreparedOperator, forward_eval_stream_raw, ingest
    P, m, n, B, K = 5, 64, 256, 16, 2
    A, b, _ = O.make_problem(P, m, n, B, seed=15)
    g = ingest(_graphs(P, B, False, 3), P, B, cuda)
    with pytest.raises(ValueError, match="does not serve"):
        forward_eval_stream_raw(PreparedOperator(_t(A, cuda)), _t(b, cuda), g, _t(_hyp(K, P, 1), cuda),
                                _t(_label(B, n, 1), cuda), *(_t(x, cuda) for x in _inits(B, P, n)))
