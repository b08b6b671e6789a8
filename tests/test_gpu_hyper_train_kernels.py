"""GPU: the training hypernetwork's kernels one at a time, through the C ABI, in every kernel form
the launches choose from the shape (dadmm_hyper_gcn_train, _gcn_train_bwd, _linear_gcn_bwd,
_linear_ln_train, _rownorm_bwd, _head_train, _head_act, _bn_running_update; csrc/dadmm_hyper.hip,
dadmm_hyper_train.hip).

Every test first asks dadmm_hyper_form (tests/test_hyper_form.py pins the same shapes on the CPU)
that its shape takes the form it is meant to reach — the row tile WR in {1, 2, 4, 5}, the LDS-DMA
ring, the K split over two wave sets, the split input, the four (NT, PR) forms of gcn_bwd_kernel —
and fails with "inputs unsuitable" otherwise, before it looks at any output.

Bars.
  GEMM outputs (m_out, xd, z): test_gpu_hyper._close against the float64 product.
  Everything else, the element bar of test_gpu_saturation.test_gnn_step_adjoint:
      |got - want64| <= r max|want64| + r |want64|,
      r = max(2^-23, 4 x the distance of a float32 torch restatement of the same ops on the same
          inputs from the float64 one, relative to max|want64|),
  against float64 torch autograd of the literal ops (leaky_relu -> BatchNorm over a sample's P nodes
  -> Dropout; Dropout -> LayerNorm -> LeakyReLU; sigmoid -> clamp -> x max -> clamp(max=0.9999) of
  gnn_dlasso_models_progressive.py:167-196). The epilogues are checked on the kernel's own GEMM
  output (m_out, xd), so the leaky_relu / dropout masks are exact and GEMM rounding stays out of it.
  dadmm_hyper_bn_running_update sums in float64 and rounds once: within 1 ulp of float32(want64).
  Bit identity where the header promises it (two launches; linear_gcn_bwd == linear + gcn_train_bwd;
  head_train's hyp == linear + head_act).
  The float32 restatement of the BatchNorm forward sums the P nodes in node order, as the kernel does:
  a float32 sum's rounding depends on its order, and torch's pairwise mean says little about 130
  sequential terms (with torch.mean / torch.var the P = 130 case sat at 1.2e-6 of the maximum against
  r = 1.0e-6, and the zero-variance columns at up to 1.8e-4 against a restatement that was exact).
  The fused dadmm_hyper_linear_gcn_bwd is compared with dadmm_hyper_linear + dadmm_hyper_gcn_train_bwd
  at K = 128 on a small grid too, where it used to split its K loop over two wave sets, which
  dadmm_hyper_linear never does: dz differed by 1.1e-5 and part by 3.4e-5 there. The C-ABI entry now
  runs dadmm_hyper_linear's GEMM (the training backward keeps the split on an entry of its own, whose
  pair test_gpu_hyper_train.test_fused_gcn_backward_bit_identical holds bit for bit).
Inputs come from CPU generators (the same on every machine); the dropout masks are regenerated from
the kernels' counter-based stream (test_gpu_hyper_train._drop_hash). Preconditions, on the float64
reference ("inputs unsuitable"): >= 32 kept and >= 32 dropped lanes where drop_p > 0, >= 32 lanes
on each side of the leaky_relu (both where the shape has the lanes: the 5 x 8 decoder block has 40),
no row / sample whose reference output is all zero, and for the head every class of each clamp
populated (>= min(32, lanes / 16) lanes: the (7, 1) head has 28 lanes).

Two columns of W are zero in the gcn_train cases: every node of a sample then has m = bias exactly
(asserted bit for bit), the batch variance is 0 up to the rounding of the mean of P equal numbers
(exactly 0 at P = 2, where the output is then exactly bn_bias / (1 - p) or 0), and rstd sits at
1 / sqrt(eps). Those columns get a bar of their own so that their amplification does not loosen the
other columns'.

Measured float32 scales (MI355X, this module's inputs; r = max(2^-23, 4 x scale)):
  gcn_train y                            6.5e-08 .. 1.6e-05   (kernel error / max 6.5e-08 .. 1.3e-05; 66 cases)
  gcn_train mean                         2.5e-08 .. 4.2e-07   (kernel error / max 2.5e-08 .. 4.2e-07; 33 cases)
  gcn_train var                          3.7e-08 .. 4.3e-07   (kernel error / max 3.7e-08 .. 4.3e-07; 33 cases)
  gcn_train zero-variance columns y      0.0e+00 .. 1.8e-04   (kernel error / max 0.0e+00 .. 1.8e-04; 33 cases)
  gcn_train zero-variance columns mean   0.0e+00 .. 1.6e-06   (kernel error / max 0.0e+00 .. 1.6e-06; 33 cases)
  gcn_train_bwd dz                       5.9e-08 .. 1.4e-05   (kernel error / max 4.7e-08 .. 1.4e-05; 36 cases)
  gcn_train_bwd dgamma                   5.5e-08 .. 7.6e-06   (kernel error / max 5.7e-08 .. 7.6e-06; 36 cases)
  gcn_train_bwd dbeta                    3.7e-08 .. 1.2e-07   (kernel error / max 3.7e-08 .. 2.9e-07; 36 cases)
  gcn_train_bwd dbias                    7.2e-08 .. 2.2e-05   (kernel error / max 7.4e-08 .. 2.2e-05; 36 cases)
  linear_gcn_bwd dz                      1.7e-07 .. 4.6e-06   (kernel error / max 1.7e-07 .. 4.8e-06; 9 cases)
  linear_gcn_bwd dgamma                  2.1e-07 .. 7.0e-06   (kernel error / max 2.2e-07 .. 7.0e-06; 9 cases)
  linear_gcn_bwd dbeta                   2.0e-07 .. 7.2e-07   (kernel error / max 1.9e-07 .. 7.2e-07; 9 cases)
  linear_gcn_bwd dbias                   2.1e-07 .. 1.1e-04   (kernel error / max 1.9e-07 .. 1.1e-04; 9 cases)
  rownorm_bwd dx                         6.6e-08 .. 4.0e-07   (kernel error / max 6.2e-08 .. 2.8e-07; 70 cases)
  rownorm_bwd dweight                    4.0e-08 .. 1.6e-07   (kernel error / max 3.8e-08 .. 1.7e-07; 70 cases)
  rownorm_bwd dbias                      0.0e+00 .. 1.2e-07   (kernel error / max 0.0e+00 .. 1.1e-07; 70 cases)
  linear_ln_train y                      6.6e-08 .. 1.5e-07   (kernel error / max 6.2e-08 .. 2.1e-07; 10 cases)
  head_act hyp                           4.4e-08 .. 1.2e-07   (kernel error / max 4.4e-08 .. 1.2e-07; 6 cases)
  head_act dz                            9.2e-08 .. 1.8e-05   (kernel error / max 9.2e-08 .. 1.8e-05; 6 cases)
  head_train hyp                         1.9e-08 .. 1.1e-07   (kernel error / max 1.9e-08 .. 1.1e-07; 6 cases)
  head_train dz                          2.6e-08 .. 2.9e-07   (kernel error / max 2.6e-08 .. 2.9e-07; 6 cases)
The largest scales are the few-node BatchNorm (a sample whose variance is small against eps), the
dbias sums that cancel, and sigmoid'(z) = s (1 - s) near s = 1 in float32; the kernel's error follows
the restatement's in each.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_hyper import _close as _gemm_close
from test_gpu_hyper import _p, _s
from test_gpu_hyper_train import HEAD_MAXIMA_BINDING, _drop_hash, _head_ladder, _keep  # noqa: F401

pytestmark = pytest.mark.gpu

SLOPE = float(np.float32(0.01))      # F.leaky_relu / nn.LeakyReLU default, as the kernels receive it
EPS = float(np.float32(1e-5))
SEED = 0x5DEE_CE66_D123


def _p32(p):
    return float(np.float32(p))


def _scale32(p):
    """Dropout's 1 / (1 - p) as the kernels form it (float32)."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


@pytest.fixture(scope="module")
def L():
    from dadmm_hip import _lib
    return _lib.load()


def _need(cond, what):
    if not cond:
        pytest.fail(f"inputs unsuitable: {what}")


def _need_form(kind, dims, **want):
    from dadmm_hip import hyper_form
    f = hyper_form(kind, *dims)
    _need(isinstance(f, dict), f"{kind}{dims} is refused ({f})")
    got = {k: f[k] for k in want}
    _need(got == want, f"{kind}{dims} takes {f}, not {want}")
    return f


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ahat(G, P, gen, dev):
    """D^-1/2 (Adj + I) D^-1/2 of G random symmetric graphs (edge probability 1/2). One shared graph
    of two nodes gets no edge: with one, both nodes of every sample carry the same M and every
    variance is 0 (the per-sample graphs of two nodes keep such samples)."""
    a = (torch.rand(G, P, P, generator=gen) < 0.5).float().triu(1)
    if G == 1 and P == 2:
        a = torch.zeros(1, 2, 2)
    a = a + a.transpose(1, 2) + torch.eye(P)
    d = a.sum(2).rsqrt()
    return (d[:, :, None] * a * d[:, None, :]).contiguous().to(dev)


def _bar(tag, got, ref):
    """The element bar. got: {name: tensor}; ref(dtype) -> {name: tensor} (float64 and float32)."""
    w64, w32 = ref(torch.float64), ref(torch.float32)
    for name, g in got.items():
        w = w64[name].double()
        top = float(w.abs().max())
        _need(top > 0, f"{tag} {name}: the reference is all zero")
        scale = float((w32[name].double() - w).abs().max()) / top
        r = max(2.0 ** -23, 4.0 * scale)
        err = (g.double() - w).abs()
        print(f"{tag} {name}: fp32 scale {scale:.3e}, kernel max err / max {float(err.max()) / top:.3e}")
        assert torch.isfinite(g).all(), f"{tag} {name}"
        bad = err > r * top + r * w.abs()
        assert not bad.any(), (f"{tag} {name}: {int(bad.sum())} entries over the bar, max err / max "
                               f"{float(err.max()) / top:.3e}, r {r:.3e}")


def _mask_preconditions(keep, p, what):
    if p > 0:
        _need(int((keep != 0).sum()) >= 32 and int((keep == 0).sum()) >= 32, f"{what}: dropout lanes")


# ---- dadmm_hyper_gcn_train ------------------------------------------------------------------------
# id -> ((B, P, K, N, K1), the form it must take)
GCN_FORMS = {
    "wr1-ntail": ((12, 5, 64, 68, 64), dict(wr=1, ks=1, dma=0, split=0, samples_per_tile=6)),
    "wr1-ks2": ((12, 5, 256, 100, 256), dict(wr=1, ks=2, dma=0, split=0)),
    "wr2": ((640, 8, 64, 384, 64), dict(wr=2, ks=1, dma=0, samples_per_tile=8)),
    "wr2-one-sample": ((3, 50, 64, 68, 64), dict(wr=2, ks=1, samples_per_tile=1)),
    "wr4": ((1230, 7, 64, 448, 64), dict(wr=4, ks=1, dma=0, samples_per_tile=18)),
    "wr5-partial-tile": ((2250, 5, 64, 448, 64), dict(wr=5, ks=1, dma=0, samples_per_tile=32, grid=71 * 7)),
    "wr5-dma": ((2250, 5, 512, 448, 512), dict(wr=5, ks=1, dma=1, samples_per_tile=32)),
    "split-input": ((12, 5, 128, 68, 64), dict(wr=1, ks=1, dma=0, split=1)),
    "P2": ((12, 2, 64, 68, 64), dict(wr=1, ks=1, samples_per_tile=16)),
    "P64": ((12, 64, 64, 68, 64), dict(wr=2, ks=1, samples_per_tile=1)),
    "P130-small-grid": ((3, 130, 64, 68, 64), dict(wr=5, ks=1, dma=0, samples_per_tile=1)),
}
# (drop_p, eval statistics); per-sample / shared A_hat alternate over them
GCN_MODES = [(0.0, False), (0.1, False), (0.5, False), (0.0, True), (0.1, True), (0.5, True)]


def _epilogue_ref(m_out, B, P, N, bw, bb, keep, p, run):
    """leaky_relu -> BatchNorm (the sample's P nodes, or the running statistics) -> Dropout of the
    kernel's own M, in `dtype`: {mean, var, y, y_undropped}."""
    def ref(dtype):
        t = F.leaky_relu(m_out.to(dtype), SLOPE).view(B, P, N)
        if run is not None:
            mean = run[0].to(dtype).expand(B, N)
            var = run[1].to(dtype).expand(B, N)
        else:   # the sums over the P nodes in node order, as the kernel runs them (a float32 sum's
            # rounding depends on its order: a pairwise one says little about 130 sequential terms)
            mean = torch.zeros(B, N, dtype=dtype, device=t.device)
            for q in range(P):
                mean = mean + t[:, q]
            mean = mean / P
            var = torch.zeros_like(mean)
            for q in range(P):
                var = var + (t[:, q] - mean) * (t[:, q] - mean)
            var = var / P
        u = (t - mean[:, None]) * torch.rsqrt(var[:, None] + EPS) * bw.to(dtype) + bb.to(dtype)
        y = u * keep.to(dtype).view(B, P, N) * (1.0 / (1.0 - p)) if p > 0 else u
        return dict(mean=mean, var=var, y=y.reshape(B * P, N), u=u.reshape(B * P, N))
    return ref


@pytest.mark.parametrize("mode", range(len(GCN_MODES)))
@pytest.mark.parametrize("form", list(GCN_FORMS))
def test_gcn_train(cuda, L, form, mode):
    (B, P, K, N, K1), want_form = GCN_FORMS[form]
    _need_form("gcn_train", (B, P, K, N, K1), **want_form)
    drop, bn_eval = GCN_MODES[mode]
    p = _p32(drop)
    per_sample = mode % 2 == 0
    rows, ldy, site = B * P, N + 4, 3
    gen = _gen(1000 * mode + B + P + K + N)
    x = torch.randn(rows, K, generator=gen)
    W = torch.randn(N, K, generator=gen) / np.sqrt(K)
    zc = [1, N - 2]                      # zero rows of W: one in the first column tile, one in the last
    W[zc] = 0.0
    bias, bb = torch.randn(N, generator=gen), torch.randn(N, generator=gen)
    bw = 1.0 + 0.1 * torch.randn(N, generator=gen)
    rm, rv = 0.3 * torch.randn(N, generator=gen), 0.5 + torch.rand(N, generator=gen)
    ahat = _ahat(B if per_sample else 1, P, gen, cuda)
    x, W, bias, bb, bw, rm, rv = (t.to(cuda) for t in (x, W, bias, bb, bw, rm, rv))
    if K1 < K:   # columns [0, K1) and [K1, K) from separate buffers with padded rows
        x1 = torch.full((rows, K1 + 4), 1e3, device=cuda)
        x2 = torch.full((rows, K - K1 + 8), 1e3, device=cuda)
        x1[:, :K1], x2[:, :K - K1] = x[:, :K1], x[:, K1:]
        xin = (_p(x1), K1 + 4, K1, _p(x2), K - K1 + 8)
    else:
        xin = (_p(x), K, K, None, 0)
    outs = []
    for _ in range(2):
        y = torch.full((rows, ldy), 7.0, device=cuda)
        m_out = torch.full((rows, N), 7.0, device=cuda)
        mean_out, var_out = torch.full((B, N), 7.0, device=cuda), torch.full((B, N), 7.0, device=cuda)
        rc = L.dadmm_hyper_gcn_train(B, P, K, N, *xin, _p(W), _p(bias), _p(ahat), int(per_sample), _p(bw),
                                     _p(bb), EPS, SLOPE, p, SEED, site, _p(y), ldy, _p(m_out), _p(mean_out),
                                     _p(var_out), _p(rm) if bn_eval else None, _p(rv) if bn_eval else None,
                                     _s())
        assert rc == 0, L.dadmm_last_error()
        outs.append((y, m_out, mean_out, var_out))
    for a_, b_ in zip(*outs):
        assert torch.equal(a_, b_)                                   # deterministic
    y, m_out, mean_out, var_out = outs[0]
    assert (y[:, N:] == 7.0).all()                                   # ldy > N: the pad columns survive
    y = y[:, :N]
    # M = A_hat (x W^T) + bias against float64
    m64 = (torch.matmul(ahat.double(), (x.double() @ W.double().t()).view(B, P, N)) + bias.double())
    _gemm_close(m_out, m64.reshape(rows, N), K)
    assert torch.equal(m_out[:, zc], bias[zc].expand(rows, 2))       # x 0 = 0, A_hat 0 = 0, + bias: exact
    # the epilogue on the kernel's own M
    keep = _keep(SEED, site, rows, N, p, cuda) if p > 0 else torch.ones(rows, N, device=cuda)
    ref = _epilogue_ref(m_out, B, P, N, bw, bb, keep, p, (rm, rv) if bn_eval else None)
    w = ref(torch.float64)
    _mask_preconditions(keep, p, form)
    _need(int((m_out > 0).sum()) >= 32 and int((m_out <= 0).sum()) >= 32, "leaky_relu sides")
    _need(bool((w["y"] != 0).any(1).all()), "a reference row is all zero")
    # the zero pattern is the mask, wherever the undropped value is not within rounding of zero (of
    # millions of lanes a few cancel to an exact float32 zero)
    nz = w["u"].abs() > 1e-4 * w["u"].abs().max()
    assert torch.equal((y == 0)[nz], (keep == 0)[nz])
    tag = f"gcn_train {form} p={drop} eval={int(bn_eval)}"
    if bn_eval:
        assert torch.equal(mean_out, rm.expand(B, N)) and torch.equal(var_out, rv.expand(B, N))
        _bar(tag, dict(y=y), lambda dt: dict(y=ref(dt)["y"]))
        return
    reg = torch.ones(N, dtype=torch.bool, device=cuda)
    reg[zc] = False
    for cols, name in ((reg, ""), (~reg, " zero-variance columns")):
        pick = lambda dt: {k: v[:, cols] for k, v in ref(dt).items() if k != "u"}   # noqa: E731
        got = dict(y=y[:, cols], mean=mean_out[:, cols])
        if name == "":
            got["var"] = var_out[:, cols]
        _bar(tag + name, got, pick)
    # the variance of P equal numbers t: the P - 1 additions and the division each round by 2^-24,
    # so |mean - t| <= P 2^-24 |t| and var <= (P 2^-24 t)^2; asserted with a factor 2 on the mean
    tb = F.leaky_relu(bias[zc], SLOPE)
    assert bool((var_out[:, zc] <= (P * 2.0 ** -23 * tb.abs()) ** 2).all())
    if P == 2:   # t + t and / 2 are exact: variance 0, output bn_bias / (1 - p) or 0
        assert bool((var_out[:, zc] == 0).all())
        exp = (bb[zc] * torch.tensor(_scale32(p) if p > 0 else 1.0, device=cuda)).expand(rows, 2)
        assert torch.equal(y[:, zc], torch.where(keep[:, zc] != 0, exp, torch.zeros_like(exp)))


# ---- dadmm_hyper_gcn_train_bwd and the fused dadmm_hyper_linear_gcn_bwd ---------------------------
def _gcn_bwd_ref(m, dy_of, mean_in, var_in, bw, ahat, keep, p, bn_eval, B, P, N):
    """float64 / float32 torch autograd of M = A_hat Z + bias -> leaky_relu -> BatchNorm -> Dropout
    with respect to Z and the per-sample gamma, beta, bias; mean and var are functions of M unless
    bn_eval. dy_of(dtype) -> dy."""
    def ref(dtype):
        Z = torch.zeros(B, P, N, dtype=dtype, device=m.device, requires_grad=True)
        bs = torch.zeros(B, 1, N, dtype=dtype, device=m.device, requires_grad=True)
        gam = bw.to(dtype).expand(B, 1, N).clone().requires_grad_(True)
        bet = torch.zeros(B, 1, N, dtype=dtype, device=m.device, requires_grad=True)
        M = torch.matmul(ahat.to(dtype), Z) + bs + m.to(dtype).view(B, P, N)   # its value is m
        t = F.leaky_relu(M, SLOPE)
        if bn_eval:
            mean, var = mean_in.to(dtype)[:, None], var_in.to(dtype)[:, None]
        else:
            mean, var = t.mean(1, keepdim=True), t.var(1, unbiased=False, keepdim=True)
        y = (t - mean) * torch.rsqrt(var + EPS) * gam + bet
        if p > 0:
            y = y * keep.to(dtype).view(B, P, N) * (1.0 / (1.0 - p))
        (y * dy_of(dtype).view(B, P, N)).sum().backward()
        return dict(dz=Z.grad.reshape(B * P, N), dgamma=gam.grad[:, 0], dbeta=bet.grad[:, 0], dbias=bs.grad[:, 0])
    return ref


def _gcn_bwd_inputs(B, P, N, bn_eval, per_sample, gen, dev):
    rows = B * P
    m = torch.randn(rows, N, generator=gen)
    idx = torch.randperm(rows * N, generator=gen)[:128]
    m.view(-1)[idx[:64]] = 0.0                 # leaky_relu'(+-0) = slope, as torch's
    m.view(-1)[idx[64:]] = -0.0
    bw = 1.0 + 0.1 * torch.randn(N, generator=gen)
    if bn_eval:
        mean, var = 0.3 * torch.randn(B, N, generator=gen), 0.5 + torch.rand(B, N, generator=gen)
    else:   # the forward's saved statistics
        t = F.leaky_relu(m, SLOPE).view(B, P, N)
        mean, var = t.mean(1), t.var(1, unbiased=False)
    ahat = _ahat(B if per_sample else 1, P, gen, dev)
    return m.to(dev), mean.contiguous().to(dev), var.contiguous().to(dev), bw.to(dev), ahat


def _parts(part):
    return dict(dgamma=part[0], dbeta=part[1], dbias=part[2])


GCN_BWD_SHAPES = {   # (B, P, N) -> (NT, PR)
    (12, 5, 68): (256, 8), (5, 9, 68): (256, 0), (2048, 2, 64): (64, 8), (1024, 9, 128): (64, 0),
    (12, 8, 68): (256, 8), (3, 64, 68): (256, 0),
}


@pytest.mark.parametrize("drop", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("bn_eval", [0, 1])
@pytest.mark.parametrize("shape", list(GCN_BWD_SHAPES))
def test_gcn_train_bwd(cuda, L, shape, bn_eval, drop):
    B, P, N = shape
    nt, pr = GCN_BWD_SHAPES[shape]
    _need_form("gcn_bwd", (B, P, 4, N), nt=nt, pr=pr)
    p, site, rows = _p32(drop), 2, B * P
    per_sample = (bn_eval + int(drop * 10)) % 2 == 0
    gen = _gen(B + 7 * P + N + 100 * bn_eval + int(1000 * drop))
    m, mean, var, bw, ahat = _gcn_bwd_inputs(B, P, N, bn_eval, per_sample, gen, cuda)
    dy = torch.randn(rows, N, generator=gen).to(cuda)
    assert int((m == 0).sum()) >= 128 and int(torch.signbit(m[m == 0]).sum()) >= 64
    outs = []
    for _ in range(2):
        dz = torch.full((rows, N), 7.0, device=cuda)
        part = torch.full((3, B, N), 7.0, device=cuda)
        rc = L.dadmm_hyper_gcn_train_bwd(B, P, N, _p(dy), _p(m), _p(mean), _p(var), _p(bw), EPS, _p(ahat),
                                         int(per_sample), SLOPE, p, SEED, site, _p(dz), _p(part), bn_eval, _s())
        assert rc == 0, L.dadmm_last_error()
        outs.append((dz, part))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    dz, part = outs[0]
    keep = _keep(SEED, site, rows, N, p, cuda) if p > 0 else torch.ones(rows, N, device=cuda)
    _mask_preconditions(keep, p, str(shape))
    _need(int((m > 0).sum()) >= 32 and int((m < 0).sum()) >= 32, "leaky_relu sides")
    ref = _gcn_bwd_ref(m, lambda dt: dy.to(dt), mean, var, bw, ahat, keep, p, bn_eval, B, P, N)
    _need(bool((ref(torch.float64)["dz"] != 0).any(1).all()), "a reference row is all zero")
    _bar(f"gcn_train_bwd {shape} nt={nt} pr={pr} eval={bn_eval} p={drop}", dict(dz=dz, **_parts(part)), ref)


BWD_FORMS = {   # (B, P, K, N): K = the GEMM's depth (the layer above's width), N = this layer's width
    "wr1-ntail": ((12, 5, 64, 68), dict(wr=1, ks=1, dma=0, samples_per_tile=6)),
    # 8 k-steps on a small grid, where the GCN-class GEMMs split K over two wave sets: the C ABI's
    # fused launch must not (dadmm_hyper_linear, its promised pair, never does)
    "wr1-k128": ((12, 5, 128, 68), dict(wr=1, ks=1, dma=0)),
    "wr2": ((640, 8, 64, 384), dict(wr=2, ks=1, dma=0, samples_per_tile=8)),
    "wr2-one-sample": ((3, 50, 64, 68), dict(wr=2, ks=1, samples_per_tile=1)),
    "wr4": ((1230, 7, 64, 448), dict(wr=4, ks=1, dma=0, samples_per_tile=18)),
    "wr5-partial-tile": ((2250, 5, 64, 448), dict(wr=5, ks=1, dma=0, samples_per_tile=32)),
    "wr5-dma": ((2250, 5, 512, 448), dict(wr=5, ks=1, dma=1, samples_per_tile=32)),
    "P2": ((12, 2, 64, 68), dict(wr=1, ks=1, samples_per_tile=16)),
    "P64": ((12, 64, 64, 68), dict(wr=2, ks=1, samples_per_tile=1)),
}


@pytest.mark.parametrize("cfg", [(0.1, 0, True), (0.5, 1, False), (0.0, 0, False)])
@pytest.mark.parametrize("form", list(BWD_FORMS))
def test_linear_gcn_bwd(cuda, L, form, cfg):
    """The fused launch == dadmm_hyper_linear then dadmm_hyper_gcn_train_bwd, bit for bit (the
    header's promise), and the pair against float64 once per form."""
    (B, P, K, N), want_form = BWD_FORMS[form]
    _need_form("linear_gcn_bwd", (B, P, K, N), **want_form)
    drop, bn_eval, per_sample = cfg
    p, site, rows = _p32(drop), 1, B * P
    gen = _gen(B + 3 * P + K + N + int(100 * drop))
    m, mean, var, bw, ahat = _gcn_bwd_inputs(B, P, N, bn_eval, per_sample, gen, cuda)
    x = torch.randn(rows, K, generator=gen).to(cuda)
    W = (torch.randn(N, K, generator=gen) / np.sqrt(K)).to(cuda)
    dz, part = torch.full((rows, N), 7.0, device=cuda), torch.full((3, B, N), 7.0, device=cuda)
    rc = L.dadmm_hyper_linear_gcn_bwd(B, P, K, N, _p(x), K, _p(W), _p(m), _p(mean), _p(var), _p(bw), EPS,
                                      _p(ahat), int(per_sample), SLOPE, p, SEED, site, _p(dz), _p(part), bn_eval,
                                      _s())
    assert rc == 0, L.dadmm_last_error()
    dy = torch.empty(rows, N, device=cuda)
    assert L.dadmm_hyper_linear(rows, K, N, _p(x), K, K, None, 0, _p(W), None, _p(dy), N, _s()) == 0
    dz2, part2 = torch.full((rows, N), 7.0, device=cuda), torch.full((3, B, N), 7.0, device=cuda)
    rc = L.dadmm_hyper_gcn_train_bwd(B, P, N, _p(dy), _p(m), _p(mean), _p(var), _p(bw), EPS, _p(ahat),
                                     int(per_sample), SLOPE, p, SEED, site, _p(dz2), _p(part2), bn_eval, _s())
    assert rc == 0, L.dadmm_last_error()
    same = torch.equal(dz, dz2) and torch.equal(part, part2)
    print(f"linear_gcn_bwd {form} cfg={cfg}: fused vs pair max |diff| dz {float((dz - dz2).abs().max()):.3e} "
          f"part {float((part - part2).abs().max()):.3e}")
    assert same, "the fused launch and the pair of launches differ"
    if cfg[1] == 0 and cfg[0] > 0:   # against float64, once per form
        keep = _keep(SEED, site, rows, N, p, cuda)
        _mask_preconditions(keep, p, form)
        ref = _gcn_bwd_ref(m, lambda dt: x.to(dt) @ W.to(dt).t(), mean, var, bw, ahat, keep, p, bn_eval, B, P, N)
        _bar(f"linear_gcn_bwd {form}", dict(dz=dz, **_parts(part)), ref)


# ---- dadmm_hyper_rownorm_bwd ----------------------------------------------------------------------
# both sides of every CH boundary (C = 256, 512, 1024) and of the 8-row partial block; the sizes
# whose lanes cannot populate the preconditions (C = 4 at 37 rows and dropout) run at more rows
ROWNORM_SHAPES = ([(C, 37) for C in (4, 36, 256, 260, 512, 516, 1024, 1028, 2048)] + [(4, 1001)] +
                  [(C, r) for C in (260, 1028) for r in (7, 8, 9)] + [(1028, 1), (2048, 1)])
# (dropout needs the lanes for 32 dropped ones at p = 0.1: C = 4 has them at 1001 rows, not at 37)
ROWNORM_CASES = [(C, r, act, drop) for C, r in ROWNORM_SHAPES for act in (0, 1) for drop in (0.0, 0.1)
                 if drop == 0.0 or r * C >= 640]


@pytest.mark.parametrize("C,rows,act,drop", ROWNORM_CASES)
def test_rownorm_bwd(cuda, L, C, rows, act, drop):
    p, site = _p32(drop), 5
    gen = _gen(C + 13 * rows + act + int(100 * drop))
    keep = _keep(SEED, site, rows, C, p, cuda) if p > 0 else torch.ones(rows, C, device=cuda)
    xd = (torch.randn(rows, C, generator=gen).to(cuda) * keep * (_scale32(p) if p > 0 else 1.0)).contiguous()
    dy = torch.randn(rows, C, generator=gen).to(cuda)
    w = (1.0 + 0.1 * torch.randn(C, generator=gen)).to(cuda)
    b = (0.1 * torch.randn(C, generator=gen)).to(cuda)
    nblk = (rows + 7) // 8
    assert L.dadmm_hyper_rownorm_bwd_part_bytes(rows, C) == 4 * nblk * 2 * C
    outs = []
    for _ in range(2):
        dx = torch.full((rows + 8, C), 7.0, device=cuda)            # guard rows past the last one
        part = torch.full((nblk + 1, 2, C), 7.0, device=cuda)
        rc = L.dadmm_hyper_rownorm_bwd(rows, C, _p(dy), _p(xd), _p(w), _p(b), EPS, act, SLOPE, p, SEED, site,
                                       _p(dx), _p(part), _s())
        assert rc == 0, L.dadmm_last_error()
        outs.append((dx, part))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    dx, part = outs[0]
    assert (dx[rows:] == 7.0).all() and (part[nblk] == 7.0).all()
    dx, part = dx[:rows], part[:nblk]

    def ref(dtype):
        v = xd.to(dtype).requires_grad_(True)                       # the LayerNorm input (post-dropout)
        wv = w.to(dtype).expand(rows, C).clone().requires_grad_(True)
        bv = b.to(dtype).expand(rows, C).clone().requires_grad_(True)
        xh = (v - v.mean(1, keepdim=True)) * torch.rsqrt(v.var(1, unbiased=False, keepdim=True) + EPS)
        t = xh * wv + bv
        y = F.leaky_relu(t, SLOPE) if act else t
        (y * dy.to(dtype)).sum().backward()
        g = v.grad * keep.to(dtype) * (1.0 / (1.0 - p)) if p > 0 else v.grad   # Dropout's derivative
        pad = nblk * 8 - rows
        blk = lambda z: F.pad(z, (0, 0, 0, pad)).view(nblk, 8, C).sum(1)       # noqa: E731
        return dict(dx=g, dweight=blk(wv.grad), dbias=blk(bv.grad), t=t.detach(), gv=v.grad)
    w64 = ref(torch.float64)
    _mask_preconditions(keep, p, f"C={C} rows={rows}")
    if act and rows * C >= 128:
        _need(int((w64["t"] > 0).sum()) >= 32 and int((w64["t"] < 0).sum()) >= 32, "LeakyReLU sides")
    _need(bool((w64["dx"] != 0).any(1).all()), "a reference row is all zero")
    nz = w64["gv"].abs() > 1e-4 * w64["gv"].abs().max()              # the zero pattern is the mask
    assert torch.equal((dx == 0)[nz], (keep == 0)[nz])
    _bar(f"rownorm_bwd C={C} rows={rows} act={act} p={drop}",
         dict(dx=dx, dweight=part[:, 0], dbias=part[:, 1]),
         lambda dt: {k: v for k, v in ref(dt).items() if k not in ("t", "gv")})


# ---- dadmm_hyper_linear_ln_train ------------------------------------------------------------------
@pytest.mark.parametrize("drop", [0.0, 0.1])
@pytest.mark.parametrize("rows,K,N,what", [(37, 36, 100, ""), (5, 200, 8, ""), (64, 1024, 400, "split-k"),
                                          (2064, 448, 224, ""), (15400, 64, 256, "wr4")])
def test_linear_ln_train(cuda, L, rows, K, N, what, drop):
    nb = L.dadmm_hyper_linear_ln_scratch_bytes(rows, K, N)
    splits = nb // (4 * rows * N)
    _need(nb == 4 * splits * rows * N and splits >= 1, "scratch bytes")
    if what == "split-k":
        _need(splits > 1, f"{rows}x{K}x{N} does not split K")
    elif what == "wr4":    # unsplit, the block's GEMM plans as the plain linear: 128-row tiles
        _need(splits == 1, "splits K")
        _need_form("linear", (rows, 1, K, N), wr=4, ks=1)
    p, site = _p32(drop), 6
    gen = _gen(rows + K + N + int(100 * drop))
    x = torch.randn(rows, K, generator=gen).to(cuda)
    W = (torch.randn(N, K, generator=gen) / np.sqrt(K)).to(cuda)
    bias = torch.randn(N, generator=gen).to(cuda)
    lw = (1.0 + 0.1 * torch.randn(N, generator=gen)).to(cuda)
    lb = (0.1 * torch.randn(N, generator=gen)).to(cuda)
    scratch = torch.empty(nb // 4 + 4, device=cuda)
    outs = []
    for _ in range(2):
        y, xd = torch.full((rows, N), 7.0, device=cuda), torch.full((rows, N), 7.0, device=cuda)
        rc = L.dadmm_hyper_linear_ln_train(rows, K, N, _p(x), K, _p(W), _p(bias), _p(lw), _p(lb), EPS, 1, SLOPE,
                                           p, SEED, site, _p(y), _p(xd), _p(scratch), _s())
        assert rc == 0, L.dadmm_last_error()
        outs.append((y, xd))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    y, xd = outs[0]
    keep = _keep(SEED, site, rows, N, p, cuda) if p > 0 else torch.ones(rows, N, device=cuda)
    if rows * N >= 640:
        _mask_preconditions(keep, p, f"{rows}x{N}")
    lin = x.double() @ W.double().t() + bias.double()
    want_xd = lin * keep.double() * (1.0 / (1.0 - p)) if p > 0 else lin
    _gemm_close(xd, want_xd, K)
    nz = lin.abs() > 1e-4 * lin.abs().max()                          # the zero pattern is the mask
    assert torch.equal((xd == 0)[nz], (keep == 0)[nz])

    def ref(dtype):
        t = F.layer_norm(xd.to(dtype), (N,), lw.to(dtype), lb.to(dtype), EPS)
        return dict(y=F.leaky_relu(t, SLOPE), t=t)
    t64 = ref(torch.float64)["t"]
    if rows * N >= 128:
        _need(int((t64 > 0).sum()) >= 32 and int((t64 < 0).sum()) >= 32, "LeakyReLU sides")
    _need(bool((t64 != 0).any(1).all()), "a reference row is all zero")
    _bar(f"linear_ln_train {rows}x{K}x{N} p={drop}", dict(y=y), lambda dt: dict(y=ref(dt)["y"]))


# ---- dadmm_hyper_bn_running_update ----------------------------------------------------------------
@pytest.mark.parametrize("widths,iters,B,P,tracked", [
    ((4,), 1, 1, 2, False), ((100,), 3, 63, 5, True), ((65, 400, 4, 64, 100), 1, 64, 5, True),
    ((4, 64, 65, 100, 400, 64, 4, 65), 3, 65, 2, True), ((400, 65, 4, 100, 64), 3, 130, 5, False),
    ((64,), 1, 130, 2, True), ((65, 100, 400, 4, 64, 100, 65, 4), 1, 63, 5, False),
    ((100, 4, 65, 64, 400), 3, 64, 2, True)])
def test_bn_running_update(cuda, L, widths, iters, B, P, tracked):
    """r <- (1 - mu) r + mu s_t over the T = iters B calls in order (float64), the variance unbiased
    by P / (P - 1); the split count T / 64 changes across B = 63, 64, 65, 130."""
    nl, T, mu = len(widths), iters * B, 0.1
    gen = _gen(sum(widths) + iters + B + P)
    offs, o = [], 0
    for wd in widths:                       # per iteration block: layer i's mean, then its var
        offs.append((o, o + B * wd))
        o += 2 * B * wd
    stride = o + 24                         # block_stride > B * width: a gap between the iterations
    arena = torch.randn(iters, stride, generator=gen)
    for (om, ov), wd in zip(offs, widths):
        arena[:, ov:ov + B * wd] = arena[:, ov:ov + B * wd].abs() + 0.1
    r0m = [torch.randn(wd, generator=gen) for wd in widths]
    r0v = [torch.rand(wd, generator=gen) + 0.5 for wd in widths]
    arena_d = arena.to(cuda)
    rm, rv = [t.to(cuda) for t in r0m], [t.to(cuda) for t in r0v]
    trk = [torch.full((1,), 11 + i, dtype=torch.int64, device=cuda) for i in range(nl)]
    wts = (mu * (1.0 - mu) ** torch.arange(T - 1, -1, -1, dtype=torch.float64)).to(cuda)
    cw = (ctypes.c_int32 * nl)(*widths)
    vp = ctypes.c_void_p * nl
    nb = L.dadmm_hyper_bn_running_scratch_bytes(nl, cw, iters, B)
    assert nb == 8 * 2 * sum(widths) * max(1, min(256, T // 64))
    scratch = torch.empty(nb // 8 + 2, dtype=torch.float64, device=cuda)
    base = arena_d.data_ptr()
    rc = L.dadmm_hyper_bn_running_update(
        nl, cw, vp(*[t.data_ptr() for t in rm]), vp(*[t.data_ptr() for t in rv]),
        vp(*[t.data_ptr() for t in trk]) if tracked else None,
        vp(*[base + 4 * om for om, _ in offs]), vp(*[base + 4 * ov for _, ov in offs]),
        stride, iters, B, P, _p(wts), (1.0 - mu) ** T, _p(scratch), _s())
    assert rc == 0, L.dadmm_last_error()
    torch.cuda.synchronize()
    a64 = arena.double().numpy()
    for i, ((om, ov), wd) in enumerate(zip(offs, widths)):
        m = a64[:, om:om + B * wd].reshape(T, wd)
        v = a64[:, ov:ov + B * wd].reshape(T, wd) * (P / (P - 1))
        wm, wv = r0m[i].double().numpy(), r0v[i].double().numpy()
        for t in range(T):                  # the reference's sequential calls
            wm = (1.0 - mu) * wm + mu * m[t]
            wv = (1.0 - mu) * wv + mu * v[t]
        for got, want, name in ((rm[i], wm, "mean"), (rv[i], wv, "var")):
            w32 = want.astype(np.float32)
            ulp = np.spacing(np.abs(w32))
            err = np.abs(got.cpu().numpy().astype(np.float64) - w32.astype(np.float64))
            assert (err <= ulp).all(), f"layer {i} running_{name}: max err / ulp {float((err / ulp).max())}"
        assert int(trk[i]) == 11 + i + (T if tracked else 0)


# ---- the head where its clamps bind ---------------------------------------------------------------
LADDER = (6.0, 12.0, 50.0, 89.0, 100.0)     # +-: 89 and 100 overflow expf / reach torch's denormal sigmoid
MAXIMA = {"default": (0.1, 0.99, 0.99, 0.99), "binding": HEAD_MAXIMA_BINDING}
S_LO, S_HI, V_HI = 1e-4, 0.9999, 0.9999


def _near_bound(z64, H, maxv):
    """Lanes whose sigmoid, or scaled value, is within 1e-3 (relative) of a clamp bound; the upper
    bound of s measured on 1 - s = sigmoid(-z) against 1e-4 (every s above 0.9999 is within 1e-4 of it)."""
    s = torch.sigmoid(z64)
    near = ((s / S_LO - 1).abs() < 1e-3) | ((torch.sigmoid(-z64) / (1.0 - S_HI) - 1).abs() < 1e-3)
    ch = (torch.arange(z64.shape[1]) // H).expand_as(z64)
    for c in (1, 2, 3):
        if maxv[c] != 1.0:
            v = torch.clamp(s, S_LO, S_HI) * maxv[c]
            near |= (ch == c) & ((v / V_HI - 1).abs() < 1e-3)
    return near


def _ladder_logits(B, H, maxv, gen):
    """[B][4H] logits: 3 randn, and in every row one lane (two at H >= 2) of every channel planted on
    the ladder +-6, +-12, +-50, +-89, +-100, the rungs rotating over rows and channels; lanes within
    1e-3 of a bound are redrawn."""
    z = 3.0 * torch.randn(B, 4 * H, generator=gen)
    rungs = torch.tensor([sg * v for v in LADDER for sg in (1.0, -1.0)])
    rows = torch.arange(B)
    for c in range(4):
        for k in range(2 if H >= 2 else 1):
            z[rows, c * H + (rows + k) % H] = rungs[(rows + 3 * c + 5 * k) % len(rungs)]
    for _ in range(20):
        near = _near_bound(z.double(), H, maxv)
        if not near.any():
            break
        z[near] = 3.0 * torch.randn(int(near.sum()), generator=gen)
    _need(not _near_bound(z.double(), H, maxv).any(), "a logit on a clamp bound")
    return z


def _head_ref(z_of, dhyp, B, H, maxv):
    """float64 / float32 autograd of the literal sigmoid -> clamp -> x max -> clamp(max=0.9999)."""
    def ref(dtype):
        z = z_of(dtype).detach().requires_grad_(True)
        h = torch.clamp(torch.sigmoid(z), min=S_LO, max=S_HI).view(B, 4, H)
        hyp = torch.stack([h[:, 0] * maxv[0]] + [torch.clamp(h[:, c] * maxv[c], max=V_HI) for c in (1, 2, 3)], 1)
        hyp = hyp.reshape(B, 4 * H)
        (hyp * dhyp.to(dtype)).sum().backward()
        return dict(hyp=hyp.detach(), dz=z.grad)
    return ref


def _clamp_classes(z64, H, maxv, which):
    """The head precondition: every class of each clamp holds >= min(32, lanes / 16) lanes."""
    s = torch.sigmoid(z64)
    need = min(32, z64.numel() // 16)
    for name, cls in (("s < 1e-4", s < S_LO), ("s inside", (s >= S_LO) & (s <= S_HI)), ("s > 0.9999", s > S_HI)):
        _need(int(cls.sum()) >= max(need, 1), f"clamp 1 class {name}: {int(cls.sum())} lanes")
    if which == "binding":
        ch = (torch.arange(z64.shape[1], device=z64.device) // H).expand_as(z64)
        mx = torch.tensor(maxv, dtype=torch.float64, device=z64.device)[ch]
        v = torch.clamp(s, S_LO, S_HI) * mx
        hot = ch > 0
        for name, cls in (("v < 0.9999", v < V_HI), ("v on 0.9999", v == V_HI), ("v > 0.9999", v > V_HI)):
            _need(int((cls & hot).sum()) >= max(need, 1), f"clamp 2 class {name}: {int((cls & hot).sum())} lanes")


def _saturated_exact(z, hyp, dz, H, maxv):
    """On the +-89 and +-100 lanes (expf overflows, sigmoid is 0 or 1 in float32): the clamped value
    as float32 arithmetic gives it, and a zero gradient."""
    ch = (torch.arange(z.shape[1], device=z.device) // H).expand_as(z)
    mx = torch.tensor(maxv, dtype=torch.float32, device=z.device)[ch]
    for sg, bound in ((-1.0, np.float32(S_LO)), (1.0, np.float32(S_HI))):
        lanes = (z == sg * 89.0) | (z == sg * 100.0)
        _need(bool(lanes.any()), "no saturated lane")
        v = torch.tensor(bound, device=z.device) * mx
        v = torch.where(ch > 0, torch.clamp(v, max=float(np.float32(V_HI))), v)
        assert torch.equal(hyp[lanes], v[lanes])
        if dz is not None:
            assert bool((dz[lanes] == 0).all())


@pytest.mark.parametrize("which", list(MAXIMA))
@pytest.mark.parametrize("B,H", [(64, 5), (7, 1), (300, 16)])
def test_head_act_clamps(cuda, L, B, H, which):
    maxv = MAXIMA[which]
    gen = _gen(B + H + len(which))
    z = _ladder_logits(B, H, maxv, gen).to(cuda)
    dhyp = torch.randn(B, 4 * H, generator=gen).to(cuda)
    dhyp[dhyp == 0] = 1.0
    _clamp_classes(z.double(), H, maxv, which)
    hyp, dz = torch.full_like(z, 7.0), torch.full_like(z, 7.0)
    assert L.dadmm_hyper_head_act(0, B, H, _p(z), None, *maxv, _p(hyp), _s()) == 0, L.dadmm_last_error()
    assert L.dadmm_hyper_head_act(1, B, H, _p(z), _p(dhyp), *maxv, _p(dz), _s()) == 0, L.dadmm_last_error()
    ref = _head_ref(lambda dt: z.to(dt), dhyp, B, H, maxv)
    w = ref(torch.float64)
    assert torch.equal(dz == 0, w["dz"] == 0), \
        f"zero-gradient lanes differ on {int(((dz == 0) != (w['dz'] == 0)).sum())} lanes"
    _saturated_exact(z, hyp, dz, H, maxv)
    _bar(f"head_act B={B} H={H} maxima={which}", dict(hyp=hyp, dz=dz), ref)


@pytest.mark.parametrize("which", list(MAXIMA))
@pytest.mark.parametrize("B,K,H", [(64, 36, 5), (7, 36, 1), (300, 36, 16)])
def test_head_train_and_head_clamps(cuda, L, B, K, H, which):
    """dadmm_hyper_head_train and dadmm_hyper_head on the ladder: a bias ladder on a small x W^T.
    hyp of head_train == dadmm_hyper_linear then head_act mode 0, bit for bit."""
    maxv = MAXIMA[which]
    gen = _gen(B + K + H + len(which))
    x = torch.randn(B, K, generator=gen)
    W = 0.01 * torch.randn(4 * H, K, generator=gen) / np.sqrt(K)
    bias = _head_ladder(H)     # every class of both clamps, from H = 1 on
    z64 = x.double() @ W.double().t() + bias.double()
    _need(not _near_bound(z64, H, maxv).any(), "a logit on a clamp bound")
    x, W, bias = x.to(cuda), W.to(cuda), bias.to(cuda)
    z, hyp = torch.full((B, 4 * H), 7.0, device=cuda), torch.full((B, 4 * H), 7.0, device=cuda)
    rc = L.dadmm_hyper_head_train(B, K, H, _p(x), K, _p(W), _p(bias), *maxv, _p(z), _p(hyp), _s())
    assert rc == 0, L.dadmm_last_error()
    hyp_inf = torch.full((B, 4 * H), 7.0, device=cuda)
    rc = L.dadmm_hyper_head(B, K, H, _p(x), K, _p(W), _p(bias), *maxv, _p(hyp_inf), _s())
    assert rc == 0, L.dadmm_last_error()
    z_lin, hyp_pair = torch.empty(B, 4 * H, device=cuda), torch.empty(B, 4 * H, device=cuda)
    assert L.dadmm_hyper_linear(B, K, 4 * H, _p(x), K, K, None, 0, _p(W), _p(bias), _p(z_lin), 4 * H, _s()) == 0
    assert L.dadmm_hyper_head_act(0, B, H, _p(z_lin), None, *maxv, _p(hyp_pair), _s()) == 0
    assert torch.equal(hyp, hyp_pair)
    assert torch.equal(hyp_inf, hyp)
    _gemm_close(z, z64.to(cuda), K)
    # the head of the kernel's own logits, and its backward through head_act on them
    dhyp = torch.randn(B, 4 * H, generator=gen).to(cuda)
    dhyp[dhyp == 0] = 1.0
    dz = torch.full_like(z, 7.0)
    assert L.dadmm_hyper_head_act(1, B, H, _p(z), _p(dhyp), *maxv, _p(dz), _s()) == 0
    _need(not _near_bound(z.double().cpu(), H, maxv).any(), "a kernel logit on a clamp bound")
    ref = _head_ref(lambda dt: z.to(dt), dhyp, B, H, maxv)
    w = ref(torch.float64)
    assert torch.equal(dz == 0, w["dz"] == 0)
    _clamp_classes(z.double(), H, maxv, which)
    _bar(f"head_train B={B} H={H} maxima={which}", dict(hyp=hyp, dz=dz), ref)
