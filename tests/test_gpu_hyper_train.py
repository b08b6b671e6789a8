"""GPU: the training-mode hypernetwork on the HIP kernels (hyper_ops.HyperTrainFn:
dadmm_hyper_gcn_train / _linear_ln_train / _head_act forward, dadmm_hyper_gcn_train_bwd /
_rownorm_bwd / _head_act backward, dadmm_hyper_wgrad and the transposed-weight linear for the linears' weight / input GEMMs).

Bar: against a plain torch fp32 autograd reference of the same modules in train mode
(gnn_dlasso_models_progressive.py:52-72 GCNConv -> leaky_relu -> BatchNorm1d on the sample's P
nodes -> Dropout, LayerNorm, the decoder's Linear -> Dropout -> LayerNorm -> LeakyReLU blocks, fc,
sigmoid, clamps, maxima :165-196) given the SAME dropout masks — regenerated here from the
kernels' counter-based stream (a numpy restatement of drop_hash, test infrastructure) — within
f32 rounding of the different summation orders: hyp, d(AtAy) and every parameter gradient, and
the BatchNorm running statistics after the update. Model level: a train-mode forward + loss +
backward of DLASSO_GNNHyp3_Progressive runs on the HIP hypernetwork, and with dropout off it
matches the torch backend's loss and gradients.
"""
import argparse

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle as O

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


def _drop_hash(seed, site, rows, cols):
    """numpy restatement of drop_hash (csrc/dadmm_internal.h) over a rows x cols grid."""
    r = np.arange(rows, dtype=np.uint64)[:, None]
    c = np.arange(cols, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        z = np.uint64(seed) ^ (np.uint64(site) << np.uint64(56)) ^ (r << np.uint64(20)) ^ c
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint64)


def _keep(seed, site, rows, cols, p, dev):
    thr = np.uint64(min(int(p * 4294967296.0), 0xFFFFFFFF))
    return torch.from_numpy((_drop_hash(seed, site, rows, cols) >= thr).astype(np.float32)).to(dev)


# A bias ladder for the head's fc: logits far inside and far outside [-9.2, 9.2] (where the
# clamp(1e-4, 0.9999) binds), at +-89 and +-100 (expf overflows, sigmoid is 0 or 1 in float32). Output
# i of channel c sits on HEAD_RUNGS[(c + 4 i + i // 4) % 16], so that one row per channel (H = 1)
# already meets every class of both clamps under the maxima HEAD_MAXIMA_BINDING, whose second clamp
# (<= 0.9999) binds for tau and eta and sits exactly on its bound for rho.
HEAD_RUNGS = (-100.0, 100.0, 89.0, -1.3, 12.0, -12.0, 0.4, -89.0, 50.0, -50.0, 6.0, -6.0, 1.7, -0.6, 2.5, -3.0)
HEAD_MAXIMA_BINDING = (0.1, 1.5, 1.0, 2.0)


def _head_ladder(H):
    return torch.tensor([HEAD_RUNGS[(c + 4 * i + i // 4) % 16] for c in range(4) for i in range(H)])


def _model(dev, P, n, hidden, mode, seed=0, B=64, maxima=(0.1, 0.99, 0.99, 0.99)):
    import gnn_dlasso_models_progressive as G
    A, b, _ = O.make_problem(P, 16, n, max(B, 64), seed=seed + 5)
    torch.manual_seed(seed)
    args = argparse.Namespace(GHN_iter_num=3, GHyp_hidden=hidden, DADMM_mode=mode, alpha_max=maxima[0],
                              tau_max=maxima[1], rho_max=maxima[2], eta_max=maxima[3])
    model = G.DLASSO_GNNHyp3_Progressive(torch.from_numpy(A)[None].to(dev), args).to(dev)
    with torch.no_grad():
        for i in range(1, 6):
            bn = getattr(model.encoder, f"bn{i}")
            bn.running_mean.normal_(0, 0.3)
            bn.running_var.uniform_(0.5, 2.0)
            bn.weight.normal_(1, 0.1)
            bn.bias.normal_(0, 0.1)
    return model.train(), A, b


def _torch_reference(model, AtAy, Atb, n, ahat, seed, train=True):
    """The reference's train-mode hypernetwork with explicit masks (torch autograd); train=False:
    its eval mode (BatchNorm on the running statistics, no dropout)."""
    B, P, _ = AtAy.shape
    enc = model.encoder
    x = torch.cat([AtAy[..., :n], Atb[..., :n]], dim=2)
    for i, (conv, bn) in enumerate(zip((enc.conv1, enc.conv2, enc.conv3, enc.conv4, enc.conv5),
                                       (enc.bn1, enc.bn2, enc.bn3, enc.bn4, enc.bn5))):
        m = torch.matmul(ahat, x @ conv.lin.weight.t()) + conv.bias
        t = F.leaky_relu(m, 0.01)
        if train:
            mean = t.mean(dim=1, keepdim=True)
            var = t.var(dim=1, unbiased=False, keepdim=True)
        else:
            mean, var = bn.running_mean, bn.running_var
        xn = (t - mean) * torch.rsqrt(var + bn.eps) * bn.weight + bn.bias
        if i < 4 and train:
            p = enc.dropout.p
            xn = xn * _keep(seed, i, B * P, xn.shape[2], p, x.device).view(B, P, -1) * (1.0 / (1.0 - p))
        x = xn
    x = F.layer_norm(x, (x.shape[-1],), enc.norm.weight, enc.norm.bias, enc.norm.eps).reshape(B, -1)
    for blk in range(3):
        lin, ln = model.decoder[4 * blk], model.decoder[4 * blk + 2]
        p = model.decoder[4 * blk + 1].p
        v = F.linear(x, lin.weight, lin.bias)
        if train:
            v = v * _keep(seed, 4 + blk, B, v.shape[1], p, x.device) * (1.0 / (1.0 - p))
        x = F.leaky_relu(F.layer_norm(v, (v.shape[1],), ln.weight, ln.bias, ln.eps),
                         model.decoder[4 * blk + 3].negative_slope)
    h = torch.clamp(torch.sigmoid(model.fc(x)), min=1e-4, max=0.9999)
    H = model.fc.out_features // 4
    h = h.view(B, 4, H)
    return torch.stack([h[:, 0] * float(model.alpha_max),
                        torch.clamp(h[:, 1] * float(model.tau_max), max=0.9999),
                        torch.clamp(h[:, 2] * float(model.rho_max), max=0.9999),
                        torch.clamp(h[:, 3] * float(model.eta_max), max=0.9999)], dim=1)


def _close(got, want, rel=2e-4, name=""):
    got, want = got.double(), want.double()
    scale = want.abs().max().clamp_min(1e-30)
    err = ((got - want).abs() / (scale * rel + 1e-6 * want.abs())).max()
    assert torch.isfinite(got).all(), name
    assert err <= 1.0, f"{name}: max |diff| {float((got - want).abs().max()):.3e} vs scale {float(scale):.3e}"


def _close64(got, want32, want64, name=""):
    """The HIP result's error against the fp64 reference is within 8x torch fp32's own error
    (plus 1e-5 of the tensor's scale): f32 rounding in a different order, amplified alike by the
    per-sample BatchNorm statistics of a few nodes, not a different formula."""
    got, w32, w64 = got.double(), want32.double(), want64.double()
    scale = float(w64.abs().max().clamp_min(1e-30))
    e_hip = float((got - w64).abs().max())
    e_t32 = float((w32 - w64).abs().max())
    assert torch.isfinite(got).all(), name
    assert e_hip <= 8.0 * e_t32 + 1e-5 * scale, f"{name}: |hip - fp64| {e_hip:.3e}, |torch32 - fp64| {e_t32:.3e}, scale {scale:.3e}"


@pytest.mark.parametrize("P,n,hidden,mode,per_sample,B", [(5, 64, 16, "diff", True, 12),
                                                          (5, 48, 12, "same", False, 9),
                                                          (16, 32, 8, "diff", True, 5),
                                                          (3, 100, 20, "diff", True, 70),
                                                          (5, 37, 16, "diff", True, 12),    # odd n
                                                          (4, 2, 8, "same", False, 6),      # 2n < 4
                                                          # h = 100: the 200/400-deep GEMMs split K
                                                          # over two wave sets (linear_kernel KS = 2)
                                                          (5, 64, 100, "diff", True, 12),
                                                          # the large-batch defaults (B >= 2048: the tail
                                                          # kernels, unfused input-gradient GEMMs, the
                                                          # one-wave gcn_bwd_kernel, row-split weight
                                                          # gradients); 160-row training tiles on the
                                                          # 448-wide layers, and at B = 7680 on layer 1
                                                          # with its hoisted Atb addend too
                                                          (5, 64, 112, "diff", True, 2250),
                                                          (5, 64, 112, "diff", False, 7680)])
def test_train_hypernetwork_matches_torch_autograd(cuda, monkeypatch, P, n, hidden, mode, per_sample, B):
    """n % 4 != 0: layer 1's input cat(AtAy, Atb) zero-padded to a multiple of 4 columns
    (hyper_ops.layer1_input; VERDICT r4 missing #2: such widths ran on torch before)."""
    import copy

    import gnn_dlasso_models_progressive as G
    from dadmm_hip import hyper_form, hyper_ops
    from dadmm_hip.graph import ingest
    if B >= 2048:   # what the large-batch case is there to run, asked of the launches' own planning
        for knob in ("DADMM_HYPER_TAIL", "DADMM_GCNBWD_FUSE", "DADMM_HYPER_KW"):
            monkeypatch.delenv(knob, raising=False)
        for K, N in ((2 * hidden, 4 * hidden), (4 * hidden, 4 * hidden)):          # conv3, conv4 / conv5
            assert hyper_form("gcn_train", B, P, K, N)["wr"] == 5, "inputs unsuitable: not the 160-row tile"
        if B >= 7680:                                                              # conv1 on AtAy (+ addend)
            assert hyper_form("gcn_train", B, P, n, hidden)["wr"] == 5, "inputs unsuitable: layer 1's tile"
        for N in (hidden, 2 * hidden, 4 * hidden):
            assert hyper_form("gcn_bwd", B, P, 4, N)["nt"] == 64, "inputs unsuitable: not the one-wave form"
    model, _, _ = _model(cuda, P, n, hidden, mode)
    ref = copy.deepcopy(model)
    graphs = ([O.connected_er_graph(P, 0.5, seed=s) for s in range(B)] if per_sample
              else [O.er_graph(P, 0.5, seed=3)] * B)
    gb = ingest(graphs, P, B, cuda)
    ahat = G.normalized_adjacency(gb.nbr, P)
    ahat = (ahat[None] if gb.shared else ahat).contiguous()
    ns = (n + 3) & ~3
    g = torch.Generator(device=cuda).manual_seed(P * 100 + n)
    AtAy = torch.zeros(B, P, ns, device=cuda)
    Atb = torch.zeros(B, P, ns, device=cuda)
    AtAy[..., :n] = torch.randn(B, P, n, device=cuda, generator=g)
    Atb[..., :n] = torch.randn(B, P, n, device=cuda, generator=g)
    AtAy.requires_grad_(True)
    seed = 0x1234_5678_9ABC
    hyp = hyper_ops.hypernetwork_train(model, AtAy, Atb, n, ahat, per_sample, seed=seed)
    ref64 = copy.deepcopy(ref).double()
    A2 = AtAy.detach().clone().requires_grad_(True)
    A3 = AtAy.detach().double().requires_grad_(True)
    want = _torch_reference(ref, A2, Atb, n, ahat, seed)
    want64 = _torch_reference(ref64, A3, Atb.double(), n, ahat.double(), seed)
    _close64(hyp, want, want64, name="hyp")
    R = torch.randn(hyp.shape, device=cuda, generator=g)
    (hyp * R).sum().backward()
    (want * R).sum().backward()
    (want64 * R.double()).sum().backward()
    _close64(AtAy.grad[..., :n], A2.grad[..., :n], A3.grad[..., :n], name="dAtAy")
    assert (AtAy.grad[..., n:] == 0).all()
    for (name, p1), (_, p2), (_, p3) in zip(model.named_parameters(), ref.named_parameters(),
                                            ref64.named_parameters()):
        _close64(p1.grad, p2.grad, p3.grad, name=name)
    for i in range(1, 6):
        bn = getattr(model.encoder, f"bn{i}")
        assert torch.isfinite(bn.running_mean).all() and torch.isfinite(bn.running_var).all()
        assert int(bn.num_batches_tracked) == B


def test_train_running_stats_match_sequential_updates(cuda):
    """BatchNorm running statistics after one training forward == B sequential
    nn.BatchNorm1d train-mode calls, one per sample, in sample order (the reference's loop)."""
    import copy

    import gnn_dlasso_models_progressive as G
    from dadmm_hip import hyper_ops
    from dadmm_hip.graph import ingest
    P, n, hidden, B = 5, 32, 8, 7
    model, _, _ = _model(cuda, P, n, hidden, "diff", seed=3)
    for mod in [model.encoder.dropout] + [model.decoder[i] for i in (1, 5, 9)]:
        mod.p = 0.0
    ref = copy.deepcopy(model)
    graphs = [O.connected_er_graph(P, 0.5, seed=s) for s in range(B)]
    gb = ingest(graphs, P, B, cuda)
    ahat = G.normalized_adjacency(gb.nbr, P).contiguous()
    g = torch.Generator(device=cuda).manual_seed(5)
    AtAy = torch.randn(B, P, n, device=cuda, generator=g)
    Atb = torch.randn(B, P, n, device=cuda, generator=g)
    with torch.no_grad():
        hyper_ops.hypernetwork_train(model, AtAy, Atb, n, ahat, True, seed=1)
        enc = ref.encoder
        x = torch.cat([AtAy, Atb], dim=2)
        for i, (conv, bn) in enumerate(zip((enc.conv1, enc.conv2, enc.conv3, enc.conv4, enc.conv5),
                                           (enc.bn1, enc.bn2, enc.bn3, enc.bn4, enc.bn5))):
            outs = []
            for s in range(B):   # the reference's per-sample calls (:37-40, :52-68)
                m = ahat[s] @ (x[s] @ conv.lin.weight.t()) + conv.bias
                outs.append(bn(F.leaky_relu(m, 0.01)))
            x = torch.stack(outs)
    for i in range(1, 6):
        b1, b2 = getattr(model.encoder, f"bn{i}"), getattr(ref.encoder, f"bn{i}")
        _close(b1.running_mean, b2.running_mean, rel=1e-4, name=f"bn{i}.running_mean")
        _close(b1.running_var, b2.running_var, rel=1e-4, name=f"bn{i}.running_var")
        assert int(b1.num_batches_tracked) == int(b2.num_batches_tracked) == B


def test_deferred_running_stats_match_per_call_updates(cuda):
    """The model's forward queues every iteration's BatchNorm statistics and applies them once
    (flush_running_stats): the same running statistics as one update per call, in call order."""
    import copy

    import gnn_dlasso_models_progressive as G
    from dadmm_hip import hyper_ops
    from dadmm_hip.graph import ingest
    P, n, hidden, B, calls = 5, 32, 8, 9, 3
    model, _, _ = _model(cuda, P, n, hidden, "diff", seed=4)
    ref = copy.deepcopy(model)
    graphs = [O.connected_er_graph(P, 0.5, seed=s) for s in range(B)]
    gb = ingest(graphs, P, B, cuda)
    ahat = G.normalized_adjacency(gb.nbr, P).contiguous()
    g = torch.Generator(device=cuda).manual_seed(9)
    with torch.no_grad():
        for c in range(calls):
            AtAy = torch.randn(B, P, n, device=cuda, generator=g)
            Atb = torch.randn(B, P, n, device=cuda, generator=g)
            hyper_ops.hypernetwork_train(model, AtAy, Atb, n, ahat, True, seed=c, defer=True)
            hyper_ops.hypernetwork_train(ref, AtAy, Atb, n, ahat, True, seed=c, defer=False)
        b0 = model.encoder.bn3.running_mean.clone()
        hyper_ops.flush_running_stats(model)
        assert not torch.equal(b0, model.encoder.bn3.running_mean)   # the flush applied them
    for i in range(1, 6):
        b1, b2 = getattr(model.encoder, f"bn{i}"), getattr(ref.encoder, f"bn{i}")
        _close(b1.running_mean, b2.running_mean, rel=1e-5, name=f"bn{i}.running_mean")
        _close(b1.running_var, b2.running_var, rel=1e-5, name=f"bn{i}.running_var")
        assert int(b1.num_batches_tracked) == int(b2.num_batches_tracked) == B * calls


@pytest.mark.parametrize("path", ["whole-forward", "per-iteration"])
def test_model_train_step_uses_hip_hypernetwork(cuda, path):
    """DLASSO_GNNHyp3_Progressive in train mode: forward + compute_loss + backward through the
    HIP hypernetwork; with dropout off it equals the torch backend (loss and gradients). Default:
    one GnnTrainFn node for the K iterations; with an on_hyp hook the per-iteration nodes
    (GramFn, HyperTrainFn, StepFn) run instead."""
    import copy

    import gnn_dlasso_utils as U
    from dadmm_hip import gnn_ops, hyper_ops
    P, n, hidden, B, K = 5, 64, 16, 16, 3
    model, A, b = _model(cuda, P, n, hidden, "diff", seed=7)
    for mod in [model.encoder.dropout] + [model.decoder[i] for i in (1, 5, 9)]:
        mod.p = 0.0
    ref = copy.deepcopy(model)
    ref.hyper_backend = "torch"
    graphs = [O.connected_er_graph(P, 0.5, seed=s) for s in range(B)]
    rng = np.random.default_rng(2)
    inits = tuple(torch.from_numpy((1e-2 * rng.standard_normal((B, P, n))).astype(np.float32)).to(cuda)
                  for _ in range(3))
    bt = torch.from_numpy(b[:B]).to(cuda)[..., None]
    label = torch.randn(B, n, 1, device=cuda)
    if path == "per-iteration":
        model.on_hyp = lambda *a: None
    fn = gnn_ops.GnnTrainFn if path == "whole-forward" else hyper_ops.HyperTrainFn
    calls = []
    orig = fn.apply
    fn.apply = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        Y1, _ = model(bt, graphs, K, inits=inits)
    finally:
        fn.apply = orig
    assert len(calls) == (1 if path == "whole-forward" else K)
    Y2, _ = ref(bt, graphs, K, inits=inits)
    for i in range(1, 6):   # the B K running-statistics updates of each BatchNorm, in call order
        bn1, bn2 = getattr(model.encoder, f"bn{i}"), getattr(ref.encoder, f"bn{i}")
        _close(bn1.running_mean, bn2.running_mean, rel=1e-4, name=f"bn{i}.running_mean")
        _close(bn1.running_var, bn2.running_var, rel=1e-4, name=f"bn{i}.running_var")
        assert int(bn1.num_batches_tracked) == int(bn2.num_batches_tracked)
    l1, f1 = U.compute_loss(Y1, label)
    l2, f2 = U.compute_loss(Y2, label)
    assert abs(float(l1) - float(l2)) <= 1e-4 * abs(float(l2))
    l1.backward()
    l2.backward()
    for (name, p1), (_, p2) in zip(model.named_parameters(), ref.named_parameters()):
        assert p1.grad is not None and torch.isfinite(p1.grad).all(), name
        _close(p1.grad, p2.grad, rel=5e-3, name=name)


@pytest.mark.parametrize("R,N,K,K1,beta", [(1280, 400, 400, 400, 1), (1280, 100, 512, 256, 0),
                                           (256, 400, 2000, 2000, 1), (256, 20, 100, 100, 1),
                                           (37, 13, 70, 70, 0), (51200, 100, 2048, 1024, 1)])
def test_wgrad_colsum_transpose_kernels(cuda, R, N, K, K1, beta):
    """dadmm_hyper_wgrad (G (+)= dZ^T X with the bias column sums, X read as two segments),
    dadmm_hyper_colsum and dadmm_hyper_transpose against fp64 references; deterministic."""
    import ctypes
    from dadmm_hip import _lib
    from dadmm_hip.ops import _ptr, _stream
    L = _lib.load()
    g = torch.Generator(device=cuda).manual_seed(R + N + K)
    dz = torch.randn(R, N, device=cuda, generator=g)
    x1 = torch.randn(R, K1 + 8, device=cuda, generator=g)     # padded rows: ld1 > K1
    x2 = torch.randn(R, K - K1 + 4, device=cuda, generator=g) if K1 < K else None
    G0 = torch.randn(N, K, device=cuda, generator=g)
    b0 = torch.randn(N, device=cuda, generator=g)
    nb = L.dadmm_hyper_wgrad_scratch_bytes(R, N, K)
    scratch = torch.empty(max(nb, 16) // 4 + 4, device=cuda)
    outs = []
    for _ in range(2):
        Gm, bm = G0.clone(), b0.clone()
        _lib.check("dadmm_hyper_wgrad", L.dadmm_hyper_wgrad(
            R, N, K, _ptr(dz), N, _ptr(x1), K1 + 8, K1, _ptr(x2), (K - K1 + 4) if x2 is not None else 0,
            _ptr(Gm), _ptr(bm), beta, _ptr(scratch), _stream(cuda)))
        outs.append((Gm, bm))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    X = x1[:, :K1].double() if x2 is None else torch.cat([x1[:, :K1], x2[:, :K - K1]], 1).double()
    want = dz.double().t() @ X + (G0.double() if beta else 0)
    wantb = dz.double().sum(0) + (b0.double() if beta else 0)
    scale = float((dz.double().abs().t() @ X.abs()).max())
    assert float((outs[0][0].double() - want).abs().max()) <= 2e-6 * scale + 1e-6
    assert float((outs[0][1].double() - wantb).abs().max()) <= 2e-6 * float(dz.abs().sum(0).max()) + 1e-6
    # colsum: out [G][C] (+)= sum_r part [G][R][C]
    part = torch.randn(3, min(R, 300), N, device=cuda, generator=g)
    out = torch.randn(3, N, device=cuda, generator=g)
    ref = out.double() + part.double().sum(1)
    _lib.check("dadmm_hyper_colsum", L.dadmm_hyper_colsum(_ptr(part), 3, part.shape[1], N, _ptr(out), 1,
                                                          _stream(cuda)))
    torch.testing.assert_close(out.double(), ref, rtol=1e-5, atol=1e-4)
    # transpose
    t = torch.empty(K, N, device=cuda)
    _lib.check("dadmm_hyper_transpose", L.dadmm_hyper_transpose(N, K, _ptr(G0), _ptr(t), _stream(cuda)))
    assert torch.equal(t, G0.t())


def _train_pair(cuda, P, n, hidden, mode, shared, B=12, seed=11):
    """(HIP model, torch-backend copy) with dropout off, graphs, inits, b and a label."""
    import copy
    model, A, b = _model(cuda, P, n, hidden, mode, seed=seed, B=B)
    for mod in [model.encoder.dropout] + [model.decoder[i] for i in (1, 5, 9)]:
        mod.p = 0.0
    ref = copy.deepcopy(model)
    ref.hyper_backend = "torch"
    graphs = ([O.connected_er_graph(P, 0.5, seed=3)] * B if shared
              else [O.connected_er_graph(P, 0.5, seed=40 + s) for s in range(B)])
    rng = np.random.default_rng(seed)
    inits = tuple(torch.from_numpy((1e-2 * rng.standard_normal((B, P, n))).astype(np.float32)).to(cuda)
                  for _ in range(3))
    bt = torch.from_numpy(b[:B]).to(cuda)[..., None]
    label = torch.randn(B, n, 1, device=cuda, generator=torch.Generator(device=cuda).manual_seed(seed))
    return model, ref, graphs, inits, bt, label


@pytest.mark.parametrize("mode,shared", [("same", True), ("diff", True), ("same", False)])
def test_whole_forward_node_modes(cuda, mode, shared):
    """GnnTrainFn (one autograd node for the K iterations) in 'same' mode (H = 1) and with one
    shared graph: loss and every parameter gradient equal the torch backend's; the returned
    hyper-parameters of the last iteration carry their gradient too."""
    import gnn_dlasso_utils as U
    from dadmm_hip import gnn_ops
    P, n, hidden, K = 5, 32, 8, 3
    model, ref, graphs, inits, bt, label = _train_pair(cuda, P, n, hidden, mode, shared)
    calls = []
    orig = gnn_ops.GnnTrainFn.apply
    gnn_ops.GnnTrainFn.apply = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        Y1, h1 = model(bt, graphs, K, inits=inits)
    finally:
        gnn_ops.GnnTrainFn.apply = orig
    assert calls == [1]
    Y2, h2 = ref(bt, graphs, K, inits=inits)
    _close(Y1, Y2, rel=1e-4, name="Y")
    for a_, b_ in zip(h1, h2):
        _close(a_, b_, rel=1e-4, name="hyp")
    # loss through Y and through the last iteration's hyper-parameters
    l1 = U.compute_loss(Y1, label)[1] + 0.1 * sum(h.sum() for h in h1)
    l2 = U.compute_loss(Y2, label)[1] + 0.1 * sum(h.sum() for h in h2)
    l1.backward()
    l2.backward()
    for (name, p1), (_, p2) in zip(model.named_parameters(), ref.named_parameters()):
        assert p1.grad is not None, name
        _close(p1.grad, p2.grad, rel=5e-3, name=name)


@pytest.mark.parametrize("B", [256, 51])
def test_whole_forward_node_split_weight_gradients(cuda, B):
    """The deferred weight gradients (dadmm_hyper_train_wgrad over rows x iterations, one launch
    per parameter) against the per-iteration ones (an on_hyp hook selects HyperTrainFn, whose
    backward adds each iteration's gradients as it goes): the same dZ operands summed in another
    order, so they agree to f32 rounding of the sums. At B = 256, K = 4 the rows split over several
    workgroups per output tile (the plan's row-split scratch is allocated); at B = 51 every batch
    block has an odd row count (255 rows: the kernel's odd-row tail per block). A second pass gives
    the same bits (the partials are added in a fixed order); at B = 256 the gradients also equal
    the torch backend's. (At B = 51, K = 4 both HIP paths sit 1e-2 from torch: a sample whose
    five-node BatchNorm amplifies f32 rounding, not a kernel difference.)"""
    import copy

    import gnn_dlasso_utils as U
    from dadmm_hip import hyper_ops
    P, n, hidden, K = 5, 32, 8, 4
    model, ref, graphs, inits, bt, label = _train_pair(cuda, P, n, hidden, "diff", False, B=B)
    per_iter = copy.deepcopy(model)
    per_iter.on_hyp = lambda *a: None
    grads = []
    for _ in range(2):
        model.zero_grad()
        Y1, _ = model(bt, graphs, K, inits=inits)
        U.compute_loss(Y1, label)[1].backward()
        grads.append([p.grad.clone() for p in model.parameters()])
    plans = hyper_ops._cache(model)["plans"]
    assert any(pl.wscratch is not None for pl in plans.values()) or B < 256
    for g1, g2 in zip(*grads):
        assert torch.equal(g1, g2)
    Y3, _ = per_iter(bt, graphs, K, inits=inits)
    assert torch.equal(Y1, Y3)
    U.compute_loss(Y3, label)[1].backward()
    for (name, p1), (_, p3) in zip(model.named_parameters(), per_iter.named_parameters()):
        _close(p1.grad, p3.grad, rel=2e-5, name=name)
    if B == 256:
        # (a sanity bound against torch fp32, which sums cat(AtAy, Atb) W1^T in one GEMM where the
        # HIP forward adds layer 1's hoisted Atb half after the mix: conv3.bias sits 8e-3 from
        # torch here, the five-node BatchNorm amplification described above; the fp64 comparisons
        # of test_train_hypernetwork_matches_torch_autograd are the accuracy tests)
        Y2, _ = ref(bt, graphs, K, inits=inits)
        U.compute_loss(Y2, label)[1].backward()
        for (name, p1), (_, p2) in zip(model.named_parameters(), ref.named_parameters()):
            _close(p1.grad, p2.grad, rel=2e-2, name=name)


def test_whole_forward_node_accumulates_and_respects_frozen(cuda):
    """Two backward passes add into .grad (as autograd does); a parameter with requires_grad
    False keeps .grad None; zero_grad between steps resets."""
    import gnn_dlasso_utils as U
    P, n, hidden, K = 5, 32, 8, 2
    model, ref, graphs, inits, bt, label = _train_pair(cuda, P, n, hidden, "diff", False)
    for m_ in (model, ref):
        m_.encoder.conv2.lin.weight.requires_grad_(False)
    for _ in range(2):
        for m_ in (model, ref):
            Y, _ = m_(bt, graphs, K, inits=inits)
            U.compute_loss(Y, label)[1].backward()
    for (name, p1), (_, p2) in zip(model.named_parameters(), ref.named_parameters()):
        if not p2.requires_grad:
            assert p1.grad is None and p2.grad is None, name
            continue
        _close(p1.grad, p2.grad, rel=5e-3, name=name)
    model.zero_grad()
    Y, _ = model(bt, graphs, K, inits=inits)
    U.compute_loss(Y, label)[1].backward()
    ref.zero_grad()
    Y, _ = ref(bt, graphs, K, inits=inits)
    U.compute_loss(Y, label)[1].backward()
    for (name, p1), (_, p2) in zip(model.named_parameters(), ref.named_parameters()):
        if p2.requires_grad:
            _close(p1.grad, p2.grad, rel=5e-3, name=name)


def test_whole_forward_node_autograd_grad_and_hooks(cuda):
    """GnnTrainFn returns the hypernetwork's parameter gradients to autograd, so
    torch.autograd.grad(loss, params) works (and leaves .grad alone), parameter hooks fire, and
    the result equals the torch backend's .grad; a second backward through the same node
    (retain_graph=True) raises a clear error instead of a TypeError."""
    import gnn_dlasso_utils as U
    P, n, hidden, K = 5, 32, 8, 2
    model, ref, graphs, inits, bt, label = _train_pair(cuda, P, n, hidden, "diff", False)
    names = [nm for nm, _ in model.named_parameters()]
    params = list(model.parameters())
    seen = []
    h = model.fc.weight.register_hook(lambda g: seen.append(g.shape))
    Y, _ = model(bt, graphs, K, inits=inits)
    loss = U.compute_loss(Y, label)[1]
    grads = torch.autograd.grad(loss, params, retain_graph=True)
    h.remove()
    assert seen == [model.fc.weight.shape]
    assert all(p.grad is None for p in params)
    Y2, _ = ref(bt, graphs, K, inits=inits)
    U.compute_loss(Y2, label)[1].backward()
    for name, g1, p2 in zip(names, grads, ref.parameters()):
        assert g1 is not None, name
        _close(g1, p2.grad, rel=5e-3, name=name)
    with pytest.raises(RuntimeError, match="retain_graph"):
        loss.backward()


@pytest.mark.parametrize("P,n,hidden,mode,per_sample,B", [(5, 64, 16, "diff", True, 12),
                                                          (5, 37, 16, "same", False, 9),
                                                          (16, 32, 8, "diff", True, 5)])
def test_eval_hypernetwork_matches_torch_autograd(cuda, P, n, hidden, mode, per_sample, B):
    """model.eval() under autograd (VERDICT r4 missing #2): the training kernels with BatchNorm on
    the running statistics and no dropout (dadmm_hyper_net.bn_eval / the gcn kernels' running
    statistics), forward and backward, against torch autograd of the eval-mode modules; the
    running statistics are inputs only, and no dropout seed is drawn."""
    import copy

    import gnn_dlasso_models_progressive as G
    from dadmm_hip import hyper_ops
    from dadmm_hip.graph import ingest
    model, _, _ = _model(cuda, P, n, hidden, mode)
    model.eval()
    ref = copy.deepcopy(model)
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "tracked" in k}
    graphs = ([O.connected_er_graph(P, 0.5, seed=s) for s in range(B)] if per_sample
              else [O.er_graph(P, 0.5, seed=3)] * B)
    gb = ingest(graphs, P, B, cuda)
    ahat = G.normalized_adjacency(gb.nbr, P)
    ahat = (ahat[None] if gb.shared else ahat).contiguous()
    ns = (n + 3) & ~3
    g = torch.Generator(device=cuda).manual_seed(P * 100 + n + 1)
    AtAy = torch.zeros(B, P, ns, device=cuda)
    Atb = torch.zeros(B, P, ns, device=cuda)
    AtAy[..., :n] = torch.randn(B, P, n, device=cuda, generator=g)
    Atb[..., :n] = torch.randn(B, P, n, device=cuda, generator=g)
    AtAy.requires_grad_(True)
    hyp = hyper_ops.hypernetwork_train(model, AtAy, Atb, n, ahat, per_sample, seed=0)
    ref64 = copy.deepcopy(ref).double()
    A2 = AtAy.detach().clone().requires_grad_(True)
    A3 = AtAy.detach().double().requires_grad_(True)
    want = _torch_reference(ref, A2, Atb, n, ahat, 0, train=False)
    want64 = _torch_reference(ref64, A3, Atb.double(), n, ahat.double(), 0, train=False)
    _close64(hyp, want, want64, name="hyp")
    R = torch.randn(hyp.shape, device=cuda, generator=g)
    (hyp * R).sum().backward()
    (want * R).sum().backward()
    (want64 * R.double()).sum().backward()
    _close64(AtAy.grad[..., :n], A2.grad[..., :n], A3.grad[..., :n], name="dAtAy")
    assert (AtAy.grad[..., n:] == 0).all()
    for (name, p1), (_, p2), (_, p3) in zip(model.named_parameters(), ref.named_parameters(),
                                            ref64.named_parameters()):
        _close64(p1.grad, p2.grad, p3.grad, name=name)
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)


def test_model_eval_autograd_and_odd_n_use_hip(cuda):
    """DLASSO_GNNHyp3_Progressive never reports the torch composition unless hyper_backend is
    "torch": eval + autograd -> "hip-eval-grad", eval + no_grad at odd n -> "hip-eval-graph",
    train at odd n -> "hip-train" (VERDICT r4 next #7)."""
    P, n, B = 5, 37, 6
    model, A, b = _model(cuda, P, n, 8, "diff", B=B)
    graphs = [O.connected_er_graph(P, 0.5, seed=s) for s in range(B)]
    bt = torch.from_numpy(b[:B]).to(cuda)[..., None]
    model.eval()
    Y, _ = model(bt, graphs)
    Y.sum().backward()
    assert model.last_backend == "hip-eval-grad"
    with torch.no_grad():
        model(bt, graphs)
    assert model.last_backend == "hip-eval-graph"
    model.train()
    Y, _ = model(bt, graphs)
    Y.sum().backward()
    assert model.last_backend == "hip-train"


@pytest.mark.parametrize("knob", ["DADMM_GCNBWD_FUSE", "DADMM_HYPER_TAIL"])
@pytest.mark.parametrize("P,n,hidden,B,per_sample,ladder", [(5, 64, 16, 40, False, False),
                                                            (7, 32, 12, 33, True, False),
                                                            (5, 64, 100, 40, True, False),
                                                            # the head where both of its clamps bind: the
                                                            # tail kernels restate it (forward and backward)
                                                            (5, 64, 16, 40, True, True)],
                         ids=["5-64-16-40-False", "7-32-12-33-True", "5-64-100-40-True", "5-64-16-40-True-ladder"])
def test_fused_gcn_backward_bit_identical(cuda, monkeypatch, knob, P, n, hidden, B, per_sample, ladder):
    """Two fusions of the training hypernetwork against their separate launches, with dropout on:
    DADMM_GCNBWD_FUSE — GCN layers 4..1's block backward in the epilogue of the layer above's
    input-gradient GEMM (dadmm_hyper_linear_gcn_bwd) vs linear + dadmm_hyper_gcn_train_bwd;
    DADMM_HYPER_TAIL — decoder blocks 2, 3, fc and the head as one launch each way
    (dadmm_hyper_tail.hip) vs the ten separate ones (B = 33: a partial 16-sample tile and partial
    8-row LayerNorm blocks). d AtAy and every parameter gradient are bit-identical, through the
    per-call HyperTrainFn (immediate weight gradients) and through the whole-forward node
    (deferred weight gradients), and so are the iterates and hyper-parameters."""
    import copy

    import gnn_dlasso_models_progressive as G
    import gnn_dlasso_utils as U
    from dadmm_hip import hyper_ops
    from dadmm_hip.graph import ingest
    model0, _, b = _model(cuda, P, n, hidden, "diff", seed=3, B=B,
                          maxima=HEAD_MAXIMA_BINDING if ladder else (0.1, 0.99, 0.99, 0.99))
    if ladder:   # fc.bias on the ladder (model.fc's weights are small against it)
        with torch.no_grad():
            model0.fc.bias.copy_(_head_ladder(P))
    graphs = ([O.connected_er_graph(P, 0.5, seed=70 + s) for s in range(B)] if per_sample
              else [O.connected_er_graph(P, 0.5, seed=4)] * B)
    gb = ingest(graphs, P, B, cuda)
    ahat = G.normalized_adjacency(gb.nbr, P)
    ahat = (ahat[None] if gb.shared else ahat).contiguous()
    g = torch.Generator(device=cuda).manual_seed(9)
    AtAy0 = torch.randn(B, P, n, device=cuda, generator=g)
    Atb = torch.randn(B, P, n, device=cuda, generator=g)
    R = None
    bt = torch.from_numpy(b[:B]).to(cuda)[..., None]
    label = torch.randn(B, n, 1, device=cuda, generator=g)
    out = {}
    for fuse in ("1", "0"):   # always / never fused (the defaults decide by grid size / fit)
        monkeypatch.setenv(knob, fuse)
        model = copy.deepcopy(model0)
        AtAy = AtAy0.clone().requires_grad_(True)
        hyp = hyper_ops.hypernetwork_train(model, AtAy, Atb, n, ahat, per_sample, seed=0xABCDEF)
        if R is None:
            R = torch.randn(hyp.shape, device=cuda, generator=g)
        (hyp * R).sum().backward()
        per_call = [AtAy.grad.clone()] + [p.grad.clone() for p in model.parameters()]
        model = copy.deepcopy(model0)
        torch.manual_seed(5)
        Y, h = model(bt, graphs, 3)
        assert model.last_backend == "hip-train", model.last_backend
        (U.compute_loss(Y, label)[1] + 0.1 * sum(x.sum() for x in h)).backward()
        out[fuse] = (per_call + [hyp.detach().clone(), Y.detach().clone()] + [x.detach().clone() for x in h],
                     [p.grad.clone() for p in model.parameters()])
    for got, want in zip(out["1"][0] + out["1"][1], out["0"][0] + out["0"][1]):
        assert torch.equal(got, want), (got - want).abs().max()
    if ladder:   # the ladder reached the head: saturated lanes on both sides, in and past the second clamp
        hyp = out["1"][0][len(list(model0.parameters())) + 1]
        assert torch.isfinite(hyp).all()
        assert int((hyp[:, 0] == float(np.float32(1e-4) * np.float32(0.1))).sum()) >= B
        assert int((hyp[:, 1:] == float(np.float32(0.9999))).sum()) >= B
        assert all(torch.isfinite(t).all() for t in out["1"][0] + out["1"][1])


def test_whole_forward_node_guard_raises_in_backward(cuda):
    """A guard that fired in the training forward (a NaN in y0) makes the whole-forward node's
    backward raise GuardAdjointError (the status word is staged behind an event in the forward
    and checked after the backward's enqueue), and no parameter gradient is delivered."""
    import gnn_dlasso_utils as U
    from dadmm_hip.autograd import GuardAdjointError
    P, n, hidden, K = 5, 32, 8, 2
    model, ref, graphs, inits, bt, label = _train_pair(cuda, P, n, hidden, "diff", False)
    y0 = inits[0].clone()
    y0[3, 2, 7] = float("nan")
    Y, _ = model(bt, graphs, K, inits=(y0, inits[1], inits[2]))
    assert int(model.last_status.item()) & 1
    model.zero_grad()
    with pytest.raises(GuardAdjointError):
        U.compute_loss(Y, label)[1].backward()
    assert all(p.grad is None for p in model.parameters())
    # and a clean step afterwards works
    Y, _ = model(bt, graphs, K, inits=inits)
    U.compute_loss(Y, label)[1].backward()
    assert all(p.grad is not None for p in model.parameters())
