"""The streamed evaluation forward's host side (no GPU): the served-shape table of the C ABI's query
(dadmm_forward_eval_stream_scratch_bytes), its scratch size, ops.eval_stream_served, the two new
symbols in the header and the binding, the module's ``evaluate`` on CPU tensors at a streamed shape,
and the m0 invariant of tests/test_m0_isa.py on the evaluation kernels' own build
(csrc/dadmm_stream.hip with -DDADMM_STREAM_EVAL=1).

The query serves a shape where the streamed single launch applies as it does for recording and
dadmm_forward has no kernel. One case of the issue's table is stated here as the rule gives it, not
as the issue listed it: (P 7, m 64, n 96) was listed as refused for having "fewer than four column
blocks", but n = 96 is padded to n_pad = 128, four 32-column blocks, the streamed recording forward
serves it (dadmm_tiled_form(record) == 1) and so does the evaluation. The shape that has fewer than
four blocks is n <= 64 (n_pad = 64): (7, 64, 64) takes the refused case's place, and (7, 64, 96) is
asserted to follow the recording query."""
import argparse
import ctypes
import os
import re
import subprocess

import pytest
import torch

import oracle as O
from test_m0_isa import CSRC, FLAGS, HDRS, HIPCC, check_m0

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dims(P, m, n, shared=1, B=37, K=4):
    from dadmm_hip import _lib
    return _lib.Dims(B=B, P=P, m=m, n=n, K=K, variant=0, hyp_rows=1, graph_shared=shared)


def _bytes(d):
    from dadmm_hip import _lib
    return int(_lib.load().dadmm_forward_eval_stream_scratch_bytes(ctypes.byref(d)))


def _parts(d):
    """The three parts of the scratch, each rounded up to 256 bytes: U state, second iterate, partials."""
    up = lambda x: (x + 255) & ~255
    state = up(4 * d.B * d.P * d.n)
    return 2 * state + up(4 * d.K * 8 * ((d.B + 15) // 16))


SERVED = [(7, 64, 128, 1), (16, 64, 512, 1), (6, 64, 192, 1), (5, 100, 500, 1), (8, 128, 128, 1),
          (5, 64, 320, 1), (16, 64, 512, 0)]
REFUSED = [(5, 64, 256, 1), (4, 32, 128, 1), (6, 64, 128, 1), (17, 64, 512, 1), (9, 100, 500, 1),
           (7, 64, 64, 1), (5, 129, 500, 1), (5, 64, 256, 0)]


@pytest.mark.parametrize("P,m,n,shared", SERVED)
def test_query_serves(P, m, n, shared):
    d = _dims(P, m, n, shared)
    got = _bytes(d)
    assert got != 0 and got % 256 == 0 and got >= _parts(d), (got, _parts(d))


@pytest.mark.parametrize("P,m,n,shared", REFUSED)
def test_query_refuses(P, m, n, shared):
    from dadmm_hip import _lib
    assert _bytes(_dims(P, m, n, shared)) == 0
    assert _lib.load().dadmm_last_error() != b""          # the reason is there to read


def test_n96_is_padded_to_four_blocks_and_follows_the_recording_query():
    from dadmm_hip.ops import tiled_form
    assert tiled_form((7, 64, 96), record=True) == 1
    assert _bytes(_dims(7, 64, 96)) >= _parts(_dims(7, 64, 96))


def test_query_ignores_the_forward_form_switches(monkeypatch):
    """DADMM_TILED_STREAM / DADMM_STREAM_WAVES choose among the forward's forms; there is one
    evaluation form."""
    for k, v in (("DADMM_TILED_STREAM", "0"), ("DADMM_STREAM_WAVES", "16")):
        monkeypatch.setenv(k, v)
        assert _bytes(_dims(16, 64, 512)) != 0 and _bytes(_dims(5, 100, 500)) != 0
        monkeypatch.delenv(k)


def test_scratch_at_the_benchmark_shapes():
    for d in (_dims(16, 64, 512, B=4096, K=25), _dims(5, 100, 500, B=4096, K=25), _dims(1, 100, 128, B=1, K=1)):
        assert _bytes(d) >= _parts(d)
    assert _bytes(_dims(16, 64, 512, B=0)) == 0 and _bytes(_dims(16, 64, 512, K=0)) == 0


def test_existing_evaluation_query_is_unchanged_on_the_streamed_shapes():
    from dadmm_hip import _lib
    for P, m, n, shared in SERVED:
        assert int(_lib.load().dadmm_forward_eval_scratch_bytes(ctypes.byref(_dims(P, m, n, shared)))) == 0


def test_eval_stream_served_follows_the_query():
    from dadmm_hip.graph import ingest
    from dadmm_hip.ops import eval_served, eval_stream_served
    cpu = torch.device("cpu")
    for P, m, n, shared in SERVED:
        assert eval_stream_served(_dims(P, m, n), 16, 3), (P, m, n)
        assert not eval_served(_dims(P, m, n), 16, 3)
    for P, m, n, shared in REFUSED:
        if shared:
            assert not eval_stream_served(_dims(P, m, n), 16, 3), (P, m, n)
    for n in range(449, 513):                       # n is padded to the stored row length
        assert eval_stream_served(_dims(16, 64, n), 16, 3), n
    shared = ingest([O.er_graph(16, 0.3, seed=1)] * 16, 16, 16, cpu)
    per_sample = ingest([O.er_graph(16, 0.3, seed=s) for s in range(16)], 16, 16, cpu)
    assert eval_stream_served(_dims(16, 64, 512), 16, 3, shared)
    assert eval_stream_served(_dims(16, 64, 512), 16, 3, per_sample)
    p5 = ingest([O.er_graph(5, 0.5, seed=s) for s in range(16)], 5, 16, cpu)
    assert not eval_stream_served(_dims(5, 64, 256), 16, 3, p5)     # a fused shape, per-sample or not
    assert eval_stream_served(_dims(5, 100, 500), 16, 3, p5)


def test_header_and_binding_declare_the_new_symbols():
    from dadmm_hip import _lib
    import dadmm_hip
    header = open(os.path.join(ROOT, "include", "dadmm.h")).read()
    for sym in ("dadmm_forward_eval_stream_scratch_bytes", "dadmm_forward_eval_stream"):
        assert re.search(r"\b%s\(" % sym, header), sym
        assert sym in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), sym)
    assert _lib.ABI_VERSION >= 23 and _lib.load().dadmm_abi_version() == _lib.ABI_VERSION
    assert re.search(r"#define DADMM_ABI_VERSION %d\b" % _lib.ABI_VERSION, header)
    for name in ("eval_stream_served", "forward_eval_stream_raw"):
        assert callable(getattr(dadmm_hip, name))
    assert isinstance(dadmm_hip.ops.STREAM_EVAL_M128_MIN_B, int) and dadmm_hip.ops.STREAM_EVAL_M128_MIN_B >= 1


def test_evaluate_on_cpu_at_a_streamed_shape_is_forward_plus_losses():
    import gnn_dlasso_utils
    import unfolded_DLASSO as U
    P, m, n, B, K = 7, 12, 128, 3, 2
    args = argparse.Namespace(GHN_iter_num=K, DADMM_mode="diff", alpha_max=0.1, tau_max=0.99, rho_max=0.99,
                              eta_max=0.99, max_penalty_threshold=0.8, penalty_reduction_factor=0.95)
    A, b, _ = O.make_problem(P, m, n, B, seed=5)
    mod = U.DLASSO_unfolded(torch.from_numpy(A)[None], args).requires_grad_(False)
    with torch.no_grad():
        mod.seq_hyp.param.copy_(0.3 * torch.randn(mod.seq_hyp.param.shape,
                                                  generator=torch.Generator().manual_seed(1)))
    g = torch.Generator().manual_seed(3)
    inits = tuple(1e-2 * torch.randn((B, P, n, 1), generator=g) for _ in range(3))
    label = torch.randn((B, n, 1), generator=g)
    bt = torch.from_numpy(b)[..., None]
    graphs = [O.er_graph(P, 0.5, seed=s) for s in range(B)]
    from dadmm_hip.ops import eval_stream_served
    assert eval_stream_served(_dims(P, m, n, shared=0), B, K)
    ev = mod.evaluate(bt, graphs, label, inits=inits)
    with torch.no_grad():
        Y, hyp = mod(bt, graphs, inits=inits)
        lm, lf = gnn_dlasso_utils.compute_loss(Y, label)
        losses = gnn_dlasso_utils.layer_losses(Y, label)
    assert torch.equal(ev.losses, losses) and torch.equal(ev.loss_mean, lm) and torch.equal(ev.loss_final, lf)
    assert torch.equal(ev.y_final, Y[-1]) and torch.equal(ev.hyp, hyp) and int(ev.status.item()) == 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_m0_invariant_of_the_evaluation_kernels(tmp_path):
    """The evaluation kernels issue one more inline-asm LDS-DMA per step (the label block): the same
    invariant as the forward's unit, on the second build's own assembly."""
    built = os.path.join(CSRC, "build", "dadmm_stream_eval.s")
    deps = [os.path.join(CSRC, f) for f in ("dadmm_stream.hip", *HDRS)]
    if os.path.exists(built) and os.path.getmtime(built) >= max(os.path.getmtime(f) for f in deps):
        lines = open(built).read().splitlines()
    else:
        out = tmp_path / "dadmm_stream_eval.s"
        subprocess.run([HIPCC, *FLAGS, "-DDADMM_STREAM_EVAL=1", "-x", "hip", "--cuda-device-only", "-S",
                        os.path.join(CSRC, "dadmm_stream.hip"), "-o", str(out)], check=True,
                       capture_output=True, text=True, timeout=600)
        lines = out.read_text().splitlines()
    kernels = [ln for ln in lines if re.match(r"^_ZN5dadmm6stream18stream_eval_kernel\w+:", ln)]
    assert len(kernels) == 3, kernels                  # <8,1>, <8,2>, <8,1,.,2>; no 16-wave form
    assert not any("13stream_kernel" in ln for ln in lines)          # the evaluation kernels alone
    assert any("m0" in ln for ln in lines)
    assert check_m0(lines) == []
