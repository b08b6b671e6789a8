"""Torch-facing wrappers over the C ABI (device memory, streams and autograd plumbing only).

All arithmetic of the D-ADMM recurrence runs in ``libdadmm.so``; this module validates tensors,
allocates outputs with the torch caching allocator and passes raw device pointers plus the
current HIP stream.
"""
from __future__ import annotations

import ctypes
import dataclasses
import types

import torch

from . import _lib
from .graph import GraphBatch


def _dev_check(*tensors):
    for t in tensors:
        if t is not None and t.device.type != "cuda":
            raise RuntimeError(
                "dadmm_hip runs on a ROCm GPU only (tensors must be on a cuda/hip device); "
                f"got a tensor on {t.device}")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class PreparedOperator:
    """The per-agent operator prepared once per A (replaces ``self.AtA = compute_Atx(self.A)``,
    unfolded_DLASSO.py:16): padded A and A^T in one device workspace."""

    def __init__(self, A: torch.Tensor):
        if A.dim() == 4:
            if A.shape[0] != 1:
                raise ValueError(f"A must be [1, P, m, n], got {tuple(A.shape)}")
            A = A[0]
        if A.dim() != 3:
            raise ValueError(f"A must be [1, P, m, n] or [P, m, n], got {tuple(A.shape)}")
        _dev_check(A)
        self.P, self.m, self.n = (int(x) for x in A.shape)
        self.n_store = (self.n + 3) & ~3          # kernel needs n % 4 == 0: zero-pad columns
        A = A.detach().to(torch.float32)
        if self.n_store != self.n:
            A = torch.nn.functional.pad(A, (0, self.n_store - self.n))
        A = A.contiguous()
        self.device = A.device
        L = _lib.load()
        d = self.dims(B=0, K=0)
        nbytes = L.dadmm_operator_bytes(ctypes.byref(d))
        if nbytes == 0:
            _lib.check("dadmm_operator_bytes", _lib.DADMM_EINVAL)
        self.workspace = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check("dadmm_prepare_operator",
                       L.dadmm_prepare_operator(ctypes.byref(d), _ptr(A), _ptr(self.workspace),
                                                _stream(self.device)))

    def dims(self, B, K, variant=_lib.VARIANT_UNFOLDED, hyp_rows=1, graph_shared=0):
        return _lib.Dims(B=B, P=self.P, m=self.m, n=self.n_store, K=K, variant=variant,
                         hyp_rows=hyp_rows, graph_shared=int(graph_shared))


def _pad_n(t, n_store):
    if t.shape[-1] == n_store:
        return t
    return torch.nn.functional.pad(t, (0, n_store - t.shape[-1]))


def _sw_flag_bytes(K):
    return 4 * (8 + 4 * K)   # SW_FLAG_WORDS(K) of csrc/dadmm_internal.h


def draw_inits(shape, device, n_store=None, zero=None, nzero=0):
    """(y0, U0, d0) = torch.randn(shape) * 1e-2 x 3 in that order (unfolded_DLASSO.py:49-51),
    bit-identical to torch's own draws, from the device's default generator (advanced exactly as
    the three torch calls would), in ONE launch that also zeroes ``nzero`` int32 words at
    ``zero``. shape = (B, P, n); outputs are [B, P, n_store] (padding columns zero)."""
    B, P, n = shape
    ns = n if n_store is None else n_store
    L = _lib.load()
    alloc = torch.zeros if ns != n else torch.empty
    y0, U0, d0 = (alloc((B, P, ns), dtype=torch.float32, device=device) for _ in range(3))
    numel = B * P * n
    gen = torch.cuda.default_generators[device.index if device.index is not None
                                        else torch.cuda.current_device()]
    seed, off = gen.initial_seed(), gen.get_offset()
    if numel > 0:
        step = L.dadmm_normal_offset_step(numel)
        if step == 0:
            _lib.check("dadmm_normal_offset_step", _lib.DADMM_EHIP)
        gen.set_offset(off + 3 * step)
    with torch.cuda.device(device):
        _lib.check("dadmm_prologue", L.dadmm_prologue(
            seed, off, numel, n, ns, 0.0, 1e-2, _ptr(y0), _ptr(U0), _ptr(d0),
            _ptr(zero), nzero, _stream(device)))
    return y0, U0, d0


@dataclasses.dataclass(frozen=True)
class ForwardPlan:
    """What one forward launches (plan_forward): a decision over the Dims alone."""
    candidates: tuple       # launcher names (_FORWARD_LAUNCHERS), tried in this order
    gated: bool             # the stepwise launch follows
    split_bytes: int        # the split launch's exchange buffer (0: "split" is no candidate)
    split_flag_bytes: int   # its epoch words
    stepwise_bytes: int     # the stepwise scratch, guard flags first (0 unless gated)
    nzero: int              # int32 words the prologue zeroes: status + pad, epochs, guard flags


# The streamed recording launch with two m-groups (64 < m <= 128, P <= 8) runs one workgroup per
# 16 samples, one wave per agent, and its time barely depends on the batch (2.9 ms at B = 32,
# 3.5 ms at B = 4096 for P = 5, m = 100, n = 500, K = 25), while the stepwise recording spreads a
# small batch over (tile, agent) workgroups (1.0 ms at B = 32, 5.2 ms at B = 4096). On "auto" a
# recording forward at m > 64 therefore takes the streamed launch only from this batch size on
# (DESIGN.md §4.7b has the sweep); path="tiled" takes it at every batch size.
STREAM_RECORD_M128_MIN_B = 4096

# The same trade for DLASSO_unfolded.evaluate at m > 64: the streamed evaluation launch (two
# m-groups, one workgroup per 16 samples) against forward + compute_loss on the per-iteration
# launches, which is what forward runs there by default. The module routes to the streamed
# evaluation only from this batch size on; forward_eval_stream_raw serves every batch size.
# Measured at P = 5, m = 100, n = 500, K = 25 (scripts/time_eval_stream.py, DESIGN.md §4.11b,
# profiles/r14/time_eval_stream_default_sweep_r14.json), ms per validation step, evaluate against
# forward + compute_loss: B = 32: 2.84 / 1.13, 256: 2.85 / 1.22, 1024: 2.89 / 1.40, 2048: 2.93 /
# 2.50, 4096: 3.01 / 3.83. Every evaluate round is below every baseline round at 4096 only.
STREAM_EVAL_M128_MIN_B = 4096


def plan_forward(d: _lib.Dims, fused_ok: bool, *, path: str = "auto", record: bool = False,
                 train_split: bool = False) -> ForwardPlan:
    """The dispatch table of forward_raw's docstring as data. No tensors, no allocation, no
    launch: only the library's size queries, which depend on the CURRENT device's CU count
    (callers enter ``torch.cuda.device`` first). fused_ok: GraphBatch.fused_ok."""
    if path not in ("auto", "fused", "split", "tiled", "stepwise"):
        raise ValueError(f"unknown path {path!r}")
    if path in ("fused", "split") and not fused_ok:
        raise ValueError("the fused kernel follows non-ascending adjacency orders only for "
                         "P <= 8; use path='auto' or 'stepwise'")
    L, dp = _lib.load(), ctypes.byref(d)
    # small batches split the columns; a recording forward only where train_split opts in
    try_split = path == "split" or (path == "auto" and fused_ok and (not record or train_split))
    split_b = L.dadmm_split_scratch_bytes(dp) if try_split else 0
    if path == "split" and not split_b:
        raise ValueError(f"the column-split forward does not serve B={d.B} P={d.P} n={d.n} "
                         "(n_pad 128 or 256, P <= 6, m <= 64, ceil(B/16) <= CUs/2)")
    tiled = "tiled_record" if record else "tiled"
    table = {"auto": ("fused", tiled) if fused_ok else (tiled,), "fused": ("fused",),
             "tiled": (tiled,), "stepwise": ()}
    candidates = ("split",) if split_b else table[path]
    if path == "auto" and record and d.m > 64 and d.B < STREAM_RECORD_M128_MIN_B:
        candidates = tuple(c for c in candidates if c != "tiled_record")   # the stepwise launch records
    gated = path in ("auto", "stepwise")
    flag_b = L.dadmm_split_flag_bytes(dp) if split_b else 0
    return ForwardPlan(candidates, gated, split_b, flag_b,
                       L.dadmm_stepwise_scratch_bytes(dp) if gated else 0,
                       (256 + flag_b + (_sw_flag_bytes(d.K) if gated else 0)) // 4)


# The forward launchers. ``a`` (forward_raw) holds what they share: the two pointer prefixes
# (d, op, b, <graph>, deg, hyp, y0, U0, d0, Y), each built once, and the pieces of their tails.
# Each returns (entry point, return code); the record bit picks the *_record entry, looked up on
# the library at every call (bench.py times the kernel by replacing L.dadmm_forward).
def _launch_fused(a):
    fn = "dadmm_forward_record" if a.rec else "dadmm_forward"
    return fn, getattr(a.L, fn)(*a.ordered, *a.rec, a.U, a.status, a.stream)


def _launch_split(a):
    fn = "dadmm_forward_split_record" if a.rec else "dadmm_forward_split"
    xbuf = torch.empty(a.plan.split_bytes, dtype=torch.uint8, device=a.device)
    return fn, getattr(a.L, fn)(*a.ordered, *a.rec, a.U, a.status, a.sflags, _ptr(xbuf), a.stream)


def _launch_tiled(a):
    fn = "dadmm_forward_tiled_record" if a.rec else "dadmm_forward_tiled"
    tscratch = torch.empty(max(a.L.dadmm_tiled_scratch_bytes(a.dp), 256), dtype=torch.uint8,
                           device=a.device)
    return fn, getattr(a.L, fn)(*a.visits, *a.rec, a.U, a.status, _ptr(tscratch), a.stream)


_FORWARD_LAUNCHERS = {"fused": _launch_fused, "split": _launch_split, "tiled": _launch_tiled,
                      "tiled_record": _launch_tiled}


def forward_raw(op: PreparedOperator, b: torch.Tensor, graphs: GraphBatch, hyp: torch.Tensor,
                y0: torch.Tensor = None, U0: torch.Tensor = None, d0: torch.Tensor = None, *,
                variant: int = _lib.VARIANT_UNFOLDED, want_U: bool = False, path: str = "auto",
                record: bool = False, train_split: bool = False):
    """The K-step forward with the reference's NaN/Inf guards, enqueued on the current stream
    (no host synchronisation). Shapes: b [B,P,m], hyp [K,H,4], y0/U0/d0 [B,P,n].

    What runs is plan_forward's table. Candidates are tried in order: on "auto" one that returns
    DADMM_EUNSUPPORTED is skipped, anything else raises. gated: the stepwise launch follows; it
    recomputes the batch only if a guard event was flagged (all of it if no candidate ran).
    Forced "fused" / "split" / "tiled" do NOT apply the guards: their status only flags them.

      path      when                                              candidates             gated
      auto      fused_ok, split serves, not record or train_split split                  yes
      auto      fused_ok, otherwise                               fused, tiled[_record]  yes
      auto      not fused_ok                                      tiled[_record]         yes
      auto      record, m > 64, B < STREAM_RECORD_M128_MIN_B      the above less tiled_record
      fused     fused_ok, else ValueError                         fused                  no
      split     fused_ok and split serves, else ValueError        split                  no
      tiled                                                       tiled[_record]         no
      stepwise                                                    none                   yes

    fused_ok: graphs.fused_ok. split serves: dadmm_split_scratch_bytes != 0 (n_pad 128 / 256,
    P <= 6, m <= 64, the fused tiles fill at most half the CUs); GEMM1 then runs in the split
    order (``split_cols``), which differs from the fused order in fp32 rounding.

    record: also store the trajectory the adjoint consumes (the *_record entry of each launcher;
    tiled_record is the streamed single launch, P <= 16 at m <= 64 or P <= 8 at m <= 128 —
    ``tiled_form(d, record=True) == 1`` —, and unsupported elsewhere; the stepwise kernels record
    when they run). It keeps the fused order at every batch size unless train_split (ignored
    without record) or path "split" opts into the split order; the adjoints consume either.

    y0 = U0 = d0 = None: the reference's random inits are drawn by the prologue launch
    (draw_inits; bit-identical to torch.randn * 1e-2 from the device's default generator).

    Returns (Y [K,B,P,n], U_K [B,P,n] or None, status int32 device tensor [1]), plus, with
    ``record``, a ``Trajectory`` as a fourth element."""
    _dev_check(b, hyp, y0, U0, d0, graphs.nbr, graphs.deg)
    draw = y0 is None
    if draw != (U0 is None) or draw != (d0 is None):
        raise ValueError("pass all of y0, U0, d0 or none of them")
    B, P, m = b.shape
    if P != op.P or m != op.m:
        raise ValueError(f"b is [B,{P},{m}], operator is P={op.P}, m={op.m}")
    K, H = int(hyp.shape[0]), int(hyp.shape[1])
    ns, dev, L = op.n_store, b.device, _lib.load()
    d = op.dims(B=B, K=K, variant=variant, hyp_rows=H, graph_shared=graphs.shared)
    with torch.cuda.device(dev):
        plan = plan_forward(d, graphs.fused_ok, path=path, record=record, train_split=train_split)
        b, hyp = b.contiguous().float(), hyp.contiguous().float()
        Y = torch.empty((K, B, P, ns), dtype=torch.float32, device=dev)
        U = torch.empty((B, P, ns), dtype=torch.float32, device=dev) if want_U else None
        rec = tuple(torch.empty_like(Y) for _ in range(2 if record else 0))   # Grec, Urec
        # one device allocation: [status word | 252 B pad | split epoch words | stepwise scratch
        # (guard flags first)]; the prologue zeroes the status word, the epoch words and the
        # guard flags in the same launch as the draws
        flag_b = plan.split_flag_bytes
        words = torch.empty(256 + flag_b + max(plan.stepwise_bytes, 256), dtype=torch.uint8,
                            device=dev)
        status, scratch = words[:4].view(torch.int32), words[256 + flag_b:]
        if draw:
            y0, U0, d0 = draw_inits((B, P, op.n), dev, ns, zero=words, nzero=plan.nzero)
        else:
            y0, U0, d0 = (_pad_n(x, ns).contiguous().float() for x in (y0, U0, d0))
            _lib.check("dadmm_prologue", L.dadmm_prologue(
                0, 0, 0, 1, 1, 0.0, 0.0, None, None, None, _ptr(words), plan.nzero, _stream(dev)))
        head = (ctypes.byref(d), _ptr(op.workspace), _ptr(b))
        tail = (_ptr(graphs.deg), _ptr(hyp), _ptr(y0), _ptr(U0), _ptr(d0), _ptr(Y))
        a = types.SimpleNamespace(
            L=L, dp=head[0], plan=plan, device=dev, stream=_stream(dev),
            ordered=(*head, _ptr(graphs.nbr), _ptr(graphs.order), *tail),     # fused, split
            visits=(*head, _ptr(graphs.vptr), _ptr(graphs.vq), *tail),        # tiled, stepwise
            rec=tuple(_ptr(x) for x in rec), U=_ptr(U), status=_ptr(status),
            sflags=_ptr(words[256:256 + flag_b]))
        ran = None
        for name in plan.candidates:
            fn, rc = _FORWARD_LAUNCHERS[name](a)
            if rc != _lib.DADMM_EUNSUPPORTED or path != "auto":
                _lib.check(fn, rc)
                ran = name
                break
        if plan.gated:
            gate = _lib.FLAGS_ZEROED | (_lib.GATE_ON if ran else 0)
            _lib.check("dadmm_forward_stepwise", L.dadmm_forward_stepwise(
                *a.visits, a.U, *(a.rec or (None, None)), a.status, gate, _ptr(scratch), a.stream))
    traj = Trajectory(Y, *rec, y0, d0, hyp, variant, ran in ("fused", "split")) if record else None
    if ns != op.n:
        Y = Y[..., : op.n]
        U = U[..., : op.n] if U is not None else None
    return (Y, U, status, traj) if record else (Y, U, status)


def _split_cols(d, fused_ok, record=False, train_split=False):
    plan = plan_forward(d, fused_ok, record=record, train_split=train_split)
    return 64 if "split" in plan.candidates else 0


def split_cols(op: PreparedOperator, B: int, K: int, graphs: GraphBatch = None, hyp_rows: int = 1,
               record: bool = False, train_split: bool = False) -> int:
    """The GEMM1 slice width forward_raw's "auto" path uses for this batch: 64 when it runs the
    column-split forward (dadmm_forward_split; with ``record``, dadmm_forward_split_record, which
    needs ``train_split``), else 0 (the oracle's ``split_cols`` argument). graphs None: a shared
    graph the fused kernel follows."""
    shared = graphs.shared if graphs is not None else 1
    d = op.dims(B=B, K=K, hyp_rows=hyp_rows, graph_shared=shared)
    with torch.cuda.device(op.device):
        return _split_cols(d, graphs is None or graphs.fused_ok, record, train_split)


def tiled_form(dims_or_shape, record: bool = False) -> int:
    """Which form the tiled launcher runs (dadmm_tiled_form; no GPU needed): 1 the streamed single
    launch, 0 the per-iteration launches, or the negative DADMM_E* code the entry point would
    return for the shape (``record``: dadmm_forward_tiled_record, which has the streamed form
    only). It reads DADMM_TILED_STREAM / DADMM_STREAM_WAVES as the launch does. dims_or_shape: a
    ``_lib.Dims``, or (P, m, n) for a batch of 16, K = 1, one hyper-parameter row, a shared graph
    (none of which the choice depends on)."""
    d = dims_or_shape
    if not isinstance(d, _lib.Dims):
        P, m, n = d
        d = _lib.Dims(B=16, P=P, m=m, n=n, K=1, variant=_lib.VARIANT_UNFOLDED, hyp_rows=1,
                      graph_shared=1)
    return int(_lib.load().dadmm_tiled_form(ctypes.byref(d), 1 if record else 0))


def eval_served(dims_or_op, B: int, K: int, graphs: GraphBatch = None) -> bool:
    """Whether the evaluation forward (forward_eval_raw, dadmm_forward_eval) serves the shape
    (dadmm_forward_eval_scratch_bytes != 0; no GPU needed): P <= 5, 128 < n <= 256, m <= 64 and
    one shared graph. dims_or_op: a ``PreparedOperator`` or a ``_lib.Dims`` (whose B, K and
    graph_shared are replaced). graphs None: a shared graph."""
    if graphs is not None and not (graphs.shared and graphs.fused_ok):
        return False
    o = dims_or_op
    n = o.n_store if isinstance(o, PreparedOperator) else (o.n + 3) & ~3
    d = _lib.Dims(B=B, P=o.P, m=o.m, n=n, K=K, variant=_lib.VARIANT_UNFOLDED, hyp_rows=1,
                  graph_shared=1)
    return _lib.load().dadmm_forward_eval_scratch_bytes(ctypes.byref(d)) != 0


def forward_eval_raw(op: PreparedOperator, b: torch.Tensor, graphs: GraphBatch, hyp: torch.Tensor,
                     label: torch.Tensor, y0: torch.Tensor = None, U0: torch.Tensor = None,
                     d0: torch.Tensor = None, *, variant: int = _lib.VARIANT_UNFOLDED,
                     want_U: bool = False):
    """The K-step forward and the drivers' loss on its iterates (gnn_dlasso_utils.compute_loss,
    reference gnn_dlasso_utils.py:27-88) without storing the iterates: the role-split kernel sums
    every iterate's squared error against ``label`` [B,n] where it holds the iterate in registers
    and stores only the last one. Three launches on the current stream (prologue, evaluation
    kernel, loss finish), no host synchronisation, one scratch allocation.

    Like forward_raw's forced paths it does NOT apply the reference's guards: ``status`` flags
    them, and without the iterates nothing here can recompute the batch (DLASSO_unfolded.evaluate
    does, through the ordinary forward). y0 = U0 = d0 = None: drawn by the prologue launch exactly
    as forward_raw draws them (same values, same generator advance).

    Returns (losses [K], out [2] = (loss_mean, loss_final) with the reference's (1, 1) fallback,
    y_final [B,P,n] = forward_raw's Y[-1] bit for bit, U_K [B,P,n] or None, status int32 [1],
    loss_flags int32 [2] (non-finite label seen, fallback fired), (y0, U0, d0) as used).
    Raises ValueError where ``eval_served`` is False."""
    _dev_check(b, hyp, label, y0, U0, d0, graphs.nbr, graphs.deg)
    draw = y0 is None
    if draw != (U0 is None) or draw != (d0 is None):
        raise ValueError("pass all of y0, U0, d0 or none of them")
    B, P, m = b.shape
    if P != op.P or m != op.m:
        raise ValueError(f"b is [B,{P},{m}], operator is P={op.P}, m={op.m}")
    K, H = int(hyp.shape[0]), int(hyp.shape[1])
    if not eval_served(op, B, K, graphs):
        raise ValueError(f"the evaluation forward does not serve B={B} K={K} P={P} m={m} n={op.n} "
                         "(P <= 5, 128 < n <= 256, m <= 64, one shared graph the fused kernel follows)")
    if label.numel() != B * op.n:
        raise ValueError(f"label must hold [B={B}, n={op.n}] values, got {tuple(label.shape)}")
    ns, dev, L = op.n_store, b.device, _lib.load()
    d = op.dims(B=B, K=K, variant=variant, hyp_rows=H, graph_shared=1)
    with torch.cuda.device(dev):
        b, hyp = b.contiguous().float(), hyp.contiguous().float()
        label = _pad_n(label.reshape(B, op.n).float(), ns).contiguous()
        y_final = torch.empty((B, P, ns), dtype=torch.float32, device=dev)
        U = torch.empty((B, P, ns), dtype=torch.float32, device=dev) if want_U else None
        res = torch.empty(K + 2, dtype=torch.float32, device=dev)      # losses, then out
        # one allocation: [status word | 12 B pad | loss flags (2 words) | pad to 256 B | partial
        # sums]; the prologue zeroes the first 256 B in the same launch as the draws
        words = torch.empty(256 + L.dadmm_forward_eval_scratch_bytes(ctypes.byref(d)),
                            dtype=torch.uint8, device=dev)
        status, flags = words[:4].view(torch.int32), words[16:24].view(torch.int32)
        if draw:
            y0, U0, d0 = draw_inits((B, P, op.n), dev, ns, zero=words, nzero=64)
        else:
            y0, U0, d0 = (_pad_n(x, ns).contiguous().float() for x in (y0, U0, d0))
            _lib.check("dadmm_prologue", L.dadmm_prologue(
                0, 0, 0, 1, 1, 0.0, 0.0, None, None, None, _ptr(words), 64, _stream(dev)))
        _lib.check("dadmm_forward_eval", L.dadmm_forward_eval(
            ctypes.byref(d), _ptr(op.workspace), _ptr(b), _ptr(graphs.nbr), None, _ptr(graphs.deg),
            _ptr(hyp), _ptr(y0), _ptr(U0), _ptr(d0), _ptr(label), op.n, _ptr(y_final), _ptr(U),
            _ptr(res), _ptr(res[K:]), _ptr(flags), _ptr(words[256:]), _ptr(status), _stream(dev)))
    if ns != op.n:
        y_final = y_final[..., : op.n]
        U = U[..., : op.n] if U is not None else None
        y0, U0, d0 = (x[..., : op.n] for x in (y0, U0, d0))
    return res[:K], res[K:], y_final, U, status, flags, (y0, U0, d0)


def eval_stream_served(dims_or_op, B: int, K: int, graphs: GraphBatch = None) -> bool:
    """Whether the streamed evaluation forward (forward_eval_stream_raw, dadmm_forward_eval_stream)
    serves the shape (dadmm_forward_eval_stream_scratch_bytes != 0; no GPU needed): the streamed
    single launch's shapes (P <= 16 at m <= 64, P <= 8 at m <= 128, n_pad >= 128) that the fused
    forward has no kernel for (P > 6, P = 6 at n_pad > 128, n_pad > 256 or m > 64), with shared or
    per-sample graphs. dims_or_op: a ``PreparedOperator`` or a ``_lib.Dims`` (whose B, K and
    graph_shared are replaced). graphs None: a shared graph; otherwise it must carry the visit
    lists of at most 16 agents."""
    o = dims_or_op
    if graphs is not None and (graphs.vptr is None or graphs.vq is None or o.P > 16):
        return False
    n = o.n_store if isinstance(o, PreparedOperator) else (o.n + 3) & ~3
    d = _lib.Dims(B=B, P=o.P, m=o.m, n=n, K=K, variant=_lib.VARIANT_UNFOLDED, hyp_rows=1,
                  graph_shared=1 if graphs is None else int(graphs.shared))
    return _lib.load().dadmm_forward_eval_stream_scratch_bytes(ctypes.byref(d)) != 0


def forward_eval_stream_raw(op: PreparedOperator, b: torch.Tensor, graphs: GraphBatch,
                            hyp: torch.Tensor, label: torch.Tensor, y0: torch.Tensor = None,
                            U0: torch.Tensor = None, d0: torch.Tensor = None, *,
                            variant: int = _lib.VARIANT_UNFOLDED, want_U: bool = False):
    """forward_eval_raw on the streamed forward (csrc/dadmm_stream.hip's evaluation kernels): the
    K-step forward and the drivers' loss on its iterates with two iterates of state (y_final and
    one in scratch, taking turns) instead of K. Same arguments, same contract (the guards are only
    flagged in ``status``; drawn inits as forward_raw draws them) and same return tuple as
    forward_eval_raw; y_final equals forward_raw's Y[-1] bit for bit. Three launches on the
    current stream (prologue, evaluation kernel, loss finish), no host synchronisation, one scratch
    allocation. It serves every batch size; raises ValueError where ``eval_stream_served`` is
    False."""
    _dev_check(b, hyp, label, y0, U0, d0, graphs.vptr, graphs.deg)
    draw = y0 is None
    if draw != (U0 is None) or draw != (d0 is None):
        raise ValueError("pass all of y0, U0, d0 or none of them")
    B, P, m = b.shape
    if P != op.P or m != op.m:
        raise ValueError(f"b is [B,{P},{m}], operator is P={op.P}, m={op.m}")
    K, H = int(hyp.shape[0]), int(hyp.shape[1])
    if not eval_stream_served(op, B, K, graphs):
        raise ValueError(f"the streamed evaluation forward does not serve B={B} K={K} P={P} m={m} "
                         f"n={op.n} (P <= 16 at m <= 64, P <= 8 at m <= 128, n_pad >= 128, and no "
                         "shape of the fused forward: P > 6, P = 6 at n > 128, n > 256 or m > 64)")
    if label.numel() != B * op.n:
        raise ValueError(f"label must hold [B={B}, n={op.n}] values, got {tuple(label.shape)}")
    ns, dev, L = op.n_store, b.device, _lib.load()
    d = op.dims(B=B, K=K, variant=variant, hyp_rows=H, graph_shared=graphs.shared)
    with torch.cuda.device(dev):
        b, hyp = b.contiguous().float(), hyp.contiguous().float()
        label = _pad_n(label.reshape(B, op.n).float(), ns).contiguous()
        y_final = torch.empty((B, P, ns), dtype=torch.float32, device=dev)
        U = torch.empty((B, P, ns), dtype=torch.float32, device=dev) if want_U else None
        res = torch.empty(K + 2, dtype=torch.float32, device=dev)      # losses, then out
        # one allocation: [status word | 12 B pad | loss flags (2 words) | pad to 256 B | U state |
        # second iterate | partial sums]; the prologue zeroes the first 256 B with the draws
        words = torch.empty(256 + L.dadmm_forward_eval_stream_scratch_bytes(ctypes.byref(d)),
                            dtype=torch.uint8, device=dev)
        status, flags = words[:4].view(torch.int32), words[16:24].view(torch.int32)
        if draw:
            y0, U0, d0 = draw_inits((B, P, op.n), dev, ns, zero=words, nzero=64)
        else:
            y0, U0, d0 = (_pad_n(x, ns).contiguous().float() for x in (y0, U0, d0))
            _lib.check("dadmm_prologue", L.dadmm_prologue(
                0, 0, 0, 1, 1, 0.0, 0.0, None, None, None, _ptr(words), 64, _stream(dev)))
        _lib.check("dadmm_forward_eval_stream", L.dadmm_forward_eval_stream(
            ctypes.byref(d), _ptr(op.workspace), _ptr(b), _ptr(graphs.vptr), _ptr(graphs.vq),
            _ptr(graphs.deg), _ptr(hyp), _ptr(y0), _ptr(U0), _ptr(d0), _ptr(label), op.n,
            _ptr(y_final), _ptr(U), _ptr(res), _ptr(res[K:]), _ptr(flags), _ptr(words[256:]),
            _ptr(status), _stream(dev)))
    if ns != op.n:
        y_final = y_final[..., : op.n]
        U = U[..., : op.n] if U is not None else None
        y0, U0, d0 = (x[..., : op.n] for x in (y0, U0, d0))
    return res[:K], res[K:], y_final, U, status, flags, (y0, U0, d0)


def hyper_form(kind: str, B: int, P: int, K: int, N: int, K1=None):
    """Which kernel form a hypernetwork launch takes (dadmm_hyper_form; no GPU needed, nothing
    launched). kind: "linear", "gcn", "head", "gcn_train", "linear_gcn_bwd" (B samples of P nodes;
    rows = B and P unused for "linear" / "head", where N = 4 H) or "gcn_bwd" (the stand-alone GCN
    block backward: K unused). Returns a dict: wr (row tile / 32), dma (the LDS-DMA ring), ks (2: the
    K loop split over two wave sets), split (K1 < K), gcn32 (the 32x32 inference kernel), nt / pr
    ("gcn_bwd" only), grid, samples_per_tile; or the negative DADMM_E* code the launch would fail
    with (``_lib.load().dadmm_last_error()`` has its text). It reads DADMM_GCN32 / DADMM_HYPER_KW as
    the launch does."""
    f = _lib.HyperForm()
    rc = int(_lib.load().dadmm_hyper_form(_lib.HYPER_FORM_KINDS[kind], B, P, K, N, K if K1 is None else K1,
                                          ctypes.byref(f)))
    return rc if rc != _lib.DADMM_OK else f.as_dict()


class Trajectory:
    """What the adjoint consumes: the n-padded iterates Y, pre-clamp gradients Grec and dual
    states Urec ([K,B,P,n_store] each), the inits y0 / d0 and the hyper-parameter table;
    ``fused``: recorded by the fused kernel (its on-chip adjoint applies), else by the stepwise
    path (the general adjoint)."""

    __slots__ = ("Y", "Grec", "Urec", "y0", "d0", "hyp", "variant", "fused")

    def __init__(self, Y, Grec, Urec, y0, d0, hyp, variant, fused=False):
        self.Y, self.Grec, self.Urec = Y, Grec, Urec
        self.y0, self.d0, self.hyp, self.variant, self.fused = y0, d0, hyp, variant, fused


def backward_raw(op: PreparedOperator, graphs: GraphBatch, traj: Trajectory,
                 gY: torch.Tensor, path: str = "auto") -> torch.Tensor:
    """dL/dhyp [K,H,4] for L = sum_k <gY[k], Y[k]> along ``traj``, enqueued on the current
    stream. gY: [K,B,P,n] (n or n_store columns).

    path "auto": the fused adjoint (dadmm_backward: one launch, state on chip) for a fused
    trajectory, otherwise the general adjoint (dadmm_adjoint: any P <= 64, any m, n); "fused" /
    "general" force one."""
    _dev_check(gY)
    if path not in ("auto", "fused", "general"):
        raise ValueError(f"unknown path {path!r}")
    # compute_delta is the sum over its visits (p, q) of (e_p - e_q)(e_p - e_q)^T: symmetric for
    # ANY adjacency, so every adjoint applies it through the forward's own visit order. Only the
    # fused adjoint's shared-graph consensus (consensus_fma) reads one edge multiplier per
    # unordered pair: a directed SHARED graph takes the general adjoint (its visit lists follow
    # the successor lists); per-sample graphs are direction-aware in either adjoint.
    directed_shared = graphs.shared and not getattr(graphs, "symmetric", True)
    K, B, P, ns = traj.Y.shape
    H = int(traj.hyp.shape[1])
    gY = _pad_n(gY.float(), ns).contiguous()
    if tuple(gY.shape) != (K, B, P, ns):
        raise ValueError(f"gY must be [{K},{B},{P},{op.n}], got {tuple(gY.shape)}")
    if path == "fused" and directed_shared:
        raise ValueError("the fused adjoint assumes a symmetric shared adjacency; use 'auto' or "
                         "'general' for a directed shared graph")
    if path == "fused" and not graphs.fused_ok:
        raise ValueError("the fused adjoint follows non-ascending adjacency orders only "
                         "for P <= 8; use path='auto' or 'general'")
    use_fused = path == "fused" or (path == "auto" and traj.fused and graphs.fused_ok
                                    and not directed_shared)
    d = op.dims(B=B, K=K, variant=traj.variant, hyp_rows=H, graph_shared=graphs.shared)
    L, dp, dev = _lib.load(), ctypes.byref(d), gY.device
    dhyp = torch.empty((K, H, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        def launch(fn, g0, g1, scratch):   # nbr / order (fused adjoint) or the visit lists
            return fn(dp, *(_ptr(t) for t in (
                op.workspace, g0, g1, graphs.deg, traj.hyp, traj.y0, traj.d0, traj.Y, traj.Grec,
                traj.Urec, gY, dhyp, scratch)), _stream(dev))
        if use_fused:
            nbytes = L.dadmm_backward_scratch_bytes(dp)
            scratch = torch.empty(max(nbytes, 16) // 4 + 4, dtype=torch.float32, device=dev)
            rc = launch(L.dadmm_backward, graphs.nbr, graphs.order, scratch)
            if rc != _lib.DADMM_EUNSUPPORTED or path == "fused":
                _lib.check("dadmm_backward", rc)
                return dhyp
        scratch = torch.empty(max(L.dadmm_adjoint_scratch_bytes(dp), 256), dtype=torch.uint8,
                              device=dev)
        _lib.check("dadmm_adjoint", launch(L.dadmm_adjoint, graphs.vptr, graphs.vq, scratch))
    return dhyp


def describe_status(st: int) -> list:
    """The reference's warnings (unfolded_DLASSO.py:56-104) for the guard bits in ``st``."""
    out = []
    if st & _lib.STATUS_Y_NONFINITE:
        out.append("NaN/Inf detected in y_k, reset to zeros")
    if st & _lib.STATUS_U_NONFINITE:
        out.append("NaN/Inf detected in U_k, reset to zeros")
    if st & _lib.STATUS_GRAD_NAN:
        out.append("NaN/Inf in gradient, update skipped")
    if st & _lib.STATUS_YNEXT_NAN:
        out.append("NaN/Inf in y_next, previous value kept")
    if st & _lib.STATUS_RECOMPUTE:
        out.append("fused kernel: asymmetric shared adjacency, batch needs the guarded recomputation")
    if st & _lib.STATUS_BARRIER_TIMEOUT:
        out.append("stepwise grid barrier timed out: Y is invalid (device shared with other work)")
    return out
