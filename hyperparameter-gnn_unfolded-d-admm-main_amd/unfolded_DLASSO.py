"""Drop-in ``unfolded_DLASSO`` module: ``DLASSO_unfolded`` and ``seq_hyperparam``.

Mirrors the reference's public interface (unfolded_DLASSO.py:9-168): constructor ``(A, args)``,
``forward(b, graph_list, K=None) -> (Y [K',B,P,n,1], hyp [H,4,1])`` with ``K' = min(K, self.K)``,
state_dict ``{'seq_hyp.param': [K, P|1, 4]}``, and ``seq_hyp(k)``. On CUDA tensors the K-step
recurrence runs in one fused HIP launch (``dadmm_hip``, C ABI ``include/dadmm.h``); CPU tensors
(the reference's default device) run its op sequence in torch eager ops (``dadmm_cpu``).
"""
from __future__ import annotations

import collections

import torch
import torch.nn as nn

import dadmm_cpu
from dadmm_hip import _lib
from dadmm_hip.autograd import check_status, dadmm_unfolded_apply, tag_status
from dadmm_hip.ops import describe_status
from dadmm_hip.graph import ingest, n_graphs
from dadmm_hip.ops import PreparedOperator

# what DLASSO_unfolded.evaluate returns
Evaluation = collections.namedtuple("Evaluation",
                                    "losses loss_mean loss_final y_final hyp status")


class DLASSO_unfolded(nn.Module):
    """Unfolded D-ADMM for distributed LASSO (reference: unfolded_DLASSO.py:9-146)."""

    def __init__(self, A, args):
        super().__init__()
        # A [1, P, m, n] — a plain attribute, as in the reference (:13): not a buffer
        self.A = A
        _, self.P, self.m, self.n = self.A.shape
        self.K = args.GHN_iter_num
        self.DADMM_mode = args.DADMM_mode
        if args.DADMM_mode == 'same':
            hyp_shape = [self.K, 1, 4]
        else:
            hyp_shape = [self.K, self.P, 4]
        max_param = torch.tensor([args.alpha_max, args.tau_max, args.rho_max, args.eta_max],
                                 device=A.device)
        self.seq_hyp = seq_hyperparam(hyp_shape, max_param, args)
        self.max_param = max_param.unsqueeze(0)
        self.args = args
        self._op = None
        self._op_key = None
        # device int32 [1]: DADMM_STATUS_* bits of the guards the last forward applied
        # (include/dadmm.h); read it with guard_warnings() (synchronises)
        self.last_status = None
        self._table = None
        self._table_key = None
        # opt-in (train_unfolded.py --train-split): a training forward (the table requires grad)
        # of a small batch runs the recording column-split kernel (dadmm_forward_split_record).
        # Its iterates follow the split GEMM1 order, which differs from the fused order in fp32
        # rounding. A plain attribute: no buffer, no parameter; CPU tensors ignore it.
        self.train_split = False

    # The reference precomputes AtA eagerly (:16). The HIP path never forms it; it is kept as a
    # lazily computed attribute for callers that read it.
    @property
    def AtA(self):
        A = self.A
        return torch.matmul(A.transpose(-1, -2), A)

    def operator(self) -> PreparedOperator:
        """The prepared operator for the current ``self.A`` (re-prepared if A changed)."""
        A = self.A
        key = (A.data_ptr(), A.device, tuple(A.shape), A._version)
        if self._op is None or self._op_key != key:
            self._op = PreparedOperator(A)
            self._op_key = key
        return self._op

    def hyp_table(self, K: int) -> torch.Tensor:
        """[K, H, 4] rows seq_hyp(0..K-1), differentiable w.r.t. seq_hyp.param. Outside autograd
        the table is memoised on (param version, K, train/eval mode)."""
        param = self.seq_hyp.param
        if torch.is_grad_enabled() and param.requires_grad:
            return self.seq_hyp.table(K)
        key = (param.data_ptr(), param._version, param.device, K, self.seq_hyp.training)
        if self._table_key != key:
            with torch.no_grad():
                self._table = self.seq_hyp.table(K)
            self._table_key = key
        return self._table

    def forward(self, b, graph_list, K=None, *, inits=None):
        """b [B,P,m,1]; graph_list: B networkx graphs on agents 0..P-1 (may repeat one object),
        or a ``dadmm_hip.graph.GraphBatch`` from an earlier ``ingest`` of them.

        ``inits`` (keyword-only, optional): (y0, U0, d0) each [B,P,n,1] or [B,P,n]; by default
        they are drawn like the reference (:49-51): randn * 1e-2 on b.device, in that order.
        """
        batch_size = max(len(b), n_graphs(graph_list, len(b)))
        device = b.device
        if K is None:
            K = self.K
        else:
            K = min(K, self.K)
        if K <= 0:
            # the reference's loop would not run and `hyp` would be unbound (NameError)
            raise RuntimeError(f"forward needs at least one iteration, got K={K}")
        if b.dim() != 4 or b.shape[1] != self.P or b.shape[2] != self.m:
            raise RuntimeError(f"b must be [B,{self.P},{self.m},1], got {tuple(b.shape)}")
        bb = b[..., 0]
        if len(b) != batch_size:
            if len(b) != 1:
                raise RuntimeError(
                    f"The size of tensor a ({len(b)}) must match the size of tensor b "
                    f"({batch_size}) at non-singleton dimension 0")
            bb = bb.expand(batch_size, -1, -1)
        graphs = ingest(graph_list, self.P, batch_size, device)

        if device.type == "cpu":
            # CPU tensors (the reference's default device): its op sequence in torch eager ops
            # (dadmm_cpu); CUDA tensors never take this path
            if inits is None:
                y0, U0, d0 = (torch.randn((batch_size, self.P, self.n, 1), device=device) * 1e-2
                              for _ in range(3))                            # :49-51, in order
            else:
                y0, U0, d0 = inits
            table = self.seq_hyp.table(K)
            Y, st = dadmm_cpu.unfolded_forward(self.A, bb, graphs, table, K, (y0, U0, d0))
            self.last_status = torch.tensor([st], dtype=torch.int32)
            return tag_status(Y.unsqueeze(-1), self.last_status), table[K - 1].unsqueeze(-1)

        if inits is None:
            # drawn by the forward's prologue launch: == torch.randn((B,P,n,1)) * 1e-2 x 3 value
            # for value, same generator stream (tests/test_gpu_parity.py::
            # test_prologue_draws_match_torch)
            y0 = U0 = d0 = None
        else:
            y0, U0, d0 = (x.reshape(batch_size, self.P, self.n) for x in inits)

        table = self.hyp_table(K)                       # [K, H, 4]
        Y, self.last_status = dadmm_unfolded_apply(self.operator(), bb, graphs, table, y0, U0,
                                                   d0, _lib.VARIANT_UNFOLDED,
                                                   train_split=bool(self.train_split))
        hyp = table[K - 1].unsqueeze(-1)                # seq_hyp(K-1): [H, 4, 1]
        return tag_status(Y.unsqueeze(-1), self.last_status), hyp

    def evaluate(self, b, graph_list, label, K=None, *, inits=None, on_guard="recompute"):
        """The validation step in one call: ``forward(b, graph_list, K)``, then
        ``gnn_dlasso_utils.compute_loss(Y, label)`` and ``layer_losses`` (the reference's loop,
        unfolded_train_new.py:102-125), without the iterates. label [B,n,1] or [B,n].

        Returns ``Evaluation(losses [K'], loss_mean, loss_final, y_final [B,P,n,1], hyp [H,4,1],
        status)``: the per-iterate losses, compute_loss's two scalars (with the reference's (1, 1)
        fallback), the last iterate, seq_hyp(K'-1) and the device status word. K' = min(K, self.K),
        the memoised table and the graph ingestion are forward's. No gradient flows: with a table
        that requires grad under enabled grad it raises (use ``forward`` to train).

        Where the evaluation kernel serves (CUDA tensors, one shared graph the fused kernel
        follows, P <= 5, 128 < n <= 256, m <= 64: ``dadmm_hip.ops.eval_served``) the K iterates
        are never stored: the losses are summed inside the fused forward (three launches, memory
        for a K times larger batch). Its losses equal compute_loss's up to fp32 summation order;
        y_final equals forward's Y[-1] bit for bit. A guard event cannot be repaired there, since
        the stepwise recomputation uses Y as its state:

          on_guard="recompute" (default) reads the 4-byte status word at the end: ONE host
            synchronisation (the drivers' validation loops synchronise on that word anyway,
            through ``timed_out`` on the next line). If any bit is set, an asymmetric shared
            adjacency's DADMM_STATUS_RECOMPUTE included, the batch is rerun through ``forward``
            with the same draws plus compute_loss: the result is that path's, bit for bit.
          on_guard="flag" never synchronises: where status != 0 the losses and y_final are NaN,
            selected on the device, and the status word rides on them (``timed_out`` /
            ``raise_if_timed_out`` read it).

        Where that kernel does not serve but the streamed forward's evaluation form does (CUDA
        tensors, shared or per-sample graphs, P <= 16 at m <= 64 or P <= 8 at m <= 128, n > 64, and
        no shape of the fused forward: P > 6, P = 6 at n > 128, n > 256 or m > 64:
        ``dadmm_hip.ops.eval_stream_served``; BASELINE configs[2] and the reference's default
        shape P = 5, m = 100, n = 500 are such shapes) the same holds with two iterates of state
        instead of K, the same three launches and the same two ``on_guard`` policies. At m > 64 it
        is taken from a batch of ``dadmm_hip.ops.STREAM_EVAL_M128_MIN_B`` on: below it the
        forward's per-iteration launches are the faster step.

        Everywhere else (CPU tensors, ordered graphs on fused shapes, other shapes) it runs
        ``forward`` plus ``compute_loss`` plus ``layer_losses`` and returns the same tuple: same
        values as those calls, and NO memory saving."""
        import gnn_dlasso_utils
        from dadmm_hip import ops
        from dadmm_hip.ops import eval_served, eval_stream_served, forward_eval_raw, forward_eval_stream_raw
        if on_guard not in ("recompute", "flag"):
            raise ValueError(f"on_guard must be 'recompute' or 'flag', got {on_guard!r}")
        if torch.is_grad_enabled() and self.seq_hyp.param.requires_grad:
            raise RuntimeError("evaluate() computes no gradient: call it under torch.no_grad() "
                               "(or with a frozen table); training goes through forward() and "
                               "gnn_dlasso_utils.compute_loss")
        batch_size = max(len(b), n_graphs(graph_list, len(b)))
        Kp = self.K if K is None else min(K, self.K)

        def through_forward(inits):
            with torch.no_grad():
                Y, hyp = self.forward(b, graph_list, K, inits=inits)
                loss_mean, loss_final = gnn_dlasso_utils.compute_loss(Y, label)
                losses = gnn_dlasso_utils.layer_losses(Y, label.reshape(batch_size, self.n))
            return Evaluation(losses, loss_mean, loss_final, Y[-1], hyp, self.last_status)

        served = (b.device.type == "cuda" and Kp > 0 and b.dim() == 4 and len(b) == batch_size
                  and b.shape[1] == self.P and b.shape[2] == self.m)
        eval_raw = forward_eval_raw
        if served:
            graphs = ingest(graph_list, self.P, batch_size, b.device)
            served = eval_served(self.operator(), batch_size, Kp, graphs)
            if not served and eval_stream_served(self.operator(), batch_size, Kp, graphs):
                served = self.m <= 64 or batch_size >= ops.STREAM_EVAL_M128_MIN_B
                eval_raw = forward_eval_stream_raw
        if not served:
            return through_forward(inits)

        with torch.no_grad():
            table = self.hyp_table(Kp)
            y0, U0, d0 = (None,) * 3 if inits is None else (
                x.reshape(batch_size, self.P, self.n) for x in inits)
            losses, out, y_final, _, status, _, used = eval_raw(
                self.operator(), b[..., 0], graphs, table, label, y0, U0, d0)
            self.last_status = status
            if on_guard == "recompute":
                if check_status(status) != 0:      # the one host synchronisation
                    return through_forward(used)
            else:
                bad = status.reshape(-1)[0] != 0
                nan = torch.full((), float("nan"), dtype=torch.float32, device=b.device)
                losses, out, y_final = (torch.where(bad, nan, t) for t in (losses, out, y_final))
            hyp = table[Kp - 1].unsqueeze(-1)
            return Evaluation(tag_status(losses, status), tag_status(out[0], status),
                              tag_status(out[1], status), tag_status(y_final.unsqueeze(-1), status),
                              hyp, status)

    def guard_warnings(self):
        """The reference's NaN/Inf warnings (unfolded_DLASSO.py:56-104) for the last forward
        (synchronises with the device)."""
        if self.last_status is None:
            return []
        return describe_status(check_status(self.last_status))

    # kept for API parity with the reference (:111-146); not used by the HIP forward
    def compute_sum_neighbors(self, graph_list, device):
        g = ingest(graph_list, self.P, len(graph_list), device)
        deg = g.deg if not g.shared else g.deg.expand(len(graph_list), -1)
        return deg.reshape(len(graph_list), self.P, 1, 1).float()

    def compute_Atx(self, x):
        A = self.A.to(x.device)
        return torch.einsum('pmn,bpmc->bpnc', A[0], x)

    def compute_delta(self, graph_list, y1, y2=None, device=None):
        if y2 is None:
            y2 = y1
        delta = torch.zeros_like(y1, device=device)
        for b in range(len(graph_list)):
            graph = graph_list[b]
            for p in range(self.P):
                y_p = y1[b, p]
                for j in graph.neighbors(p):
                    diff = y_p - y2[b, j]
                    delta[b, p] += diff
                    delta[b, j] -= diff
        return delta

    def compute_loss(self, y_k, label):
        loss = 0.0
        for p in range(self.P):
            loss += torch.nn.functional.mse_loss(y_k[:, p], label)
        return loss / self.P


class seq_hyperparam(nn.Module):
    """Per-iteration (alpha, tau, rho, eta) table (reference: unfolded_DLASSO.py:148-168)."""

    def __init__(self, hyp_shape, max_param, args=None):
        super().__init__()
        self.param = nn.Parameter(torch.zeros(hyp_shape))
        self.max_param = max_param.unsqueeze(0)
        self.args = args

    def _finish(self, hyp):
        # hyp [..., H, 4]; training-mode penalty (:161-165), then clamp (:167)
        if self.training and self.args is not None:
            mean = hyp.sum(dim=(-2, -1)) / (hyp.shape[-2] * hyp.shape[-1])
            scale = torch.where(mean > self.args.max_penalty_threshold,
                                torch.as_tensor(self.args.penalty_reduction_factor,
                                                dtype=hyp.dtype, device=hyp.device),
                                torch.ones((), dtype=hyp.dtype, device=hyp.device))
            hyp = hyp * scale[..., None, None]
        return torch.clamp(hyp, min=1e-4, max=0.99)

    def forward(self, k):
        hyp = torch.sum(self.param[:k + 1], dim=0)
        hyp = torch.sigmoid(hyp) * self.max_param.to(hyp.device)
        return self._finish(hyp).unsqueeze(-1)

    def table(self, K):
        """All rows 0..K-1 at once: [K, H, 4] (cumulative sums instead of K prefix sums)."""
        hyp = torch.cumsum(self.param[:K], dim=0)
        hyp = torch.sigmoid(hyp) * self.max_param.to(hyp.device)
        return self._finish(hyp)
