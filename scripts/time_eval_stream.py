"""Timing probe: the validation step on the streamed evaluation forward (DLASSO_unfolded.evaluate ->
dadmm_forward_eval_stream) against forward + compute_loss, at a streamed shape and a list of batch
sizes, in ONE process, the legs alternated, HIP events. scripts/time_eval.py's method and helpers.

    python scripts/time_eval_stream.py --P 16 --m 64 --n 512 --B 4096 [--K 25] [--json OUT]
    python scripts/time_eval_stream.py --P 5 --m 100 --n 500 --B 32 256 1024 2048 4096

Per batch size, `rounds` rounds of `reps` back-to-back calls per leg, the first round dropped:
  module   model(b, graphs) + gnn_dlasso_utils.compute_loss against
           model.evaluate(..., on_guard="flag"), both drawing their inits. The forward is what
           forward runs by default (at m > 64 the per-iteration launches); evaluate is forced onto
           the streamed evaluation at every batch size (STREAM_EVAL_M128_MIN_B = 1 here): the sweep
           is what sets that threshold;
  kernel   one dadmm_forward_tiled call against one dadmm_forward_eval_stream call (the evaluation
           kernel and its one-workgroup finish launch), on the same preallocated inputs.
And the peak allocated bytes of one step of each module leg. The module routes to the new path at a
shape and batch only where every evaluate round is at or below every baseline round.
"""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from time_eval import _alternate, _peak, _summary  # noqa: E402  (sets sys.path for the package)

import gnn_dlasso_utils  # noqa: E402
import oracle as O  # noqa: E402
import unfolded_DLASSO  # noqa: E402
from dadmm_hip import _lib, ingest, ops  # noqa: E402
from dadmm_hip.ops import _ptr, _stream  # noqa: E402


def one_batch(a, B, dev):
    P, M, N, K = a.P, a.m, a.n, a.K
    A, b, _ = O.make_problem(P, M, N, B, seed=1)
    args = argparse.Namespace(GHN_iter_num=K, DADMM_mode="diff", alpha_max=0.1, tau_max=0.99, rho_max=0.99,
                              eta_max=0.99, max_penalty_threshold=0.8, penalty_reduction_factor=0.95)
    model = unfolded_DLASSO.DLASSO_unfolded(torch.from_numpy(A).to(dev)[None], args).to(dev).eval()
    with torch.no_grad():
        model.seq_hyp.param.copy_(0.3 * torch.randn(model.seq_hyp.param.shape,
                                                    generator=torch.Generator().manual_seed(1)))
    model.requires_grad_(False)
    graphs = ingest([O.er_graph(P, 0.5 if P <= 8 else 0.3, seed=7)] * B, P, B, dev)
    bt = torch.from_numpy(b).to(dev)[..., None]
    label = torch.randn((B, N, 1), device=dev)
    if not ops.eval_stream_served(model.operator(), B, K, graphs):
        raise SystemExit(f"the streamed evaluation does not serve P={P} m={M} n={N}")

    def base_step():
        with torch.no_grad():
            Y, _ = model(bt, graphs)
            return gnn_dlasso_utils.compute_loss(Y, label)

    def eval_step():
        return model.evaluate(bt, graphs, label, on_guard="flag")

    lb, ev = base_step(), eval_step()
    torch.cuda.synchronize()
    res = {"B": B, "status": {"forward": int(model.last_status.item()), "evaluate": int(ev.status.item())},
           "loss_final": {"forward+compute_loss": float(lb[1]), "evaluate": float(ev.loss_final)}}
    res["module"] = _summary(_alternate({"forward+compute_loss": base_step, "evaluate": eval_step},
                                        a.rounds, a.reps), "forward+compute_loss", "evaluate")
    res["peak_allocated_bytes"] = {"forward+compute_loss": _peak(base_step, dev), "evaluate": _peak(eval_step, dev)}

    # the entry points alone, on preallocated buffers
    L, op = _lib.load(), model.operator()
    ns = op.n_store
    d = op.dims(B=B, K=K, hyp_rows=P, graph_shared=1)
    dp = ctypes.byref(d)
    res["tiled_form"] = int(L.dadmm_tiled_form(dp, 0))
    hyp = model.hyp_table(K).contiguous()
    y0, U0, d0 = (1e-2 * torch.randn((B, P, ns), device=dev) for _ in range(3))
    Y = torch.empty((K, B, P, ns), device=dev)
    yf = torch.empty((B, P, ns), device=dev)
    lab = torch.nn.functional.pad(label.reshape(B, N), (0, ns - N)).contiguous()
    tscr = torch.empty(max(L.dadmm_tiled_scratch_bytes(dp), 256), dtype=torch.uint8, device=dev)
    words = torch.zeros(256 + L.dadmm_forward_eval_stream_scratch_bytes(dp), dtype=torch.uint8, device=dev)
    status, flags, out = words[:4].view(torch.int32), words[16:24].view(torch.int32), torch.empty(K + 2, device=dev)
    common = (dp, _ptr(op.workspace), _ptr(bt[..., 0].contiguous()), _ptr(graphs.vptr), _ptr(graphs.vq),
              _ptr(graphs.deg), _ptr(hyp), _ptr(y0), _ptr(U0), _ptr(d0))
    st = _stream(dev)

    def k_forward():
        _lib.check("dadmm_forward_tiled", L.dadmm_forward_tiled(*common, _ptr(Y), None, _ptr(status), _ptr(tscr), st))

    def k_eval():
        _lib.check("dadmm_forward_eval_stream", L.dadmm_forward_eval_stream(
            *common, _ptr(lab), N, _ptr(yf), None, _ptr(out), _ptr(out[K:]), _ptr(flags), _ptr(words[256:]),
            _ptr(status), st))

    k_forward(), k_eval()
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and torch.equal(yf, Y[-1])
    res["kernel"] = _summary(_alternate({"dadmm_forward_tiled": k_forward, "dadmm_forward_eval_stream": k_eval},
                                        a.rounds, a.reps), "dadmm_forward_tiled", "dadmm_forward_eval_stream")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--P", type=int, default=16)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--K", type=int, default=25)
    ap.add_argument("--B", type=int, nargs="+", default=[4096])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.rounds < 4 or a.reps < 30:
        raise SystemExit("at least 4 kept rounds of at least 30 calls")
    dev = torch.device("cuda", 0)
    ops.STREAM_EVAL_M128_MIN_B = 1     # evaluate on the streamed evaluation at every batch size
    res = {"shape": {"P": a.P, "m": a.m, "n": a.n, "K": a.K}, "rounds": a.rounds, "reps": a.reps,
           "device": torch.cuda.get_device_name(dev), "batches": []}
    for B in a.B:
        res["batches"].append(one_batch(a, B, dev))
        print(json.dumps(res["batches"][-1]), flush=True)
        if a.json:                                # (rewritten after every batch size)
            with open(a.json, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
