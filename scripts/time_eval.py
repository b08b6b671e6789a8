"""Timing probe: the validation step without stored iterates (DLASSO_unfolded.evaluate, the
evaluation forward dadmm_forward_eval) against today's forward + compute_loss, at the headline
shape, in ONE process, the two legs alternated, HIP events.

    python scripts/time_eval.py [--rounds 5] [--reps 30] [--B 4096] [--json OUT]

Two comparisons, `rounds` rounds of `reps` back-to-back calls per leg, the first round of each leg
dropped:
  module   model(b, graphs) + gnn_dlasso_utils.compute_loss     (prologue, forward, gate, memset,
           partial, finish) against model.evaluate(..., on_guard="flag") (prologue, evaluation
           kernel, finish); both draw their inits;
  kernel   one dadmm_forward call (the forward kernel alone) against one dadmm_forward_eval call
           (the evaluation kernel AND its one-workgroup finish launch: the entry point issues both),
           on the same preallocated inputs.
It also prints the peak allocated bytes of one step of each module leg
(torch.cuda.max_memory_allocated above what was allocated before the step). The baseline is
measured here, in the same run; nothing is compared against a recorded figure. A gain is claimed
only where every kept round of the evaluation leg lies below every kept round of the baseline.
"""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "hyperparameter-gnn_unfolded-d-admm-main_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gnn_dlasso_utils  # noqa: E402
import oracle as O  # noqa: E402
import unfolded_DLASSO  # noqa: E402
from dadmm_hip import _lib, ingest  # noqa: E402
from dadmm_hip.ops import _ptr, _stream  # noqa: E402

P, M, N, K = 5, 64, 256, 25
TRAINED = os.path.join(ROOT, "tests", "golden", "fixture_25_iter_general_learning_seq_hyp_param.npy")


def _round(f, reps):
    """ms per call over `reps` back-to-back calls between two HIP events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _alternate(legs, rounds, reps):
    """{name: [ms per round]} with the legs alternated round by round; round 0 of each is dropped."""
    ms = {k: [] for k in legs}
    for _ in range(rounds + 1):
        for name, f in legs.items():
            ms[name].append(_round(f, reps))
    return {k: v[1:] for k, v in ms.items()}


def _summary(ms, base, new):
    out = {k: {"rounds_ms": [round(x, 4) for x in v], "median_ms": round(float(np.median(v)), 4),
               "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in ms.items()}
    out["verdict"] = ("gain: every round of %s below every round of %s" % (new, base)
                      if max(ms[new]) < min(ms[base]) else
                      "loss: every round of %s above every round of %s" % (new, base)
                      if min(ms[new]) > max(ms[base]) else "no separation: the rounds overlap")
    out["baseline_round_range_ms"] = round(max(ms[base]) - min(ms[base]), 4)
    out["median_difference_ms"] = round(float(np.median(ms[new]) - np.median(ms[base])), 4)
    return out


def _peak(f, dev):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    f()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated(dev) - before)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.rounds < 4 or a.reps < 30:
        raise SystemExit("at least 4 kept rounds of at least 30 calls")
    B, dev = a.B, torch.device("cuda", 0)
    A, b, _ = O.make_problem(P, M, N, B, seed=1)
    args = argparse.Namespace(GHN_iter_num=K, DADMM_mode="diff", alpha_max=0.1, tau_max=0.99, rho_max=0.99,
                              eta_max=0.99, max_penalty_threshold=0.8, penalty_reduction_factor=0.95)
    model = unfolded_DLASSO.DLASSO_unfolded(torch.from_numpy(A).to(dev)[None], args).to(dev).eval()
    with torch.no_grad():
        model.seq_hyp.param.copy_(torch.from_numpy(np.load(TRAINED)).to(dev))
    model.requires_grad_(False)
    graphs = ingest([O.er_graph(P, 0.5, seed=7)] * B, P, B, dev)
    bt = torch.from_numpy(b).to(dev)[..., None]
    label = torch.randn((B, N, 1), device=dev)

    def base_step():
        with torch.no_grad():
            Y, _ = model(bt, graphs)
            return gnn_dlasso_utils.compute_loss(Y, label)

    def eval_step():
        return model.evaluate(bt, graphs, label, on_guard="flag")

    lb, ev = base_step(), eval_step()
    torch.cuda.synchronize()
    res = {"shape": {"B": B, "P": P, "m": M, "n": N, "K": K}, "rounds": a.rounds, "reps": a.reps,
           "device": torch.cuda.get_device_name(dev),
           "status": {"forward": int(model.last_status.item()), "evaluate": int(ev.status.item())},
           "loss_final": {"forward+compute_loss": float(lb[1]), "evaluate": float(ev.loss_final)}}
    res["module"] = _summary(_alternate({"forward+compute_loss": base_step, "evaluate": eval_step},
                                        a.rounds, a.reps), "forward+compute_loss", "evaluate")
    res["peak_allocated_bytes"] = {"forward+compute_loss": _peak(base_step, dev), "evaluate": _peak(eval_step, dev)}

    # the entry points alone, on preallocated buffers
    L, op = _lib.load(), model.operator()
    d = op.dims(B=B, K=K, hyp_rows=P, graph_shared=1)
    hyp = model.hyp_table(K).contiguous()
    y0, U0, d0 = (1e-2 * torch.randn((B, P, N), device=dev) for _ in range(3))
    Y = torch.empty((K, B, P, N), device=dev)
    yf, lab = torch.empty((B, P, N), device=dev), label.reshape(B, N).contiguous()
    words = torch.zeros(256 + L.dadmm_forward_eval_scratch_bytes(ctypes.byref(d)), dtype=torch.uint8, device=dev)
    status, flags, out = words[:4].view(torch.int32), words[16:24].view(torch.int32), torch.empty(K + 2, device=dev)
    common = (ctypes.byref(d), _ptr(op.workspace), _ptr(bt[..., 0].contiguous()), _ptr(graphs.nbr), None,
              _ptr(graphs.deg), _ptr(hyp), _ptr(y0), _ptr(U0), _ptr(d0))
    st = _stream(dev)

    def k_forward():
        _lib.check("dadmm_forward", L.dadmm_forward(*common, _ptr(Y), None, _ptr(status), st))

    def k_eval():
        _lib.check("dadmm_forward_eval", L.dadmm_forward_eval(
            *common, _ptr(lab), N, _ptr(yf), None, _ptr(out), _ptr(out[K:]), _ptr(flags), _ptr(words[256:]),
            _ptr(status), st))

    k_forward(), k_eval()
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and torch.equal(yf, Y[-1])
    res["kernel"] = _summary(_alternate({"dadmm_forward": k_forward, "dadmm_forward_eval": k_eval},
                                        a.rounds, a.reps), "dadmm_forward", "dadmm_forward_eval")
    text = json.dumps(res, indent=1)
    print(text)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
