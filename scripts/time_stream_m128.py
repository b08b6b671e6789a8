#!/usr/bin/env python3
"""A/B of the forward's forms at the reference's default shape (P = 5, m = 100, n = 500, K = 25,
one shared graph), DESIGN.md §4.1d's protocol: one process per comparison, the two forms
alternated round by round, HIP events around forward_raw, 2 s of warm-up, each round the median
of --launches launches, round 0 of every form reported but left out, outputs compared bitwise.

    python scripts/time_stream_m128.py --mode infer  --batch 32   [--out FILE]
    python scripts/time_stream_m128.py --mode record --batch 4096 [--out FILE]
    python scripts/time_stream_m128.py --mode train  [--pkg DIR]  [--out FILE]

infer:  path="tiled" with DADMM_TILED_STREAM=1 (the streamed single launch) against =0 (the
        per-iteration launches); the library reads the variable at every call.
record: record=True on path="tiled" (the streamed recording launch) against path="stepwise"
        (2K + 2 launches, what recorded this shape before the streamed form reached m <= 128).
train:  the module's training step on the shipped fixture (tests/golden/fixture_25_iter_*.npy) at
        B = 32: forward in train mode, compute_loss, loss_final.backward(). --pkg names another
        build's package directory (the parent commit's), timed by a process of its own.
The verdict is the three-ranges rule: every round of the first form below every round of the
second, and the difference of medians above three times the larger round-to-round range."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rounds_of(forms, run, rounds, launches, warmup_s):
    import torch
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warmup_s:
        for f in forms:
            run(f)
        torch.cuda.synchronize()
    out = {f: [] for f in forms}
    for _ in range(rounds + 1):
        for f in forms:
            pairs = []
            for _ in range(launches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(f)
                e1.record()
                pairs.append((e0, e1))
            torch.cuda.synchronize()
            out[f].append(statistics.median(a.elapsed_time(b) for a, b in pairs))
    return out


def verdict(forms, rounds):
    kept = {f: r[1:] for f, r in rounds.items()}
    if not all(kept.values()):   # --rounds 0: a profiling run
        return {}
    med = {f: statistics.median(r) for f, r in kept.items()}
    rng = {f: max(r) - min(r) for f, r in kept.items()}
    out = {"median_ms": med, "range_ms": rng}
    if len(forms) == 2:
        a, b = forms
        out["verdict"] = {"diff_ms": med[b] - med[a], "three_ranges_ms": 3 * max(rng.values()),
                          "every_round_below": max(kept[a]) < min(kept[b]),
                          "first_is_faster": max(kept[a]) < min(kept[b])
                          and med[b] - med[a] > 3 * max(rng.values())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["infer", "record", "train"], required=True)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--shape", default="5,100,500,25", help="P,m,n,K")
    ap.add_argument("--rounds", type=int, default=5, help="rounds per form after the discarded first")
    ap.add_argument("--launches", type=int, default=32)
    ap.add_argument("--warmup-s", type=float, default=2.0)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "hyperparameter-gnn_unfolded-d-admm-main_amd"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import oracle as O   # input generator only
    from dadmm_hip import PreparedOperator, forward_raw, ingest
    dev = torch.device("cuda:0")
    B = a.batch
    P, m, n, K = (int(x) for x in a.shape.split(","))
    out = {"mode": a.mode, "shape": {"B": B, "P": P, "m": m, "n": n, "K": K}, "launches": a.launches}

    if a.mode == "train":
        import argparse as ap_
        import gnn_dlasso_utils
        import unfolded_DLASSO
        gold = os.path.join(ROOT, "tests", "golden")
        A = np.load(os.path.join(gold, "fixture_25_iter_general_learning_A.npy"))
        param = np.load(os.path.join(gold, "fixture_25_iter_general_learning_seq_hyp_param.npy"))
        args = ap_.Namespace(GHN_iter_num=K, DADMM_mode="diff", alpha_max=0.1, tau_max=0.99, rho_max=0.99,
                             eta_max=0.99, max_penalty_threshold=0.8, penalty_reduction_factor=0.95)
        model = unfolded_DLASSO.DLASSO_unfolded(torch.from_numpy(A).to(dev), args).to(dev).train()
        with torch.no_grad():
            model.seq_hyp.param.copy_(torch.from_numpy(param[:K]))
        rng = np.random.default_rng(5)
        x = (2.0 * rng.standard_normal((B, n)) * (rng.random((B, n)) <= 0.25)).astype(np.float32)
        b = np.einsum("pmn,bn->bpm", A[0].astype(np.float64), x).astype(np.float32)
        inits = tuple(torch.from_numpy(v).to(dev) for v in
                      (1e-2 * rng.standard_normal((3, B, P, n))).astype(np.float32))
        bt, label = torch.from_numpy(b).to(dev)[..., None], torch.from_numpy(x).to(dev)[..., None]
        graphs = [O.er_graph(P, 0.5, seed=7)] * B
        grads = {}

        def run(f):
            model.seq_hyp.param.grad = None
            Y, _ = model(bt, graphs, inits=inits)
            _, loss_final = gnn_dlasso_utils.compute_loss(Y, label)
            loss_final.backward()
            grads[f] = model.seq_hyp.param.grad

        forms = ["train_step"]
        out["package"] = os.path.abspath(a.pkg)
        rounds = rounds_of(forms, run, a.rounds, a.launches, a.warmup_s)
        out["grad_checksum"] = grads["train_step"].double().sum().item()
    else:
        A, b, _ = O.make_problem(P, m, n, B, seed=1234)
        op = PreparedOperator(torch.from_numpy(A).to(dev))
        g = ingest([O.er_graph(P, 0.5, seed=7)] * B, P, B, dev)
        bt = torch.from_numpy(b).to(dev)
        torch.manual_seed(0)
        y0, U0, d0 = (torch.randn(B, P, n, device=dev) * 1e-2 for _ in range(3))
        hyp = torch.full((K, P, 4), 0.05, device=dev)
        if a.mode == "infer":
            from dadmm_hip import tiled_form
            forms = ["stream", "launches"]

            def run(f):
                os.environ["DADMM_TILED_STREAM"] = "1" if f == "stream" else "0"
                return forward_raw(op, bt, g, hyp, y0, U0, d0, want_U=True, path="tiled")
            os.environ["DADMM_TILED_STREAM"] = "1"
            out["tiled_form"] = tiled_form((P, m, n))
        else:
            forms = ["tiled_record", "stepwise_record"]

            def run(f):
                return forward_raw(op, bt, g, hyp, y0, U0, d0, want_U=True, record=True,
                                   path="tiled" if f == "tiled_record" else "stepwise")
        res = {}
        for f in forms:   # values first: both forms must compute the same bits
            r = run(f)
            torch.cuda.synchronize()
            res[f] = (r[0], r[1]) + ((r[3].Grec, r[3].Urec) if a.mode == "record" else ())
            out.setdefault("status", {})[f] = int(r[2].item())
        out["bitwise_equal"] = all(torch.equal(x, y) for x, y in zip(res[forms[0]], res[forms[1]]))
        del res
        rounds = rounds_of(forms, run, a.rounds, a.launches, a.warmup_s)
    out["order"] = forms
    out["rounds_ms"] = rounds
    out.update(verdict(forms, rounds))
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
