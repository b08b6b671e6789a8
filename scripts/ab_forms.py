#!/usr/bin/env python3
"""Kernel-time A/B of the fused forward's forms in one process (DESIGN.md §4.1d's protocol).

    python scripts/ab_forms.py --forms roles-stream,roles [--rounds 5] [--launches 36] [--out FILE]

DADMM_FUSED_FORM is flipped between rounds (the library reads it at every call); HIP events sit
around dadmm_forward itself; each round is the median of --launches launches. The forms are timed
in the order given, round by round; run it again with the order swapped: one slow round follows the
position (the second form of round 0), not the form. Round 0 of every form is reported but left out
of the medians and ranges. The verdict is the three-ranges rule on the first two forms: the
difference of medians against three times the larger round-to-round range."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hyperparameter-gnn_unfolded-d-admm-main_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from dadmm_hip import PreparedOperator, _lib, forward_raw, ingest  # noqa: E402
import oracle as O  # noqa: E402  (input generator only)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forms", default="roles-stream,roles")
    ap.add_argument("--shape", default="4096,5,64,256,25", help="B,P,m,n,K")
    ap.add_argument("--rounds", type=int, default=5, help="rounds per form, the first one discarded")
    ap.add_argument("--launches", type=int, default=36)
    ap.add_argument("--warmup-s", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    forms = a.forms.split(",")
    B, P, m, n, K = (int(x) for x in a.shape.split(","))
    dev = torch.device("cuda:0")
    A, b, _ = O.make_problem(P, m, n, B, seed=1234)
    op = PreparedOperator(torch.from_numpy(A).to(dev))
    g = ingest([O.er_graph(P, 0.5, seed=7)] * B, P, B, dev)
    bt = torch.from_numpy(b).to(dev)
    torch.manual_seed(0)
    y0, U0, d0 = (torch.randn(B, P, n, device=dev) * 1e-2 for _ in range(3))
    hyp = torch.full((K, P, 4), 0.05, device=dev)

    L = _lib.load()
    orig = L.dadmm_forward
    pairs = []

    def timed(*args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = orig(*args)
        e1.record()
        pairs.append((e0, e1))
        return rc

    def run(form):
        os.environ["DADMM_FUSED_FORM"] = form
        return forward_raw(op, bt, g, hyp, y0, U0, d0, want_U=True, path="fused")

    sums = {}
    for f in forms:   # values first: every form must compute the same bits
        Y, U, st = run(f)
        torch.cuda.synchronize()
        sums[f] = (Y.double().sum().item(), U.double().sum().item(), int(st.item()), Y)
    equal = all(torch.equal(sums[f][3], sums[forms[0]][3]) for f in forms)
    sums = {f: v[:3] for f, v in sums.items()}

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.warmup_s:
        for f in forms:
            run(f)
        torch.cuda.synchronize()

    L.dadmm_forward = timed
    rounds = {f: [] for f in forms}
    try:
        for _ in range(a.rounds):
            for f in forms:
                pairs.clear()
                for _ in range(a.launches):
                    run(f)
                torch.cuda.synchronize()
                rounds[f].append(statistics.median(e0.elapsed_time(e1) for e0, e1 in pairs))
    finally:
        L.dadmm_forward = orig
    kept = {f: r[1:] for f, r in rounds.items()}
    med = {f: statistics.median(r) for f, r in kept.items()}
    rng = {f: max(r) - min(r) for f, r in kept.items()}
    out = {"shape": {"B": B, "P": P, "m": m, "n": n, "K": K}, "order": forms, "launches": a.launches,
           "rounds_ms": rounds, "median_ms": med, "range_ms": rng, "checksum": sums,
           "Y_bitwise_equal": equal}
    if len(forms) >= 2:
        diff = med[forms[0]] - med[forms[1]]
        bar = 3 * max(rng[forms[0]], rng[forms[1]])
        out["verdict"] = {"diff_ms": diff, "three_ranges_ms": bar, "passes": abs(diff) > bar,
                          "faster": forms[1] if diff > 0 else forms[0]}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
