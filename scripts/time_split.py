"""Timing probe: the column-split forward (dadmm_forward_split) against the fused forward at a
small batch, HIP events over back-to-back forward_raw calls (draws + launch + gated stepwise).

    python scripts/time_split.py [B] [reps]      (P=5, n=256, m=64, K=25, shared ER graph)

    python scripts/time_split.py --record [rounds] [reps] [B ...]
        the RECORDING forwards (training): forward_raw(record=True) (dadmm_forward_record, the
        yardstick) against forward_raw(record=True, train_split=True) (dadmm_forward_split_record),
        `rounds` alternated repetitions of `reps` forwards each way per batch size (default 5 x 50
        at B = 32, 64, 256, 1024), median and minimum per leg; then one module train step
        (DLASSO_unfolded forward, compute_loss, backward) each way at B = 64.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "hyperparameter-gnn_unfolded-d-admm-main_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import oracle as O  # noqa: E402
from dadmm_hip import PreparedOperator, forward_raw, ingest  # noqa: E402

P, M, N, K = 5, 64, 256, 25
MAXP = [0.1, 0.99, 0.99, 0.99]
TRAINED = os.path.join(ROOT, "tests", "golden", "fixture_25_iter_general_learning_seq_hyp_param.npy")


def _timed(f, reps, warm=10):
    """ms per call of f over `reps` back-to-back calls (HIP events), after `warm` calls."""
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def _report(name, B, ms_list, status):
    us = np.asarray(ms_list) * 1e3
    print(f"{name:22s} B={B:5d}: median {np.median(us):8.1f} us  min {us.min():8.1f} us  "
          f"max {us.max():8.1f} us  ({B * K / (np.median(us) * 1e-6) / 1e6:7.1f} M ADMM-iters/s at the "
          f"median)  reps {[round(float(v), 1) for v in us]}  status {status}", flush=True)


def record_mode(argv):
    from dadmm_hip.ops import split_cols
    rounds = int(argv[0]) if len(argv) > 0 else 5
    reps = int(argv[1]) if len(argv) > 1 else 50
    sizes = [int(v) for v in argv[2:]] or [32, 64, 256, 1024]
    dev = torch.device("cuda", 0)
    G = O.er_graph(P, 0.5, seed=7)
    hyp = torch.from_numpy(O.hyp_table(np.load(TRAINED), MAXP)).to(dev)
    print(f"recording forwards, P={P} n={N} m={M} K={K}: {rounds} alternated rounds of {reps} "
          f"forward_raw(record=True) calls per leg (draws + launch + gated stepwise)", flush=True)
    for B in sizes:
        A, b, _ = O.make_problem(P, M, N, B, seed=1)
        op = PreparedOperator(torch.from_numpy(A).to(dev))
        g = ingest([G] * B, P, B, dev)
        bt = torch.from_numpy(b).to(dev)
        sc = split_cols(op, B, K, g, hyp_rows=P, record=True, train_split=True)
        legs = {"record (fused order)": False, "record train_split": True}
        ms = {k: [] for k in legs}
        st = {}
        for _ in range(rounds):
            for name, ts in legs.items():
                t, out = _timed(lambda: forward_raw(op, bt, g, hyp, record=True, train_split=ts), reps)
                ms[name].append(t)
                st[name] = int(out[2].item())
        print(f"B={B}: split_cols(record, train_split) = {sc}", flush=True)
        for name in legs:
            _report(name, B, ms[name], st[name])

    # one module train step each way (the reference driver's loop, unfolded_train_new.py:74-80)
    import argparse

    import gnn_dlasso_utils
    import unfolded_DLASSO
    B = 64
    A, b, x = O.make_problem(P, M, N, B, seed=1)
    args = argparse.Namespace(GHN_iter_num=K, DADMM_mode="diff", alpha_max=0.1, tau_max=0.99,
                              rho_max=0.99, eta_max=0.99, max_penalty_threshold=0.8,
                              penalty_reduction_factor=0.95)
    model = unfolded_DLASSO.DLASSO_unfolded(torch.from_numpy(A).to(dev)[None], args).to(dev).train()
    with torch.no_grad():
        model.seq_hyp.param.copy_(torch.from_numpy(np.load(TRAINED)))
    graphs = ingest([G] * B, P, B, dev)
    bt, label = torch.from_numpy(b).to(dev)[..., None], torch.from_numpy(x).to(dev)[..., None]

    def step():
        model.zero_grad(set_to_none=True)
        Y, _ = model(bt, graphs)
        _, loss_final = gnn_dlasso_utils.compute_loss(Y, label)
        loss_final.backward()
        return None, None, model.last_status

    def fwd_only():
        Y, _ = model(bt, graphs)
        return None, None, model.last_status

    for what, f in (("train step", step), ("its forward alone", fwd_only)):
        ms = {False: [], True: []}
        for _ in range(rounds):
            for ts in (False, True):
                model.train_split = ts
                t, out = _timed(f, max(reps // 2, 1), warm=5)
                ms[ts].append(t)
        for ts in (False, True):
            _report(f"{what} split={int(ts)}", B, ms[ts], int(out[2].item()))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--record":
        return record_mode(sys.argv[2:])
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    dev = torch.device("cuda", 0)
    A, b, _ = O.make_problem(P, M, N, B, seed=1)
    G = O.er_graph(P, 0.5, seed=7)
    hyp = torch.from_numpy(O.hyp_table(np.load(TRAINED), MAXP)).to(dev)
    op = PreparedOperator(torch.from_numpy(A).to(dev))
    g = ingest([G] * B, P, B, dev)
    bt = torch.from_numpy(b).to(dev)
    for path in ("split", "fused", "split", "fused"):
        f = lambda: forward_raw(op, bt, g, hyp, path=path if path == "fused" else "auto")  # noqa
        ms, out = _timed(f, reps)
        print(f"{path:6s} B={B}: {ms * 1e3:8.1f} us per forward, {B * K / (ms * 1e-3) / 1e6:7.1f} "
              f"M ADMM-iters/s, status {int(out[2].item())}", flush=True)


if __name__ == "__main__":
    main()
