"""Time pcg_granger (all ordered pairs x 3 lags of one case) on telemetry-shaped data (GPU tool).

Per (n, T) and kind: the input is ``synth.telemetry_frame(n, T, n_constant=0)`` after ``preprocess``
(the frame granger_pagerank hands to ``granger``) — kind "iid" as it is (rows independent in time),
kind "walk" its cumulative sum over time (gauge-like metrics: strongly autocorrelated columns, which
is what sends items to the exact path). Reported:
  device_ms       pcg_granger on device-resident input and outputs, device events on the engine's
                  stream around the call (column pass, pair kernel, counter read-back, exact
                  kernel), warm, median and (min, max) over --reps calls
  granger_ms      ``granger(frame)`` end to end on the host clock (upload, pcg_granger, download,
                  the scipy tails and the threshold), warm, median over --reps calls
  pairs_per_s     n * (n - 1) ordered pairs over the median device time
  exact_share     items the exact (QR) path computed / all n * (n - 1) * 3 items
  cpu_restatement_s
                  single-process time of tests/granger_ref.py (explicit designs, pinv, matrix_rank)
                  on the same input, measured on --cpu-pairs ordered pairs drawn at random and
                  scaled to n * (n - 1) (the full loop at n = 200, T = 4200 takes minutes)
  adj_equal_on_sample
                  the engine's per-lag decisions equal the restatement's on the sampled pairs

  python tools/granger_bench.py [--out profiles/granger_bench.json] [--n 50,200] [--T 1200,4200]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", default="50,200")
    ap.add_argument("--T", default="1200,4200")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-pairs", type=int, default=40)
    args = ap.parse_args()
    import numpy as np
    import torch
    import granger_ref as gr
    from rcaeval_amd import synth
    from rcaeval_amd._lib import check
    from rcaeval_amd.engine import get_engine
    from rcaeval_amd.graph_construction.granger import granger, granger_from_stats
    from rcaeval_amd.io.time_series import preprocess
    eng = get_engine(0)
    res = {"device": torch.cuda.get_device_name(0), "maxlag": 3, "reps": args.reps, "warmup": args.warmup,
           "cpu_pairs": args.cpu_pairs, "rows": []}
    vp = ctypes.c_void_p
    for n in [int(v) for v in args.n.split(",")]:
        for T, kind in [(int(v), kd) for v in args.T.split(",") for kd in ("iid", "walk")]:
            frame = preprocess(synth.telemetry_frame(n, T, n_constant=0, seed=n + T), dataset="online-boutique")
            if kind == "walk":
                frame = (frame - frame.mean()).cumsum()
            X = frame.to_numpy().astype(float)
            n_eff = X.shape[1]
            Xd = eng.to_device(X)
            shape = (n_eff, n_eff, 3)
            f = [torch.empty(shape, dtype=torch.float64, device=eng.device) for _ in range(3)]
            k = [torch.empty(shape, dtype=torch.int32, device=eng.device) for _ in range(2)]
            exact = ctypes.c_int64()

            def call():
                check(eng.h, eng.lib.pcg_granger(eng.h, vp(Xd.data_ptr()), T, n_eff, n_eff, 3,
                                                 *(vp(t.data_ptr()) for t in f + k), ctypes.byref(exact)), "pcg_granger")
            dev, host = [], []
            for r in range(args.warmup + args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(eng.stream)
                call()
                e1.record(eng.stream)
                e1.synchronize()
                if r >= args.warmup:
                    dev.append(e0.elapsed_time(e1))
            for r in range(args.warmup + args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                adj = granger(frame)
                if r >= args.warmup:
                    host.append(1000.0 * (time.perf_counter() - t0))
            items = n_eff * (n_eff - 1) * 3
            # the CPU restatement on a sample of ordered pairs, and the decisions on that sample
            rng = np.random.default_rng(0)
            out = eng.granger(X, 3)
            _, p = granger_from_stats(out["ssr_r"], out["ssr_u"], out["tss"], out["rank"], out["status"], T, 3)
            pairs = set()
            while len(pairs) < min(args.cpu_pairs, n_eff * (n_eff - 1)):
                i, j = (int(v) for v in rng.integers(0, n_eff, 2))
                if i != j:
                    pairs.add((i, j))
            t0 = time.perf_counter()
            ref_p = {(i, j): [gr.pair_lag(X[:, i], X[:, j], L)["p"] for L in (1, 2, 3)] for i, j in sorted(pairs)}
            cpu_s = (time.perf_counter() - t0) / len(pairs) * n_eff * (n_eff - 1)
            same = all(((np.mean(ref_p[ij][L], axis=-1) < 0.05) == (p[ij[0], ij[1], L].mean() < 0.05))
                       for ij in ref_p for L in range(3))
            med = statistics.median(dev)
            row = {"n": n_eff, "T": T, "kind": kind, "items": items,
                   "device_ms": {"median": round(med, 4), "min": round(min(dev), 4), "max": round(max(dev), 4)},
                   "granger_ms": {"median": round(statistics.median(host), 3), "min": round(min(host), 3),
                                  "max": round(max(host), 3)},
                   "pairs_per_s": round(n_eff * (n_eff - 1) / (med * 1e-3)),
                   "exact_items": int(exact.value), "exact_share": round(exact.value / items, 6),
                   "edges": int(adj.sum()),
                   "cpu_restatement_s": round(cpu_s, 2), "cpu_pairs_timed": len(pairs),
                   "cpu_over_granger": round(cpu_s * 1000.0 / statistics.median(host), 1),
                   "adj_equal_on_sample": bool(same)}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
