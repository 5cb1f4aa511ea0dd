"""Time B RQ2-shaped cases (n = 44, N = 600, distinct seeds) per case against in one batch (GPU tool).

Arms, on the same engine in the same process, alternated:
  loop        eng.corr_skeleton(X) per case (the per-case path, unchanged by the batch feature:
              the baseline)
  batch       eng.skeleton_batch(Xs, from_data=True)
  pc_loop     pc(X) per case
  pc_batch    pc_batch(Xs)
Every arm is warmed up per B, then timed over at least 5 alternations and at least 0.5 s per arm,
with host clocks around calls that end in a device synchronise. Reported per B: the median and the
spread (min, max) of the per-case milliseconds over the alternations.

  python tools/batch_bench.py [--out FILE] [--n 44] [--N 600] [--B 1,16,128,512]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=44)
    ap.add_argument("--N", type=int, default=600)
    ap.add_argument("--B", default="1,16,128,512")
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    args = ap.parse_args()
    import torch
    from rcaeval_amd import synth
    from rcaeval_amd.causal import pc, pc_batch
    from rcaeval_amd.engine import get_engine
    eng = get_engine(0)
    sizes = [int(b) for b in args.B.split(",")]
    allX = [synth.gaussian_sem(args.n, args.N, seed=100 + k, w_low=0.2, w_high=0.8, edge_prob=0.1)
            for k in range(max(sizes))]
    res = {"n": args.n, "N": args.N, "device": torch.cuda.get_device_name(0), "alternations": args.alternations,
           "min_seconds_per_arm": args.min_seconds, "unit": "ms per case", "by_B": {}}
    for B in sizes:
        Xs = allX[:B]
        arms = {
            "loop": lambda: [eng.corr_skeleton(X) for X in Xs],
            "batch": lambda: eng.skeleton_batch(Xs, from_data=True),
            "pc_loop": lambda: [pc(X) for X in Xs],
            "pc_batch": lambda: pc_batch(Xs),
        }
        inner = {}
        for name, fn in arms.items():          # warm-up of this shape, and the repeats that fill the time
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = max(time.perf_counter() - t0, 1e-6)
            inner[name] = max(1, int(args.min_seconds / args.alternations / dt) + 1)
        samples = {name: [] for name in arms}
        timed = {name: 0.0 for name in arms}
        # whole alternations until every arm has its samples and its timed seconds (the calibration
        # call above is slower than the steady state, so the first estimate can fall short)
        while min(len(v) for v in samples.values()) < args.alternations or min(timed.values()) < args.min_seconds:
            for name, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(inner[name]):
                    fn()
                dt = time.perf_counter() - t0
                timed[name] += dt
                samples[name].append(1000.0 * dt / inner[name] / B)
        outs = eng.skeleton_batch(Xs, from_data=True)
        row = {"drivers": sorted({o.stats["driver"] for o in outs}), "levels_max": max(o.levels for o in outs)}
        for name, v in samples.items():
            row[name] = {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5),
                         "samples": len(v), "calls_per_sample": inner[name], "timed_s": round(timed[name], 3)}
        row["loop_over_batch"] = round(row["loop"]["median"] / row["batch"]["median"], 3)
        row["pc_loop_over_pc_batch"] = round(row["pc_loop"]["median"] / row["pc_batch"]["median"], 3)
        res["by_B"][str(B)] = row
        print(f"B={B}", json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
