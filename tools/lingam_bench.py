"""Time pcg_direct_lingam_order (DirectLiNGAM's causal-order search of one case) on telemetry-shaped
data, and record the observed tolerance ratios of pcg_lingam_pair_scores (GPU tool).

Per (n, T): the input is ``synth.telemetry_frame(n, T, n_constant=0)`` after ``preprocess`` (the frame
micro_diag hands to ``DirectLiNGAM().fit``). Reported:
  device_ms       pcg_direct_lingam_order on device-resident input and output, device events on the
                  engine's stream around the call (3 launches per step, n - 1 steps), warm, median
                  and (min, max) over --reps calls
  model_ms        the cost model of DESIGN.md ("DirectLiNGAM"): sum over the steps of
                  m (m - 1) / 2 pairs x T rows x VALU_PER_ROW fp64-class instructions per lane, at
                  CYCLES_PER_INSTR cycles per wave64 instruction on 1024 SIMDs x 2.4 GHz
  pair_rows_per_s sum over the steps of (pairs x T) over the median device time
  cpu_restatement_s  (n = --cpu-n only) single-process time of tests/lingam_ref.py's ``order`` on the
                  same input, and whether the engine's order equals it
Under "tolerance": per test shape and input kind (the three generators of tests/lingam_ref.py,
collinear(1e-3 / 1e-6 / 1e-9), raw X and the restatement's X_ at steps n // 2 and n - 2), delta =
max |D_float64 - D_longdouble| of the restatement and ratio = max |D_gpu - D_float64| /
max(delta, 2^-50); tests/test_gpu_lingam.py asserts ratio <= 32.

  python tools/lingam_bench.py [--out profiles/lingam_bench.json] [--n 32,64,128,256] [--T 500,2000]
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

VALU_PER_ROW = 500          # pass C's loop body in the gfx950 ISA of k_lingam_pairs (two residuals)
CYCLES_PER_INSTR = 5.83     # v_fma_f64 per wave64 instruction at 4 waves / SIMD (profiles/r03_issue_cost.json)
SHAPES = [(8, 2), (65, 3), (300, 9), (1000, 17), (2500, 5)]
FLOOR = 2.0 ** -50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", default="32,64,128,256")
    ap.add_argument("--T", default="500,2000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-n", type=int, default=32)
    args = ap.parse_args()
    import numpy as np
    import torch
    import lingam_ref as lr
    from rcaeval_amd import synth
    from rcaeval_amd._lib import check
    from rcaeval_amd.engine import get_engine
    from rcaeval_amd.io.time_series import preprocess
    eng = get_engine(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
           "model": {"valu_per_row": VALU_PER_ROW, "cycles_per_instr": CYCLES_PER_INSTR, "simds": 1024, "ghz": 2.4},
           "rows": [], "tolerance": []}
    vp = ctypes.c_void_p
    for n in [int(v) for v in args.n.split(",")]:
        for T in [int(v) for v in args.T.split(",")]:
            frame = preprocess(synth.telemetry_frame(n, T, n_constant=0, seed=n + T), dataset="online-boutique")
            X = frame.to_numpy().astype(float)
            n_eff = X.shape[1]
            Xd = eng.to_device(X)
            order = torch.empty(n_eff, dtype=torch.int32, device=eng.device)

            def call():
                check(eng.h, eng.lib.pcg_direct_lingam_order(eng.h, vp(Xd.data_ptr()), T, n_eff, n_eff,
                                                             vp(order.data_ptr()), None), "pcg_direct_lingam_order")
            dev = []
            for r in range(args.warmup + args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(eng.stream)
                call()
                e1.record(eng.stream)
                e1.synchronize()
                if r >= args.warmup:
                    dev.append(e0.elapsed_time(e1))
            med = statistics.median(dev)
            pair_rows = sum(m * (m - 1) // 2 for m in range(2, n_eff + 1)) * T
            row = {"n": n_eff, "T": T, "steps": n_eff - 1, "launches": 3 * (n_eff - 1) + 1,
                   "device_ms": {"median": round(med, 3), "min": round(min(dev), 3), "max": round(max(dev), 3)},
                   "model_ms": round(pair_rows * VALU_PER_ROW / 64 * CYCLES_PER_INSTR / (1024 * 2.4e9) * 1e3, 3),
                   "pair_rows_per_s": round(pair_rows / (med * 1e-3))}
            if n == args.cpu_n:
                t0 = time.perf_counter()
                K = lr.order(X)[0]
                row["cpu_restatement_s"] = round(time.perf_counter() - t0, 2)
                row["cpu_over_device"] = round(row["cpu_restatement_s"] * 1e3 / med, 1)
                row["order_equal_restatement"] = bool(order.cpu().numpy().tolist() == K)
            res["rows"].append(row)
            print(json.dumps(row), flush=True)

    def ratio(kind, T, n, what, X_):
        D = lr.pair_scores(X_)[0]
        delta = float(np.max(np.abs(D - lr.pair_scores(X_, np.longdouble)[0].astype(np.float64)))) if n > 1 else 0.0
        err = float(np.max(np.abs(eng.lingam_pair_scores(np.array(X_))[0] - D)))
        row = {"input": kind, "T": T, "n": n, "at": what, "delta": delta, "max_abs_err": err,
               "ratio": round(err / max(delta, FLOOR), 3)}
        res["tolerance"].append(row)
        print(json.dumps(row), flush=True)

    for T, n in SHAPES:
        for gen in lr.GENERATORS:
            X = lr.GENERATORS[gen](T, n, 0)
            K, _, snaps = lr.order(X)
            ratio(gen, T, n, "raw", X)
            for s in sorted({n // 2, n - 2}):
                U = sorted(set(range(n)) - set(K[:s]))
                ratio(gen, T, n, f"step {s}", snaps[s][:, U])
        for eps in (1e-3, 1e-6, 1e-9):
            ratio(f"collinear({eps:g})", T, n, "raw", lr.collinear(lr.GENERATORS["laplace"](T, n, 0), eps))
    res["worst_ratio"] = max(r["ratio"] for r in res["tolerance"])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
