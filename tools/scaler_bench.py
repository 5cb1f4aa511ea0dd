"""Time baro / nsigma against the reference's per-column sklearn loop (GPU tool).

Shapes: "rq2", the synthetic Online-Boutique-shaped case of ``bench.py --workload rq2``
(``synth.rq2_case_frame(rows=1200)`` windowed to 300 + 300 rows as ``rq2.load_case`` does, 44
metrics), and "large", one case of 2000 columns with 10 000 normal and 10 000 anomalous rows.
Per shape and method (baro = RobustScaler, nsigma = StandardScaler), each the median and (min,
max) of --reps repetitions after --warmup warm-ups:
  host_loop_ms    the reference's loop on the preprocessed halves: one sklearn fit + transform +
                  max per column, the only way to get these ranks without the engine
  device_ms       pcg_scaler_batch of the one case on device-resident input and outputs, device
                  events on the engine's stream around the call
  method_ms       the public method end to end on the host clock (window split, preprocess of both
                  halves, upload, pcg_scaler_batch, download, rank sort)
  batch_ms_per_case
                  ``baro_batch`` / ``nsigma_batch`` of --batch different cases of the shape (one
                  upload, one pcg_scaler_batch), host clock, divided by the batch size ("large":
                  --large-batch cases, 64 of them would not fit the host buffer)
  frame_ms        the part of method_ms that is not the scorer: split + preprocess + sort, timed
                  with a scorer that returns zeros
  ranks_equal     the public method's ranks equal the host loop's

  python tools/scaler_bench.py [--out profiles/scaler_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def _timed(fn, warmup, reps, sync=None):
    out = []
    for r in range(warmup + reps):
        if sync:
            sync()
        t0 = time.perf_counter()
        fn()
        if r >= warmup:
            out.append(1000.0 * (time.perf_counter() - t0))
    return out


def rq2_case(seed):
    """The frame ``rq2.load_case`` hands to a method for one synthetic case."""
    import pandas as pd
    from rcaeval_amd import synth
    df, inject = synth.rq2_case_frame(rows=1200, seed=seed)
    normal = df[df["time"] < inject].tail(300)
    anomal = df[df["time"] >= inject].head(300)
    return pd.concat([normal, anomal], ignore_index=True), inject


def large_case(seed, cols=2000, rows=10000):
    import numpy as np
    import pandas as pd
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(2 * rows, cols)) * rng.uniform(0.5, 50.0, cols) + rng.uniform(-10, 100, cols)
    X[rows:, rng.integers(0, cols, 20)] += 25.0
    df = pd.DataFrame(X, columns=[f"svc{j // 4}_m{j % 4}" for j in range(cols)])
    df.insert(0, "time", np.arange(2 * rows))
    return df, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--large-batch", type=int, default=2)
    ap.add_argument("--shapes", default="rq2,large")
    args = ap.parse_args()
    warnings.filterwarnings("ignore")
    import numpy as np
    import torch
    from sklearn.preprocessing import RobustScaler, StandardScaler
    from rcaeval_amd._lib import PcgScalerCase, check
    from rcaeval_amd.e2e import baro, baro_batch, nsigma, nsigma_batch
    from rcaeval_amd.e2e.baro import split_frames
    from rcaeval_amd.engine import get_engine
    eng = get_engine(0)
    dataset = "online-boutique"
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
           "lds_rows": eng.scaler_limits()["lds_rows"], "rows": []}
    vp = ctypes.c_void_p

    def zeros_scorer(pairs, mode):
        return [{"score": np.zeros(A.shape[1]), "status": np.zeros(A.shape[1], dtype=np.int32)} for A, _B in pairs]

    for shape in args.shapes.split(","):
        make = rq2_case if shape == "rq2" else large_case
        nb = args.batch if shape == "rq2" else args.large_batch
        cases = [make(seed) for seed in range(nb)]
        df, inject = cases[0]
        nd, ad = split_frames(df, inject, dataset=dataset)
        A = np.ascontiguousarray(nd.to_numpy(), dtype=np.float64)
        B = np.ascontiguousarray(ad.to_numpy(), dtype=np.float64)
        N, n = A.shape
        M = B.shape[0]
        Ad, Bd = eng.to_device(A), eng.to_device(B)
        vals = torch.empty((3, n), dtype=torch.float64, device=eng.device)
        st = torch.empty(n, dtype=torch.int32, device=eng.device)
        arr = (PcgScalerCase * 1)(PcgScalerCase(Ad.data_ptr(), Bd.data_ptr(), N, M, n, n, n, 0))
        for mode, name, one, many, cls in ((0, "baro", baro, baro_batch, RobustScaler),
                                           (1, "nsigma", nsigma, nsigma_batch, StandardScaler)):
            def host_loop():
                ranks = []
                for col in nd.columns:
                    a, b = nd[col].to_numpy(), ad[col].to_numpy()
                    scaler = cls().fit(a.reshape(-1, 1))
                    ranks.append((col, max(scaler.transform(b.reshape(-1, 1))[:, 0])))
                return [x[0] for x in sorted(ranks, key=lambda x: x[1], reverse=True)]

            def call():
                check(eng.h, eng.lib.pcg_scaler_batch(eng.h, arr, 1, mode, *(vp(vals.data_ptr() + k * n * 8) for k in range(3)),
                                                      vp(st.data_ptr())), "pcg_scaler_batch")
            dev = []
            for r in range(args.warmup + args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(eng.stream)
                call()
                e1.record(eng.stream)
                e1.synchronize()
                if r >= args.warmup:
                    dev.append(e0.elapsed_time(e1))
            sync = torch.cuda.synchronize

            def note(what):                        # the large shape takes minutes per phase
                print(f"# {shape} {name}: {what} timed", file=sys.stderr, flush=True)
            note("device call")
            host = _timed(host_loop, args.warmup, args.reps)
            note("host loop")
            meth = _timed(lambda: one(df, inject, dataset=dataset), args.warmup, args.reps, sync)
            note("method")
            frame = _timed(lambda: one(df, inject, dataset=dataset, scorer=zeros_scorer), args.warmup, args.reps)
            note("frame logic")
            bat = _timed(lambda: many(cases, dataset=dataset), args.warmup, args.reps, sync)
            note("batch")
            row = {"shape": shape, "method": name, "N": N, "M": M, "n": n, "batch": nb,
                   "path": "standard" if mode else ("lds sort" if N <= res["lds_rows"] else "radix select"),
                   "host_loop_ms": _stats(host), "device_ms": _stats(dev), "method_ms": _stats(meth),
                   "frame_ms": _stats(frame), "batch_ms_per_case": _stats([v / nb for v in bat]),
                   "ranks_equal": one(df, inject, dataset=dataset)["ranks"] == host_loop()}
            row["host_over_method"] = round(row["host_loop_ms"]["median"] / row["method_ms"]["median"], 2)
            row["host_over_batch_per_case"] = round(row["host_loop_ms"]["median"] / row["batch_ms_per_case"]["median"], 2)
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
