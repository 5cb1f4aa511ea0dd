#!/usr/bin/env python
"""Times the PCMCI entry points on the GPU and writes profiles/pcmci_bench.json.

Shapes: n in {16, 48, 200} at T = 600 with tau_max 3 and 10 (pc_alpha 0.1), inputs from the sparse
VAR generator of tests/pcmci_ref.py. PC1 (``Engine.pcmci_parents``: lag expansion, K1, the level
loop) and MCI (``Engine.pcmci_mci``) are timed separately, each between two HIP events on the
handle's stream and by the host clock around the same call (the calls are synchronous, so the
event span includes the host's share of the call: the critical-value table, result copies). After
``--warmup`` unrecorded calls, ``--reps`` recorded ones; min / median / max are reported. Next to
them the CPU restatement's time on the smallest shape. No threshold is attached to any of these.

    python tools/pcmci_bench.py [--reps 5] [--warmup 2] [--out profiles/pcmci_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def _stats(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcmci_bench.json"))
    args = ap.parse_args(argv)
    import torch
    from rcaeval_amd.engine import get_engine
    import pcmci_ref as pr
    eng = get_engine(0)
    T, alpha = 600, 0.1
    rows = []
    for n in (16, 48, 200):
        for tau_max in (3, 10):
            X = pr.gen_var(T, n, tau_max, seed=0)
            Xd = eng.to_device(X)
            ev = {k: ([], []) for k in ("pc1", "mci")}
            par = mci = None
            for rep in range(args.warmup + args.reps):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                t0 = time.perf_counter()
                e[0].record(eng.stream)
                par = eng.pcmci_parents(Xd, tau_max, alpha)
                e[1].record(eng.stream)
                t1 = time.perf_counter()
                mci = eng.pcmci_mci(T, n, tau_max, par)
                e[2].record(eng.stream)
                e[2].synchronize()
                t2 = time.perf_counter()
                if rep >= args.warmup:
                    ev["pc1"][0].append(e[0].elapsed_time(e[1]))
                    ev["pc1"][1].append((t1 - t0) * 1e3)
                    ev["mci"][0].append(e[1].elapsed_time(e[2]))
                    ev["mci"][1].append((t2 - t1) * 1e3)
            row = {"T": T, "n": n, "tau_max": tau_max, "pc_alpha": alpha,
                   "pc1_event_ms": _stats(ev["pc1"][0]), "pc1_wall_ms": _stats(ev["pc1"][1]),
                   "mci_event_ms": _stats(ev["mci"][0]), "mci_wall_ms": _stats(ev["mci"][1]),
                   "pc1_tests": int(par["tests"].sum()), "pc1_levels_max": int(par["levels"].max()),
                   "parents_max": max(len(p) for p in par["parents"]), "mci_items": int((mci["dim"] >= 0).sum()),
                   "dim_z_max": int(mci["dim"].max()),
                   "exact_items": {"pc1": par["exact_items"], "mci": mci["exact_items"]}}
            if (n, tau_max) == (16, 3):
                ref = pr.run_pcmci(X, tau_max, alpha)
                row["cpu_restatement_s"] = round(ref["seconds"], 3)
                row["parents_equal_restatement"] = par["parents"] == ref["parents"]
                row["max_abs_val_diff"] = float(np.max(np.abs(np.where(mci["dim"] >= 0, mci["val"], 0.0) - ref["val_matrix"])))
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
