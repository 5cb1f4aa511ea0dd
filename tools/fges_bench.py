#!/usr/bin/env python
"""Times the fGES graph learner on the GPU and writes profiles/fges_bench.json.

Shapes: n in {16, 48, 100, 200} at T = 600 on ``rcaeval_amd.synth.gaussian_sem`` data. Per shape,
by the host clock around the synchronous calls: ``fges_begin`` (upload, standardization, K1, the
depth-0 gains, the result copy), the summed ``fges_gains`` calls with their count, groups and
items, the host driver (the whole call minus those two) and the whole ``fges`` call; next to them
the exact-path and host-fallback item counts and the widest base set. After ``--warmup``
unrecorded calls, ``--reps`` recorded ones; min / median / max are reported. No threshold is
attached to any of these: the split says whether the driver should move to host C++ next.

    python tools/fges_bench.py [--reps 5] [--warmup 2] [--out profiles/fges_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}


class _Counting:
    """The engine's scorer, also counting groups, single-candidate groups and the widest base."""

    def __init__(self, inner):
        self.inner = inner
        self.groups = self.single = self.bmax = 0

    @property
    def stats(self):
        return self.inner.stats

    def begin(self, X):
        return self.inner.begin(X)

    def gains(self, groups):
        self.groups += len(groups)
        self.single += sum(len(c) == 1 for _, _, c in groups)
        self.bmax = max([self.bmax] + [len(B) for _, B, _ in groups])
        return self.inner.gains(groups)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fges_bench.json"))
    args = ap.parse_args(argv)
    import torch
    from rcaeval_amd import synth
    from rcaeval_amd.engine import get_engine
    from rcaeval_amd.graph_construction import fges as fmod
    eng = get_engine(0)
    T = 600
    rows = []
    for n in (16, 48, 100, 200):
        X = synth.gaussian_sem(n, T, seed=0)
        t = {k: [] for k in ("begin_ms", "gains_ms", "driver_ms", "total_ms")}
        sc = trace = adj = None
        for rep in range(args.warmup + args.reps):
            sc, trace = _Counting(fmod.EngineScorer(eng)), {}
            adj = fmod.fges(X, _scorer=sc, _trace=trace)
            st = trace["stats"]
            if rep >= args.warmup:
                t["begin_ms"].append(st["begin_s"] * 1e3)
                t["gains_ms"].append(st["gains_s"] * 1e3)
                t["driver_ms"].append((st["total_s"] - st["begin_s"] - st["gains_s"]) * 1e3)
                t["total_ms"].append(st["total_s"] * 1e3)
        st = trace["stats"]
        row = {"T": T, "n": n, **{k: _stats(v) for k, v in t.items()},
               "gains_calls": st["calls"], "gains_groups": sc.groups, "single_candidate_groups": sc.single,
               "gains_items": st["items"], "base_max": sc.bmax, "exact_items": st["exact_items"],
               "fallback_items": st["fallback_items"], "insertions": len(trace["inserted"]),
               "deletions": len(trace["deleted"]), "edges": int((adj | adj.T).sum() // 2)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
