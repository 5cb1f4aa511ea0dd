"""Time the cMLP ISTA iteration (pcg_cmlp_steps) against the restatement on the CPU and on the device
through PyTorch (GPU tool).

Per (p, T): the input is ``cmlp_ref.var(p, T, seed)``, the start ``cmlp_ref.random_params`` (lag 5,
hidden 100, the learner's lr / lam / lam_ridge). Reported:
  engine_ms_per_iter   one ``pcg_cmlp_steps`` call on device-resident input of enough iterations for a
                       window of about half a second (at least --iters; ``engine_iters_per_call``),
                       device events on the engine's stream around the call, divided by that count
                       (the call's one-off lag expansion and closing loss pass are inside); warm,
                       median and (min, max) over --reps calls
  torch_device_ms_per_iter
                       ``cmlp_ref.step`` (fp32, all networks batched) on the same device through
                       PyTorch, --torch-iters iterations after --torch-warmup, host clock around a
                       synchronised loop; median and (min, max) over --reps loops
  cpu_ms_per_iter      the same restatement in fp32 on the CPU over --cpu-iters iterations
  *_s_20000            seconds for the 20 000 iterations of cmlp_pagerank at that rate
  torch_over_engine, cpu_over_engine
                       the ratios of the medians
  max_abs_diff_vs_torch_device
                       largest parameter difference between the engine and the device restatement
                       after --torch-warmup iterations from the same start (sanity, fp32 both)
``deviation``: the engine against the fp64 restatement on the golden case after k = 1, 25 steps,
next to the golden's D_k (tests/test_gpu_cmlp.py asserts 8 D_k).

  python tools/cmlp_bench.py [--out profiles/cmlp_bench.json] [--shapes 20x600,50x1200,200x1200]
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


def _stats(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="20x600,50x1200,200x1200")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-iters", type=int, default=200)
    ap.add_argument("--torch-warmup", type=int, default=20)
    ap.add_argument("--cpu-iters", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    import cmlp_ref as cr
    from rcaeval_amd.engine import get_engine
    eng = get_engine(0)
    lag, hidden = 5, 100
    hp = dict(lr=5e-2, lam=0.002, lam_ridge=1e-2)
    res = {"device": torch.cuda.get_device_name(0), "lag": lag, "hidden": hidden, "iters": args.iters, "reps": args.reps,
           "warmup": args.warmup, "torch_iters": args.torch_iters, "torch_warmup": args.torch_warmup,
           "cpu_iters": args.cpu_iters, "cpu_threads": torch.get_num_threads(), **hp, "rows": []}
    for p, T in [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]:
        X = cr.var(p, T, seed=p + T)
        init = cr.random_params(p, lag, hidden, seed=p)
        Xd = torch.from_numpy(X.astype(np.float32)).to(eng.device)
        Pd = torch.from_numpy(init).to(eng.device)
        # enough iterations per timed call for a window of about half a second (at least --iters)
        t0 = time.perf_counter()
        eng.cmlp_steps(Xd, Pd, 50, lag=lag, hidden=hidden, **hp)
        eng.cmlp_steps(Xd, Pd, 50, lag=lag, hidden=hidden, **hp)
        pilot = (time.perf_counter() - t0) / 100
        iters = int(min(20000, max(args.iters, 0.5 / pilot)))
        dev = []
        for r in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(eng.stream)
            eng.cmlp_steps(Xd, Pd, iters, lag=lag, hidden=hidden, **hp)
            e1.record(eng.stream)
            e1.synchronize()
            if r >= args.warmup:
                dev.append(e0.elapsed_time(e1) / iters)
        # the restatement through PyTorch on the device
        A, Y = cr.design(X, lag, torch.float32)
        A, Y = A.to(eng.device), Y.to(eng.device)
        P = {k: v.to(eng.device) for k, v in cr.from_packed(init, p, lag, hidden, torch.float32).items()}
        for _ in range(args.torch_warmup):
            cr.step(P, A, Y, **hp)
        torch.cuda.synchronize()
        got, _ = eng.cmlp_steps(Xd, Pd, args.torch_warmup, lag=lag, hidden=hidden, **hp)
        diff = float((got.double().cpu() - torch.from_numpy(cr.to_packed({k: v.cpu() for k, v in P.items()}))).abs().max())
        tdev = []
        for r in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.torch_iters):
                cr.step(P, A, Y, **hp)
            torch.cuda.synchronize()
            tdev.append(1000.0 * (time.perf_counter() - t0) / args.torch_iters)
        # ... and on the CPU
        A, Y = cr.design(X, lag, torch.float32)
        P = cr.from_packed(init, p, lag, hidden, torch.float32)
        cr.step(P, A, Y, **hp)
        t0 = time.perf_counter()
        for _ in range(args.cpu_iters):
            cr.step(P, A, Y, **hp)
        cpu = 1000.0 * (time.perf_counter() - t0) / args.cpu_iters
        med, tmed = statistics.median(dev), statistics.median(tdev)
        row = {"p": p, "T": T, "engine_iters_per_call": iters, "engine_ms_per_iter": _stats(dev), "torch_device_ms_per_iter": _stats(tdev),
               "cpu_ms_per_iter": round(cpu, 3), "engine_s_20000": round(med * 20.0, 2),
               "torch_device_s_20000": round(tmed * 20.0, 2), "cpu_s_20000": round(cpu * 20.0, 1),
               "torch_over_engine": round(tmed / med, 2), "cpu_over_engine": round(cpu / med, 1),
               "max_abs_diff_vs_torch_device": diff}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    with open(os.path.join(ROOT, "tests", "golden", "cmlp.json")) as f:
        meta = json.load(f)
    g = np.load(os.path.join(ROOT, "tests", "golden", "cmlp.npz"))
    s = meta["steps"]
    res["deviation"] = []
    for k in (1, 25):
        kw = dict(lr=s["lr"], lam=s["lam"], lam_ridge=s["lam_ridge"])
        ref, _ = cr.steps(cr.var5(), g["init"], k, dtype=torch.float64, **kw)
        got, _ = eng.cmlp_steps(cr.var5(), g["init"], k, **kw)
        row = {"k": k, "engine_vs_fp64": float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max()),
               "D_k": s["D"][str(k)]}
        res["deviation"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
