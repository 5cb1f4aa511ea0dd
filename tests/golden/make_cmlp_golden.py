"""Regenerate tests/golden/cmlp.npz and cmlp.json: the reference's own answers for
tests/test_cmlp_cpu.py and tests/test_gpu_cmlp.py. Run from the repository root with the path of an
RCAEval checkout as the only argument (or in RCAEVAL_ROOT); its
``RCAEval/graph_construction/cmlp.py`` is loaded as a module and its ``cMLP`` / ``train_model_ista``
are run on ``cmlp_ref.var5()`` from ``torch.manual_seed(0)``.

Every run is made three times: fp32 with 1 torch thread, fp32 with 4 torch threads, and
``.double()``. D of a run is the largest absolute parameter difference between either fp32 run and
the fp64 run, so the spread over summation orders is sampled twice.

  steps   lam 0.4, lr 0.05, lam_ridge 0.01: the parameters after k = 1, 25, 400 iterations
          (``max_iter = check_every = k``: one check, at the end, keeps that iterate)
  sparse  max_iter 400, lam 0.4, check_every 50: restored parameters, GC, check losses
  early   lr 0.2, lam 0.4, check_every 10, lookback 3, max_iter 600: the same, and the stop
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import cmlp_ref as cr  # noqa: E402
from rcaeval_amd.graph_construction import cmlp as cm  # noqa: E402

P, LAG, HIDDEN = 5, 5, 100
STEPS = dict(lam=0.4, lr=0.05, lam_ridge=0.01)
SPARSE = dict(lam=0.4, lr=0.05, lam_ridge=0.01, max_iter=400, check_every=50, lookback=5)
EARLY = dict(lam=0.4, lr=0.2, lam_ridge=0.01, max_iter=600, check_every=10, lookback=3)


def load_reference(root):
    spec = importlib.util.spec_from_file_location("rcaeval_cmlp", os.path.join(root, "RCAEval", "graph_construction",
                                                                                "cmlp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(ref, X, state, double, threads, lam, lr, lam_ridge, max_iter, check_every, lookback=5):
    torch.set_num_threads(threads)
    model = ref.cMLP(P, lag=LAG, hidden=[HIDDEN])
    model.load_state_dict(state)
    Xt = torch.tensor(X[np.newaxis], dtype=torch.float32)
    if double:
        model, Xt = model.double(), Xt.double()
    losses = ref.train_model_ista(model, Xt, lam=lam, lam_ridge=lam_ridge, lr=lr, penalty="H", max_iter=max_iter,
                                  check_every=check_every, lookback=lookback, verbose=0)
    params = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for i in range(P) for a in (
        model.state_dict()[f"networks.{i}.layers.0.weight"].double().numpy(),
        model.state_dict()[f"networks.{i}.layers.0.bias"].double().numpy(),
        model.state_dict()[f"networks.{i}.layers.1.weight"].double().numpy(),
        model.state_dict()[f"networks.{i}.layers.1.bias"].double().numpy())])
    return params, np.array([float(v) for v in losses]), model.GC().numpy().astype(int)


def three(ref, X, state, **kw):
    """(fp32 1 thread, fp32 4 threads, fp64) results and D."""
    a, b, d = (run(ref, X, state, dbl, th, **kw) for dbl, th in ((False, 1), (False, 4), (True, 1)))
    D = float(max(np.abs(a[0] - d[0]).max(), np.abs(b[0] - d[0]).max()))
    return a, b, d, D


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ["RCAEVAL_ROOT"]
    ref = load_reference(root)
    X = cr.var5()
    torch.manual_seed(0)
    state = {k: v.clone() for k, v in ref.cMLP(P, lag=LAG, hidden=[HIDDEN]).state_dict().items()}
    arrays = {"init": cm.pack_state_dict(state, P)}
    meta = {"p": P, "lag": LAG, "hidden": HIDDEN, "T": int(X.shape[0]), "steps": dict(STEPS, D={}), "versions":
            {"numpy": np.__version__, "torch": torch.__version__}}
    for k in (1, 25, 400):
        a, b, d, D = three(ref, X, state, max_iter=k, check_every=k, **STEPS)
        arrays[f"steps{k}_f32"], arrays[f"steps{k}_f64"] = a[0].astype(np.float32), d[0]
        meta["steps"]["D"][str(k)] = D
    for name, kw in (("sparse", SPARSE), ("early", EARLY)):
        a, b, d, D = three(ref, X, state, **kw)
        arrays[f"{name}_f32"], arrays[f"{name}_f64"] = a[0].astype(np.float32), d[0]
        arrays[f"{name}_losses_f32"], arrays[f"{name}_losses_f64"] = a[1], d[1]
        arrays[f"{name}_gc_f32"], arrays[f"{name}_gc_f64"] = a[2], d[2]
        n32, n64 = (cr.group_norms(v[0], P, LAG, HIDDEN) for v in (a, d))
        n_checks = len(d[1])
        best = int(np.argmin(d[1]))                      # argmin takes the first minimum, as `<` does
        m = dict(kw, D=D, n_checks=n_checks, n_checks_f32=len(a[1]), best_check=best,
                 best_it=(best + 1) * kw["check_every"] - 1,
                 last_it=(n_checks * kw["check_every"] - 1),
                 loss_D=float(max(np.abs(a[1] - d[1]).max(), np.abs(b[1] - d[1]).max())),
                 runner_up_gap=float(np.sort(d[1])[1] - np.sort(d[1])[0]),
                 min_nonzero_norm=float(n64[n64 > 0].min()), norm_D=float(np.abs(n32 - n64).max()),
                 gc_ones=int(d[2].sum()), gc_equal=bool((a[2] == d[2]).all() and (b[2] == d[2]).all()))
        meta[name] = m
    np.savez_compressed(os.path.join(HERE, "cmlp.npz"), **arrays)
    with open(os.path.join(HERE, "cmlp.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(meta, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
