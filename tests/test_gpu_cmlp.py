"""GPU: pcg_cmlp_steps / pcg_cmlp_train and the cmlp graph learner against the fp64 restatement of the
reference's math (tests/cmlp_ref.py) and the reference's own recorded runs (tests/golden/cmlp.*),
and cmlp_pagerank end to end.

Tolerance of the parameters: 8 D, where D is the largest absolute parameter difference between
fp32 and fp64 runs of the REFERENCE math on the same input (for the golden cases: the reference's
own fp32 runs with 1 and 4 torch threads against its ``.double()`` run, recorded in cmlp.json; for
the other shapes: the restatement's fp32 runs with 1 and 4 threads against its fp64 run). The
engine is one more fp32 rounding of the same trajectory with its own summation order, and a single
trajectory's deviation varies severalfold with that order, hence the factor. Nothing in a tolerance
comes from the engine's output. Each test prints the engine's measured deviation next to its D.
"""
import functools
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch

import cmlp_ref as cr
from rcaeval_amd.graph_construction import cmlp as cm

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P5 = dict(p=5, lag=5, hidden=100)


@functools.lru_cache(maxsize=None)
def _golden():
    with open(os.path.join(GOLDEN, "cmlp.json")) as f:
        meta = json.load(f)
    g = dict(np.load(os.path.join(GOLDEN, "cmlp.npz")))
    for a in g.values():
        a.setflags(write=False)
    return meta, g


@functools.lru_cache(maxsize=None)
def _var5():
    X = cr.var5()
    X.setflags(write=False)
    return X


def _engine():
    from rcaeval_amd.engine import get_engine
    return get_engine(0)


def _kw(m):
    return {k: m[k] for k in ("lam", "lr", "lam_ridge", "max_iter", "check_every", "lookback")}


def _spread(X, init, k, **kw):
    """(fp64 restatement after k steps, D): D over two fp32 restatement runs, 1 and 4 threads."""
    ref64, _ = cr.steps(X, init, k, dtype=torch.float64, **kw)
    D = 0.0
    threads = torch.get_num_threads()
    try:
        for th in (1, 4):
            torch.set_num_threads(th)
            D = max(D, float(np.abs(cr.steps(X, init, k, dtype=torch.float32, **kw)[0] - ref64).max()))
    finally:
        torch.set_num_threads(threads)
    return ref64, D


# ---- 1. steps on the golden case --------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 25])
def test_steps_match_the_fp64_restatement(k):
    meta, g = _golden()
    s = meta["steps"]
    D = s["D"][str(k)]
    kw = dict(lr=s["lr"], lam=s["lam"], lam_ridge=s["lam_ridge"])
    ref, ref_mse = cr.steps(_var5(), g["init"], k, dtype=torch.float64, **kw)
    assert np.abs(ref - g[f"steps{k}_f64"]).max() <= 1e-12          # the restatement is the reference's fp64 run
    got, mse = _engine().cmlp_steps(_var5(), g["init"], k, **kw)
    got = got.cpu().numpy().astype(np.float64)
    err = np.abs(got - ref).max()
    print(f"steps k={k}: engine vs fp64 {err:.3e}, D_k = {D:.3e}, 8 D_k = {8 * D:.3e}")
    assert np.isfinite(got).all() and err <= 8 * D
    # the MSEs are those of the returned parameters: an fp32 forward pass of K + hidden + 2 terms per
    # sample against the fp64 one, 16 times the first-order bound (terms) * 2^-24 relative
    at = cr.losses_at(_var5(), got)
    assert np.abs(mse - at).max() <= 16 * (25 + 100 + 2) * 2.0 ** -24 * at.max()


# ---- 2. shapes where tiling can go wrong ------------------------------------------------------
SHAPES = [  # p, T, hidden, lag, ldx
    (1, 6, 100, 5, None),      # one sample, one group
    (2, 7, 100, 5, None),
    (13, 71, 100, 5, None),    # N = 66: a row-tile remainder
    (27, 40, 100, 5, None),    # K = 135 crosses a 128-column tile, two backward column blocks
    (13, 71, 128, 5, None),
    (13, 71, 7, 5, None),
    (13, 71, 100, 1, None),
    (13, 71, 100, 8, None),
    (27, 40, 7, 8, None),
    (13, 71, 100, 5, 16),      # row-strided X
]


@pytest.mark.parametrize("p,T,hidden,lag,ldx", SHAPES)
def test_odd_shapes_match_the_fp64_restatement(p, T, hidden, lag, ldx):
    X = cr.var(p, T, seed=p * 1000 + T)
    init = cr.random_params(p, lag, hidden, seed=hidden * 10 + lag)
    kw = dict(lag=lag, hidden=hidden, lr=0.05, lam=0.4, lam_ridge=0.01)
    ref, D = _spread(X, init, 3, **kw)
    assert D > 0
    eng = _engine()
    if ldx is None:
        Xin = X
    else:
        buf = torch.full((T, ldx), float("nan"), dtype=torch.float32, device=eng.device)
        buf[:, :p] = torch.from_numpy(X.astype(np.float32)).to(eng.device)
        Xin = buf[:, :p]
        assert Xin.stride(0) == ldx
    got, mse = eng.cmlp_steps(Xin, init, 3, **kw)
    got = got.cpu().numpy().astype(np.float64)
    err = np.abs(got - ref).max()
    print(f"p={p} T={T} hidden={hidden} lag={lag} ldx={ldx}: engine vs fp64 {err:.3e}, D = {D:.3e}, 8 D = {8 * D:.3e}")
    assert np.isfinite(got).all() and np.isfinite(mse).all() and err <= 8 * D


# ---- 3. prox edges -----------------------------------------------------------------------------
def test_prox_edges_zero_pattern_and_values():
    _meta, g = _golden()
    lam, lr = 4.0, 0.05                                      # threshold lr * lam = 0.2
    init = g["init"].copy()
    nets = cm.unpack(init, **P5)
    nets[0][0][:, 1, :] *= 1e-3                              # far below the threshold after the step
    nets[1][0][:, 3, :] *= 1e-3
    nets[2][0][:, 0, :] = 0.0                                # already zero
    nets[4][0][:, 4, :] = 0.0
    nets[3][0][:, 2, 0] = 0.0                                # zero only in its most lagged slice
    kw = dict(lr=lr, lam=lam, lam_ridge=0.01)
    ref, D = _spread(_var5(), init, 1, **kw)
    ref32, _ = cr.steps(_var5(), init, 1, dtype=torch.float32, **kw)
    W = [n[0] for n in cm.unpack(ref, **P5)]
    # preconditions, from the restatement alone: the crafted groups end at exactly zero, others
    # survive, and fp32 and fp64 agree on the pattern
    assert not W[0][:, 1, :].any() and not W[1][:, 3, :].any() and not W[2][:, 0, :].any() and not W[4][:, 4, :].any()
    assert W[0][:, 0, :].all() and np.array_equal(ref == 0, ref32 == 0)
    got, _ = _engine().cmlp_steps(_var5(), init, 1, **kw)
    got = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(got == 0, ref == 0)
    err = np.abs(got - ref).max()
    print(f"prox edges: engine vs fp64 {err:.3e}, D = {D:.3e}")
    assert err <= 8 * D
    # a zero group takes its gradient step in the next iteration like any other
    ref2, D2 = _spread(_var5(), init, 2, **kw)
    got2, _ = _engine().cmlp_steps(_var5(), init, 2, **kw)
    got2 = got2.cpu().numpy().astype(np.float64)
    np.testing.assert_array_equal(got2 == 0, ref2 == 0)
    assert np.abs(got2 - ref2).max() <= 8 * D2


# ---- 4. sparse graph ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sparse_run():
    meta, g = _golden()
    return cm.cmlp(_var5(), init=g["init"], return_info=True, **_kw(meta["sparse"]))


def test_sparse_graph_equals_the_golden():
    meta, g = _golden()
    m = meta["sparse"]
    assert m["gc_equal"] and m["min_nonzero_norm"] > 100 * m["norm_D"]       # else the case is unfit
    adj, info = _sparse_run()
    err = np.abs(info["params"].astype(np.float64) - g["sparse_f64"]).max()
    print(f"sparse: engine vs reference fp64 {err:.3e}, D = {m['D']:.3e}; losses {info['losses']}")
    np.testing.assert_array_equal(adj, g["sparse_gc_f64"])
    assert adj.dtype.kind == "i" and adj.sum() == m["gc_ones"]
    assert (info["n_checks"], info["best_it"], info["last_it"]) == (m["n_checks"], m["best_it"], m["last_it"])


# ---- 5. early stop -----------------------------------------------------------------------------
def test_early_stop_restores_the_best_snapshot():
    meta, g = _golden()
    m = meta["early"]
    assert (m["n_checks"], m["best_it"], m["last_it"]) == (9, 59, 89)
    assert m["runner_up_gap"] > 100 * m["loss_D"]                            # else the case is unfit
    ref = cr.train(_var5(), g["init"], dtype=torch.float64, **_kw(m))
    assert (ref["n_checks"], ref["best_it"], ref["last_it"]) == (9, 59, 89)
    out = _engine().cmlp_train(_var5(), g["init"], **_kw(m))
    assert (out["n_checks"], out["best_it"], out["last_it"]) == (9, 59, 89)
    got = out["params"].cpu().numpy().astype(np.float64)
    err, off = np.abs(got - ref["params"]).max(), np.abs(got - ref["last_params"]).max()
    print(f"early stop: engine vs restored fp64 {err:.3e}, vs last iterate {off:.3e}, D = {m['D']:.3e}; "
          f"loss deviation {np.abs(out['losses'] - ref['losses']).max():.3e}, loss_D = {m['loss_D']:.3e}")
    assert err <= 8 * m["D"]
    assert off > 8 * m["D"] and np.abs(ref["params"] - ref["last_params"]).max() > 16 * m["D"]
    assert np.abs(out["losses"] - ref["losses"]).max() <= 8 * max(m["loss_D"], 2.0 ** -23 * ref["losses"].max())


# ---- 6. failure paths --------------------------------------------------------------------------
def test_failure_paths():
    from rcaeval_amd.e2e import cmlp_pagerank
    from rcaeval_amd.io.time_series import preprocess
    X = _var5() * 1e3
    with pytest.raises(ValueError, match="first check"):
        cm.cmlp(X)
    df = pd.DataFrame(X, columns=["a_cpu", "b_cpu", "c_cpu", "d_cpu", "e_cpu"])
    df.insert(0, "time", np.arange(len(df)))
    names = preprocess(data=df, dataset="online-boutique", dk_select_useful=False).columns.to_list()
    out = cmlp_pagerank(df, 0, dataset="online-boutique")
    assert out == {"adj": [], "node_names": names, "ranks": names}
    eng = _engine()
    init = cr.random_params(5, 5, 100, seed=0)
    with pytest.raises(ValueError, match="no sample"):
        eng.cmlp_steps(_var5()[:5], init, 1)
    with pytest.raises(ValueError, match="no sample"):
        eng.cmlp_train(_var5()[:5], init, max_iter=10, check_every=5)
    with pytest.raises(ValueError, match="no check"):
        eng.cmlp_train(_var5(), init, max_iter=9, check_every=10)
    with pytest.raises(ValueError):
        cm.cmlp(_var5()[:5])
    with pytest.raises(ValueError):
        cm.cmlp(_var5(), max_iter=9, check_every=10)


def test_limits_are_refused_before_any_launch():
    from rcaeval_amd import _lib
    eng = _engine()
    assert eng.cmlp_limits() == {"max_hidden": 128, "max_lag": 8, "max_p": 1024}
    X = _var5()
    for lag, hidden in ((5, 129), (9, 100), (0, 100), (5, 0)):
        init = np.zeros(5 * cm.network_size(5, lag, hidden), dtype=np.float32)
        with pytest.raises(_lib.PcgError):
            eng.cmlp_steps(X, init, 1, lag=lag, hidden=hidden)
        with pytest.raises(_lib.PcgError):
            eng.cmlp_train(X, init, max_iter=10, check_every=5, lag=lag, hidden=hidden)
    with pytest.raises(_lib.PcgError):
        cm.cmlp(X, hidden=129, max_iter=10, check_every=5)
    with pytest.raises(_lib.PcgError):
        cm.cmlp(X, lag=9, max_iter=10, check_every=5)
    with pytest.raises(ValueError, match="packed parameters"):
        eng.cmlp_steps(X, np.zeros(7, dtype=np.float32), 1)


# ---- 7. determinism ----------------------------------------------------------------------------
def test_two_runs_are_bit_identical():
    meta, g = _golden()
    _adj, a = _sparse_run()
    b = _engine().cmlp_train(_var5(), g["init"], **_kw(meta["sparse"]))
    assert a["params"].tobytes() == b["params"].cpu().numpy().tobytes()
    assert a["losses"].tobytes() == b["losses"].tobytes()


# ---- 8. end to end -----------------------------------------------------------------------------
def test_cmlp_pagerank_equals_restatement_pipeline(monkeypatch):
    from rcaeval_amd.e2e import cmlp_pagerank
    from rcaeval_amd.graph_heads.page_rank import PageRank
    from rcaeval_amd.io.time_series import preprocess
    meta, g = _golden()
    kw = _kw(meta["sparse"])
    df = pd.DataFrame(_var5().copy(), columns=["a_cpu", "b_cpu", "c_cpu", "d_cpu", "e_cpu"])
    df.insert(0, "time", np.arange(len(df)))
    data = preprocess(data=df, dataset="online-boutique", dk_select_useful=False)
    names = data.columns.to_list()
    assert len(names) == 5
    runs = [cr.train(data.to_numpy(), g["init"], dtype=dt, **kw) for dt in (torch.float64, torch.float32)]
    adj = cr.gc(runs[0]["params"], **P5)
    np.testing.assert_array_equal(adj, cr.gc(runs[1]["params"], **P5))       # else the case is unfit
    assert 0 < adj.sum() < 25
    real = cm.cmlp
    seen = {}

    def sparse_cmlp(frame, max_iter=None):
        seen["max_iter"] = max_iter                         # the method's own argument
        return real(frame, init=g["init"], **kw)

    monkeypatch.setattr(cm, "cmlp", sparse_cmlp)
    out = cmlp_pagerank(df, 0, dataset="online-boutique")
    assert seen == {"max_iter": 20000}
    np.testing.assert_array_equal(out["adj"], adj)
    scores = PageRank().fit_transform(adj.T)
    want = [n for n, _ in sorted(zip(names, scores), key=lambda t: t[1], reverse=True)]
    assert out["node_names"] == names and out["ranks"] == want
