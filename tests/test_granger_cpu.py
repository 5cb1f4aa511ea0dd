"""CPU: the Granger feature's host side — the pcg_granger binding, the pure-numpy assembly of the
statistics (graph_construction.granger.granger_from_stats) against the restatement in
tests/granger_ref.py, the raising conditions, and the e2e wrappers with ``granger`` replaced by a
fixed matrix."""
import ctypes
import os
import re

import numpy as np
import pandas as pd
import pytest

import granger_ref as gr
from rcaeval_amd.graph_construction import granger as gmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_bindings_agree_on_pcg_granger():
    from rcaeval_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pcgpu.h")).read()
    decl = re.search(r"^int pcg_granger\((.*?)\);", hdr, re.S | re.M).group(1)
    params = [p.strip() for p in decl.replace("\n", " ").split(",")]
    sig = {name: (res, args) for name, res, args in _lib.SIGNATURES}["pcg_granger"]
    assert sig[0] is ctypes.c_int32 and len(sig[1]) == len(params) == 12
    for p, a in zip(params, sig[1]):
        if "*" in p:
            assert a is ctypes.c_void_p or a is ctypes.POINTER(ctypes.c_int64), (p, a)
        else:
            assert a is (ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int), (p, a)
    assert lib.pcg_granger.argtypes == sig[1]
    assert int(re.search(r"#define PCG_ABI_VERSION (\d+)", hdr).group(1)) == _lib.PCG_ABI_VERSION == 4
    # a NULL handle is refused before anything is touched
    assert lib.pcg_granger(None, None, 100, 4, 4, 3, None, None, None, None, None, None) == _lib.PCG_ERR_INVALID


@pytest.fixture(scope="module")
def case():
    """A VAR(1) input with one strong cause, and the restatement's results on it."""
    X = gr.gen_var1(80, 5, seed=2)
    X[1:, 3] += 0.8 * X[:-1, 0]
    ref = gr.all_pairs(X, 3)
    status = np.zeros(ref["rank"].shape, np.int32)
    return X, ref, status


@pytest.mark.parametrize("test", [None, "ssr_ftest", "ssr_chi2test", "lrtest", "params_ftest"])
def test_assembly_reproduces_the_restatement(case, test):
    X, ref, status = case
    adj, p = gmod.granger_from_stats(ref["ssr_r"], ref["ssr_u"], ref["tss"], ref["rank"], status, X.shape[0], 3,
                                     0.05, test)
    off = ~np.eye(5, dtype=bool)
    assert np.isnan(p[~off]).all() and np.isfinite(p[off]).all()
    # same ssr, same formulas: the tails agree to scipy's own rounding; params_ftest is served by
    # ssr_ftest's value, which the Wald statistic equals up to the rounding of a 2L+1 solve
    np.testing.assert_allclose(p[off][..., :3], ref["p"][off][..., :3], rtol=1e-12, atol=0)
    np.testing.assert_allclose(p[off][..., 3], ref["p"][off][..., 3], rtol=1e-8, atol=0)
    want = gr.adjacency(ref["p"], 0.05, test)
    v = gr.values(ref["p"], test)[off]
    assert np.min(np.abs(v - 0.05)) > 1e-6 * 0.05          # no decision rests on the rounding above
    np.testing.assert_array_equal(adj, want)
    assert adj.dtype == np.float64 and adj[3, 0] == 1 and 0 < adj.sum() < 20 and not adj.diagonal().any()


def test_assembly_threshold_and_lag_any(case):
    X, ref, status = case
    args = (ref["ssr_r"], ref["ssr_u"], ref["tss"], ref["rank"], status, X.shape[0], 3)
    assert gmod.granger_from_stats(*args, p_val_threshold=0.0)[0].sum() == 0
    full = gmod.granger_from_stats(*args, p_val_threshold=1.1)[0]
    assert full.sum() == 20
    # one lag below the threshold is enough, whichever lag it is
    _, p = gmod.granger_from_stats(*args)
    v = p.mean(axis=-1)
    i, j = 1, 2
    thr = np.sort(v[i, j])[0] * 1.0001
    assert gmod.granger_from_stats(*args, p_val_threshold=thr)[0][i, j] == 1


@pytest.mark.parametrize("code", [1, 2, 4])
def test_assembly_raises_on_status(case, code):
    X, ref, status = case
    st = status.copy()
    st[2, 4, 1] = code
    with pytest.raises(ValueError):
        gmod.granger_from_stats(ref["ssr_r"], ref["ssr_u"], ref["tss"], ref["rank"], st, X.shape[0], 3)
    st = status.copy()
    st[2, 2, 0] = code                                    # the diagonal carries no test
    gmod.granger_from_stats(ref["ssr_r"], ref["ssr_u"], ref["tss"], ref["rank"], st, X.shape[0], 3)
    st[0, 1, 0] = 3                                       # informational: the exact path was used
    gmod.granger_from_stats(ref["ssr_r"], ref["ssr_u"], ref["tss"], ref["rank"], st, X.shape[0], 3)


def test_assembly_raises_on_perfect_fit_and_short_T(case):
    X, ref, status = case
    for key, val in (("tss", 0.0), ("ssr_u", 0.0), ("ssr_u", ref["tss"][0, 1, 0] * 2.0 ** -53)):
        a = {k: ref[k].copy() for k in ("ssr_r", "ssr_u", "tss")}
        a[key][0, 1, 0] = val
        with pytest.raises(ValueError, match="perfect fit"):
            gmod.granger_from_stats(a["ssr_r"], a["ssr_u"], a["tss"], ref["rank"], status, X.shape[0], 3)
    with pytest.raises(ValueError, match="Insufficient observations"):
        gmod.granger_from_stats(ref["ssr_r"], ref["ssr_u"], ref["tss"], ref["rank"], status, 10, 3)
    with pytest.raises(ValueError, match="Insufficient observations"):      # before any engine call
        gmod.granger(pd.DataFrame(np.random.default_rng(0).normal(size=(10, 3))))
    with pytest.raises(ValueError, match="Insufficient observations"):
        gr.all_pairs(X[:10], 3)


def test_restatement_raising_conditions():
    rng = np.random.default_rng(1)
    X = rng.normal(size=(40, 3))
    bad = X.copy()
    bad[5, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        gr.all_pairs(bad)
    bad = X.copy()
    bad[:-1, 2] = 7.0                                      # constant except for its last row
    with pytest.raises(ValueError, match="constant"):
        gr.all_pairs(bad)
    bad = X.copy()
    bad[1:, 0] = bad[:-1, 1]                               # y_t = x_{t-1} exactly
    with pytest.raises(ValueError, match="perfect fit"):
        gr.all_pairs(bad)


def test_restatement_two_solves_agree():
    X = gr.gen_var1(60, 3, seed=5)
    d = gr.spread(gr.all_pairs(X), gr.all_pairs(X, solve="lstsq"))
    assert 0 <= d["ratio"] < 1e-12


def test_bound_follows_the_library_guards():
    """fast_path_bound (the GPU tests' B) is computed from the guards the library was built with."""
    tau, floor, beta_c = gmod.fast_path_guards()
    assert 0 < tau < 1 and 0 < floor < 1 and beta_c >= 14.0      # 14: (1 + |b|_1)^2 <= 2 (1 + 6 / lambda_min)
    u = 2.0 ** -53
    assert gmod.fast_path_bound(300) == pytest.approx(2 * beta_c * (5 + 1 + 27) * u / (tau * floor))
    assert gmod.fast_path_bound(2500) == pytest.approx(2 * beta_c * (40 + 2 + 27) * u / (tau * floor))


def test_single_column_frame_has_no_test():
    """granger.py:13-16 runs no test for one column: a 1 x 1 zero matrix, whatever T is."""
    adj = gmod.granger(pd.DataFrame({"a_cpu": np.arange(5.0)}))
    assert adj.shape == (1, 1) and adj.sum() == 0
    assert np.isnan(gmod.granger_pvalues(pd.DataFrame({"a_cpu": np.arange(50.0)}))).all()


def test_granger_asserts_on_unknown_test():
    with pytest.raises(AssertionError):
        gmod.granger(pd.DataFrame(np.zeros((50, 3))), test="bogus")


def test_rq2_methods_serve_granger():
    from rcaeval_amd import e2e, rq2
    m = rq2.methods()
    assert m["granger_pagerank"] is e2e.granger_pagerank and m["granger_randomwalk"] is e2e.granger_randomwalk
    assert {"pc_pagerank", "pc_randomwalk", "cloudranger", "circa"} <= set(m)


def _frame():
    from rcaeval_amd import synth
    from rcaeval_amd.io.time_series import preprocess
    df = synth.telemetry_frame(6, 80, n_constant=0, seed=3)
    return df, preprocess(data=df, dataset="online-boutique", dk_select_useful=False).columns.to_list()


def test_granger_pagerank_wrapper(monkeypatch):
    import sys
    import rcaeval_amd.e2e  # noqa: F401  (e2e.granger_pagerank is the function; its module is in sys.modules)
    mod = sys.modules["rcaeval_amd.e2e.granger_pagerank"]
    df, names = _frame()
    n = len(names)
    adj = np.zeros((n, n))
    adj[0, 1] = adj[2, 1] = adj[3, 2] = adj[4, 0] = 1.0
    monkeypatch.setattr(mod, "granger", lambda data: adj.copy())
    monkeypatch.setattr(mod, "page_rank", lambda a, node_names=None: [(nm, float(-k)) for k, nm in enumerate(node_names)][::-1])
    out = mod.granger_pagerank(df, 0, dataset="online-boutique")
    assert set(out) == {"adj", "node_names", "ranks"}
    np.testing.assert_array_equal(out["adj"], adj)
    assert out["node_names"] == names and out["ranks"] == names      # sorted by the stub's scores, descending
    # the all-zero branch never reaches page_rank
    monkeypatch.setattr(mod, "granger", lambda data: np.zeros((n, n)))
    monkeypatch.setattr(mod, "page_rank", lambda *a, **k: (_ for _ in ()).throw(AssertionError("called")))
    out = mod.granger_pagerank(df, 0, dataset="online-boutique")
    assert out["ranks"] == names and out["node_names"] == names and out["adj"].sum() == 0
    # a raising granger ends in @rca's dummy ranking
    monkeypatch.setattr(mod, "granger", lambda data: (_ for _ in ()).throw(ValueError("perfect fit")))
    assert mod.granger_pagerank(df, 0, dataset="online-boutique") == {"adj": [], "node_names": names, "ranks": names}


def test_granger_randomwalk_wrapper(monkeypatch):
    import sys
    from rcaeval_amd import e2e
    mod = sys.modules["rcaeval_amd.e2e.pc_randomwalk"]
    df, names = _frame()
    n = len(names)
    adj = np.zeros((n, n))
    adj[0, 1] = adj[2, 1] = 1.0
    seen = {}

    def walk(a, node_names, num_loop=None):
        seen["adj"], seen["num_loop"] = a, num_loop
        return [(nm, float(k)) for k, nm in enumerate(node_names)]
    monkeypatch.setattr(mod, "granger", lambda data: adj.copy())
    monkeypatch.setattr(mod, "random_walk", walk)
    out = e2e.granger_randomwalk(df, 0, dataset="online-boutique")
    assert seen["num_loop"] == n and seen["adj"].dtype.kind == "i"
    np.testing.assert_array_equal(seen["adj"], adj.astype(bool).astype(int))
    np.testing.assert_array_equal(out["adj"], adj.astype(int))
    assert out["node_names"] == names and out["ranks"] == names[::-1]
    e2e.granger_randomwalk(df, 0, dataset="online-boutique", n_iter=7)
    assert seen["num_loop"] == 7
