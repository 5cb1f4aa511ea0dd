"""GPU: pcg_granger and the granger graph learner against the numpy/scipy restatement of the
statsmodels contract (tests/granger_ref.py), and granger_pagerank / granger_randomwalk end to end.

Tolerance of the statistics (``test_statistics_match_the_restatement``): ssr_r / ssr_u and the
derived F, chi-square and LR agree within B + 10 * delta relative. B = ``fast_path_bound(T)`` is the
documented bound of an accepted fast-path ssr_r / ssr_u; delta is the restatement's own
uncertainty of that quantity on the input, the largest relative spread between its pinv and lstsq
solves over the input's items. Nothing in the tolerance comes from the engine's output.

F, chi-square and LR are multiples of rho - 1 or log rho (rho = ssr_r / ssr_u), so an error e of
rho moves them by e * rho / (rho - 1) relative: an input with an item whose rho - 1 is tiny cannot
meet the bound even with a correctly rounded rho. The seeds in ``SEEDS`` are therefore chosen per
generator and shape so that three preconditions hold, each asserted by the tests: no reference
per-lag value lies within 1e-6 relative of 0.05; on every item rho / (rho - 1) times the larger of
16 * 2^-53 and the ratio's spread stays within the tolerance of F, chi-square and LR; and the
restatement itself raises nowhere.
"""
import functools
import os

import numpy as np
import pandas as pd
import pytest

import granger_ref as gr
from rcaeval_amd import synth
from rcaeval_amd.graph_construction import granger as gmod

pytestmark = pytest.mark.gpu

SHAPES = [(11, 2), (61, 3), (300, 17), (2500, 5)]      # T = 2500 spans two LDS chunks of 2048 rows
# seed per (generator, T, n): the preconditions of the module docstring hold there
SEEDS = {("var1", 11, 2): 3, ("var1", 61, 3): 0, ("var1", 300, 17): 32, ("var1", 2500, 5): 1,
         ("random_walk", 11, 2): 3, ("random_walk", 61, 3): 0, ("random_walk", 300, 17): 149, ("random_walk", 2500, 5): 73,
         ("integrated2", 11, 2): 2, ("integrated2", 61, 3): 0, ("integrated2", 300, 17): 76, ("integrated2", 2500, 5): 4}


@functools.lru_cache(maxsize=None)
def _reference(gen, T, n):
    X = gr.GENERATORS[gen](T, n, SEEDS[gen, T, n])
    X.setflags(write=False)
    ref = gr.all_pairs(X)
    return X, ref, gr.spread(ref, gr.all_pairs(X, solve="lstsq"))


@functools.lru_cache(maxsize=None)
def _engine(gen, T, n):
    from rcaeval_amd.engine import get_engine
    return get_engine(0).granger(_reference(gen, T, n)[0].copy(), maxlag=3)


def _derived(o, T):
    L = np.arange(1, 4)[None, None, :]
    nobs = T - L
    df = nobs - o["rank"]
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = o["ssr_r"] / o["ssr_u"]
        gain = (o["ssr_r"] - o["ssr_u"]) / o["ssr_u"]
        return {"ratio": rho, "F": gain / L * df, "chi2": nobs * gain, "lr": nobs * np.log(rho)}


@pytest.mark.parametrize("T,n", SHAPES)
@pytest.mark.parametrize("gen", list(gr.GENERATORS))
def test_statistics_match_the_restatement(gen, T, n):
    X, ref, delta = _reference(gen, T, n)
    out = _engine(gen, T, n)
    off = ~np.eye(n, dtype=bool)
    assert set(np.unique(out["status"][off])) <= {0, 3}
    np.testing.assert_array_equal(out["rank"][off], ref["rank"][off])
    np.testing.assert_array_equal(out["rank"][~off], 0)
    B = gmod.fast_path_bound(T)
    got, want = _derived(out, T), _derived(ref, T)
    rho = want["ratio"][off].ravel()
    amplified = rho / np.abs(rho - 1) * max(16 * 2.0 ** -53, delta["ratio"])
    for q in ("ratio", "F", "chi2", "lr"):
        tol = B + 10 * delta[q]
        if q != "ratio":
            assert (amplified <= tol).all(), "precondition: an item's rho - 1 is too small for this tolerance"
        err = (np.abs(got[q][off] - want[q][off]) / np.abs(want[q][off])).ravel()
        k = int(np.argmax(err))
        print(f"{gen} T={T} n={n} {q}: worst err {err[k]:.3e} tol {tol:.3e} (B {B:.2e}, delta {delta[q]:.2e}, "
              f"exact {out['exact_items']}/{n * (n - 1) * 3})")
        assert (err <= tol).all(), (q, k, err[k], tol)
    np.testing.assert_allclose(out["tss"][off], ref["tss"][off], rtol=1e-9)


@pytest.mark.parametrize("T,n", SHAPES)
@pytest.mark.parametrize("gen", list(gr.GENERATORS))
def test_adjacency_equals_the_restatement(gen, T, n):
    X, ref, _ = _reference(gen, T, n)
    off = ~np.eye(n, dtype=bool)
    for test in (None,) + gr.TESTS:
        v = gr.values(ref["p"], test)[off]
        assert np.min(np.abs(v - 0.05)) > 1e-6 * 0.05, "precondition: a reference value sits on the threshold"
    out = _engine(gen, T, n)
    for test in (None,) + gr.TESTS:
        adj, _ = gmod.granger_from_stats(out["ssr_r"], out["ssr_u"], out["tss"], out["rank"], out["status"], T, 3,
                                         0.05, test)
        np.testing.assert_array_equal(adj, gr.adjacency(ref["p"], 0.05, test))
    np.testing.assert_array_equal(gmod.granger(pd.DataFrame(X.copy())), gr.adjacency(ref["p"]))


def test_both_paths_run():
    """VAR(1) is well conditioned: nothing may leave the fast path. Doubly integrated noise has
    scaled pivots or ssr_u / tss below the guards at every shape, T = 11 included, where the exact
    kernel's 256 threads share 8 to 10 rows."""
    for T, n in SHAPES:
        assert _engine("var1", T, n)["exact_items"] == 0
        out = _engine("integrated2", T, n)
        off = ~np.eye(n, dtype=bool)
        assert out["exact_items"] == int((out["status"][off] == 3).sum())
        print(f"integrated2 T={T} n={n}: exact {out['exact_items']}/{n * (n - 1) * 3}")
        assert out["exact_items"] > 0


def test_duplicated_column():
    """Column 3 a bitwise copy of column 1: the joint design of (1, 3) and (3, 1) has rank L + 1
    and the x lags add nothing, so ssr_u == ssr_r and every p is 1.0. The restatement's two pinv
    solves differ by rounding, |ssr_r - ssr_u| / ssr_u <= 1e-12, which chi2.sf(nobs * 1e-12, 1) =
    erfc(sqrt(3e-10 / 2)) keeps within 1.4e-5 of 1."""
    X = gr.gen_var1(300, 5, 5)
    X[:, 3] = X[:, 1]
    from rcaeval_amd.engine import get_engine
    out = get_engine(0).granger(X, 3)
    p = gmod.granger_from_stats(out["ssr_r"], out["ssr_u"], out["tss"], out["rank"], out["status"], 300, 3)[1]
    for i, j in ((1, 3), (3, 1)):
        np.testing.assert_array_equal(out["rank"][i, j], [2, 3, 4])
        np.testing.assert_array_equal(out["status"][i, j], [3, 3, 3])
        np.testing.assert_array_equal(p[i, j], np.ones((3, 4)))
        for L in (1, 2, 3):
            r = gr.pair_lag(X[:, i], X[:, j], L)
            assert r["rank"] == L + 1 and np.all(np.abs(r["p"] - 1.0) < 1e-4)
    ref = gr.all_pairs(X)
    np.testing.assert_array_equal(out["rank"], ref["rank"])
    np.testing.assert_array_equal(gmod.granger(pd.DataFrame(X)), gr.adjacency(ref["p"]))


def _error_inputs():
    rng = np.random.default_rng(7)
    base = rng.normal(size=(120, 4)) + 50.0
    a = base.copy()
    a[1:, 0] = a[:-1, 2]                      # y_t = x_{t-1} exactly
    b = base.copy()
    b[:-1, 1] = 3.0                           # constant except for its last row
    c = base[:10].copy()                      # T = 10 = 3 * maxlag + 1
    d = base.copy()
    d[40, 3] = np.nan
    return {"lag_copy": a, "constant_but_last": b, "short": c, "nan": d}


@pytest.mark.parametrize("name", ["lag_copy", "constant_but_last", "short", "nan"])
def test_error_cases_raise_and_rank_dummy(name):
    from rcaeval_amd.e2e import granger_pagerank
    from rcaeval_amd.io.time_series import preprocess
    X = _error_inputs()[name]
    if name != "nan":
        with pytest.raises(ValueError):
            gr.all_pairs(X)                   # the restatement raises too
    df = pd.DataFrame(X, columns=["a_cpu", "b_cpu", "c_cpu", "d_cpu"])
    with pytest.raises(ValueError):
        gmod.granger(df)
    with pytest.raises(ValueError):
        gmod.granger_pvalues(df)
    df.insert(0, "time", np.arange(len(df)))
    names = preprocess(data=df, dataset="online-boutique", dk_select_useful=False).columns.to_list()
    out = granger_pagerank(df, 0, dataset="online-boutique")
    assert out == {"adj": [], "node_names": names, "ranks": names}


def test_engine_refuses_bad_arguments():
    from rcaeval_amd import _lib
    from rcaeval_amd.engine import get_engine
    eng = get_engine(0)
    X = np.random.default_rng(0).normal(size=(50, 3))
    for maxlag in (0, 4):
        with pytest.raises(_lib.PcgError):
            eng.granger(X, maxlag)
    with pytest.raises(ValueError, match="Insufficient observations"):
        eng.granger(X[:7], 2)
    out = eng.granger(X[:8], 2)                # the smallest legal length of maxlag 2
    assert out["ssr_r"].shape == (3, 3, 2) and set(np.unique(out["status"])) <= {0, 3}
    ref = gr.all_pairs(X[:5], 1)               # ... and of maxlag 1
    out = eng.granger(X[:5], 1)
    off = ~np.eye(3, dtype=bool)
    np.testing.assert_allclose((out["ssr_r"] / out["ssr_u"])[off], (ref["ssr_r"] / ref["ssr_u"])[off], rtol=1e-9)


@pytest.fixture(scope="module")
def rq2_case():
    """One RQ2-shaped case (300 rows) and the restatement's adjacency of its preprocessed frame."""
    from rcaeval_amd.io.time_series import preprocess
    df, inject = synth.rq2_case_frame(rows=300, seed=1)
    data = preprocess(data=df, dataset="online-boutique", dk_select_useful=False)
    ref = gr.all_pairs(data.to_numpy().astype(float))
    off = ~np.eye(data.shape[1], dtype=bool)
    assert np.min(np.abs(gr.values(ref["p"])[off] - 0.05)) > 1e-6 * 0.05
    return df, inject, data.columns.to_list(), gr.adjacency(ref["p"])


def test_granger_pagerank_equals_restatement_pipeline(rq2_case):
    from rcaeval_amd.e2e import granger_pagerank
    from rcaeval_amd.graph_heads.page_rank import page_rank
    df, inject, names, adj = rq2_case
    assert adj.sum() > 0
    out = granger_pagerank(df, inject, dataset="online-boutique")
    np.testing.assert_array_equal(out["adj"], adj)
    want = [x[0] for x in sorted(page_rank(adj, node_names=names), key=lambda x: x[1], reverse=True)]
    assert out["node_names"] == names and out["ranks"] == want and len(want) > 0


def test_granger_randomwalk_equals_restatement_pipeline(rq2_case):
    from rcaeval_amd.e2e import granger_randomwalk
    from rcaeval_amd.graph_heads.random_walk import random_walk
    df, inject, names, adj = rq2_case
    np.random.seed(11)
    out = granger_randomwalk(df, inject, dataset="online-boutique")
    np.random.seed(11)
    iadj = adj.astype(bool).astype(int)
    want = [x[0] for x in sorted(random_walk(iadj, names, num_loop=len(names)), key=lambda x: x[1], reverse=True)]
    np.testing.assert_array_equal(out["adj"], iadj)
    assert out["node_names"] == names and out["ranks"] == want and len(want) > 0


def test_rq2_run_granger_pagerank(tmp_path):
    from rcaeval_amd import rq2
    root = os.path.join(str(tmp_path), "data", "online-boutique")
    synth.write_rq2_dataset(root, services=["cartservice"], faults=("cpu",), cases=2, rows=300)
    out_dir = os.path.join(str(tmp_path), "out")
    res = rq2.run(root, "granger_pagerank", "online-boutique", out_dir)
    assert res["cases"] == 2
    for p in rq2.list_cases(root):
        c = rq2.load_case(p)
        got = rq2.load_json(os.path.join(out_dir, "results", c["result_name"]))["0"]
        assert len(got) > 0 and len(set(got)) == len(got)
