"""CPU: the PCMCI feature's host side — the pcg_pcmci_* bindings, the pure-numpy assembly
(graph_construction.pcmci.pcmci_from_stats) against the restatement in tests/pcmci_ref.py, and
microcause's Q matrix and walk against the restatement's literal np.random.choice loop."""
import ctypes
import os
import re

import numpy as np
import pytest

import pcmci_ref as pr
from rcaeval_amd.graph_construction import pcmci as pmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name, nargs", [("pcg_pcmci_parents", 16), ("pcg_pcmci_mci", 11)])
def test_header_library_and_bindings_agree(name, nargs):
    from rcaeval_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pcgpu.h")).read()
    decl = re.search(r"^int %s\((.*?)\);" % name, hdr, re.S | re.M).group(1)
    params = [p.strip() for p in decl.replace("\n", " ").split(",")]
    sig = {nm: (res, args) for nm, res, args in _lib.SIGNATURES}[name]
    assert sig[0] is ctypes.c_int32 and len(sig[1]) == len(params) == nargs
    for p, a in zip(params, sig[1]):
        if "*" in p:
            assert a is ctypes.c_void_p or a is ctypes.POINTER(ctypes.c_int64), (p, a)
        elif p.startswith("int64_t"):
            assert a is ctypes.c_int64, (p, a)
        elif p.startswith("int32_t"):
            assert a is ctypes.c_int32, (p, a)
        else:
            assert a is ctypes.c_int, (p, a)
    assert getattr(lib, name).argtypes == sig[1]
    assert int(re.search(r"#define PCG_ABI_VERSION (\d+)", hdr).group(1)) == _lib.PCG_ABI_VERSION == 4
    # a NULL handle is refused before anything is touched
    args = [None if a is ctypes.c_void_p or a is ctypes.POINTER(ctypes.c_int64) else 3 for a in sig[1]]
    assert getattr(lib, name)(*args) == _lib.PCG_ERR_INVALID


def test_limits_and_bound_follow_the_library():
    lim = pmod.limits()
    assert lim["z_cap"] + 2 <= 64 and lim["max_tau"] >= 10 and lim["max_candidates"] >= 2000
    assert 0 < lim["tau"] < 1 and lim["beta_c"] >= 4.0
    assert pmod.fast_path_bound(12) == pytest.approx(2 * lim["beta_c"] * 30 * 2.0 ** -53 / lim["tau"])
    assert pmod.fast_path_bound(12) < 1e-9


@pytest.fixture(scope="module")
def ref():
    return pr.case(60, 3, 2, 0.2, 5)


def test_critical_values_decide_like_the_p_value(ref):
    """|val| < crit[d]  <=>  p > pc_alpha, on every depth the restatement reached."""
    crit = pmod.critical_values(ref["T_eff"], 0.2, 8)
    for d in range(8):
        for val in np.linspace(0.0, 0.99, 397):
            p = pr.pvalue(val, ref["T_eff"], d)
            if abs(p - 0.2) > 1e-9:
                assert (val < crit[d]) == (p > 0.2), (d, val)
    assert (pmod.critical_values(10, 0.2, 12)[8:] == 0).all()       # deg_f < 1: p is NaN, nothing is removed


def test_assembly_reproduces_the_restatement(ref):
    adj, link, p, val = pmod.pcmci_from_stats(ref["val_matrix"], ref["dim_matrix"], ref["T_eff"])
    np.testing.assert_array_equal(val, ref["val_matrix"])
    np.testing.assert_allclose(p, ref["p_matrix"], rtol=1e-13, atol=0)
    np.testing.assert_array_equal(link, ref["link"])
    np.testing.assert_array_equal(adj, ref["adj"])
    assert p[0, 0, 0] == 1 and val[0, 0, 0] == 0 and ref["dim_matrix"][0, 0, 0] == -1
    assert 0 < adj.sum() <= 9


def test_assembly_edge_cases():
    val = np.array([[[0.0, 1.0, 0.3]]])
    dim = np.array([[[-1, 0, 20]]])
    _, p = pmod.matrices_from_stats(val, dim, 10)
    assert p[0, 0, 0] == 1 and p[0, 0, 1] == 0 and np.isnan(p[0, 0, 2])
    for code in (1, 2):
        with pytest.raises(ValueError):
            pmod.raise_on_status(np.array([0, 3, code]))
    pmod.raise_on_status(np.array([0, 3, 3]))


def _graph_case():
    rng = np.random.default_rng(4)
    n = 6
    data = np.cumsum(rng.normal(size=(80, n)), axis=0) + rng.normal(size=(80, n))
    names = [f"s{k}_cpu" for k in range(n)]
    p = np.ones((n, n, 3))
    for i, j, tau in ((0, 1, 1), (1, 2, 2), (2, 1, 1), (3, 3, 1), (4, 0, 2), (0, 4, 1), (5, 2, 1), (1, 5, 0)):
        p[i, j, tau] = 1e-4
    p[2, 4, 1] = 0.0011                                    # above the 0.001 level: no link
    return data, names, p


def test_microcause_graph_q_and_walk_equal_the_literal_loop():
    import sys
    import rcaeval_amd.e2e  # noqa: F401
    mc = sys.modules["rcaeval_amd.e2e.microcause"]
    data, names, p = _graph_case()
    g = mc.significant_graph(p)
    np.testing.assert_array_equal(g, pr.significant_graph(p))
    assert g[1, 0] == 1 and g[3, 3] == 1 and g[5, 1] == 0 and g[4, 2] == 0 and g.sum() == 7
    for sli in ("s0_cpu", "s2_cpu"):
        fe = names.index(sli)
        Q = mc.q_matrix(data, g, fe)
        np.testing.assert_array_equal(Q, pr.q_matrix(data, g, fe))
        rows = Q.sum(axis=1)
        assert ((np.abs(rows - 1) < 1e-12) | (rows == 0)).all() and Q.any()
        np.random.seed(7)
        got = mc.randomwalk(Q, 20, fe + 1, walk_step=50)
        np.random.seed(7)
        want = pr.randomwalk(Q, 20, fe + 1, 50)
        assert got == want and sum(v for _, v in got) > 0
        np.random.seed(0)
        out = mc.ranks_from_p(data, names, p, sli, epochs=20, walk_step=50)
        np.random.seed(0)
        assert out["ranks"] == pr.microcause_ranks(data, names, p, sli, epochs=20, walk_step=50)["ranks"]
        assert sorted(out["ranks"]) == sorted(names)


def test_microcause_requires_its_sli():
    import pandas as pd
    from rcaeval_amd import e2e
    df = pd.DataFrame(np.random.default_rng(0).normal(size=(60, 3)), columns=["a_cpu", "b_cpu", "c_cpu"])
    df.insert(0, "time", np.arange(60))
    with pytest.raises(ValueError):
        e2e.microcause(df, 0, dataset="online-boutique", sli=None)


def test_rq2_methods_serve_microcause():
    from rcaeval_amd import e2e, rq2
    m = rq2.methods()
    assert m["microcause"] is e2e.microcause
    assert {"pc_pagerank", "granger_pagerank", "micro_diag"} <= set(m)


def test_restatement_two_solves_agree(ref):
    assert 0 <= ref["delta"] < 1e-13 and not ref["constant"]
