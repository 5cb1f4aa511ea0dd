"""GPU: pcg_fges_begin / pcg_fges_gains, the fges graph learner and fges_pagerank / fges_randomwalk
against the numpy restatement of the fGES contract (tests/fges_ref.py).

Tolerance of every g: ``fast_path_bound(zmax) + 10 * delta`` absolute. The bound is the documented
one of an accepted fast-path value ("fGES") at the largest |B| the restatement met on the
input; delta is the restatement's own uncertainty on that input, the largest difference between its
lstsq and QR solves. Nothing in the tolerance comes from the engine's output.

The adjacency, the insert / delete sequence and the e2e ranks are compared exactly, which needs
every decision stable under A = 1e3 * T * tolerance. The seeds in ``CASES`` are chosen so that the
restatement alone satisfies, as asserted in ``test_restatement_preconditions``: (a) every evaluated
|bump| >= A; (b) at every pop no other live arrow within A of the popped bump except its mirror
(b -> a on the same empty sets); (c) both orders of the mirrored initial arrows end in the same
graph; (d) zmax within the kernel's cap; (e) a BES deletion in at least one case.

Worst observed |error| / tolerance: see DESIGN.md, "fGES".
"""
import functools

import numpy as np
import pandas as pd
import pytest

import fges_ref as fr
from rcaeval_amd.graph_construction import fges as fmod

pytestmark = pytest.mark.gpu

# (kind, T, n, seed): one pair with a positive and one with a negative bump, a collider (a
# single-candidate group with |B| = 1), two random DAGs (wide groups, T-subset groups, BES)
CASES = [("pair", 40, 2, 1), ("pair", 40, 2, 0), ("collider", 80, 3, 0), ("dag", 200, 6, 1), ("dag", 300, 8, 3)]
IDS = ["%s-%dx%d-s%d" % c for c in CASES]


def _eng():
    from rcaeval_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(scope="module", autouse=True)
def _engine_first():
    """The engine (and with it torch's HIP runtime) is created before anything else loads the library."""
    _eng()


@functools.lru_cache(maxsize=None)
def _data(case):
    kind, T, n, seed = case
    if kind == "pair":
        return fr.gen_dag(T, n, seed, p_edge=1.0)
    if kind == "collider":
        return fr.gen_named("collider", T, seed)
    return fr.gen_dag(T, n, seed)


@functools.lru_cache(maxsize=None)
def _ref(case, mirror="ji"):
    return fr.search(_data(case), mirror)


def _tol(zmax, delta):
    return fmod.fast_path_bound(zmax) + 10.0 * delta


@functools.lru_cache(maxsize=None)
def _engine(case):
    trace = {}
    adj = fmod.fges(_data(case).copy(), _trace=trace)
    return adj, trace


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_preconditions(case):
    ref = _ref(case)
    tol = _tol(ref["zmax"], ref["delta"])
    A = 1e3 * ref["T"] * tol
    pre = fr.preconditions(ref)
    print(f"preconditions {case}: {pre} tol {tol:.3e} A {A:.3e} delta {ref['delta']:.2e}")
    assert pre["min_bump"] >= A                                                             # (a)
    assert pre["min_gap"] >= A                                                              # (b)
    np.testing.assert_array_equal(_ref(case, "ij")["adj"], ref["adj"])                      # (c)
    assert pre["zmax"] <= fmod.limits()["b_cap"]                                            # (d)


def test_some_case_deletes_in_bes():
    assert any(_ref(c)["deleted"] for c in CASES)                                           # (e)
    assert _ref(CASES[4])["deleted"] and _ref(CASES[4])["zmax"] >= 3


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_graph_and_sequences_equal_the_restatement(case):
    ref = _ref(case)
    adj, trace = _engine(case)
    np.testing.assert_array_equal(adj, ref["adj"])
    assert trace["inserted"] == ref["inserted"] and trace["deleted"] == ref["deleted"]
    assert {e[:3] for e in trace["evaluated"]} == {e[:3] for e in ref["evaluated"]}
    assert trace["stats"]["fallback_items"] == 0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_gain_within_the_documented_bound(case):
    ref = _ref(case)
    _, trace = _engine(case)
    tol = _tol(ref["zmax"], ref["delta"])
    want = {e[:3]: e[3] for e in ref["evaluated"]}
    worst = max(abs(e[4] - want[e[:3]]) for e in trace["evaluated"])
    print(f"gains {case}: items {len(trace['evaluated'])} worst |error| {worst:.3e} tolerance {tol:.3e} "
          f"ratio {worst / tol:.3e} exact {trace['stats']['exact_items']}")
    assert worst <= tol
    assert trace["stats"]["exact_items"] == 0                                               # nothing ill-conditioned here


def test_one_pair_both_directions_and_the_sign_of_the_bump():
    for case in CASES[:2]:
        X = _data(case)
        ref = _ref(case)
        out = _eng().fges_begin(X)
        g = fr.Scorer(X).gain(0, 1, ())
        tol = _tol(0, ref["delta"])
        assert abs(out["gain0"][0, 1] - g) <= tol and abs(out["gain0"][1, 0] - g) <= tol
        assert out["gain0"][0, 1] == out["gain0"][1, 0] and np.isnan(out["gain0"][0, 0]) and (out["status"] == 0).all()
        bump = case[1] * out["gain0"][0, 1] - 2.0 * np.log(case[1])
        assert (bump > 0) == (ref["evaluated"][0][4] > 0) == bool(ref["inserted"])
    assert _ref(CASES[0])["inserted"] and not _ref(CASES[1])["inserted"]


def test_collider_single_candidate_group():
    case = CASES[2]
    X, ref = _data(case), _ref(case)
    eng = _eng()
    eng.fges_begin(X)
    out = eng.fges_gains([(2, (0,), [1])])
    g = fr.Scorer(X).gain(1, 2, (0,))
    assert out["status"].tolist() == [0] and abs(out["gain"][0] - g) <= _tol(1, ref["delta"])
    np.testing.assert_array_equal(_engine(case)[0], [[0, 0, 1], [0, 0, 1], [0, 0, 0]])


@functools.lru_cache(maxsize=None)
def _wide():
    X = fr.gen_dag(300, 20, 4, p_edge=0.25)
    sc = fr.Scorer(X)
    groups = [(19, (0, 3, 7, 11, 15), [c for c in range(19) if c not in (0, 3, 7, 11, 15)]),   # 14 candidates, |B| = 5
              (5, (1, 2, 8, 9, 12, 17), [0, 3, 4, 6, 7]),                                        # the first wide size
              (5, (1, 2, 8, 9, 12, 17), [0, 3, 4, 6]),                                           # the last narrow size
              (6, (10,), [2]), (6, (), [2, 3]), (7, tuple(range(8, 19)), [0, 19])]
    want = np.array([sc.gain(x, y, B) for y, B, cand in groups for x in cand])
    return X, groups, want, sc.delta, sc.zmax


def test_wide_and_narrow_groups_with_a_leading_dimension():
    import torch
    X, groups, want, delta, zmax = _wide()
    eng = _eng()
    T, n = X.shape
    wide = torch.full((T, n + 5), float("nan"), dtype=torch.float64, device=eng.device)
    wide[:, :n] = torch.from_numpy(X).to(eng.device)
    beg = eng.fges_begin(wide[:, :n])
    assert (beg["status"] == 0).all()
    out = eng.fges_gains(groups)
    tol = _tol(zmax, delta)
    err = float(np.max(np.abs(out["gain"] - want)))
    print(f"wide groups: items {len(want)} zmax {zmax} worst |error| {err:.3e} tolerance {tol:.3e} ratio {err / tol:.3e}")
    assert zmax == 11 and len(groups[0][2]) == 14 > 3 * 4
    assert (out["status"] == 0).all() and out["exact_items"] == 0 and err <= tol
    sc = fr.Scorer(X)
    g0 = np.array([[sc.gain(i, j, ()) if i != j else np.nan for j in range(n)] for i in range(n)])
    assert np.nanmax(np.abs(beg["gain0"] - g0)) <= _tol(0, sc.delta)
    np.testing.assert_array_equal(beg["gain0"], beg["gain0"].T)                               # NaN diagonal, symmetric


def test_empty_base_and_a_group_without_items():
    X, _, _, delta, _ = _wide()
    eng = _eng()
    beg = eng.fges_begin(X)
    out = eng.fges_gains([(4, (), []), (4, (), [0, 9]), (2, (1,), [])])
    assert out["status"].tolist() == [0, 0] and out["exact_items"] == 0
    np.testing.assert_allclose(out["gain"], beg["gain0"][[0, 9], 4], rtol=0, atol=_tol(0, delta))
    none = eng.fges_gains([(4, (), []), (3, (1, 2), [])])
    assert len(none["gain"]) == 0 and len(none["status"]) == 0
    assert len(eng.fges_gains([])["gain"]) == 0


def test_near_duplicate_column_takes_the_exact_path():
    rng = np.random.default_rng(0)
    X = fr.gen_dag(120, 5, 0)
    X[:, 1] = X[:, 0] + 1e-9 * rng.normal(size=120)
    sc = fr.Scorer(X)
    groups = [(3, (0,), [1, 4]), (3, (0, 1), [4, 2]), (3, (0, 2), [1])]
    want = np.array([sc.gain(x, y, B) for y, B, cand in groups for x in cand])
    tol = _tol(sc.zmax, sc.delta)
    eng = _eng()
    eng.fges_begin(X)
    out = eng.fges_gains(groups)
    err = np.abs(out["gain"] - want)
    print(f"near-duplicate: status {out['status'].tolist()} |error| {err} tolerance {tol:.3e} delta {sc.delta:.2e}")
    assert out["status"].tolist() == [3, 0, 3, 3, 3] and out["exact_items"] == 4
    assert (err <= tol).all()
    # depth 0 of the pair itself (1 - r^2 ~ 1e-18): the exact path with an empty base, the same tolerance
    beg = eng.fges_begin(X)
    g01 = sc.gain(0, 1, ())
    tol0 = _tol(0, sc.delta)
    err0 = abs(beg["gain0"][0, 1] - g01)
    print(f"near-duplicate depth 0: g {g01:.6f} |error| {err0:.3e} tolerance {tol0:.3e} ratio {err0 / tol0:.3e} delta {sc.delta:.2e}")
    assert err0 <= tol0 and beg["gain0"][0, 1] == beg["gain0"][1, 0] and g01 > 30
    others = np.array([[sc.gain(i, j, ()) if i != j else np.nan for j in range(5)] for i in range(5)])
    assert np.nanmax(np.abs(beg["gain0"] - others)) <= _tol(0, sc.delta)
    # overlapping item ranges (malformed offsets): every item is listed for the exact path once
    eng.fges_begin(X)
    dup = eng.fges_gains_csr([3, 3, 3], [0, 2, 4, 6], [0, 1, 0, 1, 0, 1], [0, 2, 1, 2], [4, 2], n_narrow=3)
    assert dup["status"].tolist() == [3, 3] and dup["exact_items"] == 2
    assert (np.abs(dup["gain"] - want[2:4]) <= tol).all()


def test_exactly_duplicated_base_column_is_skipped_on_the_exact_path():
    """B = (0, 1) with column 1 an exact copy of column 0: the exact path's QR meets a column with no
    remaining norm and skips it, which is the minimum-norm residual, i.e. the gain on the base (0,).
    The restatement's unpivoted-QR solve is meaningless on the full rank-deficient base (its two
    solves differ by 0.018 there), so the expected value and delta come from the reduced base."""
    X = fr.gen_dag(120, 5, 0)
    X[:, 1] = X[:, 0]
    sc = fr.Scorer(X)
    want = sc.gain(4, 3, (0,))
    tol = _tol(1, sc.delta)
    eng = _eng()
    eng.fges_begin(X)
    out = eng.fges_gains([(3, (0, 1), [4])])
    err = abs(out["gain"][0] - want)
    print(f"duplicated base column: status {out['status'].tolist()} gain {out['gain'][0]!r} want {want!r} "
          f"|error| {err:.3e} tolerance {tol:.3e} delta {sc.delta:.2e}")
    assert out["status"].tolist() == [3] and out["exact_items"] == 1
    assert err <= tol


def test_flagged_columns_give_status_1_and_2():
    X = fr.gen_dag(60, 5, 2)
    X[:, 1] = 3.25
    X[17, 3] = np.nan
    eng = _eng()
    beg = eng.fges_begin(X)
    assert beg["status"].tolist() == [0, 1, 0, 2, 0]
    assert np.isnan(beg["gain0"][1]).all() and np.isnan(beg["gain0"][:, 3]).all() and np.isfinite(beg["gain0"][0, 2])
    out = eng.fges_gains([(4, (0,), [1, 2, 3]), (1, (0,), [2]), (4, (3, 0), [2]), (4, (1, 3), [2]), (3, (), [0])])
    assert out["status"].tolist() == [1, 0, 2, 1, 2, 2, 2]
    assert np.isnan(out["gain"][[0, 2, 3, 4, 5, 6]]).all() and np.isfinite(out["gain"][1])
    with pytest.raises(ValueError, match="constant"):
        fmod.EngineScorer(eng).begin(np.ascontiguousarray(X[:, :3]))
    with pytest.raises(ValueError, match="non-finite"):
        fmod.EngineScorer(eng).begin(np.ascontiguousarray(X[:, 2:]))


def test_refused_items_are_status_4_with_nan_and_fall_back_on_the_host():
    X = fr.gen_dag(150, 70, 3, p_edge=0.05)
    n = 70
    eng = _eng()
    assert (eng.fges_begin(X)["status"] == 0).all()
    big = tuple(range(1, 64))                                                                # 63 ids: above the cap
    groups = [(0, big, [64, 65]),
              (0, (1, 2, n), [3]), (0, (1, -1), [3]), (n, (1,), [3]), (-1, (1,), [3]),         # ids out of range
              (0, (1, 2, 1), [3]),                                                           # a duplicate
              (0, (1, 2), [1, 0, n, -5, 3]),                                                 # x in B, x == y, x out of range; then a good one
              (0, (1, 0), [3]),                                                              # y in B
              (0, tuple(range(1, 63)), [63, 64, 65, 66, 67])]                                # 62 ids: the cap itself
    out = eng.fges_gains(groups)
    st = out["status"].tolist()
    assert st[:11] == [4] * 11 and st[11] == 0 and st[12] == 4 and set(st[13:]) <= {0, 3} and len(st) == 18
    assert np.isnan(out["gain"][:11]).all() and np.isnan(out["gain"][12]) and np.isfinite(out["gain"][13:]).all()
    sc = fr.Scorer(X)
    want = [sc.gain(x, 0, tuple(range(1, 63))) for x in (63, 64, 65, 66, 67)] + [sc.gain(3, 0, (1, 2))]
    got = list(out["gain"][13:]) + [out["gain"][11]]
    assert np.max(np.abs(np.array(got) - np.array(want))) <= _tol(62, sc.delta)
    # malformed offsets: refused too, nothing is written out of bounds
    bad = eng.fges_gains_csr([0, 0], [0, 5, 1], [1, 2], [0, 1, 2], [3, 4], n_narrow=2)
    assert bad["status"].tolist() == [4, 4] and np.isnan(bad["gain"]).all()
    bad = eng.fges_gains_csr([0, 0], [0, 1, 2], [1, 2], [0, 9, 2], [3, 4], n_narrow=2)
    assert bad["status"].tolist() == [4, 4]
    # a group listed on the wrong side of n_narrow is refused; on the right side it is computed
    one = ([0], [0, 1], [1], [0, 1], [3])
    assert eng.fges_gains_csr(*one, n_narrow=0)["status"].tolist() == [4]
    good = eng.fges_gains_csr(*one, n_narrow=1)
    assert good["status"].tolist() == [0] and abs(good["gain"][0] - sc.gain(3, 0, (1,))) <= _tol(1, sc.delta)
    with pytest.raises(Exception):
        eng.fges_gains_csr(*one, n_narrow=2)                                                 # more narrow groups than groups
    # the driver's scorer computes refused items on the host
    s = fmod.EngineScorer(eng)
    s.begin(X)
    res = s.gains([(0, big, [64, 65])])
    ref = fr.Scorer(X)
    np.testing.assert_allclose(res[0], [ref.gain(64, 0, big), ref.gain(65, 0, big)], rtol=0, atol=1e-9)
    assert s.stats["fallback_items"] == 2
    with pytest.raises(ValueError):
        eng.fges_gains_csr([0], [0, 1], [1], [0, 1, 2], [3], n_narrow=1)                      # offsets of the wrong length


def test_bes_from_a_start_graph_on_the_engine():
    X = fr.gen_named("collider", 400, 1)
    start = np.array([[0, 1, 1], [0, 0, 1], [0, 0, 0]])
    trace = {}
    adj = fmod.bes(X, start, _trace=trace)
    ref = fr.bes_from(X, start)
    assert trace["deleted"] == ref["deleted"] and [d[:2] for d in ref["deleted"]] == [(0, 1)]
    np.testing.assert_array_equal(adj, ref["adj"])


def _frame(X):
    names = [f"s{k}_cpu" for k in range(X.shape[1])]
    df = pd.DataFrame(X, columns=names)
    df.insert(0, "time", np.arange(len(df)))
    return df, names


def test_e2e_ranks_equal_the_restatement_pipeline():
    from rcaeval_amd import e2e
    from rcaeval_amd.graph_heads.page_rank import page_rank
    from rcaeval_amd.graph_heads.random_walk import random_walk
    case = CASES[4]
    ref = _ref(case)
    df, names = _frame(_data(case))
    out = e2e.fges_pagerank(df, 0, dataset="online-boutique")
    want = [x[0] for x in sorted(page_rank(ref["adj"].T, node_names=names, n_iter=10), key=lambda x: x[1], reverse=True)]
    np.testing.assert_array_equal(out["adj"], ref["adj"])
    assert out["node_names"] == names and out["ranks"] == want and sorted(want) == sorted(names)
    np.random.seed(11)
    out = e2e.fges_randomwalk(df, 0, dataset="online-boutique")
    np.random.seed(11)
    want = [x[0] for x in sorted(random_walk(ref["adj"].T, names, num_loop=len(names)), key=lambda x: x[1], reverse=True)]
    np.testing.assert_array_equal(out["adj"], ref["adj"])
    assert out["ranks"] == want and len(want) > 0
