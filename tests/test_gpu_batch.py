"""GPU: many small cases (n <= 64) in one launch — pcg_skeleton_batch (k_pc_small_batch, one
workgroup per case) and the batched K1 (k_corr_small_batch) against the single-case path
(bitwise, on given C), numpy's corrcoef (K1 tolerance atol 2e-14) and the C oracle; the level-loop
fallback and per-case errors inside a batch; the flags a batch takes and refuses; the handle
after a batch; and the layers above: pc_batch == pc, pc_pagerank_batch == pc_pagerank,
rq2.run(batch=8) == rq2.run(batch=0).

Fixture note: oracle.cpc.skeleton on np.corrcoef finds no test within 1e-9 of alpha for any
fixture used here, so a 2e-14 difference in C cannot flip a decision; every comparison across K1
variants asserts that (len(ref.near_alpha) == 0) instead of assuming it."""
import json
import os

import numpy as np
import pytest

from oracle import cpc
from rcaeval_amd import _lib, synth
from tests.tests_support import assert_skeleton_matches

pytestmark = pytest.mark.gpu

# (n, N, seed, w_low, w_high, edge_prob): the small-graph suite's shapes
CASES = [(2, 50, 0, .3, .9, None), (3, 40, 1, .3, .9, None), (12, 300, 2, .3, .9, .3), (20, 500, 1, .3, .9, None),
         (33, 700, 3, .1, .5, .2), (44, 600, 4, .2, .8, .1), (48, 2000, 5, .1, .3, .3), (64, 1000, 4, .2, .8, .08),
         (40, 400, 3, .1, .3, .3)]
K1_ATOL = 2e-14


@pytest.fixture(scope="module")
def eng():
    from rcaeval_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(scope="module")
def data():
    """The CASES' data, numpy correlations and sample counts, computed once (no test writes to them)."""
    Xs = [synth.gaussian_sem(n, N, seed=seed, w_low=wl, w_high=wh, edge_prob=ep) for n, N, seed, wl, wh, ep in CASES]
    Cs = [np.corrcoef(X.T) for X in Xs]
    return Xs, Cs, [c[1] for c in CASES]


def _rows(out):
    xy, bits = np.asarray(out.sep_xy), np.asarray(out.sep_bits)
    return sorted((int(x), int(y), tuple(int(b) for b in row)) for (x, y), row in zip(xy, bits))


def _same(a, b):
    np.testing.assert_array_equal(a.removed_level, b.removed_level)
    for k in ("levels", "tests", "calls", "indep", "edges_after", "max_degree", "near_alpha", "error"):
        assert a.stats[k] == b.stats[k], k
    np.testing.assert_array_equal(a.deg_levels, b.deg_levels)
    assert _rows(a) == _rows(b)


def _near_collinear(n=40, N=800, noise=1e-4):
    """Near-duplicate columns: their tests fail the conditioning guard and queue for the exact
    path (the band queue) in threshold mode."""
    rng = np.random.default_rng(11)
    X = synth.gaussian_sem(n, N, seed=12, w_low=0.2, w_high=0.8, edge_prob=0.1)
    for j, i in ((5, 3), (17, 9), (30, 31), (22, 5)):
        X[:, j] = X[:, i] + noise * rng.standard_normal(N)
    return np.corrcoef(X.T), N


@pytest.mark.parametrize("max_depth", [-1, 0, 2])
def test_batch_equals_single_bitwise_on_given_C(eng, data, max_depth):
    from rcaeval_amd.engine import Engine
    _, Cs, Ns = data
    single = [eng.skeleton(C, N, max_depth=max_depth) for C, N in zip(Cs, Ns)]
    assert all(s.stats["driver"] == "small" for s in single)
    outs = eng.skeleton_batch(Cs, Ns, max_depth=max_depth)          # smallest n first
    assert len(outs) == len(CASES)
    for out, s in zip(outs, single):
        assert out.rc == 0 and out.stats["driver"] == "small"
        _same(out, s)
    # largest n first, as the first call of a fresh handle: the mixed-n binomial table
    order = sorted(range(len(CASES)), key=lambda i: -CASES[i][0])
    e = Engine(0)
    try:
        outs = e.skeleton_batch([Cs[i] for i in order], [Ns[i] for i in order], max_depth=max_depth)
        for i, out in zip(order, outs):
            assert out.rc == 0 and out.stats["driver"] == "small"
            _same(out, single[i])
        # the batch left the handle coherent: single runs of n = 64 and n = 12 against the oracle
        for i in (7, 2):
            s = e.skeleton(Cs[i], Ns[i], max_depth=max_depth)
            assert s.stats["driver"] == "small"
            ref = cpc.skeleton(Cs[i], Ns[i], max_depth=max_depth)
            assert assert_skeleton_matches(s, ref, CASES[i][0]) == 0
            _same(s, single[i])
    finally:
        e.close()


def test_batch_more_cases_than_compute_units(eng):
    n, N, B = 12, 300, 300
    Cs = [np.corrcoef(synth.gaussian_sem(n, N, seed=1000 + k, w_low=.3, w_high=.9, edge_prob=.3).T) for k in range(B)]
    outs = eng.skeleton_batch(Cs, N)
    assert len(outs) == B
    for C, out in zip(Cs, outs):
        ref = cpc.skeleton(C, N)
        assert out.rc == 0 and out.stats["driver"] == "small"
        np.testing.assert_array_equal(out.removed_level, ref.removed_level)
        assert list(out.stats["tests"]) == list(ref.tests)
    for k in (0, 1, 63, 128, 255, 256, 298, 299):
        _same(outs[k], eng.skeleton(Cs[k], N))


def test_batch_fallback_reruns_one_case_on_the_level_loop(eng, data):
    _, Cs, Ns = data
    Cn, Nn = _near_collinear()
    assert not cpc.skeleton(Cn, Nn).error
    batch_C, batch_N = [Cn] + list(Cs[0:4]), [Nn] + list(Ns[0:4])
    with eng.tuned(SMALL_QCAP=1):
        single = [eng.skeleton(C, N) for C, N in zip(batch_C, batch_N)]
        outs = eng.skeleton_batch(batch_C, batch_N)
    drivers = [o.stats["driver"] for o in outs]
    assert drivers == [s.stats["driver"] for s in single]
    assert "small_rerun" in drivers and "small" in drivers
    for out, s in zip(outs, single):
        assert out.rc == 0
        _same(out, s)
    # the handle serves a plain run after the reruns
    _same(eng.skeleton(Cs[3], Ns[3]), single[4])


def test_batch_per_case_errors(eng, data):
    _, Cs, Ns = data
    X = synth.gaussian_sem(12, 500, seed=1, w_low=.3, w_high=.9, edge_prob=.3)
    X[:, 7] = X[:, 2]
    outs = eng.skeleton_batch([Cs[2], np.corrcoef(X.T), Cs[3]], [Ns[2], 500, Ns[3]])   # returns: PCG_OK
    assert outs[1].rc == _lib.PCG_ERR_SINGULAR == outs[1].stats["error"]
    for out, i in ((outs[0], 2), (outs[2], 3)):
        assert out.rc == 0
        _same(out, eng.skeleton(Cs[i], Ns[i]))
    # N - d - 3 < 0 (math domain error in the reference): whatever the single path does
    X = synth.gaussian_sem(8, 5, seed=3, w_low=.5, w_high=1.0, edge_prob=.9)
    C = np.corrcoef(X.T)
    try:
        s = eng.skeleton(C, 5)
        want = (0, s.removed_level.tolist())
    except ValueError as e:
        want = (_lib.PCG_ERR_SINGULAR if "singular" in str(e) else _lib.PCG_ERR_DOMAIN, None)
    outs = eng.skeleton_batch([Cs[2], C, Cs[3]], [Ns[2], 5, Ns[3]])
    assert outs[1].rc == want[0]
    if want[0] == 0:
        assert outs[1].removed_level.tolist() == want[1]
    for out, i in ((outs[0], 2), (outs[2], 3)):
        assert out.rc == 0
        _same(out, eng.skeleton(Cs[i], Ns[i]))


def test_batch_constant_column_from_data(eng, data):
    Xs, _, _ = data
    X = synth.gaussian_sem(17, 400, seed=31, w_low=0.3, w_high=0.9, edge_prob=0.2)
    X[:, 4] = 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        Cref = np.corrcoef(X.T)
    ref = cpc.skeleton(Cref, 400)
    assert len(ref.near_alpha) == 0
    outs = eng.skeleton_batch([Xs[2], X, Xs[3]], from_data=True)
    out = outs[1]
    C = out.extra["C"].cpu().numpy()
    np.testing.assert_array_equal(np.isnan(C), np.isnan(Cref))
    assert np.isnan(C[4]).all() and np.isnan(C[:, 4]).all()
    ok = ~np.isnan(Cref)
    np.testing.assert_allclose(C[ok], Cref[ok], rtol=0, atol=K1_ATOL)
    assert out.rc == 0 and out.stats["driver"] == "small"
    np.testing.assert_array_equal(out.removed_level, ref.removed_level)
    assert out.levels == ref.levels == 16


def test_batch_flags(eng, data):
    _, Cs, Ns = data
    sel = [2, 3, 4, 5]
    outs = eng.skeleton_batch([Cs[i] for i in sel], [Ns[i] for i in sel], flags=_lib.PCG_FLAG_FULL_P)
    for i, out in zip(sel, outs):
        s = eng.skeleton(Cs[i], Ns[i], flags=_lib.PCG_FLAG_FULL_P)
        _same(out, s)
        assert len(out.near_alpha) == len(s.near_alpha)
        key = lambda r: (int(r["a"]), int(r["b"]), int(r["d"]), tuple(int(v) for v in r["s"]), float(r["p"]))  # noqa: E731
        assert sorted(map(key, out.near_alpha)) == sorted(map(key, s.near_alpha))
    outs = eng.skeleton_batch([Cs[2], Cs[3]], [Ns[2], Ns[3]], flags=_lib.PCG_FLAG_EXACT_ALL)
    for i, out in zip((2, 3), outs):
        s = eng.skeleton(Cs[i], Ns[i], flags=_lib.PCG_FLAG_EXACT_ALL)
        assert out.rc == 0 and out.stats["driver"] == s.stats["driver"]
        assert out.stats["exact"] == s.stats["exact"]
        _same(out, s)
    # what a batch does not run is refused before anything is launched
    with pytest.raises(_lib.PcgError) as ei:
        eng.skeleton_batch([Cs[2]], [Ns[2]], flags=_lib.PCG_FLAG_RECORD)
    assert ei.value.code == _lib.PCG_ERR_INVALID
    ban = np.zeros((12, 12), bool)
    ban[0, 1] = ban[1, 0] = True
    bd = eng._banned(ban, 12)
    try:
        with pytest.raises(_lib.PcgError) as ei:
            eng.skeleton_batch([Cs[2]], [Ns[2]])
        assert ei.value.code == _lib.PCG_ERR_INVALID
    finally:
        eng._unban(bd)
    with pytest.raises(_lib.PcgError) as ei:          # n = 65 does not fit the small kernel
        eng.skeleton_batch([np.eye(65)], [100])
    assert ei.value.code == _lib.PCG_ERR_INVALID
    _same(eng.skeleton_batch([Cs[2]], [Ns[2]])[0], eng.skeleton(Cs[2], Ns[2]))     # and the handle still serves


def _hard(kind):
    """test_corr_hard_columns_match_numpy's column treatments at n = 40."""
    rng = np.random.default_rng({"plain": 1, "scales": 2, "constant": 3}[kind])
    n, N = 40, 3000
    X = synth.gaussian_sem(n, N, seed=11, w_low=0.2, w_high=0.8)
    if kind == "scales":
        X *= 10.0 ** rng.uniform(-8, 7, n)
        X[:, 5] += 1e9
    elif kind == "constant":           # exactly summable: mean exact, variance 0, numpy's 0/0
        X[:, 3] = 0.0
        X[:, 7] = 2.5
    return X


def test_batched_k1_matches_numpy_and_ignores_batch_position(eng, data):
    Xs, Cs, _ = data
    outs = eng.skeleton_batch(Xs[2:], from_data=True)
    for out, Cref in zip(outs, Cs[2:]):
        np.testing.assert_allclose(out.extra["C"].cpu().numpy(), Cref, rtol=0, atol=K1_ATOL)
    hard = [_hard(k) for k in ("plain", "scales", "constant")]
    outs = eng.skeleton_batch(hard, from_data=True, max_depth=0)
    for X, out in zip(hard, outs):
        with np.errstate(invalid="ignore", divide="ignore"):
            Cref = np.corrcoef(X.T)
        C = out.extra["C"].cpu().numpy()
        np.testing.assert_array_equal(np.isnan(C), np.isnan(Cref))
        ok = ~np.isnan(Cref)
        np.testing.assert_allclose(C[ok], Cref[ok], rtol=0, atol=K1_ATOL)
    # the summation order is fixed by the case alone: same bits at position 0, at position 7, alone
    X = Xs[5]
    outs = eng.skeleton_batch([X, Xs[2], Xs[7], Xs[3], Xs[4], Xs[6], Xs[8], X], from_data=True, max_depth=0)
    alone = eng.skeleton_batch([X], from_data=True, max_depth=0)[0].extra["C"].cpu().numpy()
    c0, c7 = outs[0].extra["C"].cpu().numpy(), outs[7].extra["C"].cpu().numpy()
    assert c0.tobytes() == c7.tobytes() == alone.tobytes()


def test_batch_from_data_matches_oracle(eng, data):
    Xs, Cs, Ns = data
    outs = eng.skeleton_batch(Xs, from_data=True)
    for (n, N, *_), C, out in zip(CASES, Cs, outs):
        ref = cpc.skeleton(C, N)
        assert len(ref.near_alpha) == 0
        assert out.rc == 0 and out.stats["driver"] == "small" and len(out.near_alpha) == 0
        assert assert_skeleton_matches(out, ref, n) == 0
        assert out.levels == ref.levels


def test_pc_batch_equals_pc(eng, data):
    from rcaeval_amd.causal import pc, pc_batch
    Xs, Cs, Ns = data
    datas = [np.array(X) for X in Xs[2:6]] + [synth.gaussian_sem(70, 600, seed=9, w_low=.2, w_high=.8, edge_prob=.05)]
    for C, N in zip(Cs[2:6], Ns[2:6]):
        assert len(cpc.skeleton(C, N).near_alpha) == 0
    got = pc_batch(datas)
    assert len(got) == len(datas)
    assert [g.stats["driver"] for g in got] == ["small"] * 4 + ["levels"]
    for X, g in zip(datas, got):
        want = pc(X)
        np.testing.assert_array_equal(g.G.graph, want.G.graph)
        assert g.G.get_node_names() == want.G.get_node_names()
        assert g.no_ci_tests == want.no_ci_tests
        rl = want.skeleton.removed_level
        np.testing.assert_array_equal(g.skeleton.removed_level, rl)
        for i, j in zip(*np.nonzero(rl >= 0)):
            if i != j:
                assert g.sepset[i, j] == want.sepset[i, j], (i, j)


def test_pc_pagerank_batch_equals_pc_pagerank(eng):
    from rcaeval_amd.e2e import pc_pagerank, pc_pagerank_batch
    cases = [synth.rq2_case_frame(root_service=svc, fault=fault, rows=600, seed=40 + k)
             for k, (svc, fault) in enumerate((("cartservice", "cpu"), ("adservice", "delay"),
                                               ("emailservice", "mem"), ("cartservice", "delay")))]
    got = pc_pagerank_batch(cases, dataset="online-boutique")
    assert len(got) == 4
    for (df, inject), g in zip(cases, got):
        want = pc_pagerank(df, inject, dataset="online-boutique")
        assert np.asarray(want["adj"]).size > 0          # a real ranking, not the wrapper's dummy
        np.testing.assert_array_equal(np.asarray(g["adj"]), np.asarray(want["adj"]))
        assert g["node_names"] == want["node_names"]
        assert g["ranks"] == want["ranks"]


def test_rq2_run_batch_equals_per_case_loop(eng, tmp_path):
    from rcaeval_amd import rq2
    root = os.path.join(str(tmp_path), "data", "online-boutique")
    paths = synth.write_rq2_dataset(root, services=["cartservice", "adservice", "emailservice"],
                                    faults=("cpu", "delay"), cases=1, rows=1200)
    assert len(paths) == 6
    res = {}
    for batch in (0, 8):
        out_dir = os.path.join(str(tmp_path), f"out{batch}")
        res[batch] = rq2.run(root, "pc_pagerank", "online-boutique", out_dir, batch=batch)
    files = sorted(os.listdir(os.path.join(str(tmp_path), "out0", "results")))
    assert len(files) == 6 and files == sorted(os.listdir(os.path.join(str(tmp_path), "out8", "results")))
    for f in files:
        a = json.load(open(os.path.join(str(tmp_path), "out0", "results", f)))
        b = json.load(open(os.path.join(str(tmp_path), "out8", "results", f)))
        assert a == b and len(a["0"]) > 0, f
    for k in ("cases", "my_cases", "eval_data", "summary"):
        assert res[0][k] == res[8][k], k
    assert len(res[8]["method_s"]) == 6
