"""GPU: the CRT K1's two-class split-K plan (PCG_TUNE_K1_CRT_MIX). Tiles [0, tA) run as ksA slabs,
the rest as ksB; every plan gives the correctly rounded exact Gram, so pcg_corr under any forced
mixed plan is bitwise the uniform plan's result (knob 0) and stays within the K1 tolerance of
np.corrcoef.

The classes are two contiguous runs of the row-major upper-triangle tile order, so a non-empty
class A always holds tile 0 = (0, 0) and a non-empty class B the last tile (T - 1, T - 1): a split
class made of off-diagonal tiles only cannot be formed. The cases below cover a split class that is
one diagonal tile, and split classes that hold every off-diagonal tile (with the unsplit class one
diagonal tile), in both orders of the slab counts.
"""
import numpy as np
import pytest

from rcaeval_amd import _lib, synth
from tests_support import unions_from_engine

pytestmark = pytest.mark.gpu

ATOL = 2e-14            # the existing K1 tolerance against np.corrcoef
KS_PAIRS = [(1, 4), (2, 3), (1, 7), (4, 1)]


@pytest.fixture(scope="module")
def eng():
    from rcaeval_amd.engine import get_engine
    return get_engine(0)


def nearest_slabs(N, want):
    """the slab count the plan's k-block rounding reaches for a forced count (corr.hip crt_slabs)"""
    TB = (N + 63) // 64 * 2
    reach = []
    for ks in range(1, 17):
        kb = (TB + ks - 1) // ks
        kb = (kb + 3) // 4 * 4
        if (TB + kb - 1) // kb == ks:
            reach.append(ks)
    return min(reach, key=lambda r: (abs(r - want), r))


def check_forced_plans(eng, X, ref, finite=None):
    n, N = X.shape[1], X.shape[0]
    T = -(-n // 256)
    ntiles = T * (T + 1) // 2
    Xd = eng.to_device(X)
    with eng.tuned(K1_CRT_MIX=0):
        C0 = eng.corr(Xd).cpu().numpy()
        p0 = eng.k1_crt_plan(n, N)
    assert p0["tiles"] == ntiles and p0["tA"] == ntiles          # knob 0: one split for every tile
    ok = ~np.isnan(ref) if finite is None else finite
    np.testing.assert_array_equal(np.isnan(C0), np.isnan(ref))
    err0 = np.abs(C0[ok] - ref[ok]).max()
    print(f"n={n} N={N}: uniform ks={p0['ksA']} max|C - corrcoef| = {err0:.3g}")
    assert err0 <= ATOL
    mixed_seen = 0
    for tA in (ntiles, 0, 1, ntiles - 1):          # all A, all B, one tile in A, one tile in B
        for ksA, ksB in KS_PAIRS:
            with eng.tuned(K1_CRT_MIX=_lib.k1_crt_mix_force(tA, ksA, ksB)):
                p = eng.k1_crt_plan(n, N)
                C = eng.corr(Xd).cpu().numpy()
            ea, eb = nearest_slabs(N, ksA), nearest_slabs(N, ksB)
            if tA == 0:
                want = (ntiles, eb, eb)
            elif tA == ntiles:
                want = (ntiles, ea, ea)
            else:
                want = (tA, ea, eb)
            assert (p["tA"], p["ksA"], p["ksB"]) == want, (tA, ksA, ksB, p)
            assert p["units"] == p["moduli"] * (p["tA"] * p["ksA"] + (ntiles - p["tA"]) * p["ksB"])
            mixed_seen += p["tA"] < ntiles and p["ksA"] != p["ksB"]
            np.testing.assert_array_equal(C, C0, err_msg=f"plan {p}")      # (NaNs in the same places)
    assert mixed_seen >= 4          # every shape here reaches at least two slab counts


@pytest.mark.parametrize("N", [130, 1000, 2049])
@pytest.mark.parametrize("n", [300, 600])
def test_forced_mixed_plans_bitwise_equal_uniform(eng, n, N):
    """n = 300 (T = 2, 3 tiles), n = 600 (T = 3, 6 tiles); N = 130 (6 k-blocks: a slab of exactly
    CRT_KB = 4 and a shorter last one), 1000 (32 k-blocks), 2049 (odd, 66 k-blocks: a short last
    slab under every split)."""
    X = synth.gaussian_sem(n, N, seed=3 * n + N, w_low=0.1, w_high=0.5)
    check_forced_plans(eng, X, np.corrcoef(X.T))


def test_forced_mixed_plans_hard_columns(eng):
    """A constant column (numpy's 0/0 NaN), a NaN column and a single-spike column, in the first
    and the last tile row."""
    n, N = 300, 1000
    X = synth.gaussian_sem(n, N, seed=17, w_low=0.2, w_high=0.8)
    X[:, 3] = 2.5
    X[:, 290] = 0.0
    X[17, 4] = np.nan
    X[5, 270] = np.inf
    X[:, 9] = 0.0
    X[123, 9] = 1.0
    X[7, 280] += 100 * X[:, 280].std()
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = np.corrcoef(X.T)
    check_forced_plans(eng, X, ref)


def test_automatic_plan_equals_uniform(eng):
    n, N = 600, 1000
    X = eng.to_device(synth.gaussian_sem(n, N, seed=2, w_low=0.1, w_high=0.5))
    assert eng.get_tuning("K1_CRT_MIX") == 1           # the default: the cost model
    p = eng.k1_crt_plan(n, N)
    print("automatic plan", p)
    assert p["tiles"] == 6 and 1 <= p["tA"] <= 6 and p["ksA"] <= p["ksB"]
    C1 = eng.corr(X).cpu().numpy()
    with eng.tuned(K1_CRT_MIX=0):
        C0 = eng.corr(X).cpu().numpy()
    np.testing.assert_array_equal(C1, C0)
    with eng.tuned(K1_CRT_KS=3):                       # a forced uniform count wins over the mixed knob
        p3 = eng.k1_crt_plan(n, N)
        assert (p3["tA"], p3["ksA"], p3["ksB"]) == (6, 3, 3)
        np.testing.assert_array_equal(eng.corr(X).cpu().numpy(), C0)


def test_corr_skeleton_equals_corr_then_skeleton(eng):
    """The fused call (K1 under the automatic plan, then the skeleton on the same stream) against
    the two calls, twice in a row on one handle."""
    n, N = 300, 1000
    X = synth.gaussian_sem(n, N, seed=9, w_low=0.2, w_high=0.8, edge_prob=0.03)
    Xd = eng.to_device(X)
    C = eng.corr(Xd)
    ref = eng.skeleton(C, N, max_depth=2)
    ref_unions = unions_from_engine(ref)
    for _ in range(2):
        out, C2 = eng.corr_skeleton(Xd, max_depth=2)
        np.testing.assert_array_equal(C2.cpu().numpy(), C.cpu().numpy())
        np.testing.assert_array_equal(out.removed_level, ref.removed_level)
        assert unions_from_engine(out) == ref_unions
        assert list(out.stats["tests"]) == list(ref.stats["tests"])
        assert out.levels == ref.levels
