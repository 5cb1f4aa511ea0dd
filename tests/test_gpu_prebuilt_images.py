"""GPU: node images built behind the level summary (k_summary_fill's image-offset scan, the builder
k_node_blocks_t<true> enqueued before the host has seen the summary) and depths 2-4 staged from them.

Inputs: independent "hub" variables, each the common cause of its own group of children, plus
pure-noise variables. After depth 1 a child keeps its hub (and a few chance edges), a hub keeps its
children, so at the start of depths 2, 3 and 4 the degree sequence holds nodes with no work (below
d + 1), hubs across 5..64 (the narrow class, which gets images) and, in the depth-bounded input, a
hub above 64 (the wide class: no image, the builder must skip it). Every precondition is asserted
on the oracle's degree sequence before the engine's results are relied on.

A hub above 64 neighbours never loses them, so a run that holds one cannot end before depth 65
(C(66, 33) conditioning sets): the unlimited-depth runs use the same generator with hubs of at most
12 children, and route the hubs above 8 neighbours to the wide / large classes with
pcg_set_narrow_degree instead, so the builder's upper degree bound is exercised there too.

The depth-bounded input's oracle run is the module's one slow step (a hub above 64 neighbours alone
is 4e7 depth-4 tests on the CPU: 3-14 s); it is computed once and shared, each engine run takes
about 0.1 s.

Compared: removal depth of every pair, per-level unique-test counts and every sepset union, against
the C oracle and against the engine with node blocks off (tests_support.assert_skeleton_matches).
"""
import numpy as np
import pytest

from oracle import cpc
from tests_support import assert_skeleton_matches, unions_from_engine

pytestmark = pytest.mark.gpu

# (NODE_BLOCKS, SCREEN_MASK or None = the default): off; depth 4; depths 3-4; depths 2-4 with depth 2 screened
MASKS = [(0, None), (0x10, None), (0x18, None), (0x1c, 0x1c)]


@pytest.fixture(scope="module")
def eng():
    from rcaeval_amd.engine import get_engine
    return get_engine(0)


def hub_data(groups, noise, N, seed, a_lo=0.7, a_hi=0.9):
    """N x n samples: per group size m a hub z ~ N(0, 1) and m children a z + e; then `noise`
    independent columns. Columns are shuffled so that node ids carry no structure."""
    rng = np.random.default_rng(seed)
    cols = []
    for m in groups:
        z = rng.standard_normal(N)
        cols.append(z)
        a = rng.uniform(a_lo, a_hi, m) * rng.choice([-1.0, 1.0], m)
        cols.extend((z[:, None] * a + rng.standard_normal((N, m))).T)
    cols.extend(rng.standard_normal((noise, N)))
    X = np.column_stack(cols)
    return np.ascontiguousarray(X[:, rng.permutation(X.shape[1])])


def diamond_data(k, copies, noise, N, seed):
    """`copies` motifs x -> a_1..a_k -> y plus one more child e of x: x and y are dependent given
    any k - 1 of the a's and independent given all k, so the edge x - y falls at depth k exactly.
    x enters depth k with k + 2 neighbours (the a's, e, y) and leaves it with k + 1: depth k + 1
    has no node with work although depth k started with degrees above k + 1."""
    rng = np.random.default_rng(seed)
    cols = []
    for _ in range(copies):
        x = rng.standard_normal(N)
        a = [0.9 * x + 0.6 * rng.standard_normal(N) for _ in range(k)]
        y = sum(a) * (0.9 / np.sqrt(k)) + 0.6 * rng.standard_normal(N)
        e = 0.9 * x + 0.6 * rng.standard_normal(N)
        cols += [x, *a, y, e]
    cols.extend(rng.standard_normal((noise, N)))
    X = np.column_stack(cols)
    return np.ascontiguousarray(X[:, rng.permutation(X.shape[1])])


def image_doubles(deg, d, hi=64):
    """The image bytes / 8 of the narrow nodes with work at depth d (the layout of
    tgf_image_bytes: D rows of DS floats, 20 bytes per padded column, rounded to 1 KB)."""
    tot = 0
    for D in deg:
        D = int(D)
        if d + 1 <= D <= hi:
            DS = (D + 3) & ~3
            tot += ((4 * D * DS + 20 * DS + 1023) & ~1023) // 8
    return tot


class Case:
    def __init__(self, X, max_depth):
        self.N, self.n = X.shape
        self.C = np.corrcoef(X.T)
        self.max_depth = max_depth
        self.ref = cpc.skeleton(self.C, self.N, max_depth=max_depth)
        self.base = None   # the engine's result with node blocks off (filled by the first test that runs it)


# the depth-bounded input: hubs across the narrow class, one in the wide class, noise columns
@pytest.fixture(scope="module")
def bounded():
    c = Case(hub_data([6, 9, 13, 21, 33, 48, 57, 66], noise=8, N=1000, seed=5), max_depth=4)
    assert c.ref.levels == 5
    for d in (2, 3, 4):
        deg = c.ref.deg_at_level[d]
        assert (deg < d + 1).any() and (deg > 64).any(), (d, np.sort(deg)[-10:])
        assert ((deg >= 5) & (deg <= 16)).any() and ((deg >= 17) & (deg <= 40)).any() and ((deg >= 41) & (deg <= 64)).any()
    return c


# the unlimited-depth input: the same generator, small hubs, fewer samples, isolated nodes after depth 1
@pytest.fixture(scope="module")
def unlimited():
    c = Case(hub_data([5, 6, 7, 8, 9, 10, 11, 12] * 2, noise=20, N=400, seed=9), max_depth=-1)
    assert c.ref.levels >= 6
    for d in (2, 3, 4):
        deg = c.ref.deg_at_level[d]
        assert (deg == 0).any() and (deg < d + 1).any() and ((deg >= 5) & (deg <= 8)).any() and (deg > 8).any()
    return c


def _run(eng, c, blocks, mask, C=None, narrow=64):
    from rcaeval_amd import _lib
    knobs = {"SMALL": 0, "NODE_BLOCKS": blocks}
    if mask is not None:
        knobs["SCREEN_MASK"] = mask
    _lib.check(eng.h, eng.lib.pcg_set_narrow_degree(eng.h, narrow), "pcg_set_narrow_degree")
    try:
        with eng.tuned(**knobs):
            out = eng.skeleton(c.C if C is None else C, c.N, max_depth=c.max_depth)
            totals = {d: eng.image_totals(d) for d in (2, 3, 4)}
    finally:
        eng.lib.pcg_set_narrow_degree(eng.h, 64)
    return out, totals


def _same_as_base(eng, c, out, narrow=64):
    if c.base is None or c.base[0] != narrow:
        c.base = (narrow, _run(eng, c, 0, None, narrow=narrow)[0])
    base = c.base[1]
    assert np.array_equal(np.asarray(out.removed_level), np.asarray(base.removed_level))
    assert list(out.stats["tests"]) == list(base.stats["tests"])
    assert unions_from_engine(out) == unions_from_engine(base)


def _check_totals(c, totals, blocks, mask, hi=64):
    """Test 3: where a depth's images were built behind the previous summary, the device's scan
    and the host's decomposition agree, and both are what the oracle's degrees give."""
    eff = 0x18 if mask is None else mask   # (the built-in fp32-screened depths: skeleton.hip PCG_TG_F32)
    for d in (2, 3, 4):
        imaged = (blocks >> d) & 1 and (eff >> d) & 1 and d < c.ref.levels
        if imaged:
            want = image_doubles(c.ref.deg_at_level[d], d, hi)
            assert totals[d] == (want, want), (d, totals[d], want)
        else:
            assert totals[d] == (-1, -1), (d, totals[d])


@pytest.mark.parametrize("blocks,mask", MASKS)
def test_bounded_depth_matches_oracle_and_unstaged_engine(eng, bounded, blocks, mask):
    out, totals = _run(eng, bounded, blocks, mask)
    assert out.stats["driver"] == "levels" and out.levels == 5
    assert_skeleton_matches(out, bounded.ref, bounded.n)
    _same_as_base(eng, bounded, out)
    _check_totals(bounded, totals, blocks, mask)


@pytest.mark.parametrize("narrow", [64, 8])
@pytest.mark.parametrize("blocks,mask", MASKS)
def test_unlimited_depth_matches_oracle_and_unstaged_engine(eng, unlimited, blocks, mask, narrow):
    out, totals = _run(eng, unlimited, blocks, mask, narrow=narrow)
    assert out.levels == unlimited.ref.levels
    assert_skeleton_matches(out, unlimited.ref, unlimited.n)
    _same_as_base(eng, unlimited, out, narrow=narrow)
    _check_totals(unlimited, totals, blocks, mask, hi=narrow)


def test_leading_dimension(eng, bounded):
    """ldc > n: C as a row-strided device view inside a NaN-poisoned buffer (the builder reads whole
    rows of C: a read past column n would reach the images)."""
    import torch
    n = bounded.n
    wide = np.full((n, n + 5), np.nan)
    wide[:, 2:2 + n] = bounded.C
    view = torch.from_numpy(wide).to(eng.device)[:, 2:2 + n]
    assert view.stride() == (n + 5, 1)
    out, totals = _run(eng, bounded, 0x1c, 0x1c, C=view)
    assert_skeleton_matches(out, bounded.ref, n)
    _same_as_base(eng, bounded, out)
    _check_totals(bounded, totals, 0x1c, 0x1c)


@pytest.mark.parametrize("k,max_depth", [(2, 4), (3, -1)])
def test_run_ends_before_the_prebuilt_depth(eng, bounded, k, max_depth):
    """The last depth with work is k, the depth bound lies above it: depth k starts with degrees of
    k + 2 (so the builder for depth k + 1 is enqueued behind its summary) and ends with none above
    k + 1 (depth k + 1 never begins). The call returns the oracle's result; a second skeleton on the
    same handle, with a larger n, regrows the buffers and matches its oracle too."""
    X = diamond_data(k, copies=24, noise=16, N=1000, seed=20 + k)
    n = X.shape[1]
    assert n < bounded.n
    C = np.corrcoef(X.T)
    # (alpha = 0.001: at 0.05 one x - y edge in twenty survives depth k by chance and depth k + 1 runs)
    ref = cpc.skeleton(C, 1000, alpha=0.001, max_depth=max_depth)
    assert ref.levels == k + 1, ref.levels
    assert ref.deg_at_level[k].max() >= k + 2 and ref.deg_at_level[k].max() <= 64
    with eng.tuned(SMALL=0, NODE_BLOCKS=0x1c, SCREEN_MASK=0x1c):
        out = eng.skeleton(C, 1000, alpha=0.001, max_depth=max_depth)
        assert out.levels == k + 1
        assert_skeleton_matches(out, ref, n)
        assert eng.image_totals(k + 1) == (-1, -1)
        out2, totals = _run(eng, bounded, 0x1c, 0x1c)
    assert_skeleton_matches(out2, bounded.ref, bounded.n)
    _check_totals(bounded, totals, 0x1c, 0x1c)
