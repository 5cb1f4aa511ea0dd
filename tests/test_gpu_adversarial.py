"""GPU: the depth 2-4 T-group sweeps (k_level_lds_f, k_level_lds_t), their screens (k_screen,
k_screen_exact) and exact paths (k_exact, k_exact_lanes) on the adversarial block fixtures of
tests/adversarial_blocks.py: near-threshold tests in every decade of |p - alpha| from 1e-8 up and
conditioning sets whose C_SS has a pivot^2 of 1e-10..1e-5, at depths 2, 3 and 4, through every
kernel route those depths have. Every case compares the engine's skeleton on the constructed C
with the C oracle's (removal depth of every pair, per-level unique-test counts, sepset unions)
and checks from the oracle and C alone that the tests no fast path may decide did reach the
screen and the exact path.

Measured on an MI355X (defaults, depth d): the exact path takes exactly the must-be-exact tests
(d4_x0 363 of 720, d4_x2 3042 of 10592, d4_x7 58482 of 443552, d3_x3 2578 of 11552), the screen
list 7 to 21 more, and the fp32 sweep's screened share equals the numpy model's undecided share
to four digits; recorded p of the ill-conditioned tests stays within fisherz.p_close of the
oracle's. The table is in DESIGN.md section 4.1, "Adversarial block fixtures".
"""
import contextlib
from types import SimpleNamespace

import numpy as np
import pytest

import adversarial_blocks as ab
from oracle import fisherz
from rcaeval_amd import _lib
from tests_support import assert_skeleton_matches

pytestmark = pytest.mark.gpu

ALL = [f[0] for f in ab.FAMILIES if f[0] != ab.TINY]
DEEP = [f[0] for f in ab.FAMILIES if f[0] != ab.TINY and f[1] >= 3]
DEFAULT_MASK = 0x18                   # PCG_TG_F32: depths 3 and 4 are fp32-screened by default
REC = _lib.PCG_FLAG_RECORD
FULLP_REC = _lib.PCG_FLAG_FULL_P | _lib.PCG_FLAG_RECORD


@pytest.fixture(scope="module")
def eng():
    from rcaeval_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(scope="module")
def fixtures():
    """name -> (family, oracle run with records, depth-d records, must-be-exact count, the numpy
    screen model's undecided share), built on first use and shared by every case."""
    cache = {}

    def get(name):
        if name not in cache:
            fam, ref = ab.get_ref(name)
            rec = ab.depth_records(ref, fam.d)
            mm = ab.must_mask(fam, rec)
            cache[name] = SimpleNamespace(fam=fam, ref=ref, rec=rec, must_mask=mm, must=int(mm.sum()),
                                          must_guard=int(ab.must_mask(fam, rec, band=False).sum()),
                                          model=ab.model_undecided_share(fam, rec))
        return cache[name]
    return get


def _well_conditioned_near(fx, near):
    """Engine near-alpha records whose pair lies in a well-conditioned block."""
    ill_block = ~np.isnan(fx.fam.targets["eps"])
    return [(int(r["a"]), int(r["b"])) for r in near if not ill_block[fx.fam.block_of[int(r["a"])]]]


def _check(out, fx, mask, route, must_screened=None, must_exact=None):
    """The skeleton is the oracle's, and the tests that no fp32 or Cholesky decision may take
    (fx.must: r^2 inside decide()'s band, or a pivot^2 of C_SS below tau / 2 in any elimination
    order; from the oracle's records and C) went to the screen list and to the exact path.
    ``mask``: the fp32-screened depths; ``must_screened``: the screen list's bound when it is not
    fx.must (a recorded pair's tests go to the exact path without passing the screen);
    ``must_exact``: the exact path's bound when it is not fx.must."""
    fam, ref = fx.fam, fx.ref
    must_screened = fx.must if must_screened is None else must_screened
    must_exact = fx.must if must_exact is None else must_exact
    d = fam.d
    st = out.stats
    print(f"{fam.name} [{route}]: depth {d} tests {st['tests'][d]} screened {st['screened'][d]} "
          f"({st['screened'][d] / st['tests'][d]:.4f}; numpy model undecided {fx.model:.4f}) "
          f"exact {st['exact'][d]} must-be-exact {fx.must} near-alpha {len(out.near_alpha)}")
    assert st["driver"] == "levels"
    assert_skeleton_matches(out, ref, fam.n)
    assert st["exact"][d] >= must_exact, (st["exact"], must_exact)
    if (mask >> d) & 1:
        assert st["screened"][d] >= must_screened, (st["screened"], must_screened)
    else:
        assert st["screened"][d] == 0
    assert all(s <= t for s, t in zip(st["screened"], st["tests"]))
    assert not _well_conditioned_near(fx, out.near_alpha)


def _canonical(rec):
    """Records as sorted rows (a, b, d, s_0..s_3 with -1 beyond d) and their p in that order."""
    s = np.where(np.arange(4)[None, :] < rec["d"][:, None], rec["s"][:, :4], -1)
    rows = np.column_stack([rec["a"], rec["b"], rec["d"], s]).astype(np.int64)
    order = np.lexsort(rows.T[::-1])
    return rows[order], rec["p"][order]


def _check_records(out, ref_records, count):
    """The engine's records are the oracle's ``count`` unique tests, each with the oracle's p
    (fisherz.p_close)."""
    kg, pg = _canonical(out.records)
    kd, pd = _canonical(ref_records)
    assert len(kd) == count and not (np.diff(kd, axis=0) == 0).all(axis=1).any()
    assert kg.shape == kd.shape and np.array_equal(kg, kd)
    ok = fisherz.p_close(pg, pd)
    assert ok.all(), [(kd[i].tolist(), pg[i], pd[i]) for i in np.nonzero(~ok)[0][:5]]


@pytest.mark.parametrize("name", ALL)
def test_defaults(eng, fixtures, name):
    """k_level_lds_f<3,4> narrow (node images at depth 4), k_level_lds_t<2>, k_screen_exact."""
    fx = fixtures(name)
    out = eng.skeleton(fx.fam.C, fx.fam.N, max_depth=fx.fam.d)
    _check(out, fx, DEFAULT_MASK, "defaults")


@pytest.mark.parametrize("mask", [0x1c, 0])
@pytest.mark.parametrize("name", ALL)
def test_screen_masks(eng, fixtures, name, mask):
    """Depth 2 screened too (k_level_lds_f<2>), and nothing screened: k_level_lds_t<2,3,4> with
    k_exact."""
    fx = fixtures(name)
    with eng.tuned(SCREEN_MASK=mask):
        out = eng.skeleton(fx.fam.C, fx.fam.N, max_depth=fx.fam.d)
    _check(out, fx, mask, f"mask {mask:#x}")
    if mask == 0:
        assert sum(out.stats["screened"]) == 0


@pytest.mark.parametrize("blocks", [0, 0x18])
@pytest.mark.parametrize("name", DEEP)
def test_node_blocks(eng, fixtures, name, blocks):
    """The fp32 sweep gathering from C (0) and from node images at depths 3 and 4 (0x18)."""
    fx = fixtures(name)
    with eng.tuned(NODE_BLOCKS=blocks):
        out = eng.skeleton(fx.fam.C, fx.fam.N, max_depth=fx.fam.d)
    _check(out, fx, DEFAULT_MASK, f"node blocks {blocks:#x}")


@pytest.mark.parametrize("mask", [None, 0])
@pytest.mark.parametrize("name", ALL)
def test_wide_class(eng, fixtures, name, mask):
    """A narrow degree of d puts every node with depth-d tests (degree >= d + 1) in the wide
    class: k_level_lds_f<., true> (default mask) and k_level_lds_t<., true> (mask 0)."""
    fx = fixtures(name)
    assert fx.ref.deg_at_level[fx.fam.d].max() > fx.fam.d
    _lib.check(eng.h, eng.lib.pcg_set_narrow_degree(eng.h, fx.fam.d), "pcg_set_narrow_degree")
    try:
        with (eng.tuned(SCREEN_MASK=mask) if mask is not None else contextlib.nullcontext()):
            out = eng.skeleton(fx.fam.C, fx.fam.N, max_depth=fx.fam.d)
    finally:
        eng.lib.pcg_set_narrow_degree(eng.h, 64)
    _check(out, fx, DEFAULT_MASK if mask is None else mask, f"wide, mask {mask}")


@pytest.mark.parametrize("flags", [REC, FULLP_REC])
@pytest.mark.parametrize("name", ALL)
def test_records(eng, fixtures, name, flags):
    """Every pair recorded: the REC instantiations of the sweeps hand every test to k_exact_lanes
    (none passes the screen), in threshold-with-records and full-p mode: the oracle's skeleton,
    and every oracle record with the oracle's p. (A RECORD run computes p: its paths have
    decide()'s guard but no band.)"""
    fx = fixtures(name)
    d = fx.fam.d
    out = eng.skeleton(fx.fam.C, fx.fam.N, max_depth=d, flags=flags, record_capacity=ab.RECORD_CAP)
    _check(out, fx, DEFAULT_MASK, f"flags {flags:#x}", must_screened=0, must_exact=fx.must_guard)
    _check_records(out, fx.ref.records, sum(fx.ref.tests))


@pytest.mark.parametrize("name", ALL)
def test_records_sampled(eng, fixtures, name):
    """One pair in three recorded (record_sample): the REC instantiations decide the other pairs'
    tests in fp32 and send their undecided ones through k_screen, next to the recorded pairs'
    tests on k_exact_lanes. The records are the oracle's of those pairs, with the oracle's p."""
    fx = fixtures(name)
    fam, d = fx.fam, fx.fam.d
    mod, res = 3, 1

    def sampled(rec):
        return (rec["a"].astype(np.int64) * fam.n + rec["b"]) % mod == res
    out = eng.skeleton(fam.C, fam.N, max_depth=d, flags=REC, record_capacity=ab.RECORD_CAP, record_sample=(mod, res))
    keep = sampled(fx.ref.records)
    assert 0.2 * len(keep) < keep.sum() < 0.5 * len(keep)
    # (a RECORD run computes p: its fast paths have the guard but no band; a recorded pair's
    # tests need not pass the screen)
    guard = ab.must_mask(fam, fx.rec, band=False)
    _check(out, fx, DEFAULT_MASK, "records 1 in 3", must_screened=int((guard & ~sampled(fx.rec)).sum()),
           must_exact=fx.must_guard)
    _check_records(out, fx.ref.records[keep], int(keep.sum()))


@pytest.mark.parametrize("flags", [0, FULLP_REC])
@pytest.mark.parametrize("small", [1, 0])
def test_tiny_family_both_drivers(eng, fixtures, small, flags):
    """n = 60: k_pc_small (SMALL = 1) and the level loop (SMALL = 0) on the same blocks."""
    fx = fixtures(ab.TINY)
    fam, ref = fx.fam, fx.ref
    with eng.tuned(SMALL=small):
        out = eng.skeleton(fam.C, fam.N, max_depth=fam.d, flags=flags, record_capacity=ab.RECORD_CAP)
    assert out.stats["driver"] == ("small" if small else "levels")
    print(f"{fam.name} [SMALL={small} flags {flags:#x}]: exact {out.stats['exact']} screened "
          f"{out.stats['screened']} must-be-exact {fx.must}")
    assert_skeleton_matches(out, ref, fam.n)
    # (full-p mode has no band: k_pc_small computes a band test's p on its fast path)
    assert out.stats["exact"][fam.d] >= (fx.must_guard if flags & _lib.PCG_FLAG_FULL_P else fx.must)
    assert not _well_conditioned_near(fx, out.near_alpha)
    if not small and not flags:      # (every pair recorded: nothing passes the screen)
        assert out.stats["screened"][fam.d] >= fx.must
    if flags & REC:
        _check_records(out, ref.records, sum(ref.tests))


@pytest.mark.parametrize("name", ["d4_x2", "d3_x3"])
def test_screen_list_overflow_reruns(eng, fixtures, name):
    """A screen list of 16 entries overflows on the ill-conditioned tests, the level reports it
    with the capacity raised, and pcg_skeleton reruns: the result equals the oracle's and a run
    with room to spare."""
    fx = fixtures(name)
    fam = fx.fam
    a = eng.skeleton(fam.C, fam.N, max_depth=fam.d)
    assert fx.must > 16 and a.stats["screened"][fam.d] >= fx.must
    _lib.check(eng.h, eng.lib.pcg_set_screen_capacity(eng.h, 16), "pcg_set_screen_capacity")
    try:
        b = eng.skeleton(fam.C, fam.N, max_depth=fam.d)
    finally:
        eng.lib.pcg_set_screen_capacity(eng.h, 1 << 20)
    _check(b, fx, DEFAULT_MASK, "screen capacity 16")
    for k in ("screened", "exact", "tests", "indep"):
        assert b.stats[k] == a.stats[k], k
    assert np.array_equal(b.removed_level, a.removed_level)


@pytest.mark.timeout(300)
def test_sharded_world3(fixtures):
    """The per-rank chunk cut through these kernels (pcg_skeleton_sharded at world 3, in-process
    transport): every rank returns the oracle's skeleton, the summed counters reach the bounds."""
    from rcaeval_amd.dist import run_local_ranks
    fx = fixtures("d4_x2")
    fam = fx.fam

    def fn(eng, rank, world):
        out = eng.skeleton_sharded(fam.C, fam.N, max_depth=fam.d)
        return SimpleNamespace(removed_level=out.removed_level.copy(), sep_xy=out.sep_xy.copy(),
                               sep_bits=out.sep_bits.copy(), stats=out.stats, near_alpha=list(out.near_alpha))
    res, gst = run_local_ranks(3, fn, timeout_s=120)
    assert not gst["broken"]
    for r in res:
        _check(r, fx, DEFAULT_MASK, "world 3")


def test_near_alpha_exemptions_rare(eng, fixtures):
    """Over all families at most 1 % of the designed pairs may be exempt from the comparison
    through a near-alpha record (the oracle's lists are empty: the CPU census asserts it)."""
    exempt = total = 0
    for name in ALL + [ab.TINY]:
        fx = fixtures(name)
        fam = fx.fam
        with eng.tuned(SMALL=0):
            out = eng.skeleton(fam.C, fam.N, max_depth=fam.d)
        near = {(int(r["a"]), int(r["b"])) for r in out.near_alpha}
        tp = {tuple(sorted((int(t["x"]), int(t["y"])))) for t in fam.targets}
        exempt += len(near & tp)
        total += len(tp)
    print(f"designed pairs exempt through near-alpha: {exempt} of {total}")
    assert exempt <= total // 100
