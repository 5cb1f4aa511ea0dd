"""The adversarial block fixtures (tests/adversarial_blocks.py) against the C oracle alone: the
conditions that keep tests/test_gpu_adversarial.py from being vacuous. Per family the oracle must
run clean with an empty near-alpha list, bring the designed pairs to their depth, hold depth-d
tests in every decade of |p - alpha| from 1e-8 to 1e-3 and, beyond the conditioning guard, decide
the well-conditioned designed tests as designed; and the numpy model of the fp32 screen
(test_screen32_cpu) must make no wrong decision on the designed depth-4 blocks."""
import numpy as np
import pytest

import adversarial_blocks as ab

NAMES = [f[0] for f in ab.FAMILIES]


@pytest.mark.parametrize("name", NAMES)
def test_family_census(name):
    fam, ref = ab.get_ref(name)
    d = fam.d
    tiny = name == ab.TINY                     # 10 blocks (n <= 64): the counts scale with its size
    assert fam.n <= 640 and (not tiny or fam.n <= 64)
    assert np.array_equal(fam.C, fam.C.T) and np.all(np.diag(fam.C) == 1.0)
    # cross-block correlations are exactly 0
    assert not fam.C[fam.block_of[:, None] != fam.block_of[None, :]].any()
    assert ref.error == 0 and len(ref.near_alpha) == 0
    assert ref.levels == d + 1
    rec = ab.depth_records(ref, d)
    assert len(rec) == ref.tests[d]
    t = fam.targets
    rl = ref.removed_level[t["x"], t["y"]]
    reach = np.isin(rl, (-1, d))
    assert reach.sum() >= (len(t) if tiny else 20), int(reach.sum())
    # x > y and x < y both occur; the designed pair's depth-d test is among the oracle's records
    assert (t["x"] > t["y"]).any() and (t["x"] < t["y"]).any()
    tcode = np.minimum(t["x"], t["y"]).astype(np.int64) * fam.n + np.maximum(t["x"], t["y"])
    sel = np.nonzero(np.isin(rec["a"].astype(np.int64) * fam.n + rec["b"], tcode))[0]
    lut = {(int(rec["a"][i]), int(rec["b"][i]), tuple(sorted(int(v) for v in rec["s"][i, :d]))): i for i in sel}
    tkey = [tuple(sorted((int(q["x"]), int(q["y"])))) + (tuple(sorted(int(v) for v in q["s"][:d])),) for q in t]
    assert all(k in lut for k, r in zip(tkey, reach) if r)
    dec = ab.decade_counts(rec)
    print(f"{name}: n {fam.n} tests {ref.tests} depth-{d} tests per |p - alpha| decade 1e-8..1e-2, rest: {dec}")
    assert min(dec[:5]) >= (1 if tiny else 3), dec
    c = ab.census(fam, rec)
    # the designed value survives the inversion: r^2 / thr^2 - 1 = delta on the well-conditioned targets
    well = np.isnan(t["eps"])
    for k, tt in zip(tkey, t):
        if k in lut and np.isnan(tt["eps"]):
            rel = c["rel"][lut[k]]
            assert abs(rel - tt["delta"]) <= 1e-9 * abs(tt["delta"]) + 1e-11, (rel, tt["delta"])
    n_ill = int((c["gpiv"] < 0.5 * ab.COND_TAU).sum())
    must = ab.must_be_exact(fam, rec)
    print(f"{name}: min pivot^2 of C_SS < tau / 2 at {n_ill} depth-{d} tests, in the band "
          f"{int((np.abs(c['rel']) < ab.BAND).sum())}, must be exact {must}")
    if fam.ill:
        need = 12 if tiny else 30          # tiny: 3 ill-conditioned blocks of 6 such tests each
        assert n_ill >= need, n_ill
        # the order-free bound the GPU tests use counts the same tests here
        assert int((c["gpair"] < 0.5 * ab.COND_TAU).sum()) >= need
        assert np.all(c["gpiv"] <= c["gpair"] + 1e-12)
    # construction against oracle: dependent (edge kept) iff delta > 0
    strong = reach & well & (np.abs(t["delta"]) >= 1e-5)
    assert strong.sum() >= (1 if tiny else 5)
    assert np.array_equal(rl[strong] == -1, t["delta"][strong] > 0)


@pytest.mark.parametrize("name", [f[0] for f in ab.FAMILIES if f[1] == 4])
def test_screen_model_never_wrong_on_designed_blocks(name):
    from test_screen32_cpu import _screen_blocks
    fam = ab.get(name)
    Cb = ab.target_screen_blocks(fam)
    assert Cb.shape == (len(fam.targets) * 8, 6, 6)
    with np.errstate(all="ignore"):
        dep32, ind32, dep64, ind64 = _screen_blocks(Cb, fam.N)
    assert not np.any(dep32 & ~dep64), "fp32 screen model called a designed test dependent that fp64 does not"
    assert not np.any(ind32 & ~ind64), "fp32 screen model called a designed test independent that fp64 does not"
    und = 1.0 - (dep32 | ind32).mean()
    print(f"{name}: the numpy screen model leaves {und:.3f} of the designed depth-4 tests undecided")
    # half of the delta draws lie where the fp32 decision is made, the others (and every
    # ill-conditioned block) must stay undecided
    assert 0.5 <= und < 1.0, und
