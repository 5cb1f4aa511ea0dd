"""GPU: leading dimensions. Every entry whose ABI takes ``ldx`` / ``ldc`` / ``lda`` / ``ldp`` runs on
a row-strided device view (``ld = n + 3``, base pointer 8-byte aligned only) and must give,
bit for bit, what the same call gives on the contiguous copy — the call the rest of the suite holds
to the oracle. Every plan is a function of (n, N) alone, so no tolerance applies.

The view sits in a wider buffer with one poison column on the left and two on the right: NaN around
inputs (a read of the padding reaches the result), a finite sentinel around outputs (a write to the
padding is seen bit for bit). Each test prints the K1 plan or the skeleton driver its shape took.
"""
import numpy as np
import pytest

import granger_ref as gr
from rcaeval_amd import _lib, synth
from test_gpu_skeleton import CASES as SKELETON_CASES

pytestmark = pytest.mark.gpu

LEFT, RIGHT = 1, 2
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def eng():
    from rcaeval_amd.engine import get_engine
    return get_engine(0)


def _embed(eng, a, poison=np.nan):
    """(buffer, view): ``a`` inside a buffer LEFT + RIGHT columns wider, the rest poison."""
    import torch
    a = np.asarray(a, dtype=np.float64)
    r, c = a.shape
    wide = np.full((r, LEFT + c + RIGHT), poison)
    wide[:, LEFT:LEFT + c] = a
    buf = torch.from_numpy(wide).to(eng.device)
    view = buf[:, LEFT:LEFT + c]
    assert view.stride() == (c + LEFT + RIGHT, 1)
    assert view.data_ptr() % 16 == 8
    return buf, view


def _out(eng, n):
    """(buffer, n x n view) for a result, every element the sentinel."""
    return _embed(eng, np.full((n, n), SENTINEL), poison=SENTINEL)


def _assert_padding_intact(buf, n):
    h = buf.cpu().numpy().view(np.uint64)
    want = np.array([SENTINEL]).view(np.uint64)[0]
    assert (h[:, :LEFT] == want).all() and (h[:, LEFT + n:] == want).all(), "a write reached the padding"


def _k1_path(eng, n, N):
    """(path, split-K slabs or None) of K1's plan for (n, N) under the handle's current knobs."""
    sig = eng.k1_plan_signature(n, N)
    if sig >> 62 & 1:
        return "crt", (sig >> 32) & 0xFF
    if sig >> 61 & 1:
        return "digit", (sig >> 32) & 0xFFFF
    assert sig == 2
    return "fp64", None


# (n, N, knobs, path, slabs): slabs "one" / "many" / None (the fp64 plan is not in the signature:
# split_k gives min(4096 / tiles, N / 32) slabs, so N = 40 is the single-slab shape and N = 300
# already splits)
CORR_CASES = [
    (44, 7000, {}, "digit", "many"),
    (200, 33, {}, "digit", "one"),          # one k-block: the Gram accumulates in the caller's C (G = C, ldg = ldc)
    (300, 1200, {}, "crt", None),           # ragged tiles
    (70, 40, {"K1_I8": 0}, "fp64", None),   # k_xtx, one slab: in place in C
    (70, 300, {"K1_I8": 0}, "fp64", None),
    (70, 3000, {"K1_I8": 0}, "fp64", None),
]


@pytest.mark.parametrize("n,N,knobs,path,slabs", CORR_CASES)
def test_corr_strided_in_and_out(eng, n, N, knobs, path, slabs):
    X = synth.gaussian_sem(n, N, seed=n + N, w_low=0.1, w_high=0.5)
    with eng.tuned(**knobs):
        got_path, ks = _k1_path(eng, n, N)
        print(f"corr n={n} N={N} {knobs}: path {got_path}, slabs {ks}, signature {eng.k1_plan_signature(n, N):#x}")
        assert got_path == path
        if slabs == "one":
            assert ks == 1
        if slabs == "many":
            assert ks > 1
        ref = eng.corr(X).cpu().numpy()
        _, xv = _embed(eng, X)
        obuf, ov = _out(eng, n)
        got = eng.corr(xv, out=ov)
        assert got is ov
        np.testing.assert_array_equal(got.cpu().numpy(), ref)
        _assert_padding_intact(obuf, n)


def _rows(out):
    xy, bits = np.asarray(out.sep_xy), np.asarray(out.sep_bits)
    return {(int(x), int(y), tuple(int(b) for b in row)) for (x, y), row in zip(xy, bits)}


def _records(out):
    return {(int(r["a"]), int(r["b"]), tuple(int(v) for v in r["s"][: r["d"]])): float(r["p"]) for r in out.records}


def _same_skeleton(a, b, records=False):
    np.testing.assert_array_equal(a.removed_level, b.removed_level)
    for k in ("driver", "levels", "tests", "calls", "indep", "edges_after", "max_degree", "near_alpha", "error"):
        assert a.stats[k] == b.stats[k], k
    np.testing.assert_array_equal(a.deg_levels, b.deg_levels)
    assert len(a.sep_xy) == len(b.sep_xy) and _rows(a) == _rows(b)
    if records:
        ra, rb = _records(a), _records(b)
        assert len(a.records) == len(b.records) and len(ra) > 0
        assert set(ra) == set(rb)
        np.testing.assert_array_equal([ra[k] for k in sorted(ra)], [rb[k] for k in sorted(ra)])


@pytest.mark.parametrize("flags", [0, _lib.PCG_FLAG_FULL_P | _lib.PCG_FLAG_RECORD])
@pytest.mark.parametrize("case", [3, 6])
def test_skeleton_strided_C(eng, case, flags):
    """n = 50 (the small-graph kernel) and n = 130 (the level loop, 32-bit-offset variant since
    n * ldc < 2^31), to full depth."""
    n, N, seed, wl, wh, ep = SKELETON_CASES[case]
    assert n == (50, 130)[case == 6]
    X = synth.gaussian_sem(n, N, seed=seed, w_low=wl, w_high=wh, edge_prob=ep)
    C = np.corrcoef(X.T)
    ref = eng.skeleton(C, N, flags=flags, record_capacity=2_000_000)
    _, cv = _embed(eng, C)
    got = eng.skeleton(cv, N, flags=flags, record_capacity=2_000_000)
    print(f"skeleton n={n} ldc={cv.stride(0)} flags={flags:#x}: driver {got.stats['driver']}, levels {got.levels}, "
          f"tests {list(got.stats['tests'])[:got.levels]}")
    assert got.stats["driver"] == ("small" if n <= 64 else "levels")
    _same_skeleton(got, ref, records=bool(flags & _lib.PCG_FLAG_RECORD))


def test_corr_skeleton_strided_X_and_out(eng):
    n, N, seed, wl, wh, ep = SKELETON_CASES[6]
    X = synth.gaussian_sem(n, N, seed=seed, w_low=wl, w_high=wh, edge_prob=ep)
    ref, Cref = eng.corr_skeleton(X)
    _, xv = _embed(eng, X)
    obuf, ov = _out(eng, n)
    got, C = eng.corr_skeleton(xv, out=ov)
    print(f"corr_skeleton n={n} N={N}: K1 {_k1_path(eng, n, N)}, driver {got.stats['driver']}, levels {got.levels}")
    assert C is ov
    np.testing.assert_array_equal(C.cpu().numpy(), Cref.cpu().numpy())
    _assert_padding_intact(obuf, n)
    _same_skeleton(got, ref)


BATCH_CASES = [(8, 300, 0, .3, .9, None), (33, 700, 3, .1, .5, .2), (64, 1000, 4, .2, .8, .08)]


def _stacked_views(eng, arrs):
    """The arrays as views into one NaN-filled buffer, one below the other, each LEFT columns in."""
    import torch
    width = LEFT + max(a.shape[1] for a in arrs) + RIGHT
    wide = np.full((sum(a.shape[0] for a in arrs), width), np.nan)
    r0, spans = 0, []
    for a in arrs:
        wide[r0:r0 + a.shape[0], LEFT:LEFT + a.shape[1]] = a
        spans.append((r0, a.shape))
        r0 += a.shape[0]
    buf = torch.from_numpy(wide).to(eng.device)
    views = [buf[r:r + s[0], LEFT:LEFT + s[1]] for r, s in spans]
    assert all(v.stride() == (width, 1) for v in views) and width % 2 == 1
    assert views[0].data_ptr() % 16 == 8
    return buf, views


@pytest.mark.parametrize("from_data", [True, False])
def test_skeleton_batch_views_into_one_buffer(eng, from_data):
    Xs = [synth.gaussian_sem(n, N, seed=seed, w_low=wl, w_high=wh, edge_prob=ep) for n, N, seed, wl, wh, ep in BATCH_CASES]
    Ns = [c[1] for c in BATCH_CASES]
    arrs = Xs if from_data else [np.corrcoef(X.T) for X in Xs]
    packed = eng.skeleton_batch(arrs, None if from_data else Ns, from_data=from_data)
    buf, views = _stacked_views(eng, arrs)
    before = buf.clone()
    outs = eng.skeleton_batch(views, None if from_data else Ns, from_data=from_data)
    assert len(outs) == len(packed) == 3
    for out, ref, (n, *_) in zip(outs, packed, BATCH_CASES):
        assert out.rc == ref.rc == 0 and out.n == n
        _same_skeleton(out, ref)
        Cg, Cr = out.extra["C"], ref.extra["C"]
        assert Cg.shape == (n, n)
        if from_data:
            assert Cg.is_contiguous()                     # the batched K1's output stays packed
        np.testing.assert_array_equal(Cg.cpu().numpy(), Cr.cpu().numpy())
    np.testing.assert_array_equal(buf.cpu().numpy().view(np.uint64), before.cpu().numpy().view(np.uint64))


def test_fisherz_batch_strided_C(eng):
    rng = np.random.default_rng(0)
    n, N = 40, 900
    C = np.corrcoef(synth.gaussian_sem(n, N, seed=50, w_low=0.3, w_high=0.9).T)
    rows = np.full((62, 33), -1, np.int32)
    for r, d in enumerate(list(range(0, 31)) * 2):
        v = rng.choice(n, size=d + 2, replace=False)
        rows[r, :3] = (*sorted(int(t) for t in v[:2]), d)
        rows[r, 3:3 + d] = sorted(int(t) for t in v[2:])
    p, st = eng.fisherz_batch(C, N, rows)
    _, cv = _embed(eng, C)
    pv, stv = eng.fisherz_batch(cv, N, rows)
    assert (st == 0).all()
    np.testing.assert_array_equal(stv, st)
    np.testing.assert_array_equal(pv, p)


@pytest.mark.parametrize("m", [257, 769])
def test_pagerank_dense_strided_A(eng, m):
    """m = 257: the per-node vectors in LDS; m = 769: in the global scratch."""
    rng = np.random.default_rng(m)
    A = (rng.random((m, m)) < 6.0 / m) * rng.random((m, m))
    A[rng.integers(0, m, size=m // 10)] = 0.0
    _, av = _embed(eng, A)
    np.testing.assert_array_equal(eng.pagerank_dense(av), eng.pagerank_dense(A))


@pytest.mark.parametrize("kernel", ["parallel", "serial"])
def test_random_walk_strided_P(eng, kernel):
    rng = np.random.default_rng(9)
    m = 60
    if kernel == "parallel":          # identical columns
        p = rng.random(m)
        P = np.tile((p / p.sum())[:, None], (1, m))
    else:
        P = rng.random((m, m))
        P /= P.sum(0, keepdims=True)
    st = np.random.default_rng(0).bit_generator.state["state"]
    want = eng.random_walk_counts(P, 3, 1500, st["state"], st["inc"])
    _, pv = _embed(eng, P)
    got = eng.random_walk_counts(pv, 3, 1500, st["state"], st["inc"])
    assert want.sum() == 1500
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("T,n,seed", [(300, 17, 32), (2500, 5, 1)])
def test_granger_strided_X(eng, T, n, seed):
    X = gr.GENERATORS["var1"](T, n, seed)
    want = eng.granger(X.copy(), maxlag=3)
    _, xv = _embed(eng, X)
    got = eng.granger(xv, maxlag=3)
    assert set(got) == set(want)
    assert (want["status"][~np.eye(n, dtype=bool)] != 4).all()
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
