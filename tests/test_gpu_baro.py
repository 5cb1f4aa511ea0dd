"""GPU: pcg_scaler_batch / pcg_scaler_case and baro / robust_scaler / nsigma against the numpy
restatement of the scalers' arithmetic (tests/baro_ref.py, pinned to scikit-learn bit for bit by
tests/test_baro_cpu.py).

The arithmetic is exact, so every comparison is equality (``assert_array_equal``: -0.0 equals 0.0,
NaN equals NaN): there is no tolerance anywhere in this file.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import baro_ref as br

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scaler.npz")
MODES = ("robust", "standard")
SMALL_N = (1, 2, 3, 4, 5, 8, 63, 64, 65, 255, 256, 257)


def _eng():
    from rcaeval_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(scope="module", autouse=True)
def _engine_first():
    """The engine (and with it torch's HIP runtime) is created before anything else loads the library."""
    _eng()


@functools.lru_cache(maxsize=None)
def _lds_rows():
    return _eng().scaler_limits()["lds_rows"]


@functools.lru_cache(maxsize=None)
def _case(N, M, n):
    """The (A, B) of a shape, its column kinds rotated by the shape so that n = 1 and n = 3 meet
    every kind over the N and M of the test; built once and shared."""
    s = (N + M) % len(br.KINDS)
    A, B = br.gen_case(N, M, n, seed=N * 131 + M, kinds=br.KINDS[s:] + br.KINDS[:s])
    return A, B


@functools.lru_cache(maxsize=None)
def _ref(N, M, n, mode):
    A, B = _case(N, M, n)
    return br.scores(A, B, mode)


def _check(got, ref, what):
    for key in ("center", "scale", "score"):
        assert_array_equal(got[key], ref[key], err_msg=f"{what}: {key}")
    assert_array_equal(got["status"], ref["status"], err_msg=f"{what}: status")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N", SMALL_N)
def test_bit_equality_small(N, mode):
    shapes = [(N, M, n) for M in (1, 65) for n in (1, 3, 65)]
    got = _eng().scaler_scores([_case(*s) for s in shapes], mode)
    for s, g in zip(shapes, got):
        ref = _ref(*s, mode)
        assert not ref["status"].any()
        _check(g, ref, f"N={s[0]} M={s[1]} n={s[2]} {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("over", [0, 1])
def test_bit_equality_at_the_lds_limit(over, mode):
    """N = lds_rows takes the in-LDS sort, N = lds_rows + 1 the radix select over global memory."""
    N = _lds_rows() + over
    for M in (1, 65):
        got = _eng().scaler_scores([_case(N, M, 3)], mode)[0]
        _check(got, _ref(N, M, 3, mode), f"N={N} M={M} n=3 {mode}")
        assert not got["status"].any()


@pytest.mark.parametrize("mode", MODES)
def test_radix_select_on_a_wide_tile(mode):
    """The global path with more than one tile and a ragged last one (n = 19), every column kind."""
    N = _lds_rows() + 37
    got = _eng().scaler_scores([_case(N, 17, 19)], mode)[0]
    _check(got, _ref(N, 17, 19, mode), f"N={N} n=19 {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_standard_sum_order_beyond_one_numpy_buffer(mode):
    """numpy sums in blocks of 8192 elements: N = 8192 + 130 has a second block with a tree of its own."""
    N = 8192 + 130
    got = _eng().scaler_scores([_case(N, 2, 3)], mode)[0]
    _check(got, _ref(N, 2, 3, mode), f"N={N} {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_row_strides(mode):
    import torch
    eng = _eng()
    for N in (65, _lds_rows() + 1):
        A, B = _case(N, 17, 11)
        wa = torch.full((N, 11 + 5), 7.5, dtype=torch.float64, device=eng.device)
        wb = torch.full((17, 11 + 2), -3.0, dtype=torch.float64, device=eng.device)
        wa[:, 2:13] = torch.from_numpy(A.copy()).to(eng.device)
        wb[:, 1:12] = torch.from_numpy(B.copy()).to(eng.device)
        va, vb = wa[:, 2:13], wb[:, 1:12]
        assert va.stride(0) == 16 and vb.stride(0) == 13
        _check(eng.scaler_scores([(va, vb)], mode)[0], _ref(N, 17, 11, mode), f"strided N={N} {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_batch_equals_loop(mode):
    eng = _eng()
    shapes = [(5, 1, 1), (257, 17, 65), (_lds_rows() + 1, 2, 3)]
    cases = [_case(*s) for s in shapes]
    many = eng.scaler_scores(cases, mode)
    for s, c, m in zip(shapes, cases, many):
        one = eng.scaler_scores([c], mode)[0]
        _check(m, one, f"batch vs single {s} {mode}")
        _check(m, _ref(*s, mode), f"batch {s} {mode}")


@pytest.mark.parametrize("mode", [0, 1])
def test_single_case_entry_point(mode):
    """pcg_scaler_case is the batch of one case, writing at out_off."""
    import torch
    from rcaeval_amd._lib import check
    eng = _eng()
    A, B = _case(63, 17, 11)
    Ad, Bd = eng.to_device(A), eng.to_device(B)
    vals = torch.full((3, 16), -1.0, dtype=torch.float64, device=eng.device)
    st = torch.full((16,), -1, dtype=torch.int32, device=eng.device)
    vp = ctypes.c_void_p
    check(eng.h, eng.lib.pcg_scaler_case(eng.h, vp(Ad.data_ptr()), 11, vp(Bd.data_ptr()), 11, 63, 17, 11, 4, mode,
                                         *(vp(vals.data_ptr() + k * 16 * 8) for k in range(3)), vp(st.data_ptr())),
          "pcg_scaler_case")
    v, s = vals.cpu().numpy(), st.cpu().numpy()
    ref = _ref(63, 17, 11, mode)
    for k, key in enumerate(("center", "scale", "score")):
        assert_array_equal(v[k, 4:15], ref[key])
        assert (v[k, :4] == -1.0).all() and v[k, 15] == -1.0          # slots outside the case untouched
    assert_array_equal(s[4:15], 0)
    assert (s[:4] == -1).all() and s[15] == -1


@pytest.mark.parametrize("mode", MODES)
def test_non_finite_columns_are_flagged(mode):
    """One NaN in a (column 2) and one Inf in b (column 5), both inside the first tile of 8
    columns: status 1 there, every other column as if they were finite."""
    for N in (70, _lds_rows() + 1):
        A, B = (x.copy() for x in _case(N, 17, 11))
        A[N // 2, 2] = np.nan
        B[3, 5] = np.inf
        got = _eng().scaler_scores([(A, B)], mode)[0]
        ref = _ref(N, 17, 11, mode)
        assert_array_equal(got["status"], [0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0])
        keep = got["status"] == 0
        for key in ("center", "scale", "score"):
            assert_array_equal(got[key][keep], ref[key][keep], err_msg=f"N={N} {key} {mode}")


def test_overflowing_scale_is_flagged_and_recomputed():
    """Finite values near DBL_MAX: q75 - q25 (and the median's sum) overflow, z becomes NaN and the
    reference's max depends on the row order. Robust mode flags such a column (status 1) on both
    selection paths and leaves its neighbours alone; the public method then equals the reference."""
    pd = pytest.importorskip("pandas")
    big = 1.7e308
    for N in (70, _lds_rows() + 1):
        A, B = (x.copy() for x in _case(N, 17, 11))
        A[:, 4] = np.where(np.arange(N) % 2 == 0, big, -big)
        B[:, 4] = np.linspace(-big, big, 17)
        got = _eng().scaler_scores([(A, B)], "robust")[0]
        ref = _ref(N, 17, 11, "robust")
        assert_array_equal(got["status"], [0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0])
        keep = got["status"] == 0
        for key in ("center", "scale", "score"):
            assert_array_equal(got[key][keep], ref[key][keep], err_msg=f"N={N} {key}")
    pytest.importorskip("sklearn")
    from rcaeval_amd.e2e import baro
    df, inject, split = br.small_frame()
    t = np.arange(len(df))
    df["e_cpu"] = np.where(t % 2 == 0, big, -big) * np.where(t < split, 1.0, 0.5)
    assert baro(df, inject, dataset="online-boutique") == br.reference_ranks(df, inject, dataset="online-boutique", mode="robust")


def test_non_finite_frame_through_the_public_methods():
    from rcaeval_amd.e2e import baro, nsigma
    try:
        import sklearn  # noqa: F401
        live = True
    except ImportError:
        live = False
    gold = np.load(GOLD)
    df, inject, _ = br.nonfinite_frame(with_inf=False)
    for method, mode in ((baro, "robust"), (nsigma, "standard")):
        want = (br.reference_ranks(df, inject, dataset="online-boutique", mode=mode)["ranks"] if live
                else [str(x) for x in gold["nf_" + mode]])
        assert [str(x) for x in gold["nf_" + mode]] == want
        assert method(df, inject, dataset="online-boutique")["ranks"] == want
    df, inject, _ = br.nonfinite_frame(with_inf=True)          # sklearn refuses an infinity: so does the method
    for method in (baro, nsigma):
        with pytest.raises(ValueError):
            method(df, inject, dataset="online-boutique")


def test_bad_arguments_leave_the_handle_usable():
    from rcaeval_amd._lib import PCG_ERR_INVALID, PcgError
    eng = _eng()
    A, B = _case(5, 2, 3)
    for bad in ((np.empty((0, 3)), B), (A, np.empty((0, 3)))):
        for mode in (0, 1):
            with pytest.raises(PcgError) as e:
                eng.scaler_scores([(A, B), bad], mode)
            assert e.value.code == PCG_ERR_INVALID
    with pytest.raises(PcgError) as e:
        eng.scaler_scores([(A, B)], 2)
    assert e.value.code == PCG_ERR_INVALID
    _check(eng.scaler_scores([(A, B)], 0)[0], _ref(5, 2, 3, 0), "after the refusals")


@functools.lru_cache(maxsize=None)
def _synth_cases():
    from rcaeval_amd import synth
    return tuple(synth.rq2_case_frame(rows=600, root_service=svc, fault=fault, seed=seed)
                 for svc, fault, seed in (("cartservice", "cpu", 0), ("adservice", "mem", 1), ("emailservice", "delay", 2)))


def test_end_to_end_ranks():
    """baro, nsigma and the batch entry points on RQ2-shaped frames (600 rows, 44 metrics): exactly
    the ranks of the frame logic with the restatement as the scorer."""
    from rcaeval_amd.e2e import baro, baro_batch, nsigma, nsigma_batch, robust_scaler
    cases = _synth_cases()
    for one, many in ((baro, baro_batch), (nsigma, nsigma_batch)):
        want = [one(df, t, dataset="online-boutique", scorer=br.scorer) for df, t in cases]
        assert len(want[0]["node_names"]) >= 40 and sorted(want[0]["ranks"]) == sorted(want[0]["node_names"])
        assert one(cases[0][0], cases[0][1], dataset="online-boutique") == want[0]
        assert many(list(cases), dataset="online-boutique") == want
    half = len(cases[0][0]) // 2
    assert robust_scaler(cases[0][0], anomalies=[half], dataset="online-boutique") == \
        robust_scaler(cases[0][0], anomalies=[half], dataset="online-boutique", scorer=br.scorer)
