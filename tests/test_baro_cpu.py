"""CPU: the arithmetic of baro / robust_scaler / nsigma is pinned to scikit-learn, the frame logic
of ``rcaeval_amd.e2e.baro`` to the reference's loop, and the plumbing to ``include/pcgpu.h``.

The oracle of the GPU tests is ``tests/baro_ref.py``. Here it is compared with sklearn under
``==`` (never a tolerance): live where sklearn is importable, and against
``tests/golden/scaler.npz`` (sklearn's answers, ``tests/golden/make_scaler_golden.py``) everywhere.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import baro_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "scaler.npz")
PIN_N = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 257, 1001)
PIN_M = (1, 2, 17)
PIN_KINDS = ("gauss", "ties", "const", "halfzero", "mixed")


def _same(x, y):
    """Bit equality up to the sign of zero; NaN equals NaN."""
    x, y = np.float64(x), np.float64(y)
    return bool(x == y or (np.isnan(x) and np.isnan(y)))


def _golden_cases():
    """(N, M, kind, a, b, expected[mode][center, scale, score]) of every golden column."""
    g = np.load(GOLD)
    a_off = b_off = 0
    a_of = {}
    out = []
    for row, (N, M, k) in enumerate(g["meta"]):
        if (N, k) not in a_of:
            a_of[(N, k)] = g["a"][a_off:a_off + N]
            a_off += N
        b = g["b"][b_off:b_off + M]
        b_off += M
        out.append((int(N), int(M), PIN_KINDS[k], a_of[(N, k)], b, g["exp"][row]))
    assert a_off == len(g["a"]) and b_off == len(g["b"])
    return out


def test_golden_covers_the_pin():
    seen = {(N, M, kind) for N, M, kind, *_ in _golden_cases()}
    assert seen == {(N, M, kind) for N in PIN_N for M in PIN_M for kind in PIN_KINDS}


def test_oracle_equals_sklearn_golden():
    for N, M, kind, a, b, exp in _golden_cases():
        for mode in (0, 1):
            with np.errstate(all="ignore"):
                got = br.column(a, b, mode)
            assert all(_same(x, y) for x, y in zip(got, exp[mode])), (N, M, kind, mode, got, exp[mode])


def test_oracle_equals_sklearn_live():
    pytest.importorskip("sklearn")
    for N in PIN_N:
        for M in PIN_M:
            for k, kind in enumerate(PIN_KINDS):
                a, b = br.gen_column(kind, N, M, seed=7919 * N + 13 * M + k)
                for mode in (0, 1):
                    with np.errstate(all="ignore"):
                        got, exp = br.column(a, b, mode), br.sklearn_column(a, b, mode)
                    assert all(_same(x, y) for x, y in zip(got, exp)), (N, M, kind, mode, got, exp)


def test_oracle_sum_order_beyond_one_numpy_buffer():
    """numpy sums a long column in blocks of 8192 elements; the device restates that order, so the
    pin has to hold on both sides of it."""
    pytest.importorskip("sklearn")
    for N in (8192, 8193, 20000):
        a, b = br.gen_column("gauss", N, 3, seed=N)
        got, exp = br.column(a, b, 1), br.sklearn_column(a, b, 1)
        assert all(_same(x, y) for x, y in zip(got, exp)), (N, got, exp)


def test_constant_column_scales_to_one():
    a, b = br.gen_column("const", 65, 2, seed=3)
    for mode in (0, 1):
        assert br.column(a, b, mode)[1] == 1.0


# ---- frame logic ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["robust", "standard"])
@pytest.mark.parametrize("split", ["inject_time", "anomalies"])
def test_frame_logic_equals_reference_loop(mode, split):
    pytest.importorskip("sklearn")
    from rcaeval_amd.e2e import nsigma, robust_scaler
    df, inject, k = br.small_frame()
    kw = {"inject_time": inject} if split == "inject_time" else {"anomalies": [k]}
    method = robust_scaler if mode == "robust" else nsigma
    got = method(df, dataset="online-boutique", scorer=br.scorer, **kw)
    ref = br.reference_ranks(df, dataset="online-boutique", mode=mode, **kw)
    assert got == ref
    assert set(got) == {"node_names", "ranks"}
    # each half lost a different column, and only the intersection is ranked, in the normal order
    assert "a_cpu" not in got["node_names"] and "b_mem" not in got["node_names"] and "d_lat" not in got["node_names"]
    assert got["node_names"] == ["c_cpu", "c_lat", "e_cpu", "f_lat", "g_cpu", "h_mem"]
    assert got["ranks"].index("c_cpu") + 1 == got["ranks"].index("c_lat")      # the tie keeps column order


def test_frame_logic_without_dataset_keeps_every_column():
    """``dataset=None``: preprocess is the identity, so ``time`` is scored like any column."""
    pytest.importorskip("sklearn")
    from rcaeval_amd.e2e import baro
    df, inject, _ = br.small_frame()
    got = baro(df, inject, scorer=br.scorer)
    assert got == br.reference_ranks(df, inject, mode="robust")
    assert got["node_names"] == list(df.columns)


def test_batch_equals_per_case_calls_on_the_host():
    from rcaeval_amd.e2e import baro, baro_batch, nsigma, nsigma_batch
    df, inject, _ = br.small_frame()
    df2 = df.iloc[::-1].reset_index(drop=True).assign(time=df["time"].to_numpy())
    cases = [(df, inject), (df2, inject + 3)]
    for one, many in ((baro, baro_batch), (nsigma, nsigma_batch)):
        got = many(cases, dataset="online-boutique", scorer=br.scorer)
        assert got == [one(d, t, dataset="online-boutique", scorer=br.scorer) for d, t in cases]


def test_status_one_columns_are_recomputed_by_sklearn():
    """A NaN column is flagged by the scorer and recomputed on the host; an Inf is refused as sklearn refuses it."""
    pytest.importorskip("sklearn")
    from rcaeval_amd.e2e import baro, nsigma
    df, inject, _ = br.nonfinite_frame(with_inf=False)
    for method, mode in ((baro, "robust"), (nsigma, "standard")):
        assert method(df, inject, dataset="online-boutique", scorer=br.scorer) == \
            br.reference_ranks(df, inject, dataset="online-boutique", mode=mode)
    df, inject, _ = br.nonfinite_frame(with_inf=True)
    for method, mode in ((baro, "robust"), (nsigma, "standard")):
        with pytest.raises(ValueError):
            br.reference_ranks(df, inject, dataset="online-boutique", mode=mode)
        with pytest.raises(ValueError):
            method(df, inject, dataset="online-boutique", scorer=br.scorer)


def test_empty_inputs_follow_the_reference():
    from rcaeval_amd.e2e import baro, nsigma
    df, inject, _ = br.small_frame()
    # no common column: both halves keep only columns the other lost
    none = df[["time", "a_cpu", "b_mem", "d_lat"]]
    assert baro(none, inject, dataset="online-boutique", scorer=br.scorer) == {"node_names": [], "ranks": []}
    # a half without rows: preprocess fails on df.iloc[0] when a dataset is named, sklearn's
    # ValueError otherwise
    for method in (baro, nsigma):
        with pytest.raises(IndexError):
            method(df, inject - 1000, dataset="online-boutique", scorer=br.scorer)
        with pytest.raises(ValueError, match="0 sample"):
            method(df, inject - 1000, scorer=br.scorer)
        with pytest.raises(ValueError, match="0 sample"):
            method(df, inject + 1000, scorer=br.scorer)


# ---- plumbing ------------------------------------------------------------------------------------
def test_header_declares_the_scaler_entry_points():
    hdr = open(os.path.join(ROOT, "include", "pcgpu.h")).read()
    for name in ("pcg_scaler_case", "pcg_scaler_batch", "pcg_scaler_abi_info", "pcg_scaler_limits"):
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
    assert int(re.search(r"#define PCG_ABI_VERSION (\d+)", hdr).group(1)) == 4


def test_scaler_case_struct_matches_library():
    from rcaeval_amd import _lib
    lib = _lib.load()
    assert _lib.PCG_ABI_VERSION == 4 and _lib.abi_info(lib)[2] == 4
    nb = ctypes.c_int64()
    assert lib.pcg_scaler_abi_info(ctypes.byref(nb)) == 0
    assert nb.value == ctypes.sizeof(_lib.PcgScalerCase) == 64
    rows = ctypes.c_int64()
    assert lib.pcg_scaler_limits(ctypes.byref(rows)) == 0
    assert rows.value >= 256 and rows.value & (rows.value - 1) == 0


def test_methods_are_exported_and_served():
    from rcaeval_amd import rq2
    from rcaeval_amd.e2e import baro, baro_batch, nsigma, nsigma_batch, robust_scaler
    assert baro is robust_scaler
    m = rq2.methods()
    assert m["baro"] is baro and m["robust_scaler"] is robust_scaler and m["nsigma"] is nsigma
    b = rq2.batch_methods()
    assert b["baro"] is baro_batch and b["robust_scaler"] is baro_batch and b["nsigma"] is nsigma_batch
    assert "pc_pagerank" in b
    for f in (baro, nsigma):
        assert not hasattr(f, "__wrapped__")          # no @rca wrapper, as in the reference


def test_narrow_float_columns_are_scored_in_their_own_precision():
    """sklearn fits a float32 column in float32; such a column goes to sklearn itself, in a frame
    whose other columns stay on the scorer."""
    pytest.importorskip("sklearn")
    from rcaeval_amd.e2e import baro, nsigma
    df, inject, _ = br.small_frame()
    df = df.astype({"e_cpu": np.float32, "h_mem": np.float32})
    seen = []

    def scorer(pairs, mode):
        seen.append(len(pairs))
        return br.scorer(pairs, mode)
    for method, mode in ((baro, "robust"), (nsigma, "standard")):
        for dataset in ("online-boutique", None):
            assert method(df, inject, dataset=dataset, scorer=scorer) == \
                br.reference_ranks(df, inject, dataset=dataset, mode=mode)
    assert seen == [1, 1, 1, 1]


# ---- the RQ2 harness's batch path ------------------------------------------------------------------
@pytest.mark.parametrize("method", ["baro", "robust_scaler", "nsigma"])
def test_rq2_batch_path_writes_the_per_case_files(method, tmp_path, monkeypatch):
    """``process_loaded_batch`` with a scaler method: the JSON files equal those of the per-case
    loop, and they come from the batch entry point, not from the fall-back behind its ``except``."""
    import json
    from rcaeval_amd import rq2
    from rcaeval_amd.e2e import baro as _  # noqa: F401  (the package is imported before its module is patched)
    import sys
    monkeypatch.setattr(sys.modules["rcaeval_amd.e2e.baro"], "device_scorer", br.scorer)
    df, inject, _k = br.small_frame()
    df2 = df.iloc[::-1].reset_index(drop=True).assign(time=df["time"].to_numpy())
    cs = [{"data": d, "inject_time": t, "sli": "e_cpu", "num_node": len(d.columns) - 1,
           "result_name": f"svc{i}_cpu_{i}.json"} for i, (d, t) in enumerate(((df, inject), (df2, inject + 3)))]
    one_dir, many_dir = tmp_path / "one", tmp_path / "many"
    one_dir.mkdir()
    many_dir.mkdir()
    per_case = rq2.process_loaded

    def no_fallback(*a, **k):
        raise AssertionError("the batch path fell back to the per-case loop")
    monkeypatch.setattr(rq2, "process_loaded", no_fallback)
    many = rq2.process_loaded_batch(cs, "online-boutique", str(many_dir), method)
    monkeypatch.setattr(rq2, "process_loaded", per_case)
    one = [rq2.process_loaded(c, method, "online-boutique", str(one_dir)) for c in cs]
    assert [m["ranks"] for m in many] == [o["ranks"] for o in one]
    assert many[0]["ranks"] != many[1]["ranks"] and len(many[0]["ranks"]) == 6
    for i, c in enumerate(cs):
        a = json.load(open(one_dir / c["result_name"]))
        b = json.load(open(many_dir / c["result_name"]))
        assert a == b and a["0"] == one[i]["ranks"]
