"""CPU: the batched small-graph entry points exist and are bound (pcg_skeleton_batch,
pcg_batch_abi_info, pcg_batch_near_export, the two ctypes structs), the Python layers expose
them (Engine.skeleton_batch, causal.pc_batch, e2e.pc_pagerank_batch, rq2.run(batch=)), and
the option checks refuse what a batch does not run before any device is touched."""
import ctypes
import inspect

import numpy as np
import pytest


def test_batch_abi_info_equals_ctypes_structs():
    from rcaeval_amd import _lib
    lib = _lib.load()
    cb, rb = ctypes.c_int64(), ctypes.c_int64()
    assert lib.pcg_batch_abi_info(ctypes.byref(cb), ctypes.byref(rb)) == 0
    assert (cb.value, rb.value) == (ctypes.sizeof(_lib.PcgCase), ctypes.sizeof(_lib.PcgCaseResult))
    assert lib.pcg_batch_abi_info(None, None) == 0
    # the result embeds pcg_stats unchanged and one 64-wide degree row per level
    assert _lib.PcgCaseResult.stats.size == ctypes.sizeof(_lib.PcgStats)
    assert _lib.PcgCaseResult.deg.size == 4 * 64 * _lib.PCG_MAX_LEVELS
    assert _lib.PCG_ABI_VERSION == 4


def test_batch_symbols_are_bound():
    from rcaeval_amd import _lib
    lib = _lib.load()
    bound = {name for name, _, _ in _lib.SIGNATURES}
    for name in ("pcg_skeleton_batch", "pcg_batch_abi_info", "pcg_batch_near_export"):
        assert name in bound and hasattr(lib, name), name


def test_batch_null_handle_is_refused():
    from rcaeval_amd import _lib
    lib = _lib.load()
    assert lib.pcg_skeleton_batch(None, None, 0, 0.05, -1, 0, None) == _lib.PCG_ERR_INVALID
    assert lib.pcg_batch_near_export(None, 0, None, 0) == _lib.PCG_ERR_INVALID


def test_python_layers_expose_the_batch():
    from rcaeval_amd import causal, e2e, rq2
    from rcaeval_amd.engine import Engine, SkeletonOut
    sig = inspect.signature(rq2.run)
    assert sig.parameters["batch"].default == 0
    sig = inspect.signature(Engine.skeleton_batch)
    assert [p for p in sig.parameters][1:] == ["Cs_or_Xs", "Ns", "alpha", "max_depth", "flags", "from_data"]
    assert sig.parameters["from_data"].default is False and sig.parameters["alpha"].default == 0.05
    sig = inspect.signature(causal.pc_batch)
    assert [p for p in sig.parameters][:5] == ["datas", "alpha", "node_names", "max_depth", "device"]
    assert callable(e2e.pc_pagerank_batch) and "pc_pagerank_batch" in e2e.__all__
    assert SkeletonOut.rc == 0


def test_rq2_main_has_batch_option():
    from rcaeval_amd import rq2
    with pytest.raises(SystemExit):          # the data root does not exist: parsed, then refused
        rq2.main(["--method", "pc_pagerank", "--dataset", "online-boutique", "--data-root", "/nonexistent-root",
                  "--batch", "8"])


def test_pc_batch_of_nothing_is_empty():
    from rcaeval_amd.causal import pc_batch
    assert pc_batch([]) == []
    assert pc_batch(iter(())) == []


@pytest.mark.parametrize("opt", [{"indep_test": "chisq"}, {"stable": False}, {"uc_rule": 1}, {"uc_priority": 3},
                                 {"uc_priority": -1}, {"mvpc": True}, {"background_knowledge": object()}])
def test_pc_batch_refuses_other_options_without_the_device(opt, monkeypatch):
    from rcaeval_amd import causal

    def no_engine(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(causal, "get_engine", no_engine)
    X = np.random.default_rng(0).standard_normal((50, 4))
    with pytest.raises(NotImplementedError):
        causal.pc_batch([X], **opt)
    with pytest.raises(TypeError):
        causal.pc_batch([X], no_such_option=1)
    # the defaults, spelled out, pass the check (and then reach the engine)
    with pytest.raises(AssertionError, match="device was touched"):
        causal.pc_batch([X], indep_test="fisherz", stable=True, uc_rule=0, uc_priority=2, mvpc=False,
                        background_knowledge=None)
    with pytest.raises(ValueError):
        causal.pc_batch([X], node_names=[["a"] * 4, ["b"] * 4])


def test_pc_pagerank_batch_of_nothing_is_empty():
    from rcaeval_amd.e2e import pc_pagerank_batch
    assert pc_pagerank_batch([]) == []
