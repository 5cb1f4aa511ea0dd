"""CPU: the CRT K1's split-K plan search (corr.hip crt_plan_mix) through the host-only
pcg_k1_crt_plan query: the headline shape takes the whole-round plan, knob 0 and a forced uniform
count keep one split for every tile, a forced (tA, ksA, ksB) is taken as given."""
import ctypes

import pytest

from rcaeval_amd import _lib

KEYS = ("tiles", "moduli", "tA", "ksA", "kbA", "ksB", "kbB", "units")


def plan(lib, n, N):
    v = (ctypes.c_int64 * 8)()
    assert lib.pcg_k1_crt_plan(None, n, N, v) == 0        # a NULL handle: the environment's defaults
    return dict(zip(KEYS, (int(x) for x in v)))


def test_headline_plan_fills_whole_rounds():
    """n = 2000, N = 10^4: 36 tiles x 16 moduli, 314 k-blocks. 32 tiles unsplit (512 units, two rounds
    of the 256 CUs) and 4 tiles in 4 slabs (256 units, one round)."""
    p = plan(_lib.load(), 2000, 10000)
    assert p == {"tiles": 36, "moduli": 16, "tA": 32, "ksA": 1, "kbA": 316, "ksB": 4, "kbB": 80, "units": 768}
    assert p["moduli"] * p["tA"] * p["ksA"] % 256 == 0 and p["moduli"] * (36 - p["tA"]) * p["ksB"] == 256


@pytest.mark.parametrize("n,N", [(300, 130), (600, 1000), (1000, 10000), (4000, 10000), (8000, 3000)])
def test_plan_is_consistent(n, N):
    p = plan(_lib.load(), n, N)
    T = -(-n // 256)
    TB = (N + 63) // 64 * 2
    assert p["tiles"] == T * (T + 1) // 2 and 1 <= p["tA"] <= p["tiles"]
    assert p["units"] == p["moduli"] * (p["tA"] * p["ksA"] + (p["tiles"] - p["tA"]) * p["ksB"])
    for ks, kb in ((p["ksA"], p["kbA"]), (p["ksB"], p["kbB"])):
        assert kb % 4 == 0 and -(-TB // kb) == ks and 1 <= ks <= 16
    assert p["ksA"] <= p["ksB"]                 # the long class is dispatched first


def test_knobs_select_the_plan(monkeypatch):
    lib = _lib.load()
    monkeypatch.setenv("PCG_K1_CRT_MIX", "0")
    p = plan(lib, 2000, 10000)
    assert (p["tA"], p["ksA"], p["kbA"], p["units"]) == (36, 2, 160, 1152)      # the uniform plan
    monkeypatch.setenv("PCG_K1_CRT_MIX", str(_lib.k1_crt_mix_force(5, 2, 3)))
    p = plan(lib, 2000, 10000)
    assert (p["tA"], p["ksA"], p["ksB"], p["units"]) == (5, 2, 3, 16 * (5 * 2 + 31 * 3))
    monkeypatch.setenv("PCG_K1_CRT_KS", "4")    # a forced uniform count wins
    p = plan(lib, 2000, 10000)
    assert (p["tA"], p["ksA"], p["ksB"], p["units"]) == (36, 4, 4, 2304)
    monkeypatch.delenv("PCG_K1_CRT_KS")
    monkeypatch.delenv("PCG_K1_CRT_MIX")
    assert plan(lib, 2000, 10000)["tA"] == 32
    sig = ctypes.c_int64()                      # the sharded plan (signature) stays uniform: 2 slabs
    assert lib.pcg_k1_plan_signature(None, 2000, 10000, ctypes.byref(sig)) == 0
    assert (sig.value >> 32) & 0xFF == 2 and sig.value & 0xFFFFFFFF == 1152
    assert plan(lib, 100, 1000) == dict.fromkeys(KEYS, 0)      # below PCG_TUNE_K1_CRT_MINN: not the CRT path
