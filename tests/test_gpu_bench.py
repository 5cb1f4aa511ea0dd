"""GPU: bench.py's skeleton workload run in-process at a small size (n = 300, N = 1200, the level
loop with its CRT K1). A plain run times exactly --steps steps and runs nothing besides; its
--dump-outputs arrays are what the engine returns for the same input, the same from run to run;
--full fills the K1 roofline and the full-p comparison that a plain run leaves out."""
import json
import os
import sys

import numpy as np
import pytest

import bench
from rcaeval_amd import synth

pytestmark = pytest.mark.gpu

SIZE = ["--n", "300", "--samples", "1200", "--seed", "4"]


def _bench(monkeypatch, capsys, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", *SIZE, *argv])
    capsys.readouterr()
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_plain_run_times_the_steps_and_dumps_the_engine_outputs(monkeypatch, capsys, tmp_path):
    from rcaeval_amd.engine import get_engine
    calls = []
    monkeypatch.setattr(bench, "cpu_baseline", lambda *a, **k: calls.append("cpu_baseline"))
    eng = get_engine(0)
    corr = eng.corr
    monkeypatch.setattr(eng, "corr", lambda *a, **k: (calls.append("corr"), corr(*a, **k))[1])
    line = _bench(monkeypatch, capsys, "--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path / "a"))
    assert calls == []                                  # no K1-alone, full-p or CPU run
    assert (line["steps"], line["warmup"], len(line["step_ms_all"])) == (3, 2, 3)
    assert line["unit"] == "CI tests/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] == pytest.approx(np.mean(line["step_ms_all"]), abs=1e-3)
    assert line["value"] == pytest.approx(sum(line["tests_per_level"]) / (line["ms_per_step"] / 1e3), rel=1e-9)
    assert line["roofline"]["k1"] is None and line["sampled_records"] is None and "cpu_baseline" not in line

    got = _load(str(tmp_path / "a"))
    assert not any(k.endswith("_rows") for k in got)    # nothing sampled at this size
    X = synth.gaussian_sem(300, 1200, seed=4)
    out, C = eng.corr_skeleton(X, alpha=0.05, max_depth=4)
    assert np.array_equal(got["corr"], C.cpu().numpy())
    assert np.array_equal(got["removed_level"], out.removed_level)
    assert np.array_equal(got["deg_levels"], out.deg_levels.T)
    assert np.array_equal(got["tests_per_level"], out.stats["tests"]) and got["tests_per_level"].sum() > 0
    order = np.lexsort((out.sep_xy[:, 1], out.sep_xy[:, 0]))
    assert len(order) > 0 and np.array_equal(got["sep_xy"], out.sep_xy[order])
    h = got["sep_bits_u32"].astype(np.uint64)
    assert np.array_equal(h[:, 0::2] | (h[:, 1::2] << np.uint64(32)), out.sep_bits[order])

    _bench(monkeypatch, capsys, "--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path / "b"))
    again = _load(str(tmp_path / "b"))
    assert set(again) == set(got) and all(np.array_equal(again[k], got[k]) for k in got)


def test_full_run_adds_the_k1_roofline_and_the_full_p_comparison(monkeypatch, capsys):
    line = _bench(monkeypatch, capsys, "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert (line["steps"], len(line["step_ms_all"])) == (2, 2)
    assert line["roofline"]["k1"]["path"] == "int8 CRT" and line["roofline"]["k1"]["ms"] > 0
    assert line["sampled_records"]["same_skeleton_as_threshold"] is True
    assert "cpu_baseline" not in line
