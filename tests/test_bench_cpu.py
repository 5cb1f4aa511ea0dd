"""bench.py's command line and its --dump-outputs writer, without a device: --full is off by
default and leaves --full-p alone; dump_outputs writes float32 / float64 arrays in a canonical
row order, and cuts an array over its byte budget to a fixed, seeded sample of its rows."""
import os
import sys

import numpy as np

import bench


class _Out:
    """The fields of engine.SkeletonOut that dump_outputs reads."""

    def __init__(self, n=70, rows=500, words=2, seed=0):
        rng = np.random.default_rng(seed)
        self.removed_level = rng.integers(-1, 4, (n, n)).astype(np.int8)
        pairs = rng.permutation(n * n)[:rows]
        self.sep_xy = np.stack([pairs // n, pairs % n], axis=1).astype(np.int32)
        self.sep_bits = rng.integers(0, 2 ** 63, (rows, words)).astype(np.uint64) * np.uint64(2) + np.uint64(1)
        self.deg_levels = rng.integers(0, 9, (5, n)).astype(np.int32)
        self.stats = {"tests": [2415, 300, 20, 1, 0]}


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_full_and_dump_options_are_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.full_p, a.steps, a.warmup) == (False, None, False, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.full_p) == (True, "d", False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full-p"])
    a = bench.parse()
    assert (a.full, a.full_p) == (False, True)


def test_dump_outputs_writes_every_array_exactly(tmp_path):
    import torch
    o = _Out()
    C = torch.from_numpy(np.random.default_rng(1).standard_normal((70, 70)))
    shapes = bench.dump_outputs(str(tmp_path / "d"), o, C)
    got = _load(str(tmp_path / "d"))
    assert set(got) == {"corr", "removed_level", "sep_xy", "sep_bits_u32", "deg_levels", "tests_per_level"}
    assert {k: list(v.shape) for k, v in got.items()} == shapes
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert np.array_equal(got["corr"], C.numpy()) and got["corr"].dtype == np.float64
    assert np.array_equal(got["removed_level"], o.removed_level)
    assert np.array_equal(got["deg_levels"], o.deg_levels.T)
    assert np.array_equal(got["tests_per_level"], o.stats["tests"])
    # rows in (x, y) order; the 64-bit words come back bit for bit from their 32-bit halves
    order = np.lexsort((o.sep_xy[:, 1], o.sep_xy[:, 0]))
    assert np.array_equal(got["sep_xy"], o.sep_xy[order])
    h = got["sep_bits_u32"].astype(np.uint64)
    assert np.array_equal(h[:, 0::2] | (h[:, 1::2] << np.uint64(32)), o.sep_bits[order])


def test_dump_outputs_does_not_depend_on_the_export_order(tmp_path):
    a, b = _Out(), _Out()
    p = np.random.default_rng(5).permutation(len(b.sep_xy))
    b.sep_xy, b.sep_bits = b.sep_xy[p], b.sep_bits[p]
    bench.dump_outputs(str(tmp_path / "a"), a, None)
    bench.dump_outputs(str(tmp_path / "b"), b, None)
    ga, gb = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert "corr" not in ga and set(ga) == set(gb)
    assert all(np.array_equal(ga[k], gb[k]) for k in ga)


def test_dump_outputs_samples_an_array_over_its_budget(tmp_path, monkeypatch):
    import torch
    o = _Out()
    C = torch.from_numpy(np.random.default_rng(1).standard_normal((70, 70)))
    monkeypatch.setattr(bench, "DUMP_BUDGET", {"corr": 70 * 8 * 10 + 5, "removed_level": 70 * 4 * 70,
                                               "sep": (8 + 32 + 16) * 33, "small": 500_000})
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), o, C)
    ga, gb = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert set(ga) == set(gb) and all(np.array_equal(ga[k], gb[k]) for k in ga)      # a fixed sample
    assert ga["corr"].shape == (10, 70) and ga["removed_level"].shape == (70, 70)
    assert "removed_level_rows" not in ga                                            # exactly at its budget
    rows = ga["corr_rows"].astype(np.int64)
    assert len(set(rows)) == 10 and np.array_equal(rows, np.sort(rows))
    assert np.array_equal(ga["corr"], C.numpy()[rows])
    order = np.lexsort((o.sep_xy[:, 1], o.sep_xy[:, 0]))
    rows = ga["sep_xy_rows"].astype(np.int64)
    assert len(rows) == 33 and np.array_equal(rows, ga["sep_bits_u32_rows"])
    assert np.array_equal(ga["sep_xy"], o.sep_xy[order][rows])
    assert ga["sep_bits_u32"].shape == (33, 4)


def test_default_budgets_stay_under_64_mb():
    # two arrays share "small"; the row-index files of sampled arrays fit the rest
    assert sum(bench.DUMP_BUDGET.values()) + bench.DUMP_BUDGET["small"] <= 62_000_000
