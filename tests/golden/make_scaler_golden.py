"""Regenerate tests/golden/scaler.npz: scikit-learn's own answers for the oracle pin of
tests/test_baro_cpu.py (run from the repository root with scikit-learn installed).

For every (N, M, kind) of the pin: the column's inputs (the normal rows stored once per (N, kind),
shared by the three M) and (center, scale, score) of ``RobustScaler`` and ``StandardScaler`` as
``baro_ref.sklearn_column`` reads them off sklearn; and
the ranks of the reference's loop on ``baro_ref.nonfinite_frame(with_inf=False)`` for both modes.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import baro_ref as br  # noqa: E402

PIN_N = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 257, 1001)
PIN_M = (1, 2, 17)
PIN_KINDS = ("gauss", "ties", "const", "halfzero", "mixed")


def main():
    import sklearn
    warnings.filterwarnings("ignore")
    meta, a_all, b_all, exp = [], [], [], []
    for N in PIN_N:
        for k, kind in enumerate(PIN_KINDS):
            a = br.gen_column(kind, N, PIN_M[-1], seed=N * 31 + k)[0]
            a_all.append(a)
            for M in PIN_M:
                b = br.gen_column(kind, N, M, seed=N * 31 + k)[1]     # same seed: "const" keeps its level
                meta.append((N, M, k))
                b_all.append(b)
                with np.errstate(all="ignore"):
                    exp.append([br.sklearn_column(a, b, mode) for mode in (0, 1)])
    df, inject, _ = br.nonfinite_frame(with_inf=False)
    nf = {m: br.reference_ranks(df, inject, dataset="online-boutique", mode=m)["ranks"] for m in ("robust", "standard")}
    np.savez_compressed(os.path.join(HERE, "scaler.npz"), meta=np.array(meta, dtype=np.int64),
                        a=np.concatenate(a_all), b=np.concatenate(b_all), exp=np.array(exp, dtype=np.float64),
                        nf_robust=np.array(nf["robust"]), nf_standard=np.array(nf["standard"]),
                        versions=np.array([np.__version__, sklearn.__version__]))


if __name__ == "__main__":
    main()
