"""``pcmci`` — mirror of ``RCAEval/graph_construction/pcmci.py:71-103`` on the MI355X engine.

The reference runs tigramite 4.2.2.1 [U] ``PCMCI(dataframe, _ParCorr(significance='analytic'))
.run_pcmci(tau_max, pc_alpha, max_conds_dim=None)`` (not installed here, restated from its source in
``tests/pcmci_ref.py``), takes the minimum of ``p_matrix[i, j, :]`` over the lags, rounds it to 3
decimals and draws the edge i -> j wherever the rounded value is non-zero. With tigramite's default
``cut_off='2xtau_max'`` every ParCorr test of a run uses the rows ``2 tau_max .. T-1``, so every
value is a partial correlation inside one correlation matrix of the lag-expanded data; the engine
computes that matrix with K1 and runs PC1 (``pcg_pcmci_parents``) and MCI (``pcg_pcmci_mci``) on it
(``csrc/pcmci.hip``). The Student-t side stays on the host, as ``granger.py`` keeps its tails:
``critical_values`` gives the kernel the |val| below which ``p > pc_alpha`` per conditioning
dimension (the decision is monotone in |val| at fixed ``deg_f``), and ``matrices_from_stats`` /
``pcmci_from_stats`` turn the kernel's ``val`` and ``|Z|`` into p-values, the gathered link
matrix and the adjacency — pure numpy.

Deviation: ``_ParCorr`` drops conditioning columns that are constant over the window; the engine
reports them (status 1) and this layer raises ``ValueError``. ``preprocess`` removes constant
columns before any method sees the data, so only a column constant over the window but not over the
whole frame can get here. Non-finite input raises ``ValueError`` as tigramite does.
"""
from __future__ import annotations

import numpy as np

_EPS = float(np.finfo(np.float64).eps)


def limits() -> dict:
    """The limits and the fast-path guards the library's PCMCI kernels were built with
    (``pcg_pcmci_limits``): max_tau, z_cap, max_width, max_candidates, tau, beta_c."""
    import ctypes
    from .. import _lib
    i = [ctypes.c_int32() for _ in range(4)]
    d = [ctypes.c_double() for _ in range(2)]
    _lib.load().pcg_pcmci_limits(*(ctypes.byref(v) for v in i + d))
    return {"max_tau": i[0].value, "z_cap": i[1].value, "max_width": i[2].value, "max_candidates": i[3].value,
            "tau": d[0].value, "beta_c": d[1].value}


def fast_path_bound(dim_z: int) -> float:
    """B: the absolute error bound of an accepted fast-path ``val`` with ``|Z| = dim_z`` (DESIGN.md,
    "PCMCI": first-order, 2 * beta_c * eps_R / tau with eps_R = (|Z| + 18) * 2^-53 the entry-wise
    backward error of the factorisation of the (|Z| + 2)-square block plus K1's own rounding)."""
    lim = limits()
    return 2.0 * lim["beta_c"] * (int(dim_z) + 18) * 2.0 ** -53 / lim["tau"]


def critical_values(T_eff: int, pc_alpha: float, count: int) -> np.ndarray:
    """crit[d], d = 0..count-1: a ParCorr test with |Z| = d has ``p > pc_alpha`` iff
    ``|val| < crit[d]``: with deg_f = T_eff - 2 - d and t_c = t.isf(pc_alpha / 2, deg_f),
    crit = t_c / sqrt(deg_f + t_c^2). 0 where deg_f < 1 (p is NaN there: nothing is removed)."""
    from scipy import stats
    crit = np.zeros(int(count), dtype=np.float64)
    for d in range(int(count)):
        deg_f = int(T_eff) - 2 - d
        if deg_f < 1:
            continue
        t_c = float(stats.t.isf(pc_alpha / 2.0, deg_f))
        crit[d] = t_c / np.sqrt(deg_f + t_c * t_c) if np.isfinite(t_c) else 1.0
    return crit


def raise_on_status(status) -> None:
    """``ValueError`` for a constant window (1) or non-finite input (2); ``PcgError`` for a test
    beyond the kernel's |Z| cap (4), which is the engine's limit and not an outcome of the data."""
    status = np.asarray(status)
    if (status == 2).any():
        raise ValueError("pcmci: non-finite input")
    if (status == 1).any():
        raise ValueError("pcmci: a lagged column is constant over the window")
    if (status == 4).any():
        from .._lib import PCG_ERR_INVALID, PcgError
        raise PcgError(PCG_ERR_INVALID, "pcmci: a conditioning set is larger than the kernel's cap")


def matrices_from_stats(val, dim, T_eff: int):
    """(val_matrix, p_matrix) from ``pcg_pcmci_mci``'s ``val`` and ``|Z|`` (n x n x (tau_max + 1);
    dim < 0: untested, val 0 and p 1): p = 2 t.sf(|val| sqrt(deg_f / (1 - val^2)), deg_f) with
    deg_f = T_eff - 2 - |Z|; 0 when ||val| - 1| <= eps; NaN when deg_f < 1."""
    from scipy import stats
    val = np.array(val, dtype=np.float64)
    dim = np.asarray(dim)
    tested = dim >= 0
    val[~tested] = 0.0
    p = np.ones(val.shape)
    deg_f = (int(T_eff) - 2 - dim).astype(np.float64)
    v = val[tested]
    f = deg_f[tested]
    one = np.abs(np.abs(v) - 1.0) <= _EPS
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.abs(v) * np.sqrt(f / (1.0 - v * v))
        pt = 2.0 * stats.t.sf(t, np.where(f >= 1, f, 1.0))
    pt = np.where(one, 0.0, pt)
    pt = np.where(f < 1, np.nan, pt)
    p[tested] = pt
    return val, p


def pcmci_from_stats(val, dim, T_eff: int):
    """(adj, link, p_matrix, val_matrix): ``pcmci.py:60-97`` from the kernel's arrays. ``link`` is
    the minimum p over the lags rounded to 3 decimals, ``adj[cause, effect] = 1`` wherever it is
    non-zero (the reference's test, ``np.where(matrix)``)."""
    val_matrix, p_matrix = matrices_from_stats(val, dim, T_eff)
    adj, link = adjacency_from_p(p_matrix)
    return adj, link, p_matrix, val_matrix


def adjacency_from_p(p_matrix):
    """(adj, link) of ``pcmci.py:83-97``: ``_gather_tau``, ``np.around(.., 3)``, ``np.where``."""
    n = p_matrix.shape[0]
    link = np.around(np.array([[min(p_matrix[i][j]) for j in range(n)] for i in range(n)]).reshape(n, n), 3)
    adj = np.zeros((n, n), dtype=np.int64)
    adj[np.where(link)] = 1
    return adj, link


def run_pcmci(data, tau_max: int, pc_alpha: float) -> dict:
    """``Engine.pcmci`` of a frame or array (T x n)."""
    from ..engine import get_engine
    X = data.to_numpy() if hasattr(data, "to_numpy") else np.asarray(data)
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("pcmci: data must be T x n")
    return get_engine().pcmci(X, int(tau_max), float(pc_alpha))


def pcmci(data, tau_max=3, alpha=0.2):
    """``pcmci.py:71-103``: n x n adjacency in column order, ``adj[cause, effect] = 1``."""
    return adjacency_from_p(run_pcmci(data, tau_max, alpha)["p_matrix"])[0]


__all__ = ["adjacency_from_p", "critical_values", "fast_path_bound", "limits", "matrices_from_stats", "pcmci", "pcmci_from_stats",
           "raise_on_status", "run_pcmci"]
