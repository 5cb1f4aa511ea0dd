"""``granger`` — mirror of ``RCAEval/graph_construction/granger.py:4-35`` on the MI355X engine.

The reference calls statsmodels' ``grangercausalitytests`` [U] (statsmodels 0.14.0, the version of
RCAEval's ``requirements.txt``; not installed here, restated from its source) once per ordered
pair: column i is the caused series y, column j the causing series x, and ``adj[i, j] = 1`` when
for any lag L in 1..maxlag the mean of the four tests' p-values (or the named test's p) is below
``p_val_threshold``. All n * (n - 1) * maxlag pairs of regressions run in one engine call
(``pcg_granger``: ssr of the restricted and the joint OLS, the centred tss, the joint design's
rank); the statistics, their tails (``scipy.special.fdtrc`` / ``chdtrc``, one vectorised call
each), the average, the threshold and the raising conditions are ``granger_from_stats`` below,
pure numpy on the kernel's arrays — as ``ChiSqTester`` leaves ``chi2.sf`` to the host.

Per lag L, nobs = T - L, df = nobs - rank(joint) [U] (``stattools.py`` grangercausalitytests):

    ssr_ftest     F = (ssr_r - ssr_u) / ssr_u / L * df          p = f.sf(F, L, df)
    ssr_chi2test  chi2 = nobs * (ssr_r - ssr_u) / ssr_u          p = chi2.sf(chi2, L)
    lrtest        LR = nobs * log(ssr_r / ssr_u)                 p = chi2.sf(LR, L)
    params_ftest  the Wald F test that the L coefficients on x are zero: the same degrees of
                  freedom as ssr_ftest, and algebraically its F (they differ by rounding only),
                  so it is served by ssr_ftest's value

The whole call raises ``ValueError`` — through ``@rca`` the method then returns the dummy
ranking — where statsmodels raises [U]: non-finite input; ``T <= 3 * maxlag + 1`` ("Insufficient
observations"); a lagged column of the joint design constant over its window
(``InfeasibleTestError``, a ``ValueError``); a perfect fit, i.e. centred tss == 0, ssr_u == 0 or
ssr_u / tss < 2^-52 (``InfeasibleTestError``).
"""
from __future__ import annotations

import numpy as np

TESTS = ("ssr_ftest", "ssr_chi2test", "lrtest", "params_ftest")
_EPS = float(np.finfo(np.float64).eps)          # 2^-52


def fast_path_guards() -> tuple:
    """(tau, floor, beta_c) of the library's moment / Cholesky path (``pcg_granger_guards``): an item
    keeps that path's result only if every scaled pivot is >= tau, ssr_u / tss >= floor and
    (1 + |beta|_1)^2 <= beta_c / tau; everything else is recomputed by the QR path."""
    import ctypes
    from .. import _lib
    t, f, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    _lib.load().pcg_granger_guards(ctypes.byref(t), ctypes.byref(f), ctypes.byref(c))
    return t.value, f.value, c.value


def fast_path_bound(T: int) -> float:
    """B(tau): the relative error bound of an accepted fast-path ``ssr_r / ssr_u`` (DESIGN.md,
    "Granger": first-order, c * u / tau with c = 2 * beta_c * (ceil(T / 64) + ceil(T / 2048) + 27) / floor,
    the bracket counting the roundings behind one scaled Gram entry, u = 2^-53)."""
    T = int(T)
    tau, floor, beta_c = fast_path_guards()
    return 2.0 * beta_c * (-(-T // 64) + -(-T // 2048) + 27) * 2.0 ** -53 / (tau * floor)


def granger_from_stats(ssr_r, ssr_u, tss, rank, status, T: int, maxlag: int = 3, p_val_threshold: float = 0.05,
                       test=None):
    """(adj, p) from ``pcg_granger``'s arrays (each n x n x maxlag, item (i, j, L - 1)): ``p`` is
    n x n x maxlag x 4 in the order of ``TESTS`` with a NaN diagonal; ``adj`` is the reference's
    n x n float matrix. Raises ``ValueError`` where the reference's call raises (module docstring)."""
    assert test in (None,) + TESTS
    ssr_r, ssr_u, tss = (np.asarray(a, dtype=np.float64) for a in (ssr_r, ssr_u, tss))
    rank, status = np.asarray(rank), np.asarray(status)
    n = ssr_r.shape[0]
    if ssr_r.shape != (n, n, maxlag):
        raise ValueError(f"expected n x n x {maxlag} arrays, got {ssr_r.shape}")
    if n < 2:
        return np.zeros((n, n)), np.full((n, n, maxlag, 4), np.nan)
    if T <= 3 * maxlag + 1:
        raise ValueError(f"Insufficient observations. Maximum allowable lag is {int((T - 1) / 3) - 1}")
    off = ~np.eye(n, dtype=bool)
    st = status[off]
    if (st == 4).any():
        raise ValueError("granger: non-finite input")
    if (st == 1).any():
        raise ValueError("granger: a lagged column is constant over its window (InfeasibleTestError)")
    r, u, t = ssr_r[off], ssr_u[off], tss[off]                      # pairs x maxlag
    with np.errstate(divide="ignore", invalid="ignore"):
        perfect = (st == 2) | (t == 0) | (u == 0) | (u / t < _EPS)
    if perfect.any():
        raise ValueError("granger: perfect fit (InfeasibleTestError)")
    from scipy.special import chdtrc, fdtrc
    L = np.arange(1, maxlag + 1, dtype=np.float64)[None, :]
    nobs = float(T) - L
    df = nobs - rank[off]
    gain = (r - u) / u
    # a rounding-negative statistic has sf = 1, as the distributions' sf gives below their support
    F = np.maximum(gain / L * df, 0.0)
    chi2 = np.maximum(nobs * gain, 0.0)
    lr = np.maximum(nobs * np.log(r / u), 0.0)
    pf = fdtrc(L, df, F)
    pp = np.stack([pf, chdtrc(L, chi2), chdtrc(L, lr), pf], axis=-1)
    p = np.full((n, n, maxlag, 4), np.nan)
    p[off] = pp
    value = pp.mean(axis=-1) if test is None else pp[..., TESTS.index(test)]
    adj = np.zeros((n, n))
    adj[off] = (value < p_val_threshold).any(axis=-1)
    return adj, p


def _engine_stats(data, maxlag: int):
    from ..engine import get_engine
    X = data.to_numpy() if hasattr(data, "to_numpy") else np.asarray(data)
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("granger: data must be T x n")
    T, n = X.shape
    if n < 2:        # no ordered pair: the reference's loops run no test (granger.py:13-16)
        return {k: np.zeros((n, n, maxlag), d) for k, d in (("ssr_r", float), ("ssr_u", float), ("tss", float),
                                                            ("rank", np.int32), ("status", np.int32))}, T
    if T <= 3 * maxlag + 1:
        raise ValueError(f"Insufficient observations. Maximum allowable lag is {int((T - 1) / 3) - 1}")
    return get_engine().granger(X, maxlag=maxlag), T


def granger_pvalues(data, maxlag: int = 3):
    """n x n x maxlag x 4 p-values (``TESTS`` order; item [i, j]: does column j cause column i);
    NaN on the diagonal."""
    out, T = _engine_stats(data, maxlag)
    return granger_from_stats(out["ssr_r"], out["ssr_u"], out["tss"], out["rank"], out["status"], T, maxlag)[1]


def granger(data, maxlag=None, p_val_threshold=0.05, test=None):
    """``granger.py:4-35``: n x n float adjacency, ``adj[i, j] = 1`` iff column j Granger-causes
    column i at some lag 1..maxlag (default 3)."""
    assert test in [None, 'ssr_ftest', 'ssr_chi2test', 'lrtest', 'params_ftest']
    if maxlag is None:
        maxlag = 3
    out, T = _engine_stats(data, maxlag)
    return granger_from_stats(out["ssr_r"], out["ssr_u"], out["tss"], out["rank"], out["status"], T, maxlag,
                              p_val_threshold, test)[0]


__all__ = ["TESTS", "fast_path_bound", "fast_path_guards", "granger", "granger_from_stats", "granger_pvalues"]
