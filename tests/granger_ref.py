"""CPU restatement of the Granger contract (helper, not a test).

Written from the semantics of statsmodels 0.14.0 ``grangercausalitytests`` [U] as RCAEval's
``graph_construction/granger.py`` uses it — explicit design matrices, ``numpy.linalg.pinv`` for the
OLS fits, ``numpy.linalg.matrix_rank`` for the degrees of freedom, the four tests — and not from
the engine's moment / Cholesky formulation. ``solve="lstsq"`` repeats every fit with
``numpy.linalg.lstsq``; the spread between the two solves on an input is the restatement's own
uncertainty (``spread``).
"""
import numpy as np
from scipy import stats

TESTS = ("ssr_ftest", "ssr_chi2test", "lrtest", "params_ftest")
EPS = float(np.finfo(np.float64).eps)


def _lagmat(c, L):
    """Columns c_{t-1} .. c_{t-L} over t = L..T-1."""
    T = len(c)
    return np.column_stack([c[L - k:T - k] for k in range(1, L + 1)])


def _fit(A, y, solve):
    if solve == "pinv":
        beta = np.linalg.pinv(A) @ y
    else:
        beta = np.linalg.lstsq(A, y, rcond=None)[0]
    res = y - A @ beta
    return beta, float(res @ res)


def pair_lag(y, x, L, solve="pinv"):
    """One (caused y, causing x, lag L) item: dict of ssr_r, ssr_u, tss, rank, nobs, df, the
    statistics F, chi2, lr, wald and the four p-values ``p`` (TESTS order). Raises ValueError
    where the reference raises InfeasibleTestError."""
    T = len(y)
    nobs = T - L
    y0 = y[L:]
    ylags, xlags = _lagmat(y, L), _lagmat(x, L)
    one = np.ones((nobs, 1))
    own = np.column_stack([ylags, one])
    joint = np.column_stack([ylags, xlags, one])
    if (np.ptp(joint[:, :-1], axis=0) == 0).any():
        raise ValueError("constant lagged column")
    _, ssr_r = _fit(own, y0, solve)
    beta, ssr_u = _fit(joint, y0, solve)
    yc = y0 - y0.mean()
    tss = float(yc @ yc)
    if tss == 0 or ssr_u == 0 or ssr_u / tss < EPS:
        raise ValueError("perfect fit")
    rank = int(np.linalg.matrix_rank(joint))
    df = nobs - rank
    F = (ssr_r - ssr_u) / ssr_u / L * df
    chi2 = nobs * (ssr_r - ssr_u) / ssr_u
    lr = nobs * np.log(ssr_r / ssr_u)
    if rank == joint.shape[1]:
        # Wald F that the L coefficients on x are zero: cov = scale * (A'A)^-1, scale = ssr_u / df
        cov = np.linalg.pinv(joint.T @ joint) * (ssr_u / df)
        b = beta[L:2 * L]
        wald = float(b @ np.linalg.solve(cov[L:2 * L, L:2 * L], b)) / L
    else:
        wald = F                 # a deficient design: the contract's identity wald == F
    p = np.array([stats.f.sf(F, L, df), stats.chi2.sf(chi2, L), stats.chi2.sf(lr, L), stats.f.sf(wald, L, df)])
    return {"ssr_r": ssr_r, "ssr_u": ssr_u, "tss": tss, "rank": rank, "nobs": nobs, "df": df, "F": F, "chi2": chi2,
            "lr": lr, "wald": wald, "p": p}


def all_pairs(X, maxlag=3, solve="pinv"):
    """Arrays over every ordered pair and lag of a T x n array, each n x n x maxlag (``p``:
    n x n x maxlag x 4), NaN / 0 on the diagonal. Raises ValueError where the reference's call does."""
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    if not np.isfinite(X).all():
        raise ValueError("non-finite input")
    if T <= 3 * maxlag + 1:
        raise ValueError("Insufficient observations")
    out = {k: np.full((n, n, maxlag), np.nan) for k in ("ssr_r", "ssr_u", "tss", "F", "chi2", "lr", "wald")}
    out["rank"] = np.zeros((n, n, maxlag), np.int32)
    out["p"] = np.full((n, n, maxlag, 4), np.nan)
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            for L in range(1, maxlag + 1):
                r = pair_lag(X[:, i], X[:, j], L, solve)
                for k in out:
                    out[k][i, j, L - 1] = r[k]
    return out


def values(p, test=None):
    """The per-lag value the reference thresholds: the mean of the four p-values, or one test's."""
    return p.mean(axis=-1) if test is None else p[..., TESTS.index(test)]


def adjacency(p, p_val_threshold=0.05, test=None):
    n = p.shape[0]
    off = ~np.eye(n, dtype=bool)
    adj = np.zeros((n, n))
    adj[off] = (values(p, test)[off] < p_val_threshold).any(axis=-1)
    return adj


def granger(X, maxlag=3, p_val_threshold=0.05, test=None):
    return adjacency(all_pairs(X, maxlag)["p"], p_val_threshold, test)


def spread(a, b, keys=("ratio", "F", "chi2", "lr")):
    """Largest relative difference between two solves' results, per quantity (ratio = ssr_r / ssr_u)."""
    n = a["ssr_r"].shape[0]
    off = ~np.eye(n, dtype=bool)
    out = {}
    for k in keys:
        va = (a["ssr_r"] / a["ssr_u"] if k == "ratio" else a[k])[off]
        vb = (b["ssr_r"] / b["ssr_u"] if k == "ratio" else b[k])[off]
        out[k] = float(np.max(np.abs(va - vb) / np.abs(va)))
    return out


# ---- the inputs of the GPU tests ----------------------------------------------------------------
def gen_var1(T, n, seed):
    rng = np.random.default_rng(seed)
    A = 0.5 * np.eye(n) + rng.uniform(-0.3, 0.3, (n, n)) / max(1.0, np.sqrt(n) / 2)
    X = np.zeros((T, n))
    e = rng.standard_normal((T, n))
    for t in range(1, T):
        X[t] = X[t - 1] @ A + e[t]
    return X


def gen_random_walk(T, n, seed):
    rng = np.random.default_rng(seed)
    return 1000.0 + np.cumsum(rng.standard_normal((T, n)), axis=0)


def gen_integrated2(T, n, seed):
    rng = np.random.default_rng(seed)
    return np.cumsum(np.cumsum(rng.standard_normal((T, n)), axis=0), axis=0)


GENERATORS = {"var1": gen_var1, "random_walk": gen_random_walk, "integrated2": gen_integrated2}
