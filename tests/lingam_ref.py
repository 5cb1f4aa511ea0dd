"""CPU restatement of the DirectLiNGAM contract (helper, not a test).

Written loop for loop from the semantics of causal-learn 0.1.3.3 ``DirectLiNGAM`` [U] (measure
'pwling', no prior knowledge) — ``_residual``, ``_entropy``, ``_diff_mutual_info``,
``_search_causal_order`` and ``fit`` — with numpy's own ``np.cov`` / ``np.var`` / ``np.std`` / ``np.mean`` /
``np.min`` / ``np.argmax``, and not from the engine's three-pass formulation. ``dtype=np.longdouble``
repeats the same arithmetic in extended precision; the difference between the two on an input is
the restatement's own rounding spread.
"""
import numpy as np


def _residual(a, b, lsq=False):
    """The residual when a is regressed on b. ``lsq`` swaps in the least-squares coefficient
    (cov and var on the same ddof) that the reference does *not* use."""
    if lsq:
        return a - (np.cov(a, b, ddof=0)[0, 1] / np.var(b)) * b
    return a - (np.cov(a, b)[0, 1] / np.var(b)) * b


def _entropy(u):
    k1 = 79.047
    k2 = 7.4129
    gamma = 0.37457
    return (1 + np.log(2 * np.pi)) / 2 - k1 * (np.mean(np.log(np.cosh(u))) - gamma) ** 2 \
        - k2 * (np.mean(u * np.exp((-(u ** 2)) / 2))) ** 2


def _diff_mutual_info(xi_std, xj_std, ri_j, rj_i):
    return (_entropy(xj_std) + _entropy(ri_j / np.std(ri_j))) - (_entropy(xi_std) + _entropy(rj_i / np.std(rj_i)))


def pair_scores(X_, dtype=np.float64, lsq=False):
    """One search step over all columns of X_ (the search's ``U`` is every column): D (m x m, zero
    diagonal) and M (m), both in ``dtype``. Every ordered pair is evaluated, as the reference does."""
    with np.errstate(all="ignore"):
        X_ = np.asarray(X_, dtype=dtype)
        m = X_.shape[1]
        D = np.zeros((m, m), dtype=dtype)
        M = np.zeros(m, dtype=dtype)
        for i in range(m):
            acc = 0
            for j in range(m):
                if i == j:
                    continue
                xi_std = (X_[:, i] - np.mean(X_[:, i])) / np.std(X_[:, i])
                xj_std = (X_[:, j] - np.mean(X_[:, j])) / np.std(X_[:, j])
                ri_j = _residual(xi_std, xj_std, lsq)
                rj_i = _residual(xj_std, xi_std, lsq)
                D[i, j] = _diff_mutual_info(xi_std, xj_std, ri_j, rj_i)
                acc += np.min([0, D[i, j]]) ** 2
            M[i] = -1.0 * acc
        return D, M


def order(X, dtype=np.float64):
    """``fit``'s search: (K, Ms, snaps). K is the causal order; Ms[s] the step's M as an array over
    the original columns (-inf for columns ordered earlier, 0 for the last step's lone candidate);
    snaps[s] the working copy X_ at the start of step s (all n columns)."""
    with np.errstate(all="ignore"):
        X = np.asarray(X, dtype=dtype)
        n = X.shape[1]
        U = np.arange(n)
        K, Ms, snaps = [], [], []
        X_ = np.copy(X)
        for _ in range(n):
            snaps.append(X_.copy())
            row = np.full(n, -np.inf, dtype=dtype)
            if len(U) == 1:
                m = U[0]
                row[m] = 0
            else:
                _, M = pair_scores(X_[:, U], dtype)
                row[U] = M
                m = U[np.argmax(M)]
            for i in U:
                if i != m:
                    X_[:, i] = _residual(X_[:, i], X_[:, m])
            K.append(int(m))
            U = U[U != m]
            Ms.append(row)
        return K, Ms, snaps


# ---- generators ---------------------------------------------------------------------------------
def sem(T, n, seed, noise):
    """A random lower-triangular linear SEM (edge probability 0.4, weights +-U(0.5, 1.5)) with
    ``noise`` in 'uniform', 'laplace', 'gauss', columns permuted. Returns (X, B, perm): column c of
    X is variable perm[c]; B[a, b] != 0 is the edge b -> a between variables (b < a)."""
    rng = np.random.default_rng(seed)
    B = np.tril((rng.random((n, n)) < 0.4) * rng.uniform(0.5, 1.5, (n, n)) * rng.choice([-1.0, 1.0], (n, n)), -1)
    if noise == "uniform":
        E = rng.uniform(-1.0, 1.0, (T, n))
    elif noise == "laplace":
        E = rng.laplace(0.0, 1.0, (T, n))
    else:
        E = rng.normal(0.0, 1.0, (T, n))
    V = np.zeros((T, n))
    for a in range(n):
        V[:, a] = V[:, :a] @ B[a, :a] + E[:, a]
    perm = rng.permutation(n)
    return np.ascontiguousarray(V[:, perm]), B, perm


GENERATORS = {
    "uniform": lambda T, n, seed: sem(T, n, seed, "uniform")[0],
    "laplace": lambda T, n, seed: sem(T, n, seed, "laplace")[0],
    "gauss": lambda T, n, seed: sem(T, n, seed, "gauss")[0],      # unidentifiable: near-tied scores
}


def collinear(X, eps):
    """X with its last column set to the first + eps * itself (n >= 2)."""
    Y = np.array(X, dtype=np.float64)
    Y[:, -1] = Y[:, 0] + eps * Y[:, -1]
    return Y
