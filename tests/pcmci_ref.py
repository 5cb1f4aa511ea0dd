"""CPU restatement of the PCMCI contract (helper, not a test).

Written loop for loop from the semantics of tigramite 4.2.2.1 [U] as RCAEval's
``graph_construction/pcmci.py`` and ``e2e/microcause.py`` use it: ``ParCorr`` with analytic
significance on freshly gathered lagged arrays (standardize, two ``numpy.linalg.lstsq`` residuals,
Pearson r, Student-t tail), ``run_pc_stable`` with ``max_combinations = 1`` and ``run_mci`` with the
default ``cut_off='2xtau_max'`` window, and pingouin 0.5.3 ``partial_corr`` [U] for microcause's Q
matrix. Nothing here comes from the engine's correlation-matrix formulation. Every ParCorr value
is computed a second time from a Householder QR of Z (``numpy.linalg.qr``); the largest difference
between the two solves over a run is the restatement's own uncertainty ``delta``.
"""
import functools
import time

import numpy as np
from scipy import stats

EPS = float(np.finfo(np.float64).eps)


# ---- input ------------------------------------------------------------------------------------
def gen_var(T, n, tau_max, seed):
    """A sparse stable VAR: own lag-1 coefficient 0.6, and for every column j >= 1 one cross link
    +-0.35 from a random column i < j at a random lag in 1..tau_max (a triangular system, so it
    is stable whatever the draw), unit Gaussian noise, 200 rows of burn-in dropped."""
    rng = np.random.default_rng(seed)
    links = []
    for j in range(1, n):
        links.append((int(rng.integers(0, j)), j, int(rng.integers(1, tau_max + 1)),
                      0.35 * (1.0 if rng.random() < 0.5 else -1.0)))
    burn = 200
    X = np.zeros((T + burn, n))
    e = rng.normal(size=(T + burn, n))
    for t in range(T + burn):
        X[t] = e[t]
        if t >= 1:
            X[t] += 0.6 * X[t - 1]
        for i, j, lag, c in links:
            if t >= lag:
                X[t, j] += c * X[t - lag, i]
    return np.ascontiguousarray(X[burn:])


def gen_collinear(T, n, seed):
    """Doubly integrated noise: neighbouring lags of a column are nearly collinear."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.cumsum(np.cumsum(rng.normal(size=(T, n)), axis=0), axis=0))


# ---- ParCorr ----------------------------------------------------------------------------------
def _column(X, node, tau_max):
    i, lag = node[0], -node[1]
    T = X.shape[0]
    return X[2 * tau_max - lag:T - lag, i].astype(np.float64)


class Run:
    """One input's tests: counts them, tracks the two-solve spread, flags constant windows."""

    def __init__(self, X, tau_max):
        self.X = np.asarray(X, dtype=np.float64)
        self.tau_max = int(tau_max)
        self.T_eff = self.X.shape[0] - 2 * self.tau_max
        self.delta = 0.0
        self.constant = False
        self.tests = 0

    def parcorr(self, x, y, Z):
        """(val, p, |Z|) of node x against node y given the node list Z."""
        self.tests += 1
        arr = np.array([_column(self.X, q, self.tau_max) for q in [x, y] + list(Z)])
        arr -= arr.mean(axis=1).reshape(-1, 1)
        std = arr.std(axis=1)
        if (std == 0).any():
            self.constant = True
            return np.nan, np.nan, len(Z)
        arr /= std.reshape(-1, 1)
        xs, ys, z = arr[0], arr[1], arr[2:].T
        if z.shape[1] > 0:
            rx = xs - z @ np.linalg.lstsq(z, xs, rcond=None)[0]
            ry = ys - z @ np.linalg.lstsq(z, ys, rcond=None)[0]
            q, _ = np.linalg.qr(z)
            rx2 = xs - q @ (q.T @ xs)
            ry2 = ys - q @ (q.T @ ys)
            rx2 = rx2 - q @ (q.T @ rx2)          # second pass: orthogonal to working precision
            ry2 = ry2 - q @ (q.T @ ry2)
        else:
            rx, ry, rx2, ry2 = xs, ys, xs, ys
        val = float(stats.pearsonr(rx, ry)[0])
        val2 = float(stats.pearsonr(rx2, ry2)[0])
        self.delta = max(self.delta, abs(val - val2))
        return val, pvalue(val, self.T_eff, len(Z)), len(Z)


def pvalue(val, T_eff, dim_z):
    deg_f = T_eff - (2 + dim_z)
    if deg_f < 1:
        return np.nan
    if abs(abs(val) - 1.0) <= EPS:
        return 0.0
    return float(2.0 * stats.t.sf(abs(val) * np.sqrt(deg_f / (1.0 - val * val)), deg_f))


# ---- PC1 --------------------------------------------------------------------------------------
def pc1_target(run, j, n, pc_alpha):
    """run_pc_stable for target j: dict parents (ordered), val_min (same order), levels, tests,
    ps (every p met) and sorts (the val_min sequence of every sort, descending)."""
    tau_max = run.tau_max
    parents = [(i, -lag) for i in range(n) for lag in range(1, tau_max + 1)]
    val_min = {q: np.inf for q in parents}
    levels, tests, ps, sorts, zmax = 0, 0, [], [], 0
    d = 0
    while True:
        if len(parents) - 1 < d:
            break
        levels += 1
        nonsig = []
        for parent in parents:
            Z = [q for q in parents if q != parent][:d]
            val, p, dz = run.parcorr(parent, (j, 0), Z)
            tests += 1
            zmax = max(zmax, dz)
            ps.append(p)
            val_min[parent] = min(abs(val), val_min[parent])
            if p > pc_alpha:
                nonsig.append(parent)
        for q in nonsig:
            parents.remove(q)
        keys = [val_min[q] for q in parents]
        order = sorted(range(len(parents)), key=lambda k: keys[k], reverse=True)      # stable
        parents = [parents[k] for k in order]
        sorts.append([keys[k] for k in order])
        d += 1
    return {"parents": parents, "val_min": [val_min[q] for q in parents], "levels": levels, "tests": tests,
            "ps": ps, "sorts": sorts, "zmax": zmax}


# ---- MCI --------------------------------------------------------------------------------------
def mci(run, parents, n):
    """run_mci with tau_min = 0: val_matrix, p_matrix, dim_matrix (|Z|; -1 untested), n x n x (tau_max + 1)."""
    tau_max = run.tau_max
    val = np.zeros((n, n, tau_max + 1))
    p = np.ones((n, n, tau_max + 1))
    dim = np.full((n, n, tau_max + 1), -1, dtype=np.int64)
    for j in range(n):
        for i in range(n):
            for tau in range(tau_max + 1):
                if i == j and tau == 0:
                    continue
                Z = [q for q in parents[j] if q != (i, -tau)]
                for k, neg in parents[i]:
                    q = (k, neg - tau)
                    if q not in Z:
                        Z.append(q)
                val[i, j, tau], p[i, j, tau], dim[i, j, tau] = run.parcorr((i, -tau), (j, 0), Z)
    return val, p, dim


def adjacency(p_matrix):
    """pcmci.py:83-97: min over tau, rounded to 3 decimals, an edge wherever it is non-zero."""
    link = np.around(p_matrix.min(axis=2), 3)
    n = link.shape[0]
    adj = np.zeros((n, n), dtype=np.int64)
    for cause, effect in zip(*np.where(link)):
        adj[cause, effect] = 1
    return adj, link


@functools.lru_cache(maxsize=None)
def case(T, n, tau_max, pc_alpha, seed, kind="var"):
    """The restatement's whole PCMCI run on one generated input, computed once and shared; callers
    must not change it."""
    X = gen_var(T, n, tau_max, seed) if kind == "var" else gen_collinear(T, n, seed)
    return run_pcmci(X, tau_max, pc_alpha)


def run_pcmci(X, tau_max, pc_alpha):
    n = X.shape[1]
    t0 = time.perf_counter()
    run = Run(X, tau_max)
    pc1 = [pc1_target(run, j, n, pc_alpha) for j in range(n)]
    parents = [r["parents"] for r in pc1]
    val, p, dim = mci(run, parents, n)
    adj, link = adjacency(p)
    return {"X": X, "tau_max": tau_max, "pc_alpha": pc_alpha, "T_eff": run.T_eff, "pc1": pc1, "parents": parents,
            "val_matrix": val, "p_matrix": p, "dim_matrix": dim, "adj": adj, "link": link, "delta": run.delta,
            "constant": run.constant, "seconds": time.perf_counter() - t0}


def preconditions(ref, tol):
    """The smallest margins of a run, for the tests' preconditions: rel_p, the closest relative
    distance of a PC1 p to pc_alpha or of a final p to 0.001 / 0.0005; gap, the smallest difference
    of consecutive sorted val_min values; zmax, the largest |Z|."""
    rel = np.inf
    for r in ref["pc1"]:
        ps = np.asarray(r["ps"], dtype=np.float64)
        rel = min(rel, float(np.nanmin(np.abs(ps - ref["pc_alpha"]) / ref["pc_alpha"])))
    tested = ref["dim_matrix"] >= 0
    pm = ref["p_matrix"][tested]
    link = ref["p_matrix"].min(axis=2).ravel()
    for thr, arr in ((0.001, pm), (0.0005, link)):
        rel = min(rel, float(np.nanmin(np.abs(arr - thr) / thr)))
    gap = np.inf
    for r in ref["pc1"]:
        for s in r["sorts"]:
            if len(s) > 1:
                gap = min(gap, float(np.min(-np.diff(np.asarray(s)))))
    zmax = max(int(ref["dim_matrix"].max()), max(r["zmax"] for r in ref["pc1"]))
    return {"rel_p": rel, "gap": gap, "zmax": zmax, "ok_gap": gap >= 1e3 * tol}


# ---- microcause -------------------------------------------------------------------------------
def significant_graph(p_matrix, alpha_level=0.001):
    """return_significant_links(include_lagzero_links=False) then get_links: for every target j and
    every (i, -tau), tau >= 1, with p <= alpha_level, the edge j -> i. Dense adjacency g[u, v]."""
    n = p_matrix.shape[0]
    g = np.zeros((n, n), dtype=np.int64)
    for j in range(n):
        for i in range(n):
            for tau in range(1, p_matrix.shape[2]):
                if p_matrix[i, j, tau] <= alpha_level:
                    g[j, i] = 1
    return g


def partial_corr(data, x, y, covar):
    """pingouin 0.5.3 partial_corr(method='pearson').r [U]."""
    cols = [x, y] + list(covar)
    V = np.cov(data[:, cols], rowvar=False, ddof=1)
    V = np.atleast_2d(V)
    Vi = np.linalg.pinv(V, hermitian=True)
    D = np.diag(np.sqrt(1.0 / Vi.diagonal()))
    pcor = -1.0 * (D @ Vi @ D)
    return float(pcor[0, 1])


def q_matrix(data, g, fe, rho=0.2):
    """get_Q_matrix_part_corr: g dense adjacency (g[u, v]: edge u -> v), fe the frontend's index."""
    n = g.shape[0]
    edges = [(u, v) for u in range(n) for v in range(n) if g[u, v]]
    pa = {v: set() for v in range(n)}
    for u, v in edges:
        if u != v:
            pa[v].add(u)

    def part(x, y):
        cond = pa[fe].difference([y]).union(pa[y])
        cond.discard(x)
        cond.discard(y)
        return abs(partial_corr(data, x, y, sorted(cond)))

    Q = np.zeros((n, n))
    for u, v in edges:
        if u == v:
            continue
        if fe != u:
            Q[v, u] = part(fe, u)
        if not g[v, u] and fe != v:
            Q[u, v] = rho * part(fe, v)
    for i in range(n):
        pmax = [part(fe, k) for k in np.nonzero(g[:, i])[0] if fe != k]
        pmax = np.max(pmax) if len(pmax) > 0 else 0
        if fe != i:
            q = part(fe, i)
            Q[i, i] = q - pmax if q > pmax else 0
    scale = [1.0 / s if s > 0 else 0.0 for s in np.sum(Q, axis=1)]
    return np.dot(np.diag(scale), Q)


def randomwalk(P, epochs, start_node, walk_step):
    """microcause.py:2148-2175 with the literal np.random.choice; start_node is 1-based."""
    n = P.shape[0]
    score = np.zeros([n])
    for _ in range(epochs):
        current = start_node - 1
        for _ in range(walk_step):
            if np.sum(P[current]) == 0:
                break
            nxt = np.random.choice(range(n), p=P[current])
            score[nxt] += 1
            current = nxt
    out = list(zip(range(n), score))
    out.sort(key=lambda x: x[1], reverse=True)
    return out


def microcause_ranks(data, names, p_matrix, sli, epochs=1000, walk_step=1000):
    """Steps 3-8 of microcause on preprocessed data and a PCMCI p_matrix; draws from numpy's global state."""
    g = significant_graph(p_matrix, 0.001)
    fe = names.index(sli)
    Q = q_matrix(np.asarray(data, dtype=np.float64), g, fe, 0.2)
    vis = randomwalk(Q, epochs, fe + 1, walk_step)
    eta = np.ones(len(names))
    gamma = [0.0] * len(names)
    vmax = np.max([v for _, v in vis])
    for k, v in vis:
        gamma[k] = 0.5 * v / vmax + 0.5 * eta[k] / np.max(eta)
    order = sorted(zip(range(len(names)), gamma), key=lambda x: x[1], reverse=True)
    return {"adj": g, "Q": Q, "ranks": [names[k] for k, _ in order]}
