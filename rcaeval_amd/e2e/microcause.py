"""``microcause`` — mirror of ``RCAEval/e2e/microcause.py:2178-2364`` on the MI355X engine:
preprocess -> PCMCI (``tau_max=10, pc_alpha=0.1``, the engine's ``pcg_pcmci_*``) -> the links with
``p_matrix <= 0.001`` at lags >= 1, added as ``get_links`` adds them (the edge j -> i for a parent
(i, -tau) of j) -> ``get_Q_matrix_part_corr`` (pingouin 0.5.3 ``partial_corr`` [U]: a Pearson
partial correlation through ``pinv`` of the covariance of ``[x, y] + covar``; ``rho = 0.2``) ->
``randomwalk(Q, 1000, frontend, walk_step=1000)`` -> ``gamma`` with ``eta = 1``, ``lambda = 0.5`` ->
the ranking. Q and the walk are host numpy (n is tens). Each step of the walk takes one
``np.random.random_sample()`` from numpy's global state and ``searchsorted(cdf, u, side='right')``
on the normalised cumulative row, which is what the reference's legacy
``np.random.choice(range(n), p=P[current])`` does: ``np.random.seed(s)`` reproduces its walk.

As in the reference the method carries no ``@rca``: a missing ``sli`` raises. The SPOT code of the
reference is dead (``eta`` is all ones) and is not built. ``epochs`` and ``walk_step`` are additive
keyword arguments."""
from __future__ import annotations

import numpy as np

from ..graph_construction.pcmci import run_pcmci
from ..io.time_series import preprocess


def significant_graph(p_matrix, alpha_level: float = 0.001) -> np.ndarray:
    """``return_significant_links(include_lagzero_links=False)`` then ``get_links``: dense adjacency
    ``g[j, i] = 1`` for every (i, -tau), tau >= 1, with ``p_matrix[i, j, tau] <= alpha_level``."""
    sig = np.asarray(p_matrix) <= alpha_level
    sig[:, :, 0] = False
    return np.ascontiguousarray(sig.any(axis=2).T).astype(np.int64)


def partial_corr(data, x: int, y: int, covar) -> float:
    """pingouin 0.5.3 ``partial_corr(method='pearson').r`` [U] on the columns of ``data``."""
    V = np.atleast_2d(np.cov(data[:, [x, y] + list(covar)], rowvar=False, ddof=1))
    Vi = np.linalg.pinv(V, hermitian=True)
    D = np.diag(np.sqrt(1.0 / Vi.diagonal()))
    return float((-1.0 * (D @ Vi @ D))[0, 1])


def q_matrix(data, g, fe: int, rho: float = 0.2) -> np.ndarray:
    """``get_Q_matrix_part_corr`` (``microcause.py:2192-2278``): ``g[u, v]`` is the edge u -> v,
    ``fe`` the frontend's column."""
    data = np.asarray(data, dtype=np.float64)
    n = g.shape[0]
    edges = [(int(u), int(v)) for u, v in zip(*np.nonzero(g))]
    pa_set = {v: set() for v in range(n)}
    for u, v in edges:
        if u != v:
            pa_set[v].add(u)
    cache: dict = {}

    def get_part_corr(x, y):
        if y not in cache:
            cond = pa_set[fe].difference([y]).union(pa_set[y])
            cond.discard(x)
            cond.discard(y)
            cache[y] = abs(partial_corr(data, x, y, sorted(cond)))
        return cache[y]

    Q = np.zeros([n, n])
    for u, v in edges:
        if u == v:
            continue
        if fe != u:                                    # forward step
            Q[v, u] = get_part_corr(fe, u)
        if not g[v, u] and fe != v:                    # backward step
            Q[u, v] = rho * get_part_corr(fe, v)
    for i in range(n):
        P_pc_max = [get_part_corr(fe, int(k)) for k in np.nonzero(g[:, i])[0] if fe != k]
        P_pc_max = np.max(P_pc_max) if len(P_pc_max) > 0 else 0
        if fe != i:
            q_ii = get_part_corr(fe, i)
            Q[i, i] = q_ii - P_pc_max if q_ii > P_pc_max else 0
    scale = [1.0 / s if s > 0 else 0.0 for s in np.sum(Q, axis=1)]
    return np.dot(np.diag(scale), Q)


def randomwalk(P, epochs: int, start_node: int, walk_step: int = 50):
    """``microcause.py:2148-2175`` (``start_node`` is 1-based): the visit counts as a list of
    (node, count) sorted by count, descending."""
    P = np.asarray(P, dtype=np.float64)
    n = P.shape[0]
    live = P.sum(axis=1) != 0
    cdf = np.cumsum(P, axis=1)
    cdf[live] /= cdf[live, -1:]
    score = np.zeros([n])
    draw = np.random.random_sample
    for _ in range(epochs):
        current = start_node - 1
        for _ in range(walk_step):
            if not live[current]:
                break
            current = int(cdf[current].searchsorted(draw(), side="right"))
            score[current] += 1
    score_list = list(zip(range(n), score))
    score_list.sort(key=lambda x: x[1], reverse=True)
    return score_list


def ranks_from_p(data, node_names, p_matrix, sli, epochs: int = 1000, walk_step: int = 1000) -> dict:
    """Steps 3-8 of the method on the preprocessed array and PCMCI's p_matrix."""
    g = significant_graph(p_matrix, alpha_level=0.001)
    frontend = node_names.index(sli) + 1
    Q = q_matrix(data, g, frontend - 1, rho=0.2)
    vis_list = randomwalk(Q, epochs, frontend, walk_step=walk_step)
    eta = np.ones([len(node_names)])
    gamma = [0 for _ in range(len(node_names))]
    with np.errstate(divide="ignore", invalid="ignore"):
        max_vis_time = np.max([i[1] for i in vis_list])
        for k, vis in vis_list:
            gamma[k] = 0.5 * vis / max_vis_time + (1 - 0.5) * eta[k] / np.max(eta)
    score_list = sorted(zip(range(len(node_names)), gamma), key=lambda x: x[1], reverse=True)
    return {"adj": g, "Q": Q, "node_names": node_names, "ranks": [node_names[k] for k, _ in score_list]}


def microcause(data, inject_time=None, dataset=None, num_loop=None, sli=None, epochs=1000, walk_step=1000, **kwargs):
    data = preprocess(data=data, dataset=dataset, dk_select_useful=kwargs.get("dk_select_useful", False))
    np_data = data.to_numpy().astype(float)
    node_names = data.columns.to_list()
    node_names.index(sli)                              # a missing sli raises here, as in the reference
    res = run_pcmci(np_data, tau_max=10, pc_alpha=0.1)
    out = ranks_from_p(np_data, node_names, res["p_matrix"], sli, epochs=epochs, walk_step=walk_step)
    return {"adj": out["adj"], "node_names": node_names, "ranks": out["ranks"]}
