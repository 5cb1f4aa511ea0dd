"""``pc_pagerank`` — mirror of ``RCAEval/e2e/pc_pagerank.py:12-40`` on the MI355X engine.

preprocess -> ``pc(data.to_numpy())`` with causal-learn defaults (alpha 0.05, fisherz,
stable, uc_priority 2) -> directed graph from endpoint codes (``:20-27``) -> isolated nodes
dropped, remaining nodes sorted (``:28``) -> dense matrix as networkx 2.5
``to_numpy_matrix`` (``:29``) -> GPU PageRank on its transpose (``:31-32``) -> scores zipped
with the *unfiltered* ``node_names`` (``:33``: names and scores misalign, and the list is
truncated, whenever a node is isolated — reproduced on purpose) -> stable descending sort.

``cmlp_pagerank`` — mirror of ``:43-63``: preprocess -> ``cmlp(data, max_iter=20000)`` (the int
Granger-causality matrix of the trained cMLP, ``graph_construction/cmlp.py``) -> GPU PageRank on
its transpose -> scores zipped with ``node_names`` -> stable descending sort.
"""
from __future__ import annotations

import numpy as np

from ..causal import pc
from ..graph_heads.page_rank import PageRank
from ..io.time_series import preprocess
from ..phases import phase
from . import rca


def digraph_matrix(adj: np.ndarray):
    """(matrix, nodes) for ``pc_pagerank.py:20-29``: edge i->j when adj[i,j] == -1 or
    adj[j,i] == 1; nodes = sorted non-isolated; M[a,b] = 1.0 iff nodes[a] -> nodes[b]."""
    adj = np.asarray(adj)
    E = (adj == -1) | (adj == 1).T
    nodes = np.nonzero(E.any(axis=0) | E.any(axis=1))[0]
    M = E[np.ix_(nodes, nodes)].astype(np.float64)
    return M, [int(v) for v in nodes]


@rca
def pc_pagerank(data, inject_time=None, dataset=None, dk_select_useful=False, with_bg=False, n_iter=10,
                **kwargs):
    with phase("preprocess"):
        data = preprocess(data=data, dataset=dataset, dk_select_useful=dk_select_useful)
        node_names = data.columns.to_list()
        X = data.to_numpy()
    cg = pc(X)
    with phase("digraph"):
        M, _nodes = digraph_matrix(cg.G.graph)
    with phase("pagerank"):
        scores = PageRank().fit_transform(M.T)
    with phase("rank sort"):
        ranked = sorted(zip(node_names, scores), key=lambda t: t[1], reverse=True)
    return {"adj": M, "node_names": node_names, "ranks": [name for name, _ in ranked]}


@rca
def cmlp_pagerank(data, inject_time=None, dataset=None, dk_select_useful=False, with_bg=False, n_iter=10,
                  **kwargs):
    from ..graph_construction.cmlp import cmlp
    with phase("preprocess"):
        data = preprocess(data=data, dataset=dataset, dk_select_useful=dk_select_useful)
        node_names = data.columns.to_list()
    adj = cmlp(data, max_iter=20000)
    with phase("pagerank"):
        scores = PageRank().fit_transform(adj.T)
    with phase("rank sort"):
        ranked = sorted(zip(node_names, scores), key=lambda t: t[1], reverse=True)
    return {"adj": adj, "node_names": node_names, "ranks": [name for name, _ in ranked]}


def pc_pagerank_batch(cases, dataset=None, dk_select_useful=False, **kwargs) -> list:
    """``[pc_pagerank(data, inject_time, dataset=dataset) for (data, inject_time) in cases]`` with
    the PC runs of all cases batched (``causal.pc_batch``: one K1 launch, one skeleton launch, one
    host wait). ``cases``: data frames, or (data, inject_time) pairs. Preprocessing, the digraph,
    PageRank and the rank sort stay per case, as in ``pc_pagerank``. A case whose preprocessing
    or PC raises goes through ``pc_pagerank`` itself, i.e. the ``@rca`` wrapper's route (dummy
    ranks for data errors, engine faults propagate)."""
    from ..causal import pc_batch
    items = [c if isinstance(c, (tuple, list)) else (c, None) for c in cases]
    out: list = [None] * len(items)
    pre = []
    for i, (data, _inject) in enumerate(items):
        try:
            with phase("preprocess"):
                d = preprocess(data=data, dataset=dataset, dk_select_useful=dk_select_useful)
                pre.append((i, d.columns.to_list(), d.to_numpy()))
        except Exception:      # noqa: BLE001 - pc_pagerank below repeats it under @rca
            pass
    cgs = pc_batch([X for _, _, X in pre], return_exceptions=True) if pre else []
    for (i, node_names, _X), cg in zip(pre, cgs):
        if isinstance(cg, Exception):
            continue
        try:
            with phase("digraph"):
                M, _nodes = digraph_matrix(cg.G.graph)
            with phase("pagerank"):
                scores = PageRank().fit_transform(M.T)
            with phase("rank sort"):
                ranked = sorted(zip(node_names, scores), key=lambda t: t[1], reverse=True)
            out[i] = {"adj": M, "node_names": node_names, "ranks": [name for name, _ in ranked]}
        except Exception:      # noqa: BLE001
            out[i] = None
    for i, (data, inject) in enumerate(items):
        if out[i] is None:
            out[i] = pc_pagerank(data, inject, dataset=dataset, dk_select_useful=dk_select_useful, **kwargs)
    return out
