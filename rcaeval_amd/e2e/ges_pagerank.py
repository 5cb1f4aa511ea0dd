"""``fges_pagerank`` / ``fges_randomwalk`` — mirrors of ``RCAEval/e2e/ges_pagerank.py:30-67`` on the
MI355X engine: preprocess -> ``fges(data)`` (linear-Gaussian score, ``graph_construction/fges.py``)
-> the ranking head on ``adj.T``, sorted by score afterwards as the reference does. ``ges_pagerank``
(causal-learn's GES) is not served."""
from __future__ import annotations

from ..graph_construction.fges import fges
from ..graph_heads.page_rank import page_rank
from ..graph_heads.random_walk import random_walk
from ..io.time_series import preprocess
from . import rca


@rca
def fges_pagerank(data, inject_time=None, dataset=None, dk_select_useful=False, with_bg=False, n_iter=10, **kwargs):
    data = preprocess(data=data, dataset=dataset, dk_select_useful=dk_select_useful)
    node_names = data.columns.to_list()
    adj = fges(data)
    ranks = page_rank(adj.T, node_names=node_names, n_iter=n_iter)
    ranks = sorted(ranks, key=lambda x: x[1], reverse=True)
    return {"adj": adj, "node_names": node_names, "ranks": [x[0] for x in ranks]}


@rca
def fges_randomwalk(data, inject_time=None, dataset=None, n_iter=None, **kwargs):
    data = preprocess(data=data, dataset=dataset, dk_select_useful=kwargs.get("dk_select_useful", False))
    node_names = data.columns.to_list()
    if n_iter is None:
        n_iter = len(node_names)
    adj = fges(data)
    ranks = random_walk(adj.T, node_names, num_loop=n_iter)
    ranks = sorted(ranks, key=lambda x: x[1], reverse=True)
    return {"adj": adj, "node_names": node_names, "ranks": [x[0] for x in ranks]}
