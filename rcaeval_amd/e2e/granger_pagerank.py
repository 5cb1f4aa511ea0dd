"""``granger_pagerank`` — mirror of ``RCAEval/e2e/granger_pagerank.py:15-41`` on the MI355X engine:
preprocess -> ``granger(data)`` (maxlag 3, mean of the four tests' p-values against 0.05) ->
``page_rank(adj, node_names)`` on the float adjacency; an all-zero ``adj`` returns the node names
in column order (``:27-32``)."""
from __future__ import annotations

from ..graph_construction.granger import granger
from ..graph_heads.page_rank import page_rank
from ..io.time_series import preprocess
from . import rca


@rca
def granger_pagerank(data, inject_time=None, dataset=None, num_loop=None, sli=None, **kwargs):
    data = preprocess(data=data, dataset=dataset, dk_select_useful=kwargs.get("dk_select_useful", False))
    node_names = data.columns.to_list()
    adj = granger(data)
    if adj.sum().sum() == 0:
        return {"adj": adj, "node_names": node_names, "ranks": node_names}
    ranks = page_rank(adj, node_names=data.columns.to_list())
    ranks = sorted(ranks, key=lambda x: x[1], reverse=True)
    return {"adj": adj, "node_names": node_names, "ranks": [x[0] for x in ranks]}
