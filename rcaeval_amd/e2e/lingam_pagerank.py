"""``micro_diag`` — mirror of ``RCAEval/e2e/lingam_pagerank.py:52-81`` on the MI355X engine:
preprocess -> ``DirectLiNGAM().fit`` -> ``adj.astype(bool).astype(int)`` -> ``page_rank``; an all-zero
``adj`` returns the node names in column order (``:66-72``). As in the reference it carries no
``@rca``: an exception propagates to the caller. ``lingam_pagerank`` (``:21-49``, ``ICALiNGAM``) is
not built."""
from __future__ import annotations

from ..graph_construction.lingam import DirectLiNGAM
from ..graph_heads.page_rank import page_rank
from ..io.time_series import preprocess


def micro_diag(data, inject_time=None, dataset=None, num_loop=None, sli=None, **kwargs):
    data = preprocess(data=data, dataset=dataset, dk_select_useful=kwargs.get("dk_select_useful", False))
    node_names = data.columns.to_list()
    model = DirectLiNGAM()
    model.fit(data.to_numpy().astype(float))
    adj = model.adjacency_matrix_
    adj = adj.astype(bool).astype(int)
    if adj.sum().sum() == 0:
        return {"adj": adj, "node_names": node_names, "ranks": node_names}
    ranks = page_rank(adj, node_names=node_names)
    ranks = sorted(ranks, key=lambda x: x[1], reverse=True)
    ranks = [x[0] for x in ranks]
    return {"adj": adj, "node_names": node_names, "ranks": ranks}
