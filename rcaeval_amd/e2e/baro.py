"""``baro`` / ``robust_scaler`` / ``nsigma`` — mirror of ``RCAEval/e2e/__init__.py:83-170`` on the MI355X engine.

The reference splits the frame into the rows before and from the injection (``time <
inject_time`` / ``>=``, or ``head(anomalies[0])`` / the rest), preprocesses each half on its own
(``dk_select_useful`` from kwargs), keeps the columns both halves still have, in the normal
half's order, and per column fits ``RobustScaler()`` (baro) or ``StandardScaler()`` (nsigma) on
the normal rows, transforms the anomalous rows and scores the column by ``max``. Columns are
ranked by ``sorted(..., key=score, reverse=True)``, which is stable: ties keep column order. The
result has ``node_names`` and ``ranks`` and no ``adj``, and the methods carry no ``@rca`` wrapper.

Here the frame logic runs on the host line for line and every column of every case is scored by
one ``Engine.scaler_scores`` call (``pcg_scaler_batch``), bit for bit sklearn's values. A column
the device flags (status 1: a NaN or Inf, or a center / scale that overflowed) and a column of a
narrower float dtype (float32, float16: sklearn fits those in their own precision) are recomputed
on the host by sklearn itself, so any numeric input gives the reference's answer (or its
exception: sklearn refuses an infinity).

Empty inputs, as the reference has them:
* no common column: ``{"node_names": [], "ranks": []}`` (its loop does not run);
* a half without rows and ``dataset`` given: ``preprocess`` raises ``IndexError`` (``df.iloc[0]``
  of ``drop_constant``);
* a half without rows and ``dataset=None``: sklearn's ``ValueError`` ("Found array with 0
  sample(s)"), from ``fit`` for the normal half and from ``transform`` for the anomalous one.
"""
from __future__ import annotations

import numpy as np

from ..io.time_series import preprocess
from ..phases import phase

ROBUST, STANDARD = 0, 1


def split_frames(data, inject_time=None, dataset=None, anomalies=None, **kwargs):
    """(normal_df, anomal_df) of the reference: the window split, ``preprocess`` of each half and
    the column intersection in the normal frame's order (``e2e/__init__.py:84-103``)."""
    if anomalies is None:
        normal_df = data[data["time"] < inject_time]
        anomal_df = data[data["time"] >= inject_time]
    else:
        normal_df = data.head(anomalies[0])
        anomal_df = data.tail(len(data) - anomalies[0])
    normal_df = preprocess(data=normal_df, dataset=dataset, dk_select_useful=kwargs.get("dk_select_useful", False))
    anomal_df = preprocess(data=anomal_df, dataset=dataset, dk_select_useful=kwargs.get("dk_select_useful", False))
    intersects = [x for x in normal_df.columns if x in anomal_df.columns]
    return normal_df[intersects], anomal_df[intersects]


def _arrays(normal_df, anomal_df, mode):
    """(names, A, B, host): the halves as float64 arrays, and the positions of the columns the
    device does not take: sklearn fits a float32 / float16 column in its own precision, so such
    a column is scored by sklearn itself on the original values (float64, integer and bool columns
    reach sklearn as float64 and go to the device). A half without rows raises what sklearn raises."""
    names = normal_df.columns.to_list()
    who = "RobustScaler" if mode == ROBUST else "StandardScaler"
    for df in (normal_df, anomal_df):
        if names and len(df) == 0:
            raise ValueError(f"Found array with 0 sample(s) (shape=(0, 1)) while a minimum of 1 is required by {who}.")
    A = np.ascontiguousarray(normal_df.to_numpy(), dtype=np.float64).reshape(len(normal_df), len(names))
    B = np.ascontiguousarray(anomal_df.to_numpy(), dtype=np.float64).reshape(len(anomal_df), len(names))
    host = [j for j, (da, db) in enumerate(zip(normal_df.dtypes, anomal_df.dtypes))
            if any(getattr(d, "kind", "O") == "f" and d != np.float64 for d in (da, db))]
    return names, A, B, host


def device_scorer(pairs, mode) -> list:
    """The default scorer: ``Engine.scaler_scores`` on all pairs at once. The windows of every
    pair travel in one upload and are read in place as views of that buffer."""
    from ..engine import get_engine
    eng = get_engine()
    pairs = [(A, B) for A, B in pairs]
    if not pairs:
        return []
    flat = eng.to_device(np.concatenate([x.ravel() for pair in pairs for x in pair]))
    views, off = [], 0
    for A, B in pairs:
        pair = []
        for x in (A, B):
            pair.append(flat[off:off + x.size].view(x.shape[0], x.shape[1]))
            off += x.size
        views.append(tuple(pair))
    return eng.scaler_scores(views, mode)


def sklearn_column(a, b, mode):
    """One column's score by the reference's own statements (``e2e/__init__.py:108-113``)."""
    from sklearn.preprocessing import RobustScaler, StandardScaler
    scaler = (RobustScaler() if mode == ROBUST else StandardScaler()).fit(a.reshape(-1, 1))
    zscores = scaler.transform(b.reshape(-1, 1))[:, 0]
    return max(zscores)


def rank_cases(frames, mode, scorer=None) -> list:
    """The result dicts of several (normal_df, anomal_df) pairs scored in one ``scorer`` call.
    ``scorer(pairs, mode)`` takes the (A, B) float64 arrays of the cases that have columns and
    returns per pair a dict with the arrays ``score`` and ``status``; the default is the engine."""
    scorer = scorer or device_scorer
    cases = [_arrays(nd, ad, mode) for nd, ad in frames]
    live = [i for i, c in enumerate(cases) if c[0]]
    with phase("scaler scores"):
        scored = scorer([(cases[i][1], cases[i][2]) for i in live], mode) if live else []
    out = [{"node_names": c[0], "ranks": []} for c in cases]
    for i, res in zip(live, scored):
        names, A, B, host = cases[i]
        score = [float(v) for v in res["score"]]
        for j in np.flatnonzero(np.asarray(res["status"]) != 0):
            score[j] = sklearn_column(np.ascontiguousarray(A[:, j]), np.ascontiguousarray(B[:, j]), mode)
        for j in host:                                  # in the column's own dtype, as the reference
            score[j] = sklearn_column(frames[i][0].iloc[:, j].to_numpy(), frames[i][1].iloc[:, j].to_numpy(), mode)
        ranks = sorted(zip(names, score), key=lambda x: x[1], reverse=True)
        out[i]["ranks"] = [x[0] for x in ranks]
    return out


def _method(mode, data, inject_time, dataset, anomalies, kwargs):
    scorer = kwargs.pop("scorer", None)
    with phase("preprocess"):
        frames = split_frames(data, inject_time, dataset=dataset, anomalies=anomalies, **kwargs)
    return rank_cases([frames], mode, scorer)[0]


def nsigma(data, inject_time=None, dataset=None, num_loop=None, sli=None, anomalies=None, **kwargs):
    """``nsigma`` (``e2e/__init__.py:83-122``): columns ranked by their largest z-score."""
    return _method(STANDARD, data, inject_time, dataset, anomalies, kwargs)


def robust_scaler(data, inject_time=None, dataset=None, num_loop=None, sli=None, anomalies=None, **kwargs):
    """``robust_scaler`` = ``baro`` (``e2e/__init__.py:125-170``): columns ranked by their largest
    value scaled by the normal window's median and inter-quartile range."""
    return _method(ROBUST, data, inject_time, dataset, anomalies, kwargs)


baro = robust_scaler


def _batch(mode, cases, dataset, kwargs):
    scorer = kwargs.pop("scorer", None)
    anomalies = kwargs.pop("anomalies", None)
    items = [c if isinstance(c, (tuple, list)) else (c, None) for c in cases]
    with phase("preprocess"):
        frames = [split_frames(data, inject, dataset=dataset, anomalies=anomalies, **kwargs) for data, inject in items]
    return rank_cases(frames, mode, scorer)


def baro_batch(cases, dataset=None, **kwargs) -> list:
    """``[baro(data, inject_time, dataset=dataset, **kwargs) for (data, inject_time) in cases]``
    with the columns of all cases scored in one ``scaler_scores`` call."""
    return _batch(ROBUST, cases, dataset, kwargs)


def nsigma_batch(cases, dataset=None, **kwargs) -> list:
    """``nsigma`` of several (data, inject_time) cases, scored in one ``scaler_scores`` call."""
    return _batch(STANDARD, cases, dataset, kwargs)
