"""``DirectLiNGAM`` — mirror of ``RCAEval/graph_construction/lingam.py``'s ``DirectLiNGAM`` (causal-learn
0.1.3.3 [U], the pin of RCAEval's ``requirements.txt``; not installed here, restated from its
source) on the MI355X engine.

``fit(X)`` has two parts. The causal-order search — n steps, each scoring every pair of the
remaining columns with the pairwise likelihood-ratio measure and regressing the chosen column out
of the others — runs in one engine call (``pcg_direct_lingam_order``, ``csrc/lingam.hip``). The
adjacency matrix is then estimated on the host from the original X exactly as the reference does,
with the installed scikit-learn (``adjacency_from_order``): for i = 1..n-1, target = K[i],
predictors = K[:i], ``w = |LinearRegression().fit(X[:, pred], X[:, target]).coef_|``,
``B[target, pred] = LassoLarsIC(criterion='bic').fit(X[:, pred] * w, X[:, target]).coef_ * w``.

Three properties of the reference's search that the engine keeps ("DirectLiNGAM"):
the regression coefficient is cov(ddof=1) / var(ddof=0) = r * T / (T - 1), not the least-squares
r; D_ji = -D_ij exactly; a residual's scale is the std of its own values.

Not built: ``prior_knowledge``, ``measure='kernel'`` (``NotImplementedError``), ``ICALiNGAM`` (FastICA
from an unseeded random start: the reference does not reproduce itself) and the VAR / VARMA
variants. Deviation: T < 2 raises ``ValueError`` (the reference divides by T - 1 = 0 and carries
NaN on).
"""
from __future__ import annotations

import numpy as np


def adjacency_from_order(X, order) -> np.ndarray:
    """The reference's ``_estimate_adjacency_matrix`` / ``predict_adaptive_lasso`` [U] (gamma = 1):
    ``B[i, j]`` is the coefficient of column j in column i's adaptive-lasso regression on the
    columns before it in ``order``. Pure host code on the original X."""
    from sklearn.linear_model import LassoLarsIC, LinearRegression
    X = np.asarray(X, dtype=np.float64)
    order = [int(k) for k in order]
    B = np.zeros([X.shape[1], X.shape[1]], dtype="float64")
    for i in range(1, len(order)):
        target = order[i]
        predictors = order[:i]
        lr = LinearRegression()
        lr.fit(X[:, predictors], X[:, target])
        weight = np.power(np.abs(lr.coef_), 1.0)
        reg = LassoLarsIC(criterion="bic")
        reg.fit(X[:, predictors] * weight, X[:, target])
        B[target, predictors] = reg.coef_ * weight
    return B


class DirectLiNGAM:
    """``DirectLiNGAM(random_state=None, prior_knowledge=None, apply_prior_knowledge_softly=False,
    measure='pwling')`` with ``fit(X)``, ``causal_order_`` and ``adjacency_matrix_``."""

    def __init__(self, random_state=None, prior_knowledge=None, apply_prior_knowledge_softly=False, measure="pwling"):
        if prior_knowledge is not None:
            raise NotImplementedError("DirectLiNGAM: prior_knowledge is not built")
        if measure != "pwling":
            raise NotImplementedError(f"DirectLiNGAM: measure={measure!r}: only 'pwling' is built")
        self._random_state = random_state
        self._apply_prior_knowledge_softly = apply_prior_knowledge_softly
        self._measure = measure
        self._causal_order = None
        self._adjacency_matrix = None

    def fit(self, X) -> "DirectLiNGAM":
        from ..engine import get_engine
        X = X.to_numpy() if hasattr(X, "to_numpy") else np.asarray(X)
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError(f"Expected 2D array, got {X.ndim}D array instead")
        if not np.isfinite(X).all():
            raise ValueError("Input X contains NaN or infinity.")      # sklearn check_array [U]
        T, n = X.shape
        if n < 1:
            raise ValueError(f"Found array with {n} feature(s) while a minimum of 1 is required.")
        if T < 2:
            raise ValueError(f"DirectLiNGAM: T = {T} samples; the coefficient's T - 1 needs T >= 2")
        self._causal_order = [int(k) for k in get_engine().direct_lingam_order(X)]
        self._adjacency_matrix = adjacency_from_order(X, self._causal_order)
        return self

    @property
    def causal_order_(self):
        return self._causal_order

    @property
    def adjacency_matrix_(self):
        return self._adjacency_matrix


__all__ = ["DirectLiNGAM", "adjacency_from_order"]
