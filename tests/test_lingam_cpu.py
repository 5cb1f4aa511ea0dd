"""CPU: the DirectLiNGAM feature's host side — properties of the numpy restatement of the contract
(tests/lingam_ref.py), ``adjacency_from_order`` against the scikit-learn formulas written out, the
argument and error cases of ``DirectLiNGAM``, ``micro_diag`` with the engine's order replaced by the
restatement's, the method registry and the new bindings."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import lingam_ref as lr
from rcaeval_amd import synth
from rcaeval_amd.graph_construction import lingam as lmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("gen", list(lr.GENERATORS))
def test_restatement_D_is_exactly_antisymmetric(gen):
    X = lr.GENERATORS[gen](200, 5, 1)
    for Y in (X, lr.collinear(X, 1e-6)):
        D, M = lr.pair_scores(Y)
        assert np.array_equal(D, -D.T) and not np.isnan(D).any() and (np.diag(D) == 0).all()
        np.testing.assert_array_equal(M, [-sum(min(0.0, D[i, j]) ** 2 for j in range(5) if j != i) for i in range(5)])


def test_restatement_recovers_a_topological_order():
    X, B, perm = lr.sem(5000, 6, 0, "uniform")
    assert np.count_nonzero(B) >= 3
    K, Ms, snaps = lr.order(X)
    assert sorted(K) == list(range(6)) and len(Ms) == len(snaps) == 6
    pos = {int(perm[c]): s for s, c in enumerate(K)}          # variable -> its step
    for a, b in zip(*np.nonzero(B)):                           # edge b -> a
        assert pos[int(b)] < pos[int(a)], (a, b, K)
    # Ms rows: -inf once ordered, 0 for the lone last candidate
    for s in range(6):
        assert np.isneginf(Ms[s][K[:s]]).all() and np.isfinite(Ms[s][K[s:]]).all()
    assert Ms[5][K[5]] == 0
    np.testing.assert_array_equal(snaps[0], X)


def test_restatement_coefficient_is_cov1_over_var0():
    """residual() uses cov(ddof=1) / var(ddof=0) = r * T / (T - 1): on collinear columns the
    residual is about -z / (T - 1), where the least-squares coefficient leaves rounding noise. At
    T = 8 the factor is 8 / 7 and the scores of a frame with a collinear pair move by far more than
    any tolerance (H is even, so the collinear pair's own D stays near 0 under either coefficient;
    the pairs with the third column carry the difference)."""
    X = lr.collinear(lr.GENERATORS["uniform"](8, 3, 0), 1e-9)
    D, M = lr.pair_scores(X)
    Dq, Mq = lr.pair_scores(X, lsq=True)
    assert np.abs(D - Dq).max() > 1e-3
    X = lr.GENERATORS["uniform"](300, 3, 0)
    z = (X[:, 0] - X[:, 0].mean()) / X[:, 0].std()
    np.testing.assert_allclose(lr._residual(z, z), -z / 299.0, rtol=0, atol=1e-12)
    a = np.arange(8.0) ** 2
    b = np.arange(8.0)
    r = np.corrcoef(a, b)[0, 1] * a.std() / b.std()            # the least-squares slope
    np.testing.assert_allclose(a - lr._residual(a, b), r * 8.0 / 7.0 * b, rtol=1e-13)


def test_restatement_nan_semantics():
    """A constant column standardizes to NaN, every M of the step is NaN and np.argmax takes the
    first remaining column."""
    X = lr.GENERATORS["laplace"](300, 4, 0)
    X[:, 2] = 3.0
    K, Ms, _ = lr.order(X)
    assert K == [0, 1, 2, 3] and all(np.isnan(Ms[s][K[s:]]).all() for s in range(3))


# ---- adjacency -----------------------------------------------------------------------------------
def test_adjacency_from_order_matches_the_formulas():
    from sklearn.linear_model import LassoLarsIC, LinearRegression
    X, B, perm = lr.sem(400, 5, 3, "uniform")
    K = lr.order(X)[0]
    got = lmod.adjacency_from_order(X, K)
    want = np.zeros((5, 5))
    for i in range(1, 5):
        target, pred = K[i], K[:i]
        w = np.abs(LinearRegression().fit(X[:, pred], X[:, target]).coef_)
        want[target, pred] = LassoLarsIC(criterion="bic").fit(X[:, pred] * w, X[:, target]).coef_ * w
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.float64 and np.count_nonzero(got)
    assert not got[K[0]].any()                                 # the first in the order has no parents
    at = {c: s for s, c in enumerate(K)}
    for a, b in zip(*np.nonzero(got)):
        assert at[b] < at[a]
    assert lmod.adjacency_from_order(X[:, :1], [0]).tolist() == [[0.0]]


# ---- DirectLiNGAM's arguments ----------------------------------------------------------------------
class _StubEngine:
    """Stands in for the device: the restatement's order."""

    def __init__(self):
        self.calls = 0

    def direct_lingam_order(self, X, scores=False):
        self.calls += 1
        return np.asarray(lr.order(X)[0], dtype=np.int32)


@pytest.fixture
def stub_engine(monkeypatch):
    import rcaeval_amd.e2e  # noqa: F401  (imported before the patch: its modules bind the real get_engine)
    import rcaeval_amd.engine as engine
    stub = _StubEngine()
    monkeypatch.setattr(engine, "get_engine", lambda device=None: stub)
    return stub


def test_direct_lingam_arguments_and_errors(stub_engine):
    import rcaeval_amd.graph_construction as gc
    assert gc.DirectLiNGAM is lmod.DirectLiNGAM
    m = lmod.DirectLiNGAM(random_state=None, prior_knowledge=None, apply_prior_knowledge_softly=False, measure="pwling")
    assert m.causal_order_ is None and m.adjacency_matrix_ is None
    with pytest.raises(NotImplementedError):
        lmod.DirectLiNGAM(prior_knowledge=np.zeros((3, 3)))
    with pytest.raises(NotImplementedError):
        lmod.DirectLiNGAM(measure="kernel")
    X = lr.GENERATORS["uniform"](120, 4, 2)
    for bad in (np.nan, np.inf, -np.inf):
        Y = X.copy()
        Y[7, 1] = bad
        with pytest.raises(ValueError):
            m.fit(Y)
    with pytest.raises(ValueError):
        m.fit(X[:1])                                           # T < 2: the documented deviation
    with pytest.raises(ValueError):
        m.fit(X[:, 0])
    assert stub_engine.calls == 0                              # all refused on the host, before upload
    assert m.fit(X) is m and stub_engine.calls == 1
    K = lr.order(X)[0]
    assert m.causal_order_ == K and all(type(k) is int for k in m.causal_order_)
    np.testing.assert_array_equal(m.adjacency_matrix_, lmod.adjacency_from_order(X, K))


# ---- micro_diag ------------------------------------------------------------------------------------
def _frame():
    from rcaeval_amd.io.time_series import preprocess
    df = synth.telemetry_frame(6, 80, n_constant=0, seed=3)
    return df, preprocess(data=df, dataset="online-boutique", dk_select_useful=False)


def test_micro_diag_wrapper(stub_engine, monkeypatch):
    import rcaeval_amd.e2e.lingam_pagerank as mod
    from rcaeval_amd import e2e
    assert e2e.micro_diag is mod.micro_diag and "micro_diag" in e2e.__all__
    df, pre = _frame()
    names = pre.columns.to_list()
    X = pre.to_numpy().astype(float)
    adj = lmod.adjacency_from_order(X, lr.order(X)[0]).astype(bool).astype(int)
    assert adj.sum() > 0
    seen = {}

    def head(a, node_names=None):
        seen["adj"] = a
        return [(nm, float(k)) for k, nm in enumerate(node_names)]
    monkeypatch.setattr(mod, "page_rank", head)
    out = mod.micro_diag(df, 0, dataset="online-boutique")
    assert set(out) == {"adj", "node_names", "ranks"}
    np.testing.assert_array_equal(out["adj"], adj)
    assert out["adj"].dtype.kind == "i" and seen["adj"] is out["adj"]
    assert out["node_names"] == names and out["ranks"] == names[::-1]      # the stub's scores, descending
    # the all-zero shortcut returns the names and never reaches page_rank
    monkeypatch.setattr(mod, "page_rank", lambda *a, **k: (_ for _ in ()).throw(AssertionError("called")))
    monkeypatch.setattr(lmod, "adjacency_from_order", lambda X, order: np.zeros((len(order), len(order))))
    out = mod.micro_diag(df, 0, dataset="online-boutique")
    assert out["ranks"] == names and out["node_names"] == names and out["adj"].sum() == 0


def test_micro_diag_has_no_rca_wrapper(stub_engine, monkeypatch):
    """The reference's micro_diag carries no @rca: an exception propagates instead of becoming the
    dummy ranking."""
    import rcaeval_amd.e2e.lingam_pagerank as mod
    df, _ = _frame()
    monkeypatch.setattr(stub_engine, "direct_lingam_order",
                        lambda X, scores=False: (_ for _ in ()).throw(ValueError("order failed")))
    with pytest.raises(ValueError, match="order failed"):
        mod.micro_diag(df, 0, dataset="online-boutique")
    assert not hasattr(mod.micro_diag, "__wrapped__")


def test_rq2_serves_micro_diag():
    from rcaeval_amd import e2e, rq2
    m = rq2.methods()
    assert m["micro_diag"] is e2e.micro_diag
    for name in ("pc_pagerank", "pc_randomwalk", "cloudranger", "circa", "granger_pagerank", "granger_randomwalk"):
        assert m[name] is getattr(e2e, name)


# ---- bindings --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pcg_lingam_pair_scores", "pcg_direct_lingam_order"])
def test_header_library_and_bindings_agree(name):
    from rcaeval_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pcgpu.h")).read()
    decl = re.search(r"^int %s\((.*?)\);" % name, hdr, re.S | re.M).group(1)
    params = [p.strip() for p in decl.replace("\n", " ").split(",")]
    sig = {nm: (res, args) for nm, res, args in _lib.SIGNATURES}[name]
    assert sig[0] is ctypes.c_int32 and len(sig[1]) == len(params) == 7
    for p, a in zip(params, sig[1]):
        assert a is (ctypes.c_void_p if "*" in p else ctypes.c_int64), (p, a)
    assert getattr(lib, name).argtypes == sig[1]
    assert int(re.search(r"#define PCG_ABI_VERSION (\d+)", hdr).group(1)) == _lib.PCG_ABI_VERSION == 4
    # a NULL handle is refused before anything is touched
    assert getattr(lib, name)(None, None, 100, 4, 4, None, None) == _lib.PCG_ERR_INVALID
