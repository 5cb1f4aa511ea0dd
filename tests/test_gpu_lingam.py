"""GPU: pcg_lingam_pair_scores / pcg_direct_lingam_order and the DirectLiNGAM learner against the
numpy restatement of the causal-learn contract (tests/lingam_ref.py), and micro_diag end to end.

Tolerance of D (``test_pair_scores_match_the_restatement``): |D_gpu - D_ref| <= 32 * max(delta, 2^-50),
elementwise absolute. delta is the largest |D_float64 - D_longdouble| of the restatement on that
input — the reference's own rounding spread; nothing in it comes from the engine. (Where long
double is no wider than 2^-60 the delta term is skipped and the floor stands alone.) The factor 32
covers the engine's summation order (64 lanes striding over t) and the device's log / cosh / exp
differing from the host's by an ulp or two per term. M is compared within
tolM_i = 2 * sum_j |D_ij| * tolD + m * tolD^2. The observed |dD| / max(delta, 2^-50) is printed per
case (measured on an MI355X: at most 4.2 against the limit of 32; profiles/lingam_bench.json).

The order is compared for equality. That needs a precondition, asserted from the restatement
alone: at every step the best and the second-best M differ by more than 2 * max tolM, and no M is
NaN. The seeds in ``SEEDS`` are fixed per (generator, T, n) so that it holds.
"""
import functools

import numpy as np
import pytest

import lingam_ref as lr
from rcaeval_amd import synth
from rcaeval_amd.graph_construction import lingam as lmod

pytestmark = pytest.mark.gpu

SHAPES = [(8, 2), (65, 3), (300, 9), (1000, 17), (2500, 5)]      # T = 2500 spans two LDS chunks of 2048 rows
SEEDS = {(gen, T, n): 0 for gen in lr.GENERATORS for T, n in SHAPES}
FLOOR = 2.0 ** -50
WIDE = np.finfo(np.longdouble).eps < 2.0 ** -60


def _engine():
    from rcaeval_amd.engine import get_engine
    return get_engine(0)


def _tolerances(X_):
    """(D, M, delta, tolD, tolM) of the restatement on one step's input."""
    D, M = lr.pair_scores(X_)
    delta = 0.0
    if WIDE and D.size > 1:
        delta = float(np.max(np.abs(D - lr.pair_scores(X_, np.longdouble)[0].astype(np.float64))))
    tolD = 32.0 * max(delta, FLOOR)
    tolM = 2.0 * np.abs(D).sum(axis=1) * tolD + len(M) * tolD ** 2
    return D, M, delta, tolD, tolM


@functools.lru_cache(maxsize=None)
def _reference(gen, T, n):
    """X, the restatement's order / per-step M / snapshots, and each step's tolerances."""
    X = lr.GENERATORS[gen](T, n, SEEDS[gen, T, n])
    X.setflags(write=False)
    K, Ms, snaps = lr.order(X)
    U, steps = list(range(n)), []
    for s in range(n - 1):
        steps.append(_tolerances(snaps[s][:, U]))
        U.remove(K[s])
    return X, K, Ms, snaps, steps


def _assert_margins(K, steps):
    for s, (D, M, delta, tolD, tolM) in enumerate(steps):
        assert not np.isnan(M).any(), f"precondition: step {s} has a NaN score"
        top = np.sort(M)[::-1]
        assert top[0] - top[1] > 2.0 * tolM.max(), f"precondition: step {s} is a near-tie ({top[0] - top[1]:.3e})"


def _check_scores(tag, X_):
    D, M, delta, tolD, tolM = _tolerances(X_)
    gD, gM = _engine().lingam_pair_scores(np.array(X_))
    assert np.array_equal(gD, -gD.T) and (np.diag(gD) == 0).all(), "D is not exactly antisymmetric"
    errD = np.abs(gD - D)
    errM = np.abs(gM - M)
    print(f"{tag}: delta {delta:.2e} tolD {tolD:.2e} worst |dD| {errD.max():.2e} ratio "
          f"{errD.max() / max(delta, FLOOR):.2f} (limit 32); worst dM/tolM {np.max(errM / tolM):.3f}")
    assert (errD <= tolD).all(), (tag, errD.max(), tolD)
    assert (errM <= tolM).all(), (tag, errM, tolM)


@pytest.mark.parametrize("T,n", SHAPES)
@pytest.mark.parametrize("gen", list(lr.GENERATORS))
def test_pair_scores_match_the_restatement(gen, T, n):
    X, K, Ms, snaps, steps = _reference(gen, T, n)
    _check_scores(f"{gen} T={T} n={n} raw", X)
    for s in sorted({n // 2, n - 2}):
        U = sorted(set(range(n)) - set(K[:s]))
        _check_scores(f"{gen} T={T} n={n} X_ at step {s}", snaps[s][:, U])


@pytest.mark.parametrize("T,m", [(300, 70), (150, 130)])
def test_pair_scores_rows_wider_than_a_wavefront(T, m):
    """k_lingam_reduce's 64 lanes stride over a row of D: m = 70 gives lanes 0..5 a second
    element, m = 130 every lane a third pass. (T keeps the float64 + long double restatement at
    about ten seconds on the host.) Same tolerances as above."""
    _check_scores(f"laplace T={T} m={m}", lr.GENERATORS["laplace"](T, m, 0))


def test_order_wider_than_the_argmax_block():
    """n = 260: block_argmax's 256 threads stride over M (threads 0..3 take a second candidate)
    and k_lingam_reduce runs five passes per row. The restatement is too slow at this size, so
    the order is checked against the engine's own scores: a permutation, each step's choice
    np.argmax of that step's row, row 0 bit for bit the single step's M, ordered columns -inf."""
    T, n = 300, 260
    X = lr.GENERATORS["laplace"](T, n, 0)
    eng = _engine()
    order, S = eng.direct_lingam_order(X.copy(), scores=True)
    assert order.dtype == np.int32 and sorted(order.tolist()) == list(range(n))
    assert S.shape == (n, n) and not np.isnan(S).any()
    np.testing.assert_array_equal(S[0], eng.lingam_pair_scores(X.copy())[1])
    for s in range(n):
        assert int(order[s]) == int(np.argmax(S[s])), s
        assert np.isneginf(S[s, order[:s]]).all() and np.isfinite(S[s, order[s:]]).all(), s
    assert S[n - 1, order[n - 1]] == 0


@pytest.mark.parametrize("T,n", SHAPES)
@pytest.mark.parametrize("eps", [1e-3, 1e-6, 1e-9])
def test_pair_scores_on_collinear_columns(eps, T, n):
    X = _reference("laplace", T, n)[0]
    _check_scores(f"collinear({eps:g}) T={T} n={n}", lr.collinear(X, eps))


@pytest.mark.parametrize("T,n", SHAPES)
@pytest.mark.parametrize("gen", list(lr.GENERATORS))
def test_order_equals_the_restatement(gen, T, n):
    X, K, Ms, snaps, steps = _reference(gen, T, n)
    _assert_margins(K, steps)
    eng = _engine()
    order, S = eng.direct_lingam_order(X.copy(), scores=True)
    assert order.dtype == np.int32 and order.tolist() == K
    np.testing.assert_array_equal(eng.direct_lingam_order(X.copy()), order)
    # row 0 is the single step's M, bit for bit; ordered columns hold -inf, the lone candidate 0
    np.testing.assert_array_equal(S[0], eng.lingam_pair_scores(X.copy())[1])
    for s in range(n):
        assert np.isneginf(S[s, K[:s]]).all() and np.isfinite(S[s, K[s:]]).all(), s
    assert S[n - 1, K[n - 1]] == 0
    for s, (D, M, delta, tolD, tolM) in enumerate(steps):
        # later steps run on the engine's own X_, whose rounding differs from the snapshot's: the
        # margin bounds that too, so only the first step's M is held to tolM
        if s == 0:
            assert (np.abs(S[0] - Ms[0]) <= tolM).all()
        assert int(np.argmax(S[s])) == K[s]


def test_nan_semantics_of_a_constant_column():
    """Column 2 is constant (3.0: every partial sum is exact, so its mean is too): it standardizes
    to 0 / 0, every M of every step is NaN, np.argmax takes the first remaining column."""
    X = lr.GENERATORS["laplace"](300, 4, 0).copy()
    X[:, 2] = 3.0
    K, Ms, _ = lr.order(X)
    order, S = _engine().direct_lingam_order(X, scores=True)
    assert order.tolist() == K == [0, 1, 2, 3]
    for s in range(3):
        assert np.isnan(S[s, K[s:]]).all() and np.isneginf(S[s, K[:s]]).all()
    D, M = _engine().lingam_pair_scores(X)
    Dr, Mr = lr.pair_scores(X)
    np.testing.assert_array_equal(np.isnan(D), np.isnan(Dr))
    assert np.isnan(M).all() and np.isnan(Mr).all()


def test_single_column_and_domain():
    eng = _engine()
    X = lr.GENERATORS["uniform"](50, 1, 0)
    order, S = eng.direct_lingam_order(X, scores=True)
    assert order.tolist() == [0] and S.tolist() == [[0.0]]
    D, M = eng.lingam_pair_scores(X)
    assert D.tolist() == [[0.0]] and M.tolist() == [0.0]
    with pytest.raises(ValueError):
        eng.direct_lingam_order(X[:1])                          # T < 2
    with pytest.raises(ValueError):
        eng.lingam_pair_scores(np.zeros((10, 4097)))


def test_row_stride_larger_than_n():
    import torch
    eng = _engine()
    X = _reference("uniform", 300, 9)[0]
    wide = np.full((300, 14), np.nan)
    wide[:, 2:11] = X
    view = torch.from_numpy(wide).to(eng.device)[:, 2:11]
    assert view.stride() == (14, 1)
    order, S = eng.direct_lingam_order(view, scores=True)
    want, Sw = eng.direct_lingam_order(X.copy(), scores=True)
    np.testing.assert_array_equal(order, want)
    np.testing.assert_array_equal(S, Sw)
    for got, ref in zip(eng.lingam_pair_scores(view), eng.lingam_pair_scores(X.copy())):
        np.testing.assert_array_equal(got, ref)


def test_direct_lingam_adjacency():
    X, K, *_ = _reference("uniform", 300, 9)
    _assert_margins(K, _reference("uniform", 300, 9)[4])
    model = lmod.DirectLiNGAM().fit(X.copy())
    assert model.causal_order_ == K
    np.testing.assert_array_equal(model.adjacency_matrix_, lmod.adjacency_from_order(X, K))


def test_micro_diag_end_to_end():
    from rcaeval_amd.e2e import micro_diag
    from rcaeval_amd.graph_heads.page_rank import page_rank
    from rcaeval_amd.io.time_series import preprocess
    df = synth.telemetry_frame(6, 80, n_constant=0, seed=3)
    pre = preprocess(data=df, dataset="online-boutique", dk_select_useful=False)
    X = pre.to_numpy().astype(float)
    names = pre.columns.to_list()
    K, Ms, snaps = lr.order(X)
    U, steps = list(range(X.shape[1])), []
    for s in range(X.shape[1] - 1):
        steps.append(_tolerances(snaps[s][:, U]))
        U.remove(K[s])
    _assert_margins(K, steps)
    adj = lmod.adjacency_from_order(X, K).astype(bool).astype(int)
    assert adj.sum() > 0
    out = micro_diag(df, 0, dataset="online-boutique")
    assert set(out) == {"adj", "node_names", "ranks"} and out["node_names"] == names
    np.testing.assert_array_equal(out["adj"], adj)
    ranks = sorted(page_rank(adj, node_names=names), key=lambda x: x[1], reverse=True)
    assert out["ranks"] == [x[0] for x in ranks]
