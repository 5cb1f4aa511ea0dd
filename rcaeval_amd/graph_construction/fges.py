"""``fges`` — mirror of ``RCAEval/graph_construction/fges.py:49-76`` on the MI355X engine.

The reference runs ``LIB/libraries/FGES`` (``FGES.search()``: ``mode = "heuristic"``,
``cycle_bound = -1``, no knowledge) with the linear-Gaussian local score of
``LIB/python/scores.py:142-171`` (``penalty = 2``), one ``statsmodels.OLS`` fit on all T rows per
local score. With that score the bump of adding x to the parents P of y is

    bump(x -> y | P) = T g - 2 log T,   g = log(SSR(y|P) / SSR(y|P + x)) = -log(1 - rho^2(x, y . P)),

rho the partial correlation inside the ddof-0 correlation matrix R of the data. The engine keeps R
(``pcg_fges_begin``, K1's kernels) and evaluates g for batches of (x, y | B) grouped by (y, B)
(``pcg_fges_gains``, ``csrc/fges.hip``); T and the penalty are applied here. The search itself —
the graph, the arrow list, the Meek rules and the validity tests — runs on the host: per step it
gathers every bump that the re-evaluation needs, groups them by (y, B) and makes one call.

Deviations from the reference ("fGES"): sets are iterated in ascending node order;
``fges.log`` is not written and "Returning early..." is not printed; ``score_func`` "p2" / "p3" raise
``NotImplementedError``; the result is an integer ndarray (``adj[i, j] = 1`` for i -> j, both
entries for an undirected edge); the caller's column labels are not renamed; a constant column
raises ``ValueError``.
"""
from __future__ import annotations

import heapq
import itertools
import math
import time

import numpy as np


def limits() -> dict:
    """The limits and fast-path guards the library's fGES kernels were built with
    (``pcg_fges_limits``): b_cap, max_n, narrow_max, tau, beta_c."""
    import ctypes
    from .. import _lib
    i = [ctypes.c_int32() for _ in range(3)]
    d = [ctypes.c_double() for _ in range(2)]
    _lib.load().pcg_fges_limits(*(ctypes.byref(v) for v in i + d))
    return {"b_cap": i[0].value, "max_n": i[1].value, "narrow_max": i[2].value, "tau": d[0].value, "beta_c": d[1].value}


def fast_path_bound(dim_b: int) -> float:
    """The absolute error bound of an accepted fast-path g with ``|B| = dim_b`` ("fGES"):
    2 * beta_c * (|B| + 20) * 2^-53 / tau."""
    lim = limits()
    return 2.0 * lim["beta_c"] * (int(dim_b) + 20) * 2.0 ** -53 / lim["tau"]


def host_gain(X, x: int, y: int, B) -> float:
    """g(x, y | B) by ``numpy.linalg.lstsq`` on the raw columns with an intercept: the scorer of
    items the kernel refuses (status 4) and of ``HostScorer``."""
    T = X.shape[0]
    t = X[:, y]
    ssr = []
    for cols in (list(B), list(B) + [x]):
        D = np.column_stack([X[:, cols], np.ones(T)])
        r = t - D @ np.linalg.lstsq(D, t, rcond=None)[0]
        ssr.append(float(r @ r))
    return math.log(ssr[0] / ssr[1])


class HostScorer:
    """The scorer's interface in numpy (no engine): ``begin`` gives the n x n depth-0 gains,
    ``gains`` one array of g per group (y, B, candidates)."""

    def __init__(self):
        self.stats = {"begin_s": 0.0, "gains_s": 0.0, "calls": 0, "items": 0, "exact_items": 0, "fallback_items": 0}

    def begin(self, X):
        self.X = X
        if (X.std(axis=0) == 0).any():
            raise ValueError("fges: a column is constant")
        n = X.shape[1]
        g0 = np.full((n, n), np.nan)
        for i in range(n):
            for j in range(i + 1, n):
                g0[i, j] = g0[j, i] = host_gain(X, i, j, ())
        return g0

    def gains(self, groups):
        self.stats["calls"] += 1
        self.stats["items"] += sum(len(c) for _, _, c in groups)
        return [np.array([host_gain(self.X, x, y, B) for x in cand]) for y, B, cand in groups]


class EngineScorer:
    """``pcg_fges_begin`` / ``pcg_fges_gains`` behind the scorer's interface. Items the kernel
    refuses for its |B| cap (status 4) are scored by ``host_gain``; a constant or non-finite
    column raises ``ValueError``."""

    def __init__(self, engine=None):
        self.engine = engine
        self.stats = {"begin_s": 0.0, "gains_s": 0.0, "calls": 0, "items": 0, "exact_items": 0, "fallback_items": 0}

    def begin(self, X):
        from ..engine import get_engine
        if self.engine is None:
            self.engine = get_engine()
        self.X = X
        t0 = time.perf_counter()
        out = self.engine.fges_begin(X)
        self.stats["begin_s"] += time.perf_counter() - t0
        raise_on_status(out["status"])
        return out["gain0"]

    def gains(self, groups):
        t0 = time.perf_counter()
        out = self.engine.fges_gains(groups)
        self.stats["gains_s"] += time.perf_counter() - t0
        self.stats["calls"] += 1
        self.stats["items"] += len(out["gain"])
        self.stats["exact_items"] += out["exact_items"]
        raise_on_status(out["status"])
        res, pos = [], 0
        for y, B, cand in groups:
            g = out["gain"][pos:pos + len(cand)].copy()
            for k in np.nonzero(out["status"][pos:pos + len(cand)] == 4)[0]:
                g[k] = host_gain(self.X, cand[k], y, B)
                self.stats["fallback_items"] += 1
            res.append(g)
            pos += len(cand)
        return res


def raise_on_status(status) -> None:
    """``ValueError`` for a constant (1) or non-finite (2) column."""
    status = np.asarray(status)
    if (status == 2).any():
        raise ValueError("fges: non-finite input")
    if (status == 1).any():
        raise ValueError("fges: a column is constant")


# ---- the graph: A[i, j] = 1 is the arc i -> j, an undirected edge is both arcs -------------------
def _adjacent(A, x, y):
    return bool(A[x, y] or A[y, x])


def _directed(A, x, y):
    return bool(A[x, y] and not A[y, x])


def _undirected(A, x, y):
    return bool(A[x, y] and A[y, x])


def _around(A, x):
    return [int(v) for v in np.nonzero(A[x] | A[:, x])[0]]


def _parents(A, x):
    return [int(v) for v in np.nonzero(A[:, x] & ~A[x])[0]]


def _children(A, x):
    return [int(v) for v in np.nonzero(A[x] & ~A[:, x])[0]]


def _neighbours(A, x):
    return frozenset(int(v) for v in np.nonzero(A[x] & A[:, x])[0])


def _na_y_x(A, x, y):
    return frozenset(int(v) for v in np.nonzero(A[y] & A[:, y] & (A[x] | A[:, x]))[0])


def _t_neighbours(A, x, y):
    return frozenset(int(v) for v in np.nonzero(A[y] & A[:, y] & ~(A[x] | A[:, x]))[0])


def _clique(A, nodes):
    nodes = list(nodes)
    return all(_adjacent(A, a, b) for k, a in enumerate(nodes) for b in nodes[k + 1:])


def _orient(A, x, y):
    """Keep only x -> y of an edge that is x - y or already x -> y (``graph_util.undir_to_dir``)."""
    if not A[x, y]:
        raise AssertionError("fges: no such edge, or it points the other way")
    A[y, x] = False


def _semi_directed_path(A, origin, dest, blocked):
    """``exists_unblocked_semi_directed_path`` with ``cycle_bound = -1``."""
    seen = {origin}
    frontier = [origin]
    while frontier:
        nxt = []
        for t in frontier:
            if t == dest:
                return True
            for u in np.nonzero(A[t])[0]:
                u = int(u)
                if u in blocked:
                    continue
                if u == dest:
                    return True
                if u not in seen:
                    seen.add(u)
                    nxt.append(u)
        frontier = nxt
    return False


class _Meek:
    """``meekrules.MeekRules`` with ``undirect_unforced_edges=True`` and no knowledge, restricted to
    a node subset (``orient_implied_subset``): R1-R4, un-forcing of parents no unshielded collider
    holds, and the reference's work stack."""

    def __init__(self, A):
        self.A = A
        self.visited = set()
        self.stack = []
        self.oriented = set()

    def run(self, subset):
        subset = sorted(subset)
        self.visited.update(subset)
        for v in subset:
            self._unforce(v)
            self.stack.extend(_around(self.A, v))
        for v in subset:
            self._rules(v)
        while self.stack:
            v = self.stack.pop()
            self._unforce(v)
            self._rules(v)
        return self.visited

    def _unforce(self, v):
        A = self.A
        par = _parents(A, v)
        keep = set()
        for p, q in itertools.combinations(par, 2):
            if not _adjacent(A, p, q):
                self.oriented.update(((p, v), (q, v)))
                keep.update((p, q))
        changed = False
        for p in par:
            if p not in keep and (p, v) not in self.oriented:
                A[v, p] = True
                self.visited.update((v, p))
                changed = True
        if changed:
            self.stack.extend(_around(A, v))
            self.stack.append(v)

    def _direct(self, a, b):
        self.A[b, a] = False
        self.A[a, b] = True
        self.visited.update((a, b))
        if (a, b) not in self.oriented and (b, a) not in self.oriented:
            self.oriented.add((a, b))
            self.stack.append(b)

    def _non_collider(self, a, b, c):
        A = self.A
        if not _adjacent(A, a, b) or not _adjacent(A, c, b) or _adjacent(A, a, c):
            return False
        return not (_directed(A, a, b) and _directed(A, c, b))

    def _rules(self, v):
        A, o = self.A, self.oriented
        for a, c in itertools.combinations(_around(A, v), 2):                  # R1
            for p, q in ((a, c), (c, a)):
                if (not _adjacent(A, p, q) and (_directed(A, p, v) or (p, v) in o) and _undirected(A, v, q)
                        and self._non_collider(p, v, q)
                        and not {(p, q), (q, p), (v, q), (q, v)} & o):
                    self._direct(v, q)
        for a, c in itertools.combinations(_around(A, v), 2):                  # R2
            for p, q, r in ((a, v, c), (v, a, c), (a, c, v), (c, a, v)):
                if _directed(A, p, q) and _directed(A, q, r) and _undirected(A, p, r):
                    self._direct(p, r)
        adj = _around(A, v)
        if len(adj) >= 3:
            for a in adj:                                                      # R3
                if not _undirected(A, v, a):
                    continue
                for b, c in itertools.combinations([u for u in adj if u != a], 2):
                    if (_undirected(A, a, v) and _undirected(A, a, b) and _undirected(A, a, c) and _directed(A, b, v)
                            and _directed(A, c, v) and self._non_collider(c, a, b)):
                        self._direct(a, v)
        adj = _around(A, v)
        if len(adj) >= 3:
            nb = _neighbours(A, v)
            for c in adj:                                                      # R4
                ba = [u for u in _parents(A, c) if u in nb]
                for d in [d for d in _children(A, c) if d in nb and any(not _adjacent(A, b, d) for b in ba)]:
                    self._direct(v, d)


class _Arrows:
    """The reference's sorted arrow list: highest bump first, ties to the earlier-added arrow."""

    def __init__(self):
        self.heap = []
        self.by_pair = {}
        self.count = 0

    def add(self, a, b, na, ht, bump):
        ar = [True, a, b, frozenset(na), frozenset(ht), bump]
        heapq.heappush(self.heap, (-bump, self.count, ar))
        self.count += 1
        self.by_pair.setdefault((a, b), []).append(ar)

    def clear(self, a, b):
        for ar in self.by_pair.pop((a, b), ()):
            ar[0] = False

    def pop(self):
        while self.heap:
            ar = heapq.heappop(self.heap)[2]
            if ar[0]:
                ar[0] = False
                return ar
        return None


class _Search:
    def __init__(self, X, scorer, trace):
        self.X, self.T, self.n = X, X.shape[0], X.shape[1]
        self.scorer = scorer
        self.A = np.zeros((self.n, self.n), dtype=bool)
        self.pen = 2.0 * math.log(self.T)
        self.trace = trace if trace is not None else {}
        for key in ("inserted", "deleted", "evaluated"):
            self.trace.setdefault(key, [])
        self.g0 = None

    # one scoring round: requests (x, y, B) -> bumps of adding x to the parents B of y
    def bumps(self, requests):
        out = [None] * len(requests)
        groups = {}
        for k, (x, y, B) in enumerate(requests):
            if not B:
                out[k] = self.g0[x, y]
            else:
                groups.setdefault((y, B), []).append(k)
        if groups:
            keys = list(groups)
            res = self.scorer.gains([(y, B, [requests[k][0] for k in groups[(y, B)]]) for y, B in keys])
            for key, g in zip(keys, res):
                for k, v in zip(groups[key], g):
                    out[k] = float(v)
        for k, (x, y, B) in enumerate(requests):
            g = out[k]
            out[k] = self.T * g - self.pen
            self.trace["evaluated"].append((x, y, B, out[k], g))
        return out

    def begin(self):
        self.g0 = np.asarray(self.scorer.begin(self.X), dtype=np.float64)

    # ---- FES
    def initial_arrows(self):
        n = self.n
        self.arrows = _Arrows()
        self.effect = {v: [] for v in range(n)}
        self.stored = {v: frozenset() for v in range(n)}
        b0 = self.T * self.g0 - self.pen
        for i in range(n):
            for j in range(i + 1, n):
                b_ij, b_ji = float(b0[i, j]), float(b0[j, i])
                self.trace["evaluated"] += [(i, j, (), b_ij, float(self.g0[i, j])), (j, i, (), b_ji, float(self.g0[j, i]))]
                if b_ij >= 0 or b_ji >= 0:
                    self.effect[i].append(j)
                    self.effect[j].append(i)
                if b_ji >= 0:
                    self.arrows.add(j, i, (), (), b_ji)
                if b_ij >= 0:
                    self.arrows.add(i, j, (), (), b_ij)

    def forward_requests(self, a, b, req):
        """``calculate_arrows_forward``: the T subsets of a -> b worth scoring, clique pruning included."""
        A = self.A
        if b not in self.effect[a]:
            return
        self.stored[b] = _neighbours(A, b)
        na = _na_y_x(A, a, b)
        if not _clique(A, na):
            return
        tn = sorted(_t_neighbours(A, a, b))
        par = frozenset(_parents(A, b))
        previous = {frozenset()}
        for size in range(len(tn) + 1):
            fresh = set()
            for choice in itertools.combinations(tn, size):
                union = na | frozenset(choice)
                if not any(union >= c for c in previous):
                    return
                if not _clique(A, union):
                    continue
                fresh.add(union)
                req.append((a, b, na, frozenset(choice), tuple(sorted(union | par))))
            previous = fresh

    def score_and_add(self, req, sign):
        vals = self.bumps([(a, b, base) for a, b, _, _, base in req])
        for (a, b, na, ht, _), v in zip(req, vals):
            if sign * v > 0:
                self.arrows.add(a, b, na, ht, sign * v)

    def fes(self):
        A = self.A
        while True:
            ar = self.arrows.pop()
            if ar is None:
                return
            _, x, y, na0, T, _ = ar
            if _adjacent(A, x, y):
                continue
            na = _na_y_x(A, x, y)
            if na0 != na or not _t_neighbours(A, x, y) >= T:
                continue
            union = T | na
            if not _clique(A, union) or _semi_directed_path(A, y, x, union):
                continue
            A[x, y] = True
            for t in sorted(T):
                _orient(A, t, y)
            self.trace["inserted"].append((x, y, tuple(sorted(T))))
            visited = _Meek(A).run({x, y})
            todo = {v for v in visited if self.stored.get(v) != _neighbours(A, v)} | {x, y}
            req = []
            for v in sorted(todo):
                for w in self.effect[v]:
                    if w != v and not _adjacent(A, v, w):
                        self.arrows.clear(w, v)
                        self.forward_requests(w, v, req)
            self.score_and_add(req, 1.0)

    # ---- BES
    def backward_requests(self, a, b, req):
        """``calculate_arrows_backward``: every H = na_y_x - diff of the edge a -> b."""
        A = self.A
        na = _na_y_x(A, a, b)
        lst = sorted(na)
        par = frozenset(_parents(A, b))
        for size in range(len(lst) + 1):
            for diff in itertools.combinations(lst, size):
                base = (frozenset(diff) | par) - {a}
                req.append((a, b, na, na - frozenset(diff), tuple(sorted(base))))

    def _drop_stale(self, req, a, b):
        """A later ``clear_arrow`` of the pair removes what an earlier call gathered for it."""
        req[:] = [r for r in req if not (r[0] == a and r[1] == b)]
        self.arrows.clear(a, b)

    def initial_backward(self):
        A = self.A
        self.arrows = _Arrows()
        self.stored = {}
        req = []
        for x in range(self.n):
            for y in np.nonzero(A[x])[0]:
                y = int(y)
                self._drop_stale(req, x, y)
                self._drop_stale(req, y, x)
                self.backward_requests(x, y, req)
                self.stored[x] = _neighbours(A, x)
                self.stored[y] = _neighbours(A, y)
        self.score_and_add(req, -1.0)

    def bes(self):
        A = self.A
        while True:
            ar = self.arrows.pop()
            if ar is None:
                return
            _, x, y, na0, H, _ = ar
            if na0 != _na_y_x(A, x, y) or not _adjacent(A, x, y) or _directed(A, y, x):
                continue                      # (the reference's valid_delete is unreachable: not checked)
            A[x, y] = A[y, x] = False
            for v in sorted(H):
                if _directed(A, v, y) or _directed(A, v, x):
                    continue
                _orient(A, y, v)
                if _undirected(A, x, v):
                    _orient(A, x, v)
            self.trace["deleted"].append((x, y, tuple(sorted(H))))
            _Meek(A).run({x, y})
            self.arrows.clear(x, y)
            visited = _Meek(A).run({x, y} | H)
            todo = {v for v in visited if self.stored[v] != _neighbours(A, v)} | {x, y}
            todo |= set(_around(A, x)) & set(_around(A, y))
            req = []
            for v in sorted(todo):
                self.stored[v] = _neighbours(A, v)
                for w in _around(A, v):
                    if _directed(A, w, v):
                        self._drop_stale(req, w, v)
                        self._drop_stale(req, v, w)
                        self.backward_requests(w, v, req)
                    elif _undirected(A, w, v):
                        self._drop_stale(req, w, v)
                        self._drop_stale(req, v, w)
                        self.backward_requests(w, v, req)
                        self.backward_requests(v, w, req)
            self.score_and_add(req, -1.0)

    def adjacency(self):
        return self.A.astype(np.int64)


def _prepare(data, score_func, scorer, trace):
    if score_func not in (None, "linear", "p2", "p3"):
        raise AssertionError("fges: score_func must be None, 'linear', 'p2' or 'p3'")
    if score_func in ("p2", "p3"):
        raise NotImplementedError("fges: only the linear-Gaussian score is served")
    X = data.to_numpy() if hasattr(data, "to_numpy") else np.asarray(data)
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 3:
        raise ValueError("fges: data must be T x n with T >= 3")
    if not np.isfinite(X).all():
        raise ValueError("fges: non-finite input")
    if X.shape[1] and (X.max(axis=0) == X.min(axis=0)).any():
        raise ValueError("fges: a column is constant")
    s = _Search(X, scorer if scorer is not None else EngineScorer(), trace)
    s.begin()
    return s


def fges(data, score_func=None, **kwargs):
    """``fges.py:49-76``: the CPDAG of FES then BES as an n x n integer adjacency in column order.
    Private keywords: ``_scorer`` (an object with ``begin`` / ``gains``, default the engine's) and
    ``_trace`` (a dict that receives the insertions, deletions, the evaluated items as
    ``(x, y, B, bump, g)`` and ``stats``)."""
    t0 = time.perf_counter()
    s = _prepare(data, score_func, kwargs.get("_scorer"), kwargs.get("_trace"))
    s.initial_arrows()
    s.fes()
    s.initial_backward()
    s.bes()
    s.trace["stats"] = dict(s.scorer.stats, total_s=time.perf_counter() - t0)
    return s.adjacency()


def fes(data, start=None, score_func=None, **kwargs):
    """FES alone. ``start`` must be None (the empty graph): the reference's forward arrows are
    initialised from the empty graph only."""
    if start is not None and np.asarray(start).any():
        raise ValueError("fges: FES starts from the empty graph")
    s = _prepare(data, score_func, kwargs.get("_scorer"), kwargs.get("_trace"))
    s.initial_arrows()
    s.fes()
    return s.adjacency()


def bes(data, start, score_func=None, **kwargs):
    """BES alone from the start graph ``start`` (n x n, ``start[i, j] = 1`` for an arc i -> j)."""
    s = _prepare(data, score_func, kwargs.get("_scorer"), kwargs.get("_trace"))
    start = np.asarray(start)
    if start.shape != (s.n, s.n):
        raise ValueError("fges: start must be n x n")
    s.A[:] = start != 0
    np.fill_diagonal(s.A, False)
    s.initial_backward()
    s.bes()
    return s.adjacency()


__all__ = ["EngineScorer", "HostScorer", "bes", "fast_path_bound", "fes", "fges", "host_gain", "limits", "raise_on_status"]
