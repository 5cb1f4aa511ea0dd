"""CPU restatement of the fGES contract (helper, not a test).

Written from the semantics of the reference's ``LIB/libraries/FGES`` (``FGES.search()`` with
``mode = "heuristic"``, ``cycle_bound = -1``, no knowledge) and its linear-Gaussian local score
(``LIB/python/scores.py:142-171``, ``penalty = 2``): s(y, P) = 2 llf - 2 (|P| + 2) log T, so the
bump of adding x to the parents P of y is T g - 2 log T with g = log(SSR(y|P) / SSR(y|P + x)).
Every SSR is a ``numpy.linalg.lstsq`` fit of the raw column on the raw parent columns and an
intercept; a second solve by a Householder QR of the same design gives ``delta``, the largest
difference between the two g over a run: the restatement's own uncertainty. Nothing here comes
from the engine's correlation-matrix formulation.

The graph is a dict of successor sets (an undirected edge is both arcs, as in the reference's
DiGraph). Wherever the reference iterates a Python set, this iterates in ascending node order
(CPython's own order for the small ints of n <= 8). The two mirrored arrows of the first step,
and any other pair of bumps on an empty parent set, are equal in exact arithmetic: g(x, y | {}) is
computed once per unordered pair, so such ties fall to the earlier-added arrow. ``mirror`` chooses
which of the two initial arrows is added (and so popped) first: "ji" as the reference, "ij" the
other way round.
"""
import functools
import itertools
import math

import numpy as np


# ---- input ------------------------------------------------------------------------------------
def gen_dag(T, n, seed, p_edge=0.4):
    """A random linear-Gaussian DAG in column order: each pair i < j is an edge with probability
    p_edge, weight +-(0.5..1.0), noise scale 0.6..1.4; every column gets its own offset."""
    rng = np.random.default_rng(seed)
    W = np.zeros((n, n))
    for j in range(n):
        for i in range(j):
            if rng.random() < p_edge:
                W[i, j] = rng.uniform(0.5, 1.0) * (1.0 if rng.random() < 0.5 else -1.0)
    X = np.zeros((T, n))
    for j in range(n):
        X[:, j] = X @ W[:, j] + rng.uniform(0.6, 1.4) * rng.normal(size=T) + rng.uniform(-2, 2)
    return np.ascontiguousarray(X)


def gen_named(kind, T, seed):
    """Hand-built three-column inputs with a known CPDAG."""
    rng = np.random.default_rng(seed)
    e = rng.normal(size=(T, 3))
    if kind == "chain":                      # 0 -> 1 -> 2: the CPDAG is 0 - 1 - 2
        a = e[:, 0]
        b = 0.9 * a + e[:, 1]
        return np.ascontiguousarray(np.stack([a, b, 0.9 * b + e[:, 2]], axis=1))
    if kind == "collider":                   # 0 -> 2 <- 1
        return np.ascontiguousarray(np.stack([e[:, 0], e[:, 1], 0.8 * e[:, 0] + 0.8 * e[:, 1] + 0.5 * e[:, 2]], axis=1))
    if kind == "independent":
        return np.ascontiguousarray(e[:, :2])
    raise ValueError(kind)


# ---- score ------------------------------------------------------------------------------------
class Scorer:
    """g(x, y | B) by two solves; keeps every evaluation and the two-solve spread."""

    def __init__(self, X):
        self.X = np.asarray(X, dtype=np.float64)
        self.T = self.X.shape[0]
        if (self.X.std(axis=0) == 0).any():
            raise ValueError("fges: a column is constant")
        self.delta = 0.0
        self.zmax = 0
        self.evaluated = []                 # (x, y, B sorted, g, bump)
        self._ssr = {}

    def ssr(self, y, P):
        key = (y, tuple(sorted(P)))
        if key not in self._ssr:
            D = np.column_stack([self.X[:, list(key[1])], np.ones(self.T)])
            t = self.X[:, y]
            r1 = t - D @ np.linalg.lstsq(D, t, rcond=None)[0]
            Q = np.linalg.qr(D)[0]
            r2 = t - Q @ (Q.T @ t)
            self._ssr[key] = (float(r1 @ r1), float(r2 @ r2))
        return self._ssr[key]

    def gain(self, x, y, B):
        B = tuple(sorted(B))
        assert x != y and x not in B and y not in B
        if not B:                            # equal both ways in exact arithmetic: one value per pair
            x, y = min(x, y), max(x, y)
        a, b = self.ssr(y, B), self.ssr(y, B + (x,))
        g, g2 = math.log(a[0] / b[0]), math.log(a[1] / b[1])
        self.delta = max(self.delta, abs(g - g2))
        self.zmax = max(self.zmax, len(B))
        return g

    def bump(self, x, y, B):
        """The score change of adding x to the parents B of y."""
        g = self.gain(x, y, B)
        bump = self.T * g - 2.0 * math.log(self.T)
        self.evaluated.append((x, y, tuple(sorted(B)), g, bump))
        return bump


# ---- graph ------------------------------------------------------------------------------------
class Pdag:
    def __init__(self, n):
        self.n = n
        self.out = {v: set() for v in range(n)}

    def arc(self, x, y):
        return y in self.out[x]

    def add(self, x, y):
        self.out[x].add(y)

    def drop(self, x, y):
        self.out[x].discard(y)

    def undirected(self, x, y):
        return self.arc(x, y) and self.arc(y, x)

    def directed(self, x, y):
        return self.arc(x, y) and not self.arc(y, x)

    def adjacent(self, x, y):
        return self.arc(x, y) or self.arc(y, x)

    def around(self, x):
        """Every node with some edge to x, ascending."""
        return [v for v in range(self.n) if v != x and self.adjacent(x, v)]

    def parents(self, x):
        return [v for v in self.around(x) if self.directed(v, x)]

    def children(self, x):
        return [v for v in self.around(x) if self.directed(x, v)]

    def neighbours(self, x):
        return {v for v in self.around(x) if self.undirected(x, v)}

    def na_y_x(self, x, y):
        return {z for z in self.around(y) if self.undirected(z, y) and self.adjacent(z, x)}

    def t_neighbours(self, x, y):
        return {z for z in self.around(y) if self.undirected(z, y) and not self.adjacent(z, x)}

    def clique(self, nodes):
        return all(self.adjacent(a, b) for a in nodes for b in nodes if a != b)

    def orient(self, x, y):
        """Keep only x -> y of an edge that is x - y or already x -> y."""
        if self.undirected(x, y):
            self.drop(y, x)
        elif not self.arc(x, y):
            raise AssertionError("orient: no such edge, or it points the other way")

    def semi_directed_path(self, origin, dest, blocked):
        """Breadth first from origin along arcs that are not against the direction, never
        entering `blocked` (cycle_bound -1 is 1000 levels: no bound at these sizes)."""
        seen, queue = {origin}, [origin]
        while queue:
            t = queue.pop(0)
            if t == dest:
                return True
            for u in self.around(t):
                if not self.arc(t, u) or u in blocked:
                    continue
                if u == dest:
                    return True
                if u not in seen:
                    seen.add(u)
                    queue.append(u)
        return False

    def matrix(self):
        A = np.zeros((self.n, self.n), dtype=np.int64)
        for x in range(self.n):
            for y in self.out[x]:
                A[x, y] = 1
        return A


# ---- Meek rules -------------------------------------------------------------------------------
class Meek:
    def __init__(self, graph, unforce):
        self.g = graph
        self.unforce = unforce
        self.visited = set()
        self.stack = []
        self.oriented = set()

    def run(self, nodes):
        nodes = sorted(nodes)
        self.visited.update(nodes)
        if self.unforce:
            for v in nodes:
                self.undirect_unforced(v)
                self.stack.extend(self.g.around(v))
        for v in nodes:
            self.rules(v)
        while self.stack:
            v = self.stack.pop()
            if self.unforce:
                self.undirect_unforced(v)
            self.rules(v)
        return self.visited

    def undirect_unforced(self, v):
        g = self.g
        par = g.parents(v)
        loose = set(par)
        for p, q in itertools.combinations(par, 2):
            if not g.adjacent(p, q):         # an unshielded collider forces both arrows
                self.oriented.update([(p, v), (q, v)])
                loose.difference_update([p, q])
        changed = False
        for p in sorted(loose):
            if (p, v) not in self.oriented:
                g.drop(p, v)
                g.add(p, v)
                g.add(v, p)
                self.visited.update([v, p])
                changed = True
        if changed:
            self.stack.extend(g.around(v))
            self.stack.append(v)

    def direct(self, a, b):
        g = self.g
        g.drop(a, b)
        g.drop(b, a)
        g.add(a, b)
        self.visited.update([a, b])
        if (a, b) not in self.oriented and (b, a) not in self.oriented:
            self.oriented.add((a, b))
            self.stack.append(b)

    def unshielded_non_collider(self, a, b, c):
        g = self.g
        if not g.adjacent(a, b) or not g.adjacent(c, b) or g.adjacent(a, c):
            return False
        return not (g.directed(a, b) and g.directed(c, b))

    def rules(self, v):
        self.r1(v)
        self.r2(v)
        self.r3(v)
        self.r4(v)

    def r1(self, b):
        adj = self.g.around(b)
        for a, c in itertools.combinations(adj, 2):
            self.r1_one(a, b, c)
            self.r1_one(c, b, a)

    def r1_one(self, a, b, c):
        g, o = self.g, self.oriented
        if g.adjacent(a, c) or not (g.directed(a, b) or (a, b) in o) or not g.undirected(b, c):
            return
        if not self.unshielded_non_collider(a, b, c):
            return
        if (a, c) not in o and (c, a) not in o and (b, c) not in o and (c, b) not in o:
            self.direct(b, c)

    def r2(self, b):
        adj = self.g.around(b)
        for a, c in itertools.combinations(adj, 2):
            for p, q, r in ((a, b, c), (b, a, c), (a, c, b), (c, a, b)):
                if self.g.directed(p, q) and self.g.directed(q, r) and self.g.undirected(p, r):
                    self.direct(p, r)

    def r3(self, x):
        g = self.g
        adj = g.around(x)
        if len(adj) < 3:
            return
        for a in adj:
            if not g.undirected(x, a):
                continue
            for b, c in itertools.combinations([v for v in adj if v != a], 2):
                kite = (g.undirected(a, x) and g.undirected(a, b) and g.undirected(a, c) and g.directed(b, x)
                        and g.directed(c, x))
                if kite and self.unshielded_non_collider(c, a, b):
                    self.direct(a, x)

    def r4(self, a):
        g = self.g
        adj = g.around(a)
        if len(adj) < 3:
            return
        nb = g.neighbours(a)
        for c in adj:
            ba = [v for v in g.parents(c) if v in nb]
            da = [v for v in g.children(c) if v in nb]
            for d in [d for d in da if any(not g.adjacent(b, d) for b in ba)]:
                self.direct(a, d)


# ---- search -----------------------------------------------------------------------------------
class Arrow:
    def __init__(self, a, b, na, ht, bump, index, base):
        self.a, self.b, self.na, self.ht, self.bump, self.index = a, b, frozenset(na), frozenset(ht), bump, index
        self.base = frozenset(base)          # the parent set the bump was scored on
        self.alive = True


class Search:
    def __init__(self, X, mirror="ji"):
        self.sc = Scorer(X)
        self.n = self.sc.X.shape[1]
        self.g = Pdag(self.n)
        self.mirror = mirror
        self.arrows = []                     # the live arrows (the reference's sorted list)
        self.by_pair = {}
        self.index = 0
        self.effect = {v: [] for v in range(self.n)}
        self.stored = {}
        # (phase, a, b, na, ht, bump, gap to the nearest live non-mirror arrow, the arrows alive at the
        # pop as (a, b, na, ht, bump) in the order they were added)
        self.pops = []
        self.inserted = []                   # (x, y, T sorted)
        self.deleted = []                    # (x, y, H sorted)

    # the arrow list
    def add_arrow(self, a, b, na, ht, bump, base):
        ar = Arrow(a, b, na, ht, bump, self.index, base)
        self.index += 1
        self.arrows.append(ar)
        self.by_pair.setdefault((a, b), []).append(ar)

    def clear(self, a, b):
        for ar in self.by_pair.get((a, b), []):
            ar.alive = False
        self.by_pair[(a, b)] = []
        self.arrows = [ar for ar in self.arrows if ar.alive]

    def pop(self, phase):
        best = min(self.arrows, key=lambda ar: (-ar.bump, ar.index))
        best.alive = False
        self.arrows = [ar for ar in self.arrows if ar.alive]
        gap = math.inf
        for ar in self.arrows:
            mirror = (ar.a == best.b and ar.b == best.a
                      and not (ar.na or ar.ht or ar.base or best.na or best.ht or best.base))
            if not mirror:
                gap = min(gap, abs(ar.bump - best.bump))
        alive = [(ar.a, ar.b, tuple(sorted(ar.na)), tuple(sorted(ar.ht)), ar.bump) for ar in self.arrows]
        self.pops.append((phase, best.a, best.b, tuple(sorted(best.na)), tuple(sorted(best.ht)), best.bump, gap, alive))
        return best

    # first step
    def initial_arrows(self):
        for i in range(self.n):
            self.stored[i] = set()
            for j in range(i + 1, self.n):
                b_ij = self.sc.bump(i, j, ())
                b_ji = self.sc.bump(j, i, ())
                if b_ij >= 0 or b_ji >= 0:
                    self.effect[i].append(j)
                    self.effect[j].append(i)
                first = [(b_ji >= 0, j, i), (b_ij >= 0, i, j)]
                for ok, a, b in (first if self.mirror == "ji" else first[::-1]):
                    if ok:
                        self.add_arrow(a, b, (), (), b_ij, ())

    # forward
    def arrows_forward(self, a, b):
        g = self.g
        if b not in self.effect[a]:
            return
        self.stored[b] = g.neighbours(b)
        na = g.na_y_x(a, b)
        if not g.clique(na):
            return
        tn = sorted(g.t_neighbours(a, b))
        previous = {frozenset()}
        for size in range(len(tn) + 1):
            fresh = set()
            for choice in itertools.combinations(tn, size):
                union = set(na) | set(choice)
                if not any(union >= c for c in previous):
                    return
                if not g.clique(union):
                    continue
                fresh.add(frozenset(union))
                base = union | set(g.parents(b))
                bump = self.sc.bump(a, b, base)
                if bump > 0:
                    self.add_arrow(a, b, na, choice, bump, base)
            previous = fresh

    def valid_insert(self, x, y, T, na):
        union = set(T) | set(na)
        return self.g.clique(union) and not self.g.semi_directed_path(y, x, union)

    def fes(self):
        g = self.g
        while self.arrows:
            ar = self.pop("fes")
            x, y = ar.a, ar.b
            if g.adjacent(x, y):
                continue
            na = g.na_y_x(x, y)
            if ar.na != na:
                continue
            if not g.t_neighbours(x, y) >= ar.ht:
                continue
            if not self.valid_insert(x, y, ar.ht, na):
                continue
            g.add(x, y)
            for t in sorted(ar.ht):
                g.orient(t, y)
            self.inserted.append((x, y, tuple(sorted(ar.ht))))
            visited = Meek(g, True).run({x, y})
            todo = {v for v in visited if self.stored.get(v) != g.neighbours(v)} | {x, y}
            for v in sorted(todo):
                for w in self.effect[v]:
                    if w != v and not g.adjacent(v, w):
                        self.clear(w, v)
                        self.arrows_forward(w, v)

    # backward
    def arrows_backward(self, a, b):
        g = self.g
        na = sorted(g.na_y_x(a, b))
        for size in range(len(na) + 1):
            for diff in itertools.combinations(na, size):
                h = set(na) - set(diff)
                base = (set(diff) | set(g.parents(b))) - {a}
                bump = -self.sc.bump(a, b, base)
                if bump > 0:
                    self.add_arrow(a, b, na, h, bump, base)

    def init_backward(self):
        g = self.g
        self.arrows, self.by_pair, self.stored = [], {}, {}
        for x in range(self.n):
            for y in sorted(g.out[x]):
                self.clear(x, y)
                self.clear(y, x)
                self.arrows_backward(x, y)
                self.stored[x] = g.neighbours(x)
                self.stored[y] = g.neighbours(y)

    def bes(self):
        g = self.g
        while self.arrows:
            ar = self.pop("bes")
            x, y = ar.a, ar.b
            if ar.na != g.na_y_x(x, y) or not g.adjacent(x, y) or g.directed(y, x):
                continue                      # (valid_delete is unreachable in the reference: not checked)
            g.drop(x, y)
            g.drop(y, x)
            for v in sorted(ar.ht):
                if g.directed(v, y) or g.directed(v, x):
                    continue
                g.orient(y, v)
                if g.undirected(x, v):
                    g.orient(x, v)
            self.deleted.append((x, y, tuple(sorted(ar.ht))))
            Meek(g, True).run({x, y})
            self.clear(x, y)
            visited = Meek(g, True).run({x, y} | set(ar.ht))
            todo = {v for v in visited if self.stored[v] != g.neighbours(v)} | {x, y}
            todo |= set(g.around(x)) & set(g.around(y))
            for v in sorted(todo):
                self.stored[v] = g.neighbours(v)
                for w in g.around(v):
                    if g.directed(w, v):
                        self.clear(w, v)
                        self.clear(v, w)
                        self.arrows_backward(w, v)
                    elif g.undirected(w, v):
                        self.clear(w, v)
                        self.clear(v, w)
                        self.arrows_backward(w, v)
                        self.arrows_backward(v, w)

    def result(self):
        return {"adj": self.g.matrix(), "inserted": list(self.inserted), "deleted": list(self.deleted),
                "evaluated": list(self.sc.evaluated), "pops": list(self.pops), "delta": self.sc.delta,
                "zmax": self.sc.zmax, "T": self.sc.T, "X": self.sc.X}


def search(X, mirror="ji"):
    s = Search(X, mirror)
    s.initial_arrows()
    s.fes()
    s.init_backward()
    s.bes()
    return s.result()


def bes_from(X, adj):
    """BES alone from a start graph given as an adjacency matrix (adj[i, j] = 1: an arc i -> j)."""
    s = Search(X)
    for i, j in zip(*np.nonzero(np.asarray(adj))):
        s.g.add(int(i), int(j))
    s.init_backward()
    s.bes()
    return s.result()


@functools.lru_cache(maxsize=None)
def case(T, n, seed, mirror="ji"):
    return search(gen_dag(T, n, seed), mirror)


def preconditions(ref):
    """What the exact comparisons need of the restatement's own run: the smallest |bump| evaluated
    and the smallest gap at a pop between the popped arrow and any live arrow that is not its mirror."""
    return {"min_bump": min((abs(e[4]) for e in ref["evaluated"]), default=math.inf),
            "min_gap": min((p[6] for p in ref["pops"]), default=math.inf), "zmax": ref["zmax"]}
