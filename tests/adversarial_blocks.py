"""Block-diagonal correlation matrices that put near-threshold and ill-conditioned tests at
depths 2, 3 and 4 of the PC skeleton, with the truth known by construction.

One block at target depth d has d + 2 core nodes x, y, s_1..s_d and is built from its precision
matrix P = I - R (R symmetric, zero diagonal): with a unit diagonal in P the full-order partial
correlation of i and j is exactly R_ij. R_xy = +-thr_d sqrt(1 + delta) puts the only depth-d test
of (x, y), the one given all of s_1..s_d, at r^2 = thr_d^2 (1 + delta); every other core entry is a
positive background value, so lower-order correlations only add up and the edge x - y survives
the shallower depths. ``extra`` padding nodes are attached in R to the s nodes only: marginalising
them changes P inside the S x S block alone, so the designed test keeps its value while degrees,
T-groups and candidates per group grow. The ill-conditioned variant replaces s_2 by s_1 + eps s_2
(C <- A C A^T): span{s_1, s_2} is unchanged, so every test whose S holds both keeps its value, but
C_SS gets a Cholesky pivot^2 ~ eps^2, below the conditioning guard of the fast paths. Cross-block
correlations are exactly 0; a seeded permutation of the indices mixes the roles' order and lets
blocks straddle 64-bit mask words. A drawn block is kept only if the oracle, run on the block
alone, brings the target pair to depth d.

Everything is deterministic from the seed; numpy, scipy and the oracle only.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

ALPHA = 0.05
COND_TAU = 1e-4            # = PCG_COND_TAU (rcaeval_amd/csrc/skeleton.hip)
BAND = 1e-6                # decide()'s band on r^2: thr^2 (1 +- 1e-6)


def threshold_r(N: int, d: int, alpha: float = ALPHA) -> float:
    from scipy.stats import norm
    return math.tanh(norm.ppf(1 - alpha / 2) / math.sqrt(N - d - 3))


def _dp_ddelta(N: int, d: int, alpha: float = ALPHA) -> float:
    """|d p / d delta| at the threshold, r^2 = thr^2 (1 + delta)."""
    from scipy.stats import norm
    r = threshold_r(N, d, alpha)
    z = norm.ppf(1 - alpha / 2)
    return 2.0 * norm.pdf(z) * math.sqrt(N - d - 3) * 0.5 * r / (1.0 - r * r)


def _delta(i: int, rng, N: int, d: int) -> float:
    """Stratified log-uniform |delta|, both signs. Even draws go below the fp32 decision's reach:
    stratum j = (i / 2) mod 4 puts |p - alpha| in the decade [1e-8, 1e-7) * 10^j (floor: no
    designed test within 1e-9 of alpha); odd draws alternate over 1e-3..1e-2 and 1e-2..1e-1, where
    the fp32 decision itself is made."""
    u = rng.random()
    if i % 2 == 0:
        mag = 10.0 ** (u * 0.98 + 0.01 + (i // 2) % 4 - 8) / _dp_ddelta(N, d)
    else:
        mag = 10.0 ** (u + (i // 2) % 2 - 3)
    return mag if rng.random() < 0.5 else -mag


def _unit_diag(C):
    s = 1.0 / np.sqrt(np.diag(C))
    C = C * s[:, None] * s[None, :]
    C = 0.5 * (C + C.T)
    np.fill_diagonal(C, 1.0)
    return C


def _block(d, N, extra, rho, delta, eps, rng):
    """One block in role order (x, y, s_1..s_d, padding...); None if not positive definite."""
    m = d + 2
    k = m + extra
    R = np.zeros((k, k))
    iu = np.triu_indices(m, 1)
    R[iu] = rho * rng.uniform(0.7, 1.3, len(iu[0]))
    R[0, 1] = (1.0 if rng.random() < 0.5 else -1.0) * threshold_r(N, d) * math.sqrt(1.0 + delta)
    R[2:m, m:] = rho * rng.uniform(0.7, 1.3, (d, extra))
    R = R + R.T
    P = np.eye(k) - R
    if np.linalg.eigvalsh(P)[0] < 0.05:
        return None
    C = np.linalg.inv(P)
    if eps is not None:
        A = np.eye(k)
        A[3, 3] = eps
        A[3, 2] = 1.0
        C = A @ C @ A.T
    return _unit_diag(C)


@dataclass
class Family:
    name: str
    d: int
    N: int
    C: np.ndarray                 # n x n correlation matrix
    targets: np.ndarray           # per block: x, y, delta, eps (nan: well-conditioned), s (d indices)
    block_of: np.ndarray          # n: block of every variable
    ill: bool
    extra: int
    meta: dict = field(default_factory=dict)

    @property
    def n(self):
        return len(self.C)


TARGET_DTYPE = np.dtype([("x", np.int32), ("y", np.int32), ("delta", np.float64), ("eps", np.float64),
                         ("s", np.int32, 4)])


def family(d, N, nblocks, seed, extra=0, rho=0.1, ill=True, name=None) -> Family:
    """``nblocks`` accepted blocks of d + 2 + extra variables each, every second one
    ill-conditioned when ``ill``."""
    from oracle import cpc
    rng = np.random.default_rng(seed)
    k = d + 2 + extra
    blocks, tg = [], []
    draws = 0
    while len(blocks) < nblocks:
        i = len(blocks)
        draws += 1
        if draws > 40 * nblocks:
            raise RuntimeError(f"family {name}: too few blocks reach depth {d}")
        delta = _delta(i, rng, N, d)
        # every second block of each delta stratum (_delta's strata repeat every 8 blocks for
        # even i, every 4 for odd i), so conditioning and delta are not tied to each other
        is_ill = ill and ((i // 4) % 2 if i % 2 else (i // 8) % 2)
        eps = 10.0 ** rng.uniform(-5.0, math.log10(3e-3)) if is_ill else None
        B = _block(d, N, extra, rho, delta, eps, rng)
        if B is None:
            continue
        ref = cpc.skeleton(B, N, max_depth=d, want_union=False, nthreads=1)
        if ref.error or len(ref.near_alpha) or ref.removed_level[0, 1] not in (-1, d):
            continue
        blocks.append(B)
        tg.append((delta, np.nan if eps is None else eps))
    n = k * nblocks
    C = np.zeros((n, n))
    for b, B in enumerate(blocks):
        C[b * k:(b + 1) * k, b * k:(b + 1) * k] = B
    perm = rng.permutation(n)                 # new index of old variable i
    inv = np.argsort(perm)
    C = np.ascontiguousarray(C[np.ix_(inv, inv)])
    targets = np.zeros(nblocks, TARGET_DTYPE)
    for b, (delta, eps) in enumerate(tg):
        targets[b] = (perm[b * k], perm[b * k + 1], delta, eps, tuple(perm[b * k + 2:b * k + 2 + d]) + (-1,) * (4 - d))
    block_of = np.empty(n, np.int32)
    block_of[perm] = np.arange(n) // k
    return Family(name or f"d{d}_x{extra}_N{N}", d, N, C, targets, block_of, ill, extra,
                  {"draws": draws, "rho": rho, "seed": seed})


# (name, d, N, nblocks, seed, extra, rho, ill)
FAMILIES = [
    ("d4_x0", 4, 10000, 48, 40, 0, 0.12, True),
    ("d4_x2", 4, 10000, 32, 42, 2, 0.08, True),
    ("d4_x7", 4, 10000, 32, 47, 7, 0.05, True),        # D = 12: ragged T-groups, the largest shape
    ("d4_x2_N2500", 4, 2500, 32, 50, 2, 0.11, True),    # a second threshold (thr 0.039 instead of 0.0196)
    ("d3_x0", 3, 10000, 48, 30, 0, 0.15, True),
    ("d3_x3", 3, 10000, 32, 33, 3, 0.10, True),
    ("d2_x0", 2, 10000, 80, 20, 0, 0.20, True),
    ("d4_tiny", 4, 10000, 10, 45, 0, 0.12, True),       # n = 60: k_pc_small's range
]
TINY = "d4_tiny"
BY_NAME = {f[0]: f for f in FAMILIES}

_CACHE: dict = {}


def get(name: str) -> Family:
    if name not in _CACHE:
        nm, d, N, nb, seed, extra, rho, ill = BY_NAME[name]
        _CACHE[name] = family(d, N, nb, seed, extra=extra, rho=rho, ill=ill, name=nm)
    return _CACHE[name]


RECORD_CAP = 1 << 21      # above every family's unique tests over all depths (d4_x7: ~8.2e5)
_REF: dict = {}


def oracle_run(fam: Family, record_cap: int = RECORD_CAP):
    from oracle import cpc
    return cpc.skeleton(fam.C, fam.N, max_depth=fam.d, record_cap=record_cap)


def get_ref(name: str):
    """(family, its oracle run with every record), computed once per process and left unchanged."""
    if name not in _REF:
        fam = get(name)
        _REF[name] = (fam, oracle_run(fam))
    return _REF[name]


# ------------------------------------------------------------------ numpy census of depth-d records
def depth_records(ref, d):
    rec = ref.records
    return rec[rec["d"] == d]


def _chol_min_pivot2(M):
    """min squared Cholesky pivot of a batch (B, k, k), in the given order; <= 0 past a bad pivot."""
    B, k, _ = M.shape
    L = np.zeros_like(M)
    g = np.full(B, np.inf)
    with np.errstate(all="ignore"):
        for j in range(k):
            p2 = M[:, j, j] - (L[:, j, :j] ** 2).sum(1)
            g = np.minimum(g, np.where(np.isnan(p2), -1.0, p2))
            L[:, j, j] = np.sqrt(p2)
            for i in range(j + 1, k):
                L[:, i, j] = (M[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(1)) / L[:, j, j]
    return g


def census(fam: Family, rec):
    """Of depth-d oracle records: r^2 / thr^2 - 1 (fp64 LU on C), the min Cholesky pivot^2 of C_SS
    (S sorted), the order-free bound 1 - max C_ij^2 over i != j in S (an upper bound of the
    min pivot^2 in any elimination order) and c_xx c_yy - c_xy^2, the determinant of the
    conditional covariance of (x, y) given S."""
    d, C = fam.d, fam.C
    S = rec["s"][:, :d].astype(np.int64)
    idx = np.concatenate([rec["a"][:, None], rec["b"][:, None], S], axis=1).astype(np.int64)
    Cb = C[idx[:, :, None], idx[:, None, :]]
    Pm = np.linalg.inv(Cb)
    r2 = Pm[:, 0, 1] ** 2 / (Pm[:, 0, 0] * Pm[:, 1, 1])
    CSS = Cb[:, 2:, 2:]
    gpiv = _chol_min_pivot2(CSS)
    off = CSS - np.eye(d)[None]
    gpair = 1.0 - (off ** 2).max(axis=(1, 2))
    dn = 1.0 / (Pm[:, 0, 0] * Pm[:, 1, 1] - Pm[:, 0, 1] ** 2)
    return {"rel": r2 / threshold_r(fam.N, d) ** 2 - 1.0, "gpiv": gpiv, "gpair": gpair, "dn": dn, "blocks": Cb}


def must_mask(fam: Family, rec, band: bool = True) -> np.ndarray:
    """Depth-d tests no fp32 (or fp64 Cholesky) path may decide: r^2 inside decide()'s band, or
    decide()'s guard c_xx c_yy - c_xy^2 <= tau / g certain to hold with a factor 2 to spare,
    whatever the elimination order behind the smallest pivot^2 g of C_SS: g is at most
    1 - max C_ij^2 over S. Both sides are at most 1, so this takes in every near-collinear S
    (g < tau / 2) and every pair nearly collinear given S (left side < tau / 2, as s_1 and s_2 of
    an ill-conditioned block are). ``band=False``: the guard alone (full-p mode computes p on
    the fast path and has no band)."""
    c = census(fam, rec)
    guard = c["dn"] * c["gpair"] < 0.5 * COND_TAU
    return guard | (np.abs(c["rel"]) < BAND) if band else guard


def must_be_exact(fam: Family, rec) -> int:
    return int(must_mask(fam, rec).sum())


def decade_counts(rec, lo=-8, hi=-2):
    """Depth-d tests per decade of |p - alpha|: [1e-8, 1e-7), ..., [1e-3, 1e-2), then the rest."""
    a = np.abs(rec["p"] - ALPHA)
    e = np.floor(np.log10(np.maximum(a, 1e-300))).astype(int)
    return [int((e == k).sum()) for k in range(lo, hi)] + [int((e >= hi).sum())]


# ------------------------------------------------------------------ the numpy model of the fp32 screen
def target_screen_blocks(fam: Family):
    """The designed tests as the fp32 sweep sees them: (B, d + 2, d + 2) blocks ordered
    (x, y, c, T...) for every choice of the candidate c in S, from x's side and from y's."""
    rows = []
    for t in fam.targets:
        S = sorted(int(v) for v in t["s"][:fam.d])
        for x, y in ((int(t["x"]), int(t["y"])), (int(t["y"]), int(t["x"]))):
            for c in S:
                rows.append([x, y, c] + [s for s in S if s != c])
    idx = np.asarray(rows, dtype=np.int64)
    return fam.C[idx[:, :, None], idx[:, None, :]]


def model_undecided_share(fam: Family, rec) -> float:
    """Share of depth-d oracle tests the numpy model of the fp32 screen (test_screen32_cpu) leaves
    undecided, taking each test from a's side with c = the first of S."""
    from test_screen32_cpu import _screen_blocks
    if not len(rec):
        return float("nan")
    with np.errstate(all="ignore"):
        dep32, ind32, _, _ = _screen_blocks(census(fam, rec)["blocks"], fam.N)
    return 1.0 - float((dep32 | ind32).mean())
