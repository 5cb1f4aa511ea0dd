// fges.hip — the linear-Gaussian score of fGES (RCAEval's fges graph learner, fges_pagerank and
// fges_randomwalk).
//
// Replaces the statsmodels.OLS fits behind LIB/python/scores.py:142-171 as
// LIB/libraries/FGES/fges_main.py:553-568, :658-676 call them. The bump of adding x to the parents
// B of y is T g - 2 log T with g = log(SSR(y|B) / SSR(y|B + x)) = -log(1 - rho^2(x, y . B)), a
// function of the ddof-0 correlation matrix R of the data alone. The device computes g; the host
// (graph_construction/fges.py) applies T and the penalty and runs the search ("fGES").
//
//   k_fg_cols     one block per column: constant / non-finite flags, the standardized columns E
//                 (a flagged column is written as a +-1 pattern so K1 never sees it; every item
//                 that touches a flagged column is refused by status before R is read).
//   k_fg_gain0    the n x n depth-0 gains -log1p(-r^2); a pair with 1 - r^2 below the guard is counted
//                 and left to k_fg_gain0_exact, the exact path with an empty base.
//   k_fg_groups   one workgroup per group (y, B, candidates): R[B + y] is Cholesky-factored once in
//                 LDS, y's factor row and coefficient norm are taken once, then the candidates are
//                 spread over the waves: a forward substitution (a lane per row) and two dot
//                 products each, and a back substitution for the coefficient-norm guard. Groups of
//                 up to FG_NARROW candidates run as one wave per group (64-thread workgroups),
//                 wider ones as four waves; the caller lists the narrow groups first, so each
//                 launch covers its own groups only and an empty kind is not launched. The
//                 33 KB work matrix per workgroup leaves the one-wave kind at one wave per SIMD
//                 (four groups per CU): these batches are bound by launch latency, not occupancy.
//   k_fg_exact    the exact path: Householder QR on the columns of E themselves, one block per item.
// The block sums, the column classification, the Cholesky of the fast path (chol_eliminate) and the
// QR of the exact path (qr_eliminate) are dense_dev.h's, shared with pcmci.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "dense_dev.h"
#include "handle.h"

namespace {

constexpr int FG_BLOCK = 256;
constexpr int FG_BCAP = 62;               // largest |B|: {B, x, y} is at most 64 x 64 doubles
constexpr int FG_LD = 65;                 // row stride of the LDS work matrix: a lane per row reads a column conflict-free
constexpr int FG_MAXN = 8192;
constexpr int FG_NARROW = 4;              // groups of up to this many candidates run as one wave
// fast-path guards: smallest pivot of the unit-diagonal factorisation and smallest
// residual variance of y given B and given B + x, and the bound on (1 + |h|_1)^2 of the regression
// coefficients h of y on B + x
constexpr double FG_TAU = 1e-2;
constexpr double FG_BETA_C = 400.0;
constexpr int64_t FG_WS_BYTES = (int64_t)1 << 30;    // exact path: design workspace bound
constexpr int FG_EXACT_BLOCKS = 256;

__global__ __launch_bounds__(FG_BLOCK) void k_fg_cols(const double *X, int64_t T, int n, int64_t ldx, int32_t *flags,
                                                      int32_t *status, double *E) {
    __shared__ double red[FG_BLOCK / 64];
    __shared__ double mm[3 * (FG_BLOCK / 64)];
    const int c = blockIdx.x, tid = threadIdx.x;
    const double *x = X + c;
    double lo = INFINITY, hi = -INFINITY, bad = 0.0, s = 0.0;
    for (int64_t r = tid; r < T; r += FG_BLOCK) {
        const double v = x[r * ldx];
        if (isfinite(v)) {
            lo = fmin(lo, v);
            hi = fmax(hi, v);
            s += v;
        } else
            bad = 1.0;
    }
    const int fl = column_class<FG_BLOCK>(lo, hi, bad, mm);   // block-uniform
    const double mu = block_sum<FG_BLOCK>(s, red) / (double)T;
    double q = 0.0;
    if (!fl)
        for (int64_t r = tid; r < T; r += FG_BLOCK) {
            const double v = x[r * ldx] - mu;
            q = fma(v, v, q);
        }
    const double isd = 1.0 / sqrt(block_sum<FG_BLOCK>(q, red) / (double)T);
    for (int64_t r = tid; r < T; r += FG_BLOCK) E[r * n + c] = fl ? ((r & 1) ? 1.0 : -1.0) : (x[r * ldx] - mu) * isd;
    if (tid == 0) {
        flags[c] = fl;
        status[c] = fl;
    }
}

__global__ __launch_bounds__(FG_BLOCK) void k_fg_gain0(const double *R, int n, const int32_t *flags, double *gain0,
                                                       unsigned int *counter) {
    const int64_t total = (int64_t)n * n;
    for (int64_t idx = (int64_t)blockIdx.x * FG_BLOCK + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * FG_BLOCK) {
        const int i = (int)(idx / n), j = (int)(idx % n);
        double g = __builtin_nan("");
        if (i != j && !(flags[i] | flags[j])) {
            const int a = i < j ? i : j, b = i < j ? j : i;       // one value per unordered pair
            const double r = R[(int64_t)a * n + b];
            if (1.0 - r * r >= FG_TAU)
                g = -log1p(-r * r);
            else if (i < j)                                       // left NaN for k_fg_gain0_exact
                atomicAdd(counter, 1u);
        }
        gain0[idx] = g;
    }
}

__global__ __launch_bounds__(FG_BLOCK) void k_fg_fill(int64_t n_items, double *gain, int32_t *status) {
    for (int64_t it = (int64_t)blockIdx.x * FG_BLOCK + threadIdx.x; it < n_items; it += (int64_t)gridDim.x * FG_BLOCK) {
        gain[it] = __builtin_nan("");
        status[it] = 4;
    }
}

// |g|_1 of g = L^-T w over one wave: lane k < d enters with entry k of the factor row w; column
// oriented back substitution, lane r reads L(k, r). Every lane returns the norm. Not shared with
// pcmci.hip's one-thread form, nor are k_fg_groups' lane-per-row solves: another launch shape.
__device__ inline double fg_coef_norm1(const double *A, double w, int d, int lane) {
    double n1 = 0.0;
    for (int k = d - 1; k >= 0; --k) {
        const double gk = __shfl(w, k, 64) / A[k * FG_LD + k];
        n1 += fabs(gk);
        if (lane < k) w -= A[k * FG_LD + lane] * gk;
    }
    return n1;
}

struct FgGroups {
    const int32_t *grp_y, *base_off, *base_ids, *item_off, *item_x;
    int64_t n_groups, n_base, n_items;
};

// NT = 64: the groups of up to FG_NARROW candidates, one wave each; NT = 256: the wider ones.
template <int NT>
__global__ __launch_bounds__(NT) void k_fg_groups(const double *R, int n, const int32_t *flags, FgGroups in, double *gain,
                                                  int32_t *status, int32_t *list, unsigned int *counter, int64_t g_lo,
                                                  int64_t g_hi) {
    __shared__ double A[64 * FG_LD];
    __shared__ int cols[64];
    __shared__ int sh_st, sh_fl;
    __shared__ double sh_n1y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t g = g_lo + blockIdx.x; g < g_hi; g += gridDim.x) {
        const int64_t lo = in.item_off[g], hi = in.item_off[g + 1];
        if (lo < 0 || hi > in.n_items || hi <= lo) continue;              // nothing of this group can be written
        if (((hi - lo) > FG_NARROW) != (NT > 64)) continue;               // listed on the wrong side: refused
        const int64_t bo = in.base_off[g], be = in.base_off[g + 1];
        const int y = in.grp_y[g];
        __syncthreads();
        if (tid == 0) {
            sh_st = (bo < 0 || be > in.n_base || be < bo || be - bo > FG_BCAP || y < 0 || y >= n) ? 4 : 0;
            sh_fl = 0;
        }
        __syncthreads();
        if (sh_st) continue;                                              // block-uniform: the items keep status 4
        const int d = (int)(be - bo);
        for (int k = tid; k < d; k += NT) {
            const int q = in.base_ids[bo + k];
            const bool ok = q >= 0 && q < n && q != y;
            cols[k] = ok ? q : 0;                                         // a refused id is never used as an index
            if (!ok)
                atomicOr(&sh_st, 4);
            else if (flags[q])
                atomicOr(&sh_fl, flags[q]);
        }
        if (tid == 0) {
            cols[d] = y;
            if (flags[y]) atomicOr(&sh_fl, flags[y]);
        }
        __syncthreads();
        for (int idx = tid; idx < d * d; idx += NT) {
            const int i = idx / d, j = idx % d;
            if (i < j && cols[i] == cols[j]) atomicOr(&sh_st, 4);
        }
        __syncthreads();
        if (sh_st) continue;
        const int gfl = sh_fl;
        bool shared_ok = false;
        double syy = 0.0, n1y = 0.0;
        if (!gfl) {                                                       // block-uniform
            shared_ok = chol_eliminate<NT, FG_LD>(R, n, cols, d + 1, d, A, FG_TAU);
            if (shared_ok) {
                syy = A[d * FG_LD + d];
                if (wave == 0) {
                    const double v = fg_coef_norm1(A, lane < d ? A[d * FG_LD + lane] : 0.0, d, lane);
                    if (lane == 0) sh_n1y = v;
                }
            }
            __syncthreads();
            if (shared_ok) n1y = sh_n1y;
            shared_ok = shared_ok && syy >= FG_TAU && (1.0 + n1y) * (1.0 + n1y) <= FG_BETA_C;
        }
        for (int64_t it = lo + wave; it < hi; it += NT / 64) {            // wave-uniform from here on
            const int x = in.item_x[it];
            if (x < 0 || x >= n || x == y) continue;
            if (__any(lane < d && cols[lane] == x)) continue;
            const int fl = gfl | flags[x];
            if (fl) {
                if (lane == 0) status[it] = (fl & 2) ? 2 : 1;
                continue;
            }
            bool ok = shared_ok;
            double val = 0.0;
            if (ok) {
                const double *rx = R + (int64_t)x * n;
                double v = lane < d ? rx[cols[lane]] : 0.0, b = 0.0;
                for (int c = 0; c < d; ++c) {                             // b = L^-1 R[B, x], a lane per row
                    const double bc = __shfl(v, c, 64) / A[c * FG_LD + c];
                    if (lane == c) b = bc;
                    if (lane > c && lane < d) v -= A[lane * FG_LD + c] * bc;
                }
                const double sxx = 1.0 - wave_sum(b * b);
                const double sxy = rx[y] - wave_sum(lane < d ? b * A[d * FG_LD + lane] : 0.0);
                const double n1x = fg_coef_norm1(A, b, d, lane);
                const double gamma = sxy / sxx, syyx = syy - sxy * gamma;
                const double h1 = 1.0 + n1y + fabs(gamma) * (1.0 + n1x);
                ok = sxx >= FG_TAU && syyx >= FG_TAU && h1 * h1 <= FG_BETA_C;
                val = log(syy / syyx);
            }
            if (lane == 0) {
                if (ok) {
                    gain[it] = val;
                    status[it] = 0;
                } else {
                    // listed once, whatever overlapping item ranges of malformed offsets do
                    if (atomicExch(&status[it], 3) != 3) {
                        const unsigned int slot = atomicAdd(counter, 1u);
                        if ((int64_t)slot < in.n_items) {
                            list[2 * (int64_t)slot] = (int32_t)it;
                            list[2 * (int64_t)slot + 1] = (int32_t)g;
                        }
                    }
                }
            }
        }
    }
}

// One item on the exact path: the columns cols = [B (d), x, y] of E (already standardized) into the
// block's workspace Aw (column-major, m x T), Householder QR over the B columns, then over x
// (dense_dev.h's qr_eliminate: a dependent column is skipped); g = log of the ratio of y's remaining
// sums of squares before and after x. Each thread owns the rows r = tid, tid + FG_BLOCK, ..
__device__ double fg_exact_item(const double *E, int64_t T, int n, const int *cols, int d, double *Aw, double *red) {
    const int tid = threadIdx.x, m = d + 2;
    __syncthreads();
    for (int u = 0; u < m; ++u) {
        const double *e = E + cols[u];
        double *au = Aw + (int64_t)u * T;
        for (int64_t r = tid; r < T; r += FG_BLOCK) au[r] = e[r * n];
    }
    const double tol = (double)std::max<int64_t>(T, m) * 2.220446049250313e-16;
    const double *ay = Aw + (int64_t)(d + 1) * T;
    int64_t rdone = qr_eliminate<FG_BLOCK>(Aw, T, m, 0, d, 0, tol, red);
    double syy = 0.0;                                              // B is eliminated: SSR(y | B)
    for (int64_t r = tid; r < T; r += FG_BLOCK)
        if (r >= rdone) syy = fma(ay[r], ay[r], syy);
    syy = block_sum<FG_BLOCK>(syy, red);
    rdone = qr_eliminate<FG_BLOCK>(Aw, T, m, d, d + 1, rdone, tol, red);
    double syyx = 0.0;
    for (int64_t r = tid; r < T; r += FG_BLOCK)
        if (r >= rdone) syyx = fma(ay[r], ay[r], syyx);
    syyx = block_sum<FG_BLOCK>(syyx, red);
    return log(syy / syyx);
}

__global__ __launch_bounds__(FG_BLOCK) void k_fg_exact(const double *E, int64_t T, int n, FgGroups in, const int32_t *list,
                                                       int64_t count, double *work, int64_t slot, double *gain) {
    __shared__ double red[FG_BLOCK / 64];
    __shared__ int cols[64];
    const int tid = threadIdx.x;
    double *Aw = work + (int64_t)blockIdx.x * slot;
    for (int64_t q = blockIdx.x; q < count; q += gridDim.x) {
        // a listed item passed every check of k_fg_groups: its ids are in range and distinct
        const int64_t it = list[2 * q], g = list[2 * q + 1];
        const int64_t bo = in.base_off[g];
        const int d = (int)(in.base_off[g + 1] - bo);
        __syncthreads();
        for (int k = tid; k < d; k += FG_BLOCK) cols[k] = in.base_ids[bo + k];
        if (tid == 0) {
            cols[d] = in.item_x[it];
            cols[d + 1] = in.grp_y[g];
        }
        const double val = fg_exact_item(E, T, n, cols, d, Aw, red);
        if (tid == 0) gain[it] = val;
    }
}

// The depth-0 pairs k_fg_gain0 left: the exact path with an empty base, one block per pair (every
// block scans the pairs i < j in the same order and takes each one that fails the guard in turn).
__global__ __launch_bounds__(FG_BLOCK) void k_fg_gain0_exact(const double *R, const double *E, int64_t T, int n,
                                                             const int32_t *flags, double *work, int64_t slot,
                                                             double *gain0) {
    __shared__ double red[FG_BLOCK / 64];
    __shared__ int cols[2];
    double *Aw = work + (int64_t)blockIdx.x * slot;
    int64_t seen = 0;
    for (int i = 0; i < n; ++i) {
        if (flags[i]) continue;
        for (int j = i + 1; j < n; ++j) {
            const double r = R[(int64_t)i * n + j];
            if (flags[j] || 1.0 - r * r >= FG_TAU) continue;      // block-uniform
            if (seen++ % gridDim.x != blockIdx.x) continue;
            __syncthreads();
            if (threadIdx.x == 0) {
                cols[0] = i;
                cols[1] = j;
            }
            const double val = fg_exact_item(E, T, n, cols, 0, Aw, red);
            if (threadIdx.x == 0) gain0[(int64_t)i * n + j] = gain0[(int64_t)j * n + i] = val;
        }
    }
}

// fges_small: column flags (n int32) | the exact-list counter
struct FgSmall {
    int32_t *flags;
    unsigned int *counter;
};
bool fg_small(pcg_handle *h, int64_t n, FgSmall &s) {
    Carve cv;
    const size_t o_flags = cv.take((size_t)n * 4), o_ctr = cv.take(4);
    if (!pcg_ensure(h, h->fges_small, cv.total)) return false;
    s.flags = (int32_t *)((char *)h->fges_small.p + o_flags);
    s.counter = (unsigned int *)((char *)h->fges_small.p + o_ctr);
    return true;
}

}  // namespace

extern "C" int pcg_fges_limits(int32_t *b_cap, int32_t *max_n, int32_t *narrow_max, double *tau, double *beta_c) {
    if (b_cap) *b_cap = FG_BCAP;
    if (max_n) *max_n = FG_MAXN;
    if (narrow_max) *narrow_max = FG_NARROW;
    if (tau) *tau = FG_TAU;
    if (beta_c) *beta_c = FG_BETA_C;
    return PCG_OK;
}

extern "C" int pcg_fges_begin(pcg_handle *h, const double *X, int64_t T, int64_t n, int64_t ldx, double *gain0,
                              int32_t *status) {
    if (!h) return PCG_ERR_INVALID;
    h->fges_ok = false;
    if (n < 1 || n > FG_MAXN || T < 2 || ldx < n)
        return pcg_fail(h, PCG_ERR_INVALID, "pcg_fges_begin: bad shape (T=%lld n=%lld ldx=%lld: 1 <= n <= %d, T >= 2, ldx >= n)",
                        (long long)T, (long long)n, (long long)ldx, FG_MAXN);
    if (T * 64 * 8 > FG_WS_BYTES)
        return pcg_fail(h, PCG_ERR_INVALID, "pcg_fges_begin: T * 512 B of exact-path workspace exceeds %lld B",
                        (long long)FG_WS_BYTES);
    if (!X || !gain0 || !status) return pcg_fail(h, PCG_ERR_INVALID, "pcg_fges_begin: null pointer");
    PCG_HIP(h, hipSetDevice(h->device));
    FgSmall s;
    if (!pcg_ensure(h, h->fges_e, (size_t)(T * n * 8)) || !pcg_ensure(h, h->fges_r, (size_t)(n * n * 8)) || !fg_small(h, n, s))
        return pcg_fail(h, PCG_ERR_OOM, "pcg_fges_begin: scratch");
    double *E = (double *)h->fges_e.p, *R = (double *)h->fges_r.p;
    hipLaunchKernelGGL(k_fg_cols, dim3((unsigned)n), dim3(FG_BLOCK), 0, h->stream, X, T, (int)n, ldx, s.flags, status, E);
    PCG_HIP(h, hipGetLastError());
    const int rc = pcg_corr_launch(h, E, T, n, n, R, n);
    if (rc) return rc;
    PCG_HIP(h, hipMemsetAsync(s.counter, 0, 4, h->stream));
    const unsigned gb = (unsigned)std::min<int64_t>((n * n + FG_BLOCK - 1) / FG_BLOCK, 2048);
    hipLaunchKernelGGL(k_fg_gain0, dim3(gb), dim3(FG_BLOCK), 0, h->stream, (const double *)R, (int)n,
                       (const int32_t *)s.flags, gain0, s.counter);
    PCG_HIP(h, hipGetLastError());
    int64_t left = 0;                                             // pairs i < j, counted and not listed
    if (int rc1 = pcg_read_counter(h, "pcg_fges_begin", s.counter, n * n, &left)) return rc1;
    if (left) {                                                   // near-duplicate columns: rare
        const int64_t eblocks = std::min<int64_t>(left, FG_EXACT_BLOCKS), slot = 2 * T;
        if (!pcg_ensure(h, h->fges_work, (size_t)(eblocks * slot * 8)))
            return pcg_fail(h, PCG_ERR_OOM, "pcg_fges_begin: exact-path workspace");
        hipLaunchKernelGGL(k_fg_gain0_exact, dim3((unsigned)eblocks), dim3(FG_BLOCK), 0, h->stream, (const double *)R,
                           (const double *)E, T, (int)n, (const int32_t *)s.flags, (double *)h->fges_work.p, slot, gain0);
        PCG_HIP(h, hipGetLastError());
        PCG_HIP(h, hipStreamSynchronize(h->stream));
    }
    h->fges_shape[0] = T;
    h->fges_shape[1] = n;
    h->fges_ok = true;
    return PCG_OK;
}

extern "C" int pcg_fges_gains(pcg_handle *h, int64_t n_groups, const int32_t *grp_y, const int32_t *base_off,
                              const int32_t *base_ids, int64_t n_base, const int32_t *item_off, const int32_t *item_x,
                              int64_t n_items, int64_t n_narrow, double *gain, int32_t *status, int64_t *exact_items) {
    if (!h) return PCG_ERR_INVALID;
    if (!h->fges_ok) return pcg_fail(h, PCG_ERR_INVALID, "pcg_fges_gains: no pcg_fges_begin on the handle");
    if (n_groups < 0 || n_base < 0 || n_items < 0 || n_narrow < 0 || n_narrow > n_groups || n_groups > INT32_MAX || n_base > INT32_MAX || n_items > INT32_MAX / 2)
        return pcg_fail(h, PCG_ERR_INVALID, "pcg_fges_gains: counts out of range (groups %lld, narrow %lld, base ids %lld, items %lld)",
                        (long long)n_groups, (long long)n_narrow, (long long)n_base, (long long)n_items);
    if (exact_items) *exact_items = 0;
    if (n_items == 0) return PCG_OK;
    if (!grp_y || !base_off || !item_off || !item_x || !gain || !status || (n_base > 0 && !base_ids))
        return pcg_fail(h, PCG_ERR_INVALID, "pcg_fges_gains: null pointer");
    PCG_HIP(h, hipSetDevice(h->device));
    const int64_t T = h->fges_shape[0], n = h->fges_shape[1], slot = T * 64;
    FgSmall s;
    if (!fg_small(h, n, s) || !pcg_ensure(h, h->fges_list, (size_t)n_items * 8))
        return pcg_fail(h, PCG_ERR_OOM, "pcg_fges_gains: scratch");
    int32_t *list = (int32_t *)h->fges_list.p;
    PCG_HIP(h, hipMemsetAsync(s.counter, 0, 4, h->stream));
    const unsigned fb = (unsigned)std::min<int64_t>((n_items + FG_BLOCK - 1) / FG_BLOCK, 2048);
    hipLaunchKernelGGL(k_fg_fill, dim3(fb), dim3(FG_BLOCK), 0, h->stream, n_items, gain, status);
    PCG_HIP(h, hipGetLastError());
    if (n_groups > 0) {
        const FgGroups in{grp_y, base_off, base_ids, item_off, item_x, n_groups, n_base, n_items};
        if (n_narrow > 0) {
            hipLaunchKernelGGL(k_fg_groups<64>, dim3((unsigned)std::min<int64_t>(n_narrow, 16384)), dim3(64), 0, h->stream,
                               (const double *)h->fges_r.p, (int)n, (const int32_t *)s.flags, in, gain, status, list,
                               s.counter, (int64_t)0, n_narrow);
            PCG_HIP(h, hipGetLastError());
        }
        if (n_groups > n_narrow) {
            hipLaunchKernelGGL(k_fg_groups<FG_BLOCK>, dim3((unsigned)std::min<int64_t>(n_groups - n_narrow, 16384)),
                               dim3(FG_BLOCK), 0, h->stream, (const double *)h->fges_r.p, (int)n, (const int32_t *)s.flags,
                               in, gain, status, list, s.counter, n_narrow, n_groups);
            PCG_HIP(h, hipGetLastError());
        }
        int64_t marked = 0;
        if (int rc = pcg_read_counter(h, "pcg_fges_gains", s.counter, n_items, &marked)) return rc;
        if (marked) {
            const int64_t eblocks = std::min<int64_t>({marked, (int64_t)FG_EXACT_BLOCKS, FG_WS_BYTES / (slot * 8)});
            if (!pcg_ensure(h, h->fges_work, (size_t)(eblocks * slot * 8)))
                return pcg_fail(h, PCG_ERR_OOM, "pcg_fges_gains: exact-path workspace");
            hipLaunchKernelGGL(k_fg_exact, dim3((unsigned)eblocks), dim3(FG_BLOCK), 0, h->stream, (const double *)h->fges_e.p,
                               T, (int)n, in, (const int32_t *)list, marked, (double *)h->fges_work.p, slot, gain);
            PCG_HIP(h, hipGetLastError());
        }
        if (exact_items) *exact_items = marked;
    }
    PCG_HIP(h, hipStreamSynchronize(h->stream));
    return PCG_OK;
}
