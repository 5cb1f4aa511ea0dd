// pcmci.hip — PCMCI (tigramite ParCorr, analytic significance) for RCAEval's pcmci graph learner
// and the microcause method.
//
// Replaces tigramite 4.2.2.1 `PCMCI.run_pcmci(tau_max, pc_alpha)` [U] behind
// RCAEval/graph_construction/pcmci.py:71-103 and RCAEval/e2e/microcause.py:2298-2305. With the
// default cut_off='2xtau_max' every ParCorr test of a run uses the rows t = 2 tau_max .. T-1, so
// every test is a partial correlation inside ONE correlation matrix: R of the lag-expanded data E
// (T_eff x W, W = n (2 tau_max + 1), column i (2 tau_max + 1) + l = column i delayed by l). K1
// computes R; the rest is small factorisations of sub-blocks of R ("PCMCI").
//
//   k_pm_flags    one block per expanded column: constant / non-finite over its window.
//   k_pm_expand   E from X; a flagged column is written as a +-1 pattern so K1 never sees it (every
//                 test that touches a flagged column is refused by status before R is read).
//   k_pm_parents  PC1 (run_pc_stable, max_combinations = 1): one workgroup per target, the candidate
//                 list (id, val_min, flag) in LDS, the whole level loop on the device. Per level one
//                 Cholesky of R[S_d + y] serves every candidate outside the top d (a forward and a
//                 back solve per thread); each of the d candidates inside it gets its own block-wide
//                 factorisation of the top d + 1 without itself. Removal after the pass, then the
//                 stable descending sort keyed on (val_min, previous position) by rank counting.
//   k_pm_mci      one wave per (i, j, tau): builds Z, factorises R[Z + x + y] in LDS.
//   k_pm_mci_exact / pm_exact_item  the exact path: Householder QR on the standardized lagged
//                 columns themselves, one block per item; PC1 calls it inside its level loop.
// The block sums, the column classification, the Cholesky of the fast path (chol_eliminate) and the
// QR of the exact path (qr_eliminate) are dense_dev.h's, shared with fges.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "dense_dev.h"
#include "handle.h"

namespace {

constexpr int PM_BLOCK = 256;
constexpr int PM_ZCAP = 62;               // largest |Z|: {Z, x, y} is at most 64 x 64 doubles of LDS
constexpr int PM_LD = 64;
constexpr int PM_MAXC = 2048;             // n * tau_max candidates of one target (LDS list)
constexpr int PM_MAXW = 8192;             // lag-expanded width n * (2 tau_max + 1)
constexpr int PM_MAXTAU = 16;
constexpr int PM_PER = PM_MAXC / PM_BLOCK;
// fast-path guards: smallest pivot of the unit-diagonal factorisation (and of x, y given
// Z), and the bound on (1 + |g|_1)^2 of the regression coefficients of x and y on Z
constexpr double PM_TAU = 1e-2;
constexpr double PM_BETA_C = 400.0;
constexpr int64_t PM_WS_BYTES = (int64_t)1 << 30;    // exact path: design workspace bound

__global__ __launch_bounds__(PM_BLOCK) void k_pm_flags(const double *X, int64_t Teff, int n, int64_t ldx, int tau_max,
                                                       int32_t *flags) {
    __shared__ double red[3 * (PM_BLOCK / 64)];
    const int K = 2 * tau_max + 1, c = blockIdx.x, i = c / K, lag = c % K;
    const double *x = X + (int64_t)(2 * tau_max - lag) * ldx + i;
    double lo = INFINITY, hi = -INFINITY, bad = 0.0;
    for (int64_t r = threadIdx.x; r < Teff; r += PM_BLOCK) {
        const double v = x[r * ldx];
        if (isfinite(v)) {
            lo = fmin(lo, v);
            hi = fmax(hi, v);
        } else
            bad = 1.0;
    }
    const int fl = column_class<PM_BLOCK>(lo, hi, bad, red);
    if (threadIdx.x == 0) flags[c] = fl;
}

__global__ __launch_bounds__(PM_BLOCK) void k_pm_expand(const double *X, int64_t Teff, int n, int64_t ldx, int tau_max,
                                                        const int32_t *flags, double *E) {
    const int K = 2 * tau_max + 1;
    const int64_t W = (int64_t)n * K, total = Teff * W;
    for (int64_t idx = (int64_t)blockIdx.x * PM_BLOCK + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * PM_BLOCK) {
        const int64_t r = idx / W;
        const int c = (int)(idx % W), i = c / K, lag = c % K;
        E[idx] = flags[c] ? ((r & 1) ? 1.0 : -1.0) : X[(2 * tau_max - lag + r) * ldx + i];
    }
}

// |g|_1 of g = L11^-T b, the regression coefficients on Z of the variable whose factor row is b
// (one thread; gg: d doubles of scratch). Not shared with fges.hip's one-wave form: another launch shape.
__device__ inline double pm_coef_norm1(const double *A, const double *b, int d, double *gg) {
    double n1 = 0.0;
    for (int k = d - 1; k >= 0; --k) {
        double a = b[k];
        for (int r = k + 1; r < d; ++r) a -= A[r * PM_LD + k] * gg[r];
        gg[k] = a / A[k * PM_LD + k];
        n1 += fabs(gg[k]);
    }
    return n1;
}

// One test on the fast path: cols = [Z (d), x, y]. g: 130 doubles of LDS. False when a guard refuses.
template <int NT>
__device__ bool pm_fast_item(const double *R, int64_t W, const int *cols, int d, double *A, double *g, double &val) {
    if (!chol_eliminate<NT, PM_LD>(R, W, cols, d + 2, d, A, PM_TAU)) return false;
    const double sxx = A[d * PM_LD + d], sxy = A[(d + 1) * PM_LD + d], syy = A[(d + 1) * PM_LD + d + 1];
    const int tid = threadIdx.x;
    if (tid < 2) g[128 + tid] = pm_coef_norm1(A, A + (d + tid) * PM_LD, d, g + tid * 64);
    __syncthreads();
    const double n1 = fmax(g[128], g[129]);
    __syncthreads();
    if (!(sxx >= PM_TAU) || !(syy >= PM_TAU) || !((1.0 + n1) * (1.0 + n1) <= PM_BETA_C)) return false;
    val = sxy / sqrt(sxx * syy);
    return true;
}

// One test on the exact path: the columns cols = [Z (d), x, y] of E standardized (ddof 0) into the
// block's workspace Aw (column-major, m x Teff), Householder QR over the Z columns (dense_dev.h's
// qr_eliminate: a dependent column is skipped), val = the cosine of the two residuals. Each thread
// owns the rows r = tid, tid + NT, .. throughout.
template <int NT>
__device__ double pm_exact_item(const double *E, int64_t Teff, int64_t W, const int *cols, int d, double *Aw,
                                double *red) {
    const int tid = threadIdx.x, m = d + 2;
    __syncthreads();
    for (int u = 0; u < m; ++u) {
        const double *e = E + cols[u];
        double *au = Aw + (int64_t)u * Teff;
        double s = 0.0;
        for (int64_t r = tid; r < Teff; r += NT) s += e[r * W];
        const double mu = block_sum<NT>(s, red) / (double)Teff;
        double q = 0.0;
        for (int64_t r = tid; r < Teff; r += NT) {
            const double v = e[r * W] - mu;
            q = fma(v, v, q);
        }
        const double isd = 1.0 / sqrt(block_sum<NT>(q, red) / (double)Teff);
        for (int64_t r = tid; r < Teff; r += NT) au[r] = (e[r * W] - mu) * isd;
    }
    const double tol = (double)std::max<int64_t>(Teff, m) * 2.220446049250313e-16;
    const int64_t rdone = qr_eliminate<NT>(Aw, Teff, m, 0, d, 0, tol, red);
    const double *ax = Aw + (int64_t)d * Teff, *ay = Aw + (int64_t)(d + 1) * Teff;
    double sxx = 0.0, sxy = 0.0, syy = 0.0;
    for (int64_t r = tid; r < Teff; r += NT)
        if (r >= rdone) {
            sxx = fma(ax[r], ax[r], sxx);
            sxy = fma(ax[r], ay[r], sxy);
            syy = fma(ay[r], ay[r], syy);
        }
    sxx = block_sum<NT>(sxx, red);
    sxy = block_sum<NT>(sxy, red);
    syy = block_sum<NT>(syy, red);
    return sxy / sqrt(sxx * syy);
}

// ---- PC1 ---------------------------------------------------------------------------------------
struct PmParents {
    int32_t *ids;        // n x pcap expanded column ids, in final order
    double *val_min;     // n x pcap
    int32_t *count, *levels, *status;
    int64_t *tests;
    int pcap;
};

__global__ __launch_bounds__(PM_BLOCK) void k_pm_parents(const double *R, const double *E, int64_t Teff, int n,
                                                         int tau_max, const int32_t *flags, const double *crit_tab,
                                                         double *work, int64_t slot, PmParents out,
                                                         unsigned long long *exact_ctr) {
    __shared__ double A[PM_LD * PM_LD];
    __shared__ double vmin[PM_MAXC];
    __shared__ int32_t id[PM_MAXC];
    __shared__ uint8_t fl[PM_MAXC];          // 1: remove after the pass, 2: refused by a guard
    __shared__ double g[130];
    __shared__ double red[PM_BLOCK / 64];
    __shared__ int cols[PM_LD];
    __shared__ int sh_flag, sh_len;
    const int tid = threadIdx.x, j = blockIdx.x, K = 2 * tau_max + 1, y = j * K;
    const int64_t W = (int64_t)n * K;
    const int NC = n * tau_max;
    double *Aw = work + (int64_t)j * slot;
    if (tid == 0) sh_flag = flags[y];
    __syncthreads();
    for (int p = tid; p < NC; p += PM_BLOCK) {
        id[p] = (p / tau_max) * K + p % tau_max + 1;
        vmin[p] = INFINITY;
        fl[p] = 0;
        if (flags[id[p]]) atomicOr(&sh_flag, flags[id[p]]);
    }
    __syncthreads();
    if (sh_flag) {                             // block-uniform
        if (tid == 0) {
            out.count[j] = 0;
            out.levels[j] = 0;
            out.tests[j] = 0;
            out.status[j] = (sh_flag & 2) ? 2 : 1;
        }
        return;
    }
    int len = NC, levels = 0, st = 0;
    int64_t tests = 0;
    unsigned long long nexact = 0;
    for (int d = 0;; ++d) {
        if (len - 1 < d) break;
        if (d > PM_ZCAP) {
            st = 4;
            break;
        }
        const double crit = crit_tab[d];
        ++levels;
        tests += len;
        // candidates inside the top d: Z = the top d + 1 without the candidate
        for (int p = 0; p < d; ++p) {
            __syncthreads();
            if (tid < d) cols[tid] = id[tid < p ? tid : tid + 1];
            if (tid == 0) {
                cols[d] = id[p];
                cols[d + 1] = y;
            }
            double val = 0.0;
            if (!pm_fast_item<PM_BLOCK>(R, W, cols, d, A, g, val)) {
                val = pm_exact_item<PM_BLOCK>(E, Teff, W, cols, d, Aw, red);
                ++nexact;
            }
            if (tid == 0) {
                const double a = fabs(val);
                if (a < vmin[p]) vmin[p] = a;
                fl[p] = a < crit ? 1 : 0;
            }
        }
        // candidates outside it: one factorisation of R[top d + y], two triangular solves each
        // (thread-serial in b[]; fges.hip's solves take a lane per row, so they are not shared)
        __syncthreads();
        if (tid < d) cols[tid] = id[tid];
        if (tid == 0) cols[d] = y;
        bool shared_ok = chol_eliminate<PM_BLOCK, PM_LD>(R, W, cols, d + 1, d, A, PM_TAU);
        const double syy = shared_ok ? A[d * PM_LD + d] : 0.0;
        if (shared_ok && tid == 0) g[128] = pm_coef_norm1(A, A + d * PM_LD, d, g);
        __syncthreads();
        const double n1y = shared_ok ? g[128] : 0.0;
        shared_ok = shared_ok && syy >= PM_TAU;
        for (int p = d + tid; p < len; p += PM_BLOCK) {
            if (!shared_ok) {
                fl[p] = 2;
                continue;
            }
            const int x = id[p];
            const double *rx = R + (int64_t)x * W;
            double b[PM_ZCAP];
            double sxx = 1.0, sxy = rx[y];
            for (int k = 0; k < d; ++k) {
                double s = rx[cols[k]];
                for (int c = 0; c < k; ++c) s -= A[k * PM_LD + c] * b[c];
                s /= A[k * PM_LD + k];
                b[k] = s;
                sxx -= s * s;
                sxy -= s * A[d * PM_LD + k];
            }
            double n1 = 0.0;
            for (int k = d - 1; k >= 0; --k) {
                double a = b[k];
                for (int r = k + 1; r < d; ++r) a -= A[r * PM_LD + k] * b[r];
                a /= A[k * PM_LD + k];
                b[k] = a;
                n1 += fabs(a);
            }
            n1 = fmax(n1, n1y);
            if (sxx >= PM_TAU && (1.0 + n1) * (1.0 + n1) <= PM_BETA_C) {
                const double a = fabs(sxy / sqrt(sxx * syy));
                if (a < vmin[p]) vmin[p] = a;
                fl[p] = a < crit ? 1 : 0;
            } else
                fl[p] = 2;
        }
        __syncthreads();
        for (int p = d; p < len; ++p) {        // the refused ones, one at a time by the whole block
            if (fl[p] != 2) continue;          // block-uniform (LDS, read behind a barrier)
            __syncthreads();
            if (tid == 0) {
                cols[d] = id[p];
                cols[d + 1] = y;
            }
            const double val = pm_exact_item<PM_BLOCK>(E, Teff, W, cols, d, Aw, red);
            ++nexact;
            __syncthreads();
            if (tid == 0) {
                const double a = fabs(val);
                if (a < vmin[p]) vmin[p] = a;
                fl[p] = a < crit ? 1 : 0;
            }
            __syncthreads();
        }
        // removal, then the stable sort by (val_min descending, previous position ascending)
        __syncthreads();
        if (tid == 0) sh_len = 0;
        int32_t my_id[PM_PER], my_rank[PM_PER];
        double my_key[PM_PER];
#pragma unroll
        for (int q = 0; q < PM_PER; ++q) {
            const int p = tid + q * PM_BLOCK;
            my_rank[q] = -1;
            my_id[q] = 0;
            my_key[q] = 0.0;
            if (p < len && fl[p] != 1) {
                const double key = vmin[p];
                int rank = 0;
                for (int e = 0; e < len; ++e)
                    if (fl[e] != 1 && (vmin[e] > key || (vmin[e] == key && e < p))) ++rank;
                my_rank[q] = rank;
                my_id[q] = id[p];
                my_key[q] = key;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PM_PER; ++q)
            if (my_rank[q] >= 0) {
                id[my_rank[q]] = my_id[q];
                vmin[my_rank[q]] = my_key[q];
                atomicAdd(&sh_len, 1);
            }
        __syncthreads();
        len = sh_len;
        for (int p = tid; p < len; p += PM_BLOCK) fl[p] = 0;
        __syncthreads();
    }
    for (int p = tid; p < len && p < out.pcap; p += PM_BLOCK) {
        out.ids[(int64_t)j * out.pcap + p] = id[p];
        out.val_min[(int64_t)j * out.pcap + p] = vmin[p];
    }
    if (tid == 0) {
        out.count[j] = len;
        out.levels[j] = levels;
        out.tests[j] = tests;
        out.status[j] = st;
        if (nexact) atomicAdd(exact_ctr, nexact);
    }
}

// ---- MCI ---------------------------------------------------------------------------------------
// Z of item (i, j, tau) into cols[0..d), then x, y (thread 0). Returns |Z| as specified (counted past
// the cap too) in *dz and a status: 0, 1 / 2 (a flagged column), 4 (|Z| above the cap, or a parent
// entry that is no lag 1..tau_max node: refused, never used as an index).
__device__ int pm_build_z(int i, int j, int tau, int n, int tau_max, const int32_t *par_ids, const int32_t *par_cnt,
                          int pcap, const int32_t *flags, int *cols, int *dz) {
    const int K = 2 * tau_max + 1, x = i * K + tau, y = j * K;
    const int64_t W = (int64_t)n * K;
    int d = 0, total = 0, st = 0, fb = flags[x] | flags[y];
    const int cj = par_cnt[j], ci = par_cnt[i];
    if (cj < 0 || cj > pcap || ci < 0 || ci > pcap) {
        *dz = 0;
        return 4;
    }
    auto add = [&](int q) {
        for (int k = 0; k < d; ++k)
            if (cols[k] == q) return;
        ++total;
        if (d < PM_ZCAP) {
            cols[d++] = q;
            fb |= flags[q];
        }
    };
    for (int k = 0; k < cj; ++k) {
        const int q = par_ids[(int64_t)j * pcap + k];
        if (q < 0 || q >= W || q % K < 1 || q % K > tau_max) st = 4;
        else if (q != x) add(q);
    }
    for (int k = 0; k < ci; ++k) {
        const int q = par_ids[(int64_t)i * pcap + k];
        if (q < 0 || q >= W || q % K < 1 || q % K > tau_max) st = 4;
        else add(q + tau);
    }
    if (total > PM_ZCAP) st = 4;              // (a duplicate hidden behind the cap can only overcount)
    cols[d] = x;
    cols[d + 1] = y;
    *dz = total;
    if (st) return st;
    return (fb & 2) ? 2 : ((fb & 1) ? 1 : 0);
}

struct PmMci {
    double *val;
    int32_t *dim, *status;
};

__global__ __launch_bounds__(64) void k_pm_mci(const double *R, int n, int tau_max, const int32_t *flags,
                                               const int32_t *par_ids, const int32_t *par_cnt, int pcap, PmMci out,
                                               int32_t *list, unsigned int *counter) {
    __shared__ double A[PM_LD * PM_LD];
    __shared__ double g[130];
    __shared__ int cols[PM_LD];
    __shared__ int sh_d, sh_st;
    const int tid = threadIdx.x, K = 2 * tau_max + 1;
    const int64_t W = (int64_t)n * K, items = (int64_t)n * n * (tau_max + 1);
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int tau = (int)(it % (tau_max + 1));
        const int j = (int)((it / (tau_max + 1)) % n), i = (int)(it / ((int64_t)(tau_max + 1) * n));
        if (i == j && tau == 0) {              // carries no test
            if (tid == 0) {
                out.val[it] = 0.0;
                out.dim[it] = -1;
                out.status[it] = 0;
            }
            continue;
        }
        __syncthreads();
        if (tid == 0) sh_st = pm_build_z(i, j, tau, n, tau_max, par_ids, par_cnt, pcap, flags, cols, &sh_d);
        __syncthreads();
        const int d = sh_d;
        int st = sh_st;
        double val = __builtin_nan("");
        if (st == 0 && !pm_fast_item<64>(R, W, cols, d, A, g, val)) {
            val = __builtin_nan("");
            st = 3;
            if (tid == 0) list[atomicAdd(counter, 1u)] = (int32_t)it;
        }
        if (tid == 0) {
            out.val[it] = val;
            out.dim[it] = d;
            out.status[it] = st;
        }
    }
}

__global__ __launch_bounds__(PM_BLOCK) void k_pm_mci_exact(const double *E, int64_t Teff, int n, int tau_max,
                                                           const int32_t *flags, const int32_t *par_ids,
                                                           const int32_t *par_cnt, int pcap, const int32_t *list,
                                                           int64_t count, double *work, int64_t slot, PmMci out) {
    __shared__ double red[PM_BLOCK / 64];
    __shared__ int cols[PM_LD];
    __shared__ int sh_d, sh_st;
    const int tid = threadIdx.x, K = 2 * tau_max + 1;
    const int64_t W = (int64_t)n * K;
    double *Aw = work + (int64_t)blockIdx.x * slot;
    for (int64_t q = blockIdx.x; q < count; q += gridDim.x) {
        const int64_t it = list[q];
        const int tau = (int)(it % (tau_max + 1));
        const int j = (int)((it / (tau_max + 1)) % n), i = (int)(it / ((int64_t)(tau_max + 1) * n));
        __syncthreads();
        if (tid == 0) sh_st = pm_build_z(i, j, tau, n, tau_max, par_ids, par_cnt, pcap, flags, cols, &sh_d);
        __syncthreads();
        if (sh_st != 0) continue;              // block-uniform; cannot happen for a listed item
        const double val = pm_exact_item<PM_BLOCK>(E, Teff, W, cols, sh_d, Aw, red);
        if (tid == 0) out.val[it] = val;
    }
}

int pm_check_shape(pcg_handle *h, const char *who, int64_t T, int64_t n, int tau_max) {
    if (tau_max < 1 || tau_max > PM_MAXTAU)
        return pcg_fail(h, PCG_ERR_INVALID, "%s: tau_max %d outside 1..%d", who, tau_max, PM_MAXTAU);
    if (n < 1 || n * (2 * (int64_t)tau_max + 1) > PM_MAXW || n * tau_max > PM_MAXC || T < 1)
        return pcg_fail(h, PCG_ERR_INVALID, "%s: bad shape (T=%lld n=%lld tau_max=%d: n (2 tau_max + 1) <= %d, n tau_max <= %d)",
                        who, (long long)T, (long long)n, tau_max, PM_MAXW, PM_MAXC);
    if (T - 2 * (int64_t)tau_max < 3)
        return pcg_fail(h, PCG_ERR_DOMAIN, "%s: T_eff = T - 2 tau_max = %lld leaves no degree of freedom (needs >= 3)",
                        who, (long long)(T - 2 * (int64_t)tau_max));
    if (n * (T - 2 * (int64_t)tau_max) * PM_LD * 8 > PM_WS_BYTES)
        return pcg_fail(h, PCG_ERR_INVALID, "%s: n * T_eff * 512 B of exact-path workspace exceeds %lld B", who,
                        (long long)PM_WS_BYTES);
    return PCG_OK;
}

// pcmci_small: column flags (W int32) | crit table (64 doubles) | two counters | exact list
struct PmSmall {
    int32_t *flags;
    double *crit;
    unsigned long long *exact_ctr;
    unsigned int *list_ctr;
    int32_t *list;
};
bool pm_small(pcg_handle *h, int64_t n, int tau_max, PmSmall &s) {
    const int64_t W = n * (2 * tau_max + 1), items = n * n * (tau_max + 1);
    Carve cv;
    const size_t o_flags = cv.take((size_t)W * 4), o_crit = cv.take(64 * 8), o_ctr = cv.take(16),
                 o_list = cv.take((size_t)items * 4);
    if (!pcg_ensure(h, h->pcmci_small, cv.total)) return false;
    char *base = (char *)h->pcmci_small.p;
    s.flags = (int32_t *)(base + o_flags);
    s.crit = (double *)(base + o_crit);
    s.exact_ctr = (unsigned long long *)(base + o_ctr);
    s.list_ctr = (unsigned int *)(base + o_ctr + 8);
    s.list = (int32_t *)(base + o_list);
    return true;
}

}  // namespace

extern "C" int pcg_pcmci_limits(int32_t *max_tau, int32_t *z_cap, int32_t *max_width, int32_t *max_candidates,
                                double *tau, double *beta_c) {
    if (max_tau) *max_tau = PM_MAXTAU;
    if (z_cap) *z_cap = PM_ZCAP;
    if (max_width) *max_width = PM_MAXW;
    if (max_candidates) *max_candidates = PM_MAXC;
    if (tau) *tau = PM_TAU;
    if (beta_c) *beta_c = PM_BETA_C;
    return PCG_OK;
}

extern "C" int pcg_pcmci_parents(pcg_handle *h, const double *X, int64_t T, int64_t n, int64_t ldx, int tau_max,
                                 const double *crit, int32_t ncrit, int32_t *par_ids, double *par_val_min,
                                 int32_t *par_count, int32_t pcap, int32_t *levels, int64_t *tests, int32_t *status,
                                 int64_t *exact_items) {
    if (!h) return PCG_ERR_INVALID;
    h->pcmci_ok = false;
    const int rc0 = pm_check_shape(h, "pcg_pcmci_parents", T, n, tau_max);
    if (rc0) return rc0;
    if (ldx < n || pcap < 1 || ncrit < PM_ZCAP + 1)
        return pcg_fail(h, PCG_ERR_INVALID, "pcg_pcmci_parents: ldx=%lld < n, pcap=%d < 1 or ncrit=%d < %d", (long long)ldx,
                        pcap, ncrit, PM_ZCAP + 1);
    if (!X || !crit || !par_ids || !par_val_min || !par_count || !levels || !tests || !status)
        return pcg_fail(h, PCG_ERR_INVALID, "pcg_pcmci_parents: null pointer");
    PCG_HIP(h, hipSetDevice(h->device));
    const int64_t Teff = T - 2 * (int64_t)tau_max, W = n * (2 * tau_max + 1), slot = Teff * PM_LD;
    PmSmall s;
    if (!pcg_ensure(h, h->pcmci_e, (size_t)(Teff * W * 8)) || !pcg_ensure(h, h->pcmci_r, (size_t)(W * W * 8)) ||
        !pcg_ensure(h, h->pcmci_work, (size_t)(n * slot * 8)) || !pm_small(h, n, tau_max, s))
        return pcg_fail(h, PCG_ERR_OOM, "pcg_pcmci_parents: scratch");
    double *E = (double *)h->pcmci_e.p, *R = (double *)h->pcmci_r.p;
    PCG_HIP(h, hipMemcpyAsync(s.crit, crit, (PM_ZCAP + 1) * 8, hipMemcpyHostToDevice, h->stream));
    PCG_HIP(h, hipMemsetAsync(s.exact_ctr, 0, 16, h->stream));
    hipLaunchKernelGGL(k_pm_flags, dim3((unsigned)W), dim3(PM_BLOCK), 0, h->stream, X, Teff, (int)n, ldx, tau_max, s.flags);
    PCG_HIP(h, hipGetLastError());
    const unsigned eb = (unsigned)std::min<int64_t>((Teff * W + PM_BLOCK - 1) / PM_BLOCK, 4096);
    hipLaunchKernelGGL(k_pm_expand, dim3(eb), dim3(PM_BLOCK), 0, h->stream, X, Teff, (int)n, ldx, tau_max,
                       (const int32_t *)s.flags, E);
    PCG_HIP(h, hipGetLastError());
    const int rc = pcg_corr_launch(h, E, Teff, W, W, R, W);
    if (rc) return rc;
    const PmParents out{par_ids, par_val_min, par_count, levels, status, tests, pcap};
    hipLaunchKernelGGL(k_pm_parents, dim3((unsigned)n), dim3(PM_BLOCK), 0, h->stream, (const double *)R, (const double *)E,
                       Teff, (int)n, tau_max, (const int32_t *)s.flags, (const double *)s.crit, (double *)h->pcmci_work.p,
                       slot, out, s.exact_ctr);
    PCG_HIP(h, hipGetLastError());
    int64_t ex = 0;                            // a count of tests, not an index into a list: no capacity
    if (int rc1 = pcg_read_counter(h, "pcg_pcmci_parents", s.exact_ctr, INT64_MAX, &ex)) return rc1;
    if (exact_items) *exact_items = ex;
    h->pcmci_shape[0] = T;
    h->pcmci_shape[1] = n;
    h->pcmci_shape[2] = tau_max;
    h->pcmci_ok = true;
    return PCG_OK;
}

extern "C" int pcg_pcmci_mci(pcg_handle *h, int64_t T, int64_t n, int tau_max, const int32_t *par_ids,
                             const int32_t *par_count, int32_t pcap, double *val, int32_t *dim, int32_t *status,
                             int64_t *exact_items) {
    if (!h) return PCG_ERR_INVALID;
    const int rc0 = pm_check_shape(h, "pcg_pcmci_mci", T, n, tau_max);
    if (rc0) return rc0;
    if (pcap < 1 || !par_ids || !par_count || !val || !dim || !status)
        return pcg_fail(h, PCG_ERR_INVALID, "pcg_pcmci_mci: null pointer or pcap < 1");
    if (!h->pcmci_ok || h->pcmci_shape[0] != T || h->pcmci_shape[1] != n || h->pcmci_shape[2] != tau_max)
        return pcg_fail(h, PCG_ERR_INVALID, "pcg_pcmci_mci: no pcg_pcmci_parents run of this (T, n, tau_max) on the handle");
    PCG_HIP(h, hipSetDevice(h->device));
    const int64_t Teff = T - 2 * (int64_t)tau_max, slot = Teff * PM_LD, items = n * n * (tau_max + 1);
    PmSmall s;
    if (!pm_small(h, n, tau_max, s)) return pcg_fail(h, PCG_ERR_OOM, "pcg_pcmci_mci: scratch");
    PCG_HIP(h, hipMemsetAsync(s.list_ctr, 0, 4, h->stream));
    const PmMci out{val, dim, status};
    const unsigned blocks = (unsigned)std::min<int64_t>(items, 16384);
    hipLaunchKernelGGL(k_pm_mci, dim3(blocks), dim3(64), 0, h->stream, (const double *)h->pcmci_r.p, (int)n, tau_max,
                       (const int32_t *)s.flags, par_ids, par_count, pcap, out, s.list, s.list_ctr);
    PCG_HIP(h, hipGetLastError());
    int64_t marked = 0;
    if (int rc = pcg_read_counter(h, "pcg_pcmci_mci", s.list_ctr, items, &marked)) return rc;
    if (marked) {
        const int64_t eblocks = std::min<int64_t>({marked, n, 2048});   // pcmci_work holds n slots
        hipLaunchKernelGGL(k_pm_mci_exact, dim3((unsigned)eblocks), dim3(PM_BLOCK), 0, h->stream,
                           (const double *)h->pcmci_e.p, Teff, (int)n, tau_max, (const int32_t *)s.flags, par_ids, par_count,
                           pcap, (const int32_t *)s.list, marked, (double *)h->pcmci_work.p, slot, out);
        PCG_HIP(h, hipGetLastError());
        PCG_HIP(h, hipStreamSynchronize(h->stream));
    }
    if (exact_items) *exact_items = marked;
    return PCG_OK;
}
