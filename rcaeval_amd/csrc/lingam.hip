// lingam.hip — DirectLiNGAM's causal-order search (pairwise likelihood-ratio measure, 'pwling').
//
// Replaces the nested Python loops of causal-learn's `DirectLiNGAM().fit(X)` [U] (0.1.3.3, the
// pin of RCAEval's requirements.txt) behind RCAEval/e2e/lingam_pagerank.py:52-81 (`micro_diag`).
// Step s of n: over the remaining columns U, every pair's D_ij (the difference of the two
// regression directions' entropy sums), M_i = -sum_j min(0, D_ij)^2, m = U[argmax M], and the
// working copy's X_[:, i] -= (cov_ddof1 / var_ddof0) * X_[:, m] for i in U, i != m. All fp64.
//
// Three launches per step, no host read between steps ("DirectLiNGAM"):
//   k_lingam_cols    one block per remaining column. From the second step on it first takes the
//                    numpy-semantics argmax of the previous step's M (every block derives it from
//                    the same m values; block 0 records it in `order`) and residualizes its column
//                    against the chosen one — the grid-wide argmax needs every M first, so it sits
//                    here and not behind the reduction. Then mean, std (ddof 0), the standardized
//                    z (column-major, by position in U), and z's own mean, variance and H(z).
//   k_lingam_pairs   the hot path. Block (i, *) stages z_i in LDS in T-chunks; each wave takes a
//                    partner j, lanes stride over t. Pass A: the centred dot product, giving the
//                    two coefficients. Pass B: sums of ri, ri^2, rj, rj^2, giving the residuals'
//                    own std. Pass C: the means of log(cosh(u)) and u * exp(-u^2 / 2) of both
//                    scaled residuals. Writes D_ij and D_ji = -D_ij. Every unordered pair is
//                    visited once: row i takes the partners (i + k) mod m, k = 1..(m - 1) / 2 (and
//                    k = m / 2 for i < m / 2 when m is even), so every block has the same work.
//   k_lingam_reduce  one wave per row: M with a NaN-propagating min, also into `scores`.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>

#include "dense_dev.h"
#include "handle.h"

// the reference rounds a * b and the following sum separately; sums that are fused say fma()
#pragma clang fp contract(off)

namespace {

constexpr int LG_BLOCK = 256;
constexpr int LG_WAVES = LG_BLOCK / 64;
constexpr int LG_CHUNK = 2048;            // rows of z_i staged in LDS at a time
constexpr int LG_CS = 4;                  // doubles of column statistics: H(z), mean(z), var(z), unused
constexpr int64_t LG_MAX_N = 4096;

// H(u) from mean(log(cosh(u))) and mean(u * exp(-u^2 / 2)), in the reference's operation order
__device__ inline double lg_entropy(double mlc, double mge) {
    const double a = mlc - 0.37457;
    return ((1.0 + 1.8378770664093453) / 2.0 - 79.047 * (a * a)) - 7.4129 * (mge * mge);
}

// np.argmax: does candidate (v, i) come before (w, j)? The first NaN if any, else the first maximum
__device__ inline bool lg_before(double v, int i, double w, int j) {
    const bool nv = v != v, nw = w != w;
    if (nv != nw) return nv;
    if (nv || v == w) return i < j;
    return v > w;
}

// every thread gets np.argmax(M[0..m)), m >= 1
__device__ inline int block_argmax(const double *M, int m, double *bv, int *bi) {
    const int tid = threadIdx.x;
    double v = -INFINITY;
    int at = INT_MAX;                      // no candidate yet: loses to every entry
    for (int p = tid; p < m; p += LG_BLOCK) {
        const double w = M[p];
        if (at == INT_MAX || lg_before(w, p, v, at)) {
            v = w;
            at = p;
        }
    }
    bv[tid] = v;
    bi[tid] = at;
    __syncthreads();
    for (int o = LG_BLOCK / 2; o > 0; o >>= 1) {
        if (tid < o && bi[tid + o] != INT_MAX && (bi[tid] == INT_MAX || lg_before(bv[tid + o], bi[tid + o], bv[tid], bi[tid]))) {
            bv[tid] = bv[tid + o];
            bi[tid] = bi[tid + o];
        }
        __syncthreads();
    }
    const int r = bi[0];
    __syncthreads();
    return r;
}

// ---- column pass -------------------------------------------------------------------------------
// Block p serves position p of this step's U. Mprev == nullptr (first step): U is 0..m-1 and the
// column is copied from X. Otherwise Uprev (mprev = m + 1 entries) loses the position pm =
// argmax(Mprev), and column Ucur[p] of W is residualized against column Uprev[pm].
// A thread touches the same rows t = tid, tid + 256, .. in every pass, so it only reads back what
// it wrote itself.
__global__ __launch_bounds__(LG_BLOCK) void k_lingam_cols(const double *X, int64_t ldx, double *W, double *Z, int64_t T,
                                                          const double *Mprev, int mprev, const int32_t *Uprev,
                                                          int32_t *Ucur, double *cs, int32_t *order_slot) {
    __shared__ double red[3 * LG_WAVES];
    __shared__ double bv[LG_BLOCK];
    __shared__ int bi[LG_BLOCK];
    const int p = blockIdx.x, tid = threadIdx.x;
    const double dT = (double)T;
    int col = p;
    double s1[1] = {0.0};
    if (Mprev) {
        const int pm = block_argmax(Mprev, mprev, bv, bi);
        col = Uprev[p < pm ? p : p + 1];
        const int cm = Uprev[pm];
        if (p == 0 && tid == 0) *order_slot = cm;
        double *a = W + (int64_t)col * T;
        const double *b = W + (int64_t)cm * T;
        double s[2] = {0.0, 0.0};
        for (int64_t t = tid; t < T; t += LG_BLOCK) {
            s[0] += a[t];
            s[1] += b[t];
        }
        block_sum<LG_BLOCK>(s, red);
        const double ma = s[0] / dT, mb = s[1] / dT;
        double q[2] = {0.0, 0.0};
        for (int64_t t = tid; t < T; t += LG_BLOCK) {
            const double da = a[t] - ma, db = b[t] - mb;
            q[0] = fma(da, db, q[0]);
            q[1] = fma(db, db, q[1]);
        }
        block_sum<LG_BLOCK>(q, red);
        // np.cov(a, b)[0, 1] / np.var(b): ddof 1 over ddof 0, r * T / (T - 1) and not r
        const double coef = (q[0] * (1.0 / (double)(T - 1))) / (q[1] / dT);
        for (int64_t t = tid; t < T; t += LG_BLOCK) {
            const double v = a[t] - coef * b[t];
            a[t] = v;
            s1[0] += v;
        }
    } else {
        double *w = W + (int64_t)col * T;
        for (int64_t t = tid; t < T; t += LG_BLOCK) {
            const double v = X[t * ldx + col];
            w[t] = v;
            s1[0] += v;
        }
    }
    if (tid == 0) Ucur[p] = col;
    const double *w = W + (int64_t)col * T;
    double *z = Z + (int64_t)p * T;
    block_sum<LG_BLOCK>(s1, red);
    const double mean = s1[0] / dT;
    double s2[1] = {0.0};
    for (int64_t t = tid; t < T; t += LG_BLOCK) {
        const double d = w[t] - mean;
        s2[0] = fma(d, d, s2[0]);
    }
    block_sum<LG_BLOCK>(s2, red);
    const double sd = sqrt(s2[0] / dT);
    double zs[1] = {0.0};
    for (int64_t t = tid; t < T; t += LG_BLOCK) {
        const double v = (w[t] - mean) / sd;
        z[t] = v;
        zs[0] += v;
    }
    block_sum<LG_BLOCK>(zs, red);
    const double zmean = zs[0] / dT;
    double h[3] = {0.0, 0.0, 0.0};
    for (int64_t t = tid; t < T; t += LG_BLOCK) {
        const double u = z[t], d = u - zmean;
        h[0] = fma(d, d, h[0]);
        h[1] += log(cosh(u));
        h[2] += u * exp(-(u * u) / 2.0);
    }
    block_sum<LG_BLOCK>(h, red);
    if (tid == 0) {
        double *c = cs + (int64_t)p * LG_CS;
        c[0] = lg_entropy(h[1] / dT, h[2] / dT);
        c[1] = zmean;
        c[2] = h[0] / dT;
        c[3] = 0.0;
    }
}

// ---- pair kernel -------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_BLOCK) void k_lingam_pairs(const double *Z, int64_t T, int m, const double *cs, double *D,
                                                           int64_t ldd) {
    __shared__ double zs[LG_CHUNK];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int npart = (m - 1) / 2 + ((m % 2 == 0 && i < m / 2) ? 1 : 0);
    if (blockIdx.y == 0 && tid == 0) D[(int64_t)i * ldd + i] = 0.0;
    const double *zi = Z + (int64_t)i * T;
    const double Hi = cs[(int64_t)i * LG_CS], mi = cs[(int64_t)i * LG_CS + 1], vi = cs[(int64_t)i * LG_CS + 2];
    const int nchunks = (int)((T + LG_CHUNK - 1) / LG_CHUNK);
    const double dT = (double)T;
    bool staged = false;
    // with one chunk z_i is staged once per block; with more, every pass of every round walks them
    auto stage = [&](int c) {
        const int64_t t0 = (int64_t)c * LG_CHUNK;
        const int len = (int)std::min<int64_t>(LG_CHUNK, T - t0);
        if (nchunks > 1 || !staged) {
            __syncthreads();               // the previous chunk's readers are done
            for (int s = tid; s < len; s += LG_BLOCK) zs[s] = zi[t0 + s];
            __syncthreads();
            staged = true;
        }
        return len;
    };
    // LG_WAVES partners per round, one per wave (block-uniform loop)
    for (int qb = blockIdx.y * LG_WAVES; qb < npart; qb += gridDim.y * LG_WAVES) {
        const int q = qb + wave;
        const bool live = q < npart;
        int j = i + q + 1;
        if (j >= m) j -= m;
        if (!live) j = i;
        const double *zj = Z + (int64_t)j * T;
        const double Hj = cs[(int64_t)j * LG_CS], mj = cs[(int64_t)j * LG_CS + 1], vj = cs[(int64_t)j * LG_CS + 2];
        // pass A: np.cov(zi, zj)[0, 1]
        double dot = 0.0;
        for (int c = 0; c < nchunks; ++c) {
            const int len = stage(c);
            if (!live) continue;
            const double *bj = zj + (int64_t)c * LG_CHUNK;
            for (int s = lane; s < len; s += 64) dot = fma(zs[s] - mi, bj[s] - mj, dot);
        }
        const double cov = wave_sum(dot) * (1.0 / (double)(T - 1));
        const double cij = cov / vj, cji = cov / vi;      // ri = zi - cij * zj, rj = zj - cji * zi
        // pass B: the residuals' own moments
        double b4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int c = 0; c < nchunks; ++c) {
            const int len = stage(c);
            if (!live) continue;
            const double *bj = zj + (int64_t)c * LG_CHUNK;
            for (int s = lane; s < len; s += 64) {
                const double a = zs[s], b = bj[s];
                const double ri = a - cij * b, rj = b - cji * a;
                b4[0] += ri;
                b4[1] = fma(ri, ri, b4[1]);
                b4[2] += rj;
                b4[3] = fma(rj, rj, b4[3]);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) b4[k] = wave_sum(b4[k]);
        const double sdi = sqrt((b4[1] - b4[0] * b4[0] / dT) / dT), sdj = sqrt((b4[3] - b4[2] * b4[2] / dT) / dT);
        // pass C: the entropy means of ri / std(ri) and rj / std(rj)
        double c4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int c = 0; c < nchunks; ++c) {
            const int len = stage(c);
            if (!live) continue;
            const double *bj = zj + (int64_t)c * LG_CHUNK;
            for (int s = lane; s < len; s += 64) {
                const double a = zs[s], b = bj[s];
                const double ui = (a - cij * b) / sdi, uj = (b - cji * a) / sdj;
                c4[0] += log(cosh(ui));
                c4[1] += ui * exp(-(ui * ui) / 2.0);
                c4[2] += log(cosh(uj));
                c4[3] += uj * exp(-(uj * uj) / 2.0);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) c4[k] = wave_sum(c4[k]);
        if (live && lane == 0) {
            const double Hri = lg_entropy(c4[0] / dT, c4[1] / dT), Hrj = lg_entropy(c4[2] / dT, c4[3] / dT);
            const double d = (Hj + Hri) - (Hi + Hrj);
            D[(int64_t)i * ldd + j] = d;
            D[(int64_t)j * ldd + i] = -d;
        }
    }
}

// ---- reduction ---------------------------------------------------------------------------------
// M_p = -sum_{q != p} min(0, D_pq)^2 with np.min's NaN (fmin would drop it). M is by position;
// scores_row (may be null) takes it by original column U[p].
__global__ __launch_bounds__(LG_BLOCK) void k_lingam_reduce(const double *D, int64_t ldd, int m, double *M, double *M_out,
                                                            double *scores_row, const int32_t *U) {
    const int lane = threadIdx.x & 63, p = blockIdx.x * LG_WAVES + (threadIdx.x >> 6);
    if (p >= m) return;
    const double *row = D + (int64_t)p * ldd;
    double acc = 0.0;
    for (int q = lane; q < m; q += 64) {
        if (q == p) continue;
        const double d = row[q];
        const double v = d != d ? d : (d < 0.0 ? d : 0.0);
        acc += v * v;
    }
    acc = -wave_sum(acc);
    if (lane == 0) {
        M[p] = acc;
        if (M_out) M_out[p] = acc;
        if (scores_row) scores_row[U[p]] = acc;
    }
}

__global__ void k_lingam_fill(double *a, int64_t count, double v) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += (int64_t)gridDim.x * blockDim.x) a[k] = v;
}

// The last two entries of the order: the argmax of the two-column step, then the lone candidate
// (search() returns it unscored; its score is 0). n == 1: the order is [0].
__global__ void k_lingam_finish(const double *M, const int32_t *U, int32_t *order, int n, double *scores) {
    if (threadIdx.x || blockIdx.x) return;
    int last = 0;
    if (n >= 2) {
        const int pm = lg_before(M[1], 1, M[0], 0) ? 1 : 0;
        order[n - 2] = U[pm];
        last = U[1 - pm];
    }
    order[n - 1] = last;
    if (scores) scores[(int64_t)(n - 1) * n + last] = 0.0;
}

struct LgScratch {
    double *W, *Z, *D, *cs, *M;
    int32_t *U[2];
};

int lg_check(pcg_handle *h, const char *who, const double *X, int64_t T, int64_t n, int64_t ldx) {
    if (n < 1 || n > LG_MAX_N || T < 2)
        return pcg_fail(h, PCG_ERR_DOMAIN, "%s: needs 1 <= n <= %lld and T >= 2 (T=%lld n=%lld)", who, (long long)LG_MAX_N,
                        (long long)T, (long long)n);
    if (!X || ldx < n) return pcg_fail(h, PCG_ERR_INVALID, "%s: null X or ldx=%lld < n=%lld", who, (long long)ldx, (long long)n);
    return PCG_OK;
}

int lg_scratch(pcg_handle *h, const char *who, int64_t T, int64_t n, bool want_d, LgScratch &s) {
    const size_t col_bytes = (size_t)n * (size_t)T * 8;
    // small: column statistics | M | the two U lists
    Carve cv;
    const size_t o_cs = cv.take((size_t)n * LG_CS * 8), o_m = cv.take((size_t)n * 8), o_u = cv.take(2 * (size_t)n * 4);
    if (!pcg_ensure(h, h->lingam_w, col_bytes) || !pcg_ensure(h, h->lingam_z, col_bytes) ||
        (want_d && !pcg_ensure(h, h->lingam_d, (size_t)n * n * 8)) || !pcg_ensure(h, h->lingam_small, cv.total))
        return pcg_fail(h, PCG_ERR_OOM, "%s: scratch (%lld B)", who, (long long)(2 * col_bytes + (size_t)n * n * 8 + cv.total));
    char *base = (char *)h->lingam_small.p;
    s.W = (double *)h->lingam_w.p;
    s.Z = (double *)h->lingam_z.p;
    s.D = (double *)h->lingam_d.p;
    s.cs = (double *)(base + o_cs);
    s.M = (double *)(base + o_m);
    s.U[0] = (int32_t *)(base + o_u);
    s.U[1] = s.U[0] + n;
    return PCG_OK;
}

// one step's three launches over m columns; step 0 reads X, later steps residualize W first
int lg_step(pcg_handle *h, const LgScratch &s, const double *X, int64_t ldx, int64_t T, int m, int step, double *D,
            double *M_out, double *scores_row, int32_t *order_slot) {
    int32_t *Ucur = s.U[step & 1];
    const int32_t *Uprev = s.U[(step + 1) & 1];
    hipLaunchKernelGGL(k_lingam_cols, dim3((unsigned)m), dim3(LG_BLOCK), 0, h->stream, X, ldx, s.W, s.Z, T,
                       step ? (const double *)s.M : (const double *)nullptr, m + 1, Uprev, Ucur, s.cs, order_slot);
    PCG_HIP(h, hipGetLastError());
    // blockIdx.y splits a row's partners over more blocks while m alone leaves CUs idle
    const int per_row = (m / 2 + LG_WAVES - 1) / LG_WAVES;
    const unsigned gy = (unsigned)std::max(1, std::min(per_row, 1024 / m));
    hipLaunchKernelGGL(k_lingam_pairs, dim3((unsigned)m, gy), dim3(LG_BLOCK), 0, h->stream, (const double *)s.Z, T, m,
                       (const double *)s.cs, D, (int64_t)m);
    PCG_HIP(h, hipGetLastError());
    hipLaunchKernelGGL(k_lingam_reduce, dim3((unsigned)((m + LG_WAVES - 1) / LG_WAVES)), dim3(LG_BLOCK), 0, h->stream,
                       (const double *)D, (int64_t)m, m, s.M, M_out, scores_row, (const int32_t *)Ucur);
    PCG_HIP(h, hipGetLastError());
    return PCG_OK;
}

}  // namespace

extern "C" int pcg_lingam_pair_scores(pcg_handle *h, const double *X, int64_t T, int64_t m, int64_t ldx, double *D,
                                      double *M) {
    if (!h) return PCG_ERR_INVALID;
    if (int rc = lg_check(h, "pcg_lingam_pair_scores", X, T, m, ldx)) return rc;
    if (!D) return pcg_fail(h, PCG_ERR_INVALID, "pcg_lingam_pair_scores: null D");
    PCG_HIP(h, hipSetDevice(h->device));
    LgScratch s;
    if (int rc = lg_scratch(h, "pcg_lingam_pair_scores", T, m, false, s)) return rc;
    if (int rc = lg_step(h, s, X, ldx, T, (int)m, 0, D, M, nullptr, nullptr)) return rc;
    PCG_HIP(h, hipStreamSynchronize(h->stream));
    return PCG_OK;
}

extern "C" int pcg_direct_lingam_order(pcg_handle *h, const double *X, int64_t T, int64_t n, int64_t ldx, int32_t *order,
                                       double *scores) {
    if (!h) return PCG_ERR_INVALID;
    if (int rc = lg_check(h, "pcg_direct_lingam_order", X, T, n, ldx)) return rc;
    if (!order) return pcg_fail(h, PCG_ERR_INVALID, "pcg_direct_lingam_order: null order");
    PCG_HIP(h, hipSetDevice(h->device));
    LgScratch s;
    if (int rc = lg_scratch(h, "pcg_direct_lingam_order", T, n, true, s)) return rc;
    if (scores) {
        hipLaunchKernelGGL(k_lingam_fill, dim3((unsigned)std::min<int64_t>(1024, (n * n + 255) / 256)), dim3(256), 0, h->stream,
                           scores, n * n, -INFINITY);
        PCG_HIP(h, hipGetLastError());
    }
    for (int64_t step = 0; step + 1 < n; ++step)
        if (int rc = lg_step(h, s, X, ldx, T, (int)(n - step), (int)step, s.D, nullptr, scores ? scores + step * n : nullptr,
                             step ? order + (step - 1) : nullptr))
            return rc;
    // the two-column step was step n - 2: its U list and M decide the last two entries
    hipLaunchKernelGGL(k_lingam_finish, dim3(1), dim3(64), 0, h->stream, (const double *)s.M,
                       (const int32_t *)s.U[(n >= 2 ? n - 2 : 0) & 1], order, (int)n, scores);
    PCG_HIP(h, hipGetLastError());
    PCG_HIP(h, hipStreamSynchronize(h->stream));
    return PCG_OK;
}
