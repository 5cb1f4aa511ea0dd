// granger.hip — pairwise Granger-causality regressions for RCAEval's granger graph learner.
//
// Replaces the n*(n-1) calls of statsmodels' `grangercausalitytests` [U] (statsmodels 0.14.0,
// RCAEval requirements.txt) made by RCAEval/graph_construction/granger.py:13-34. Per ordered pair
// (i caused = y, j causing = x) and lag L in 1..maxlag, over the window t = L..T-1 (nobs = T - L):
// the restricted OLS y_t ~ [y_{t-1..t-L}, 1] and the joint OLS y_t ~ [y_{t-1..t-L}, x_{t-1..t-L}, 1],
// both by pseudo-inverse (a rank-deficient design gives the least-squares SSR). Out per item
// (i, j, L): ssr_r, ssr_u, the centred tss, rank(joint) and a status. The four test statistics,
// their tails and the raising conditions are the caller's (graph_construction/granger.py), as
// ChiSqTester leaves chi2.sf to the host.
//
// Three kernels ("Granger"):
//   k_granger_cols   one block per column: mean, the mean-shifted column-major copy Z (n x T), the
//                    lag auto-moments of the L = 3 window, constant-window and non-finite bits.
//   k_granger_pairs  the hot path. Block (i, *) stages Z_i in LDS in T-chunks; each wave takes
//                    causing columns j, lanes stride over t and accumulate the 12 shifted cross
//                    moments x_{t-a} * y_{t-b} (a = 1..3, b = 0..3) of the L = 3 window in fp64.
//                    After the wave reduction, lane L-1 assembles the window-L Gram matrix of
//                    [y_{t-1..L}, x_{t-1..L}, y_t] (the L = 1, 2 windows add their first rows),
//                    eliminates the constant, scales to unit diagonal, Cholesky-factors and reads
//                    ssr_r / ssr_u off the y_t row. An item is accepted only under the guards
//                    below; every other item is appended to the exact list.
//   k_granger_exact  one block per listed item: the centred joint design in a bounded global
//                    workspace, Householder QR with block-wide reductions; a column whose
//                    remaining norm is below the matrix_rank tolerance is skipped (the pinv SSR).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "dense_dev.h"
#include "handle.h"

namespace {

constexpr int GR_BLOCK = 256;
constexpr int GR_WAVES = GR_BLOCK / 64;
constexpr int GR_CHUNK = 2048;            // rows of Z_i staged in LDS at a time (+3 rows of history)
constexpr int GR_CS = 16;                 // doubles of column statistics per column
// fast-path guards: smallest scaled pivot, floor on ssr_u / tss, and the checked step
// of the bound's derivation (1 + |beta|_1)^2 <= GR_BETA_C / GR_TAU
constexpr double GR_TAU = 1e-3;
constexpr double GR_FLOOR = 1e-2;
constexpr double GR_BETA_C = 14.0;
constexpr int64_t GR_WS_BYTES = (int64_t)256 << 20;   // exact path: design workspace bound
constexpr int64_t GR_MAX_N = 4096;        // the caller's five n x n x maxlag outputs are 1.6 GB there, the exact list 201 MB

// column status bits
constexpr int GR_BIT_Y0 = 6;              // bits 6..8: y window [L, T-1] constant
constexpr int GR_BIT_NONFINITE = 1 << 9;
__host__ __device__ constexpr int gr_lagbit(int L, int k) { return (L - 1) * L / 2 + (k - 1); }   // 0..5
__host__ __device__ constexpr int gr_lagmask(int L) { return ((1 << L) - 1) << ((L - 1) * L / 2); }
// index of the auto-moment sum z_{t-a} z_{t-b} (a <= b) in a column's statistics
__host__ __device__ constexpr int gr_pidx(int a, int b) { return 4 + a * 4 - a * (a - 1) / 2 + (b - a); }

// ---- column pass -------------------------------------------------------------------------------
// cs[c]: [0..3] sums of z_{t-k} over t = 3..T-1, [4..13] sums of z_{t-a} z_{t-b} (gr_pidx), [14] mean
__global__ __launch_bounds__(GR_BLOCK) void k_granger_cols(const double *X, int64_t T, int n, int64_t ldx, double *Zt,
                                                           double *cs, int32_t *bits) {
    __shared__ double red[14 * GR_WAVES];
    const int c = blockIdx.x, tid = threadIdx.x;
    const double *x = X + c;
    double a1[2] = {0.0, 0.0};                 // sum, count of non-finite values
    double lo = INFINITY, hi = -INFINITY;      // raw values over the core rows [3, T-4]
    for (int64_t t = tid; t < T; t += GR_BLOCK) {
        const double v = x[t * ldx];
        a1[0] += v;
        a1[1] += isfinite(v) ? 0.0 : 1.0;
        if (t >= 3 && t <= T - 4) {
            lo = fmin(lo, v);
            hi = fmax(hi, v);
        }
    }
    block_sum<GR_BLOCK>(a1, red);
    if (a1[1] > 0.0) {                         // block-uniform
        for (int64_t t = tid; t < T; t += GR_BLOCK) Zt[(int64_t)c * T + t] = __builtin_nan("");
        if (tid == 0) {
            for (int k = 0; k < GR_CS; ++k) cs[(int64_t)c * GR_CS + k] = __builtin_nan("");
            bits[c] = GR_BIT_NONFINITE;
        }
        return;
    }
    const double mean = a1[0] / (double)T;
    double *zc = Zt + (int64_t)c * T;
    for (int64_t t = tid; t < T; t += GR_BLOCK) zc[t] = x[t * ldx] - mean;
    __syncthreads();                           // the moments read rows other threads wrote
    double m[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) m[k] = 0.0;
    for (int64_t t = 3 + tid; t < T; t += GR_BLOCK) {
        double z[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) z[k] = zc[t - k];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            m[a] += z[a];
#pragma unroll
            for (int b = a; b < 4; ++b) m[gr_pidx(a, b)] = fma(z[a], z[b], m[gr_pidx(a, b)]);
        }
    }
    block_sum<GR_BLOCK>(m, red);
    block_minmax<GR_BLOCK>(lo, hi, red);
    if (tid == 0) {
        for (int k = 0; k < 14; ++k) cs[(int64_t)c * GR_CS + k] = m[k];
        cs[(int64_t)c * GR_CS + 14] = mean;
        cs[(int64_t)c * GR_CS + 15] = 0.0;
        // a window [a, b] with a <= 3 and b >= T-4 is rows a..min(2, b), the core, and
        // max(T-3, 3, a)..b
        auto constant = [&](int64_t a, int64_t b) {
            double wl = lo, wh = hi;
            for (int64_t t = a; t <= std::min<int64_t>(2, b); ++t) {
                wl = fmin(wl, x[t * ldx]);
                wh = fmax(wh, x[t * ldx]);
            }
            for (int64_t t = std::max<int64_t>(std::max<int64_t>(T - 3, 3), a); t <= b; ++t) {
                wl = fmin(wl, x[t * ldx]);
                wh = fmax(wh, x[t * ldx]);
            }
            return wl == wh;
        };
        int b = 0;
        for (int L = 1; L <= 3; ++L) {
            for (int k = 1; k <= L; ++k)
                if (constant(L - k, T - 1 - k)) b |= 1 << gr_lagbit(L, k);
            if (constant(L, T - 1)) b |= 1 << (GR_BIT_Y0 + L - 1);
        }
        bits[c] = b;
    }
}

// ---- fast pair kernel --------------------------------------------------------------------------
struct GrOut {
    double *ssr_r, *ssr_u, *tss;
    int32_t *rank, *status;
};

// variable u of the lag-L system [y_{t-1..L}, x_{t-1..L}, y_t]: its lag, and whether it is x
template <int L> __device__ constexpr int gr_lag(int u) { return u < L ? u + 1 : (u < 2 * L ? u - L + 1 : 0); }
template <int L> __device__ constexpr bool gr_isx(int u) { return u >= L && u < 2 * L; }

// One item on the fast path. zi3 / zj3: rows 0..2 of the shifted columns; csi / csj: column
// statistics; m: the cross moments sum_t x_{t-a} y_{t-b} at [(a-1)*4 + b] over t = 3..T-1.
// Returns false when a guard refuses the item.
template <int L>
__device__ bool gr_fast_item(const double *zi3, const double *zj3, const double *csi, const double *csj,
                             const double *m, int64_t T, double &ssr_r, double &ssr_u, double &tss) {
    constexpr int M = 2 * L + 1, Y0 = 2 * L;
    double s[M], G[M][M];
#pragma unroll
    for (int u = 0; u < M; ++u) {
        s[u] = (gr_isx<L>(u) ? csj : csi)[gr_lag<L>(u)];
#pragma unroll
        for (int v = u; v < M; ++v) {
            const int lu = gr_lag<L>(u), lv = gr_lag<L>(v);
            double g;
            if (gr_isx<L>(u) == gr_isx<L>(v))
                g = (gr_isx<L>(u) ? csj : csi)[gr_pidx(lu < lv ? lu : lv, lu < lv ? lv : lu)];
            else
                g = gr_isx<L>(u) ? m[(lu - 1) * 4 + lv] : m[(lv - 1) * 4 + lu];
            G[u][v] = g;
        }
    }
    // the first rows t = L..2 of the lag-L window
#pragma unroll
    for (int t = L; t <= 2; ++t) {
        double val[M];
#pragma unroll
        for (int u = 0; u < M; ++u) val[u] = (gr_isx<L>(u) ? zj3 : zi3)[t - gr_lag<L>(u)];
#pragma unroll
        for (int u = 0; u < M; ++u) {
            s[u] += val[u];
#pragma unroll
            for (int v = u; v < M; ++v) G[u][v] = fma(val[u], val[v], G[u][v]);
        }
    }
    // eliminate the constant, scale to unit diagonal
    const double inv_n = 1.0 / (double)(T - L);
    double d[M];
    bool ok = true;
#pragma unroll
    for (int u = 0; u < M; ++u) {
#pragma unroll
        for (int v = u; v < M; ++v) G[u][v] -= s[u] * s[v] * inv_n;
        ok = ok && (G[u][u] > 0.0) && isfinite(G[u][u]);
        d[u] = 1.0 / sqrt(G[u][u]);
    }
    if (!ok) return false;
    tss = G[Y0][Y0];
    // Cholesky of the scaled predictor block; ly: the y_t row of the factor
    double Lm[2 * L][2 * L], ly[2 * L];
#pragma unroll
    for (int k = 0; k < 2 * L; ++k) {
        double piv = 1.0;
#pragma unroll
        for (int c = 0; c < k; ++c) piv -= Lm[k][c] * Lm[k][c];
        ok = ok && (piv >= GR_TAU);
        const double lkk = sqrt(piv), ik = 1.0 / lkk;
        Lm[k][k] = lkk;
#pragma unroll
        for (int r = k + 1; r < 2 * L; ++r) {
            double a = G[k][r] * d[k] * d[r];
#pragma unroll
            for (int c = 0; c < k; ++c) a -= Lm[r][c] * Lm[k][c];
            Lm[r][k] = a * ik;
        }
        double a = G[k][Y0] * d[k] * d[Y0];
#pragma unroll
        for (int c = 0; c < k; ++c) a -= ly[c] * Lm[k][c];
        ly[k] = a * ik;
    }
    if (!ok) return false;
    double fit_r = 0.0, gain = 0.0;
#pragma unroll
    for (int c = 0; c < L; ++c) fit_r += ly[c] * ly[c];
#pragma unroll
    for (int c = L; c < 2 * L; ++c) gain += ly[c] * ly[c];
    const double s_r = 1.0 - fit_r, s_u = s_r - gain;
    // coefficients in scaled units (joint and restricted): the bound's (1 + |beta|_1)^2 factor
    double bu[2 * L], br[L], n1u = 0.0, n1r = 0.0;
#pragma unroll
    for (int k = 2 * L - 1; k >= 0; --k) {
        double a = ly[k];
#pragma unroll
        for (int r = k + 1; r < 2 * L; ++r) a -= Lm[r][k] * bu[r];
        bu[k] = a / Lm[k][k];
        n1u += fabs(bu[k]);
    }
#pragma unroll
    for (int k = L - 1; k >= 0; --k) {
        double a = ly[k];
#pragma unroll
        for (int r = k + 1; r < L; ++r) a -= Lm[r][k] * br[r];
        br[k] = a / Lm[k][k];
        n1r += fabs(br[k]);
    }
    const double n1 = fmax(n1u, n1r);
    if (!((1.0 + n1) * (1.0 + n1) <= GR_BETA_C / GR_TAU)) return false;
    if (!(s_u >= GR_FLOOR)) return false;
    ssr_r = tss * s_r;
    ssr_u = tss * s_u;
    return true;
}

__global__ __launch_bounds__(GR_BLOCK) void k_granger_pairs(const double *Zt, int64_t T, int n, int maxlag,
                                                            const double *cs, const int32_t *bits, GrOut out,
                                                            int32_t *list, unsigned int *counter) {
    __shared__ double ys[GR_CHUNK + 3];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *zi = Zt + (int64_t)i * T;
    const int bi = bits[i];
    const int nchunks = (int)((T - 3 + GR_CHUNK - 1) / GR_CHUNK);
    if (blockIdx.y == 0 && tid < maxlag) {     // the diagonal carries no test
        const int64_t it = ((int64_t)i * n + i) * maxlag + tid;
        out.ssr_r[it] = out.ssr_u[it] = out.tss[it] = __builtin_nan("");
        out.rank[it] = 0;
        out.status[it] = 0;
    }
    // a group of GR_WAVES causing columns per round, one per wave; a pair's 12 sums stay in
    // registers over the chunks, so with more than one chunk each round stages Z_i again
    for (int jbase = blockIdx.y * GR_WAVES; jbase < n; jbase += gridDim.y * GR_WAVES) {      // block-uniform
        const int j = jbase + wave;
        const bool live = j < n && j != i;
        const int bj = live ? bits[j] : 0;
        const bool run = live && !((bi | bj) & GR_BIT_NONFINITE);
        const double *zj = Zt + (int64_t)(live ? j : 0) * T;
        double m[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) m[k] = 0.0;
        for (int c = 0; c < nchunks; ++c) {
            const int64_t t0 = 3 + (int64_t)c * GR_CHUNK, t1 = std::min<int64_t>(T, t0 + GR_CHUNK);
            if (nchunks > 1 || jbase == (int)(blockIdx.y * GR_WAVES)) {
                __syncthreads();               // the previous chunk's readers are done
                for (int s = tid; s < (int)(t1 - t0) + 3; s += GR_BLOCK) ys[s] = zi[t0 - 3 + s];
                __syncthreads();
            }
            if (!run) continue;
            for (int64_t t = t0 + lane; t < t1; t += 64) {
                const int s = (int)(t - t0) + 3;
                double y[4], x[3];
#pragma unroll
                for (int b = 0; b < 4; ++b) y[b] = ys[s - b];
#pragma unroll
                for (int a = 0; a < 3; ++a) x[a] = zj[t - 1 - a];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) m[a * 4 + b] = fma(x[a], y[b], m[a * 4 + b]);
            }
        }
        if (!live) continue;
#pragma unroll
        for (int k = 0; k < 12; ++k) m[k] = wave_sum(m[k]);
        if (lane >= maxlag) continue;
        // lane L-1 finishes item (i, j, L)
        const int L = lane + 1;
        const int64_t it = ((int64_t)i * n + j) * maxlag + lane;
        double ssr_r = __builtin_nan(""), ssr_u = ssr_r, tss = ssr_r;
        int st = 0, rk = 0;
        if (!run) st = 4;
        else if ((bi | bj) & gr_lagmask(L)) st = 1;
        else if (bi & (1 << (GR_BIT_Y0 + L - 1))) st = 2;
        else {
            double zi3[3], zj3[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                zi3[k] = zi[k];
                zj3[k] = zj[k];
            }
            const double *csi = cs + (int64_t)i * GR_CS, *csj = cs + (int64_t)j * GR_CS;
            bool ok;
            if (L == 1) ok = gr_fast_item<1>(zi3, zj3, csi, csj, m, T, ssr_r, ssr_u, tss);
            else if (L == 2) ok = gr_fast_item<2>(zi3, zj3, csi, csj, m, T, ssr_r, ssr_u, tss);
            else ok = gr_fast_item<3>(zi3, zj3, csi, csj, m, T, ssr_r, ssr_u, tss);
            if (ok) rk = 2 * L + 1;
            else {
                list[atomicAdd(counter, 1u)] = (int32_t)it;
                st = 3;
            }
        }
        out.ssr_r[it] = ssr_r;
        out.ssr_u[it] = ssr_u;
        out.tss[it] = tss;
        out.rank[it] = rk;
        out.status[it] = st;
    }
}

// ---- exact kernel ------------------------------------------------------------------------------
// One block per listed item, each thread owning the rows r = tid, tid + 256, .. of the item's
// design for the whole factorisation (so no thread ever reads a row another thread wrote).
// A: the block's workspace slot, column-major M x nobs: [y_{t-1..L}, x_{t-1..L}, y_t] centred.
// Not dense_dev.h's qr_eliminate: up to 7 columns per row pass, rank test scaled by the column's own norm.
__global__ __launch_bounds__(GR_BLOCK) void k_granger_exact(const double *Zt, int64_t T, int n, int maxlag,
                                                            const int32_t *list, int64_t count, double *work,
                                                            int64_t slot, GrOut out) {
    __shared__ double red[7 * GR_WAVES];
    const int tid = threadIdx.x;
    double *A = work + (int64_t)blockIdx.x * slot;
    for (int64_t q = blockIdx.x; q < count; q += gridDim.x) {
        const int64_t it = list[q];
        const int L = (int)(it % maxlag) + 1, M = 2 * L + 1;
        const int64_t pair = it / maxlag;
        const int i = (int)(pair / n), j = (int)(pair % n);
        const int64_t nobs = T - L;
        const double *zi = Zt + (int64_t)i * T, *zj = Zt + (int64_t)j * T;
        // source of column u at row r (t = r + L)
        auto src = [&](int u, int64_t r) {
            const int lag = u < L ? u + 1 : (u < 2 * L ? u - L + 1 : 0);
            return ((u >= L && u < 2 * L) ? zj : zi)[r + L - lag];
        };
        double mu[7], cn[7];
#pragma unroll
        for (int u = 0; u < 7; ++u) mu[u] = 0.0;
        for (int64_t r = tid; r < nobs; r += GR_BLOCK)
#pragma unroll
            for (int u = 0; u < 7; ++u)
                if (u < M) mu[u] += src(u, r);
        block_sum<GR_BLOCK>(mu, red);
#pragma unroll
        for (int u = 0; u < 7; ++u) {
            mu[u] /= (double)nobs;
            cn[u] = 0.0;
        }
        for (int64_t r = tid; r < nobs; r += GR_BLOCK)
#pragma unroll
            for (int u = 0; u < 7; ++u)
                if (u < M) {
                    const double v = src(u, r) - mu[u];
                    A[(int64_t)u * nobs + r] = v;
                    cn[u] = fma(v, v, cn[u]);
                }
        block_sum<GR_BLOCK>(cn, red);
        const double tol = (double)std::max<int64_t>(nobs, M) * 2.220446049250313e-16;
        const double *yc = A + (int64_t)(M - 1) * nobs;
        int rdone = 0;                          // reflectors applied so far = rank of the lag columns
        double ssr_r = 0.0, ssr_u = 0.0;
        for (int k = 0; k < 2 * L; ++k) {
            double *ak = A + (int64_t)k * nobs;
            double nv[2] = {0.0, 0.0};          // remaining squared norm, the element on the diagonal
            for (int64_t r = tid; r < nobs; r += GR_BLOCK)
                if (r >= rdone) {
                    const double v = ak[r];
                    nv[0] = fma(v, v, nv[0]);
                    if (r == rdone) nv[1] = v;
                }
            block_sum<GR_BLOCK>(nv, red);
            double cnk = 0.0;
#pragma unroll
            for (int u = 0; u < 7; ++u)
                if (u == k) cnk = cn[u];
            if (cnk > 0.0 && nv[0] > tol * tol * cnk) {     // block-uniform: independent column
                const double alpha = -copysign(sqrt(nv[0]), nv[1]);
                const double vr = nv[1] - alpha;
                const double vn2 = 2.0 * (nv[0] - nv[1] * alpha);
                double dot[7];
#pragma unroll
                for (int u = 0; u < 7; ++u) dot[u] = 0.0;
                for (int64_t r = tid; r < nobs; r += GR_BLOCK)
                    if (r >= rdone) {
                        const double v = r == rdone ? vr : ak[r];
#pragma unroll
                        for (int u = 0; u < 7; ++u)
                            if (u > k && u < M) dot[u] = fma(v, A[(int64_t)u * nobs + r], dot[u]);
                    }
                block_sum<GR_BLOCK>(dot, red);
                for (int64_t r = tid; r < nobs; r += GR_BLOCK)
                    if (r >= rdone) {
                        const double v = r == rdone ? vr : ak[r];
#pragma unroll
                        for (int u = 0; u < 7; ++u)
                            if (u > k && u < M) A[(int64_t)u * nobs + r] -= (2.0 * dot[u] / vn2) * v;
                    }
                ++rdone;
            }
            if (k == L - 1 || k == 2 * L - 1) {
                double t2[1] = {0.0};
                for (int64_t r = tid; r < nobs; r += GR_BLOCK)
                    if (r >= rdone) t2[0] = fma(yc[r], yc[r], t2[0]);
                block_sum<GR_BLOCK>(t2, red);
                if (k == L - 1) ssr_r = t2[0];
                else ssr_u = t2[0];
            }
        }
        if (tid == 0) {
            double tss = 0.0;
#pragma unroll
            for (int u = 0; u < 7; ++u)
                if (u == M - 1) tss = cn[u];
            const bool perfect = !(tss > 0.0) || !(ssr_u > 0.0) || ssr_u / tss < 2.220446049250313e-16;
            out.ssr_r[it] = ssr_r;
            out.ssr_u[it] = ssr_u;
            out.tss[it] = tss;
            out.rank[it] = rdone + 1;
            out.status[it] = perfect ? 2 : 3;
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int pcg_granger_guards(double *tau, double *floor, double *beta_c) {
    if (tau) *tau = GR_TAU;
    if (floor) *floor = GR_FLOOR;
    if (beta_c) *beta_c = GR_BETA_C;
    return PCG_OK;
}

extern "C" int pcg_granger(pcg_handle *h, const double *X, int64_t T, int64_t n, int64_t ldx, int maxlag,
                           double *ssr_r, double *ssr_u, double *tss, int32_t *rank, int32_t *status,
                           int64_t *exact_items) {
    if (!h) return PCG_ERR_INVALID;
    if (maxlag < 1 || maxlag > 3) return pcg_fail(h, PCG_ERR_INVALID, "pcg_granger: maxlag %d outside 1..3", maxlag);
    if (n < 2 || n > GR_MAX_N || ldx < n || T < 1)
        return pcg_fail(h, PCG_ERR_INVALID, "pcg_granger: bad shape (T=%lld n=%lld ldx=%lld)", (long long)T,
                        (long long)n, (long long)ldx);
    if (T <= 3 * (int64_t)maxlag + 1)
        return pcg_fail(h, PCG_ERR_DOMAIN, "pcg_granger: Insufficient observations (T=%lld <= 3 * maxlag + 1 = %d)",
                        (long long)T, 3 * maxlag + 1);
    if (!X || !ssr_r || !ssr_u || !tss || !rank || !status) return pcg_fail(h, PCG_ERR_INVALID, "pcg_granger: null pointer");
    PCG_HIP(h, hipSetDevice(h->device));
    const int64_t items = n * n * maxlag;
    // scratch: Z (n x T) | column statistics | column bits | exact list | its counter
    Carve cv;
    const size_t o_z = cv.take((size_t)n * T * 8), o_cs = cv.take((size_t)n * GR_CS * 8),
                 o_bits = cv.take((size_t)n * 4), o_list = cv.take((size_t)items * 4), o_ctr = cv.take(4);
    if (!pcg_ensure(h, h->granger_scratch, cv.total))
        return pcg_fail(h, PCG_ERR_OOM, "pcg_granger: scratch (%lld B)", (long long)cv.total);
    char *base = (char *)h->granger_scratch.p;
    double *Zt = (double *)(base + o_z), *cs = (double *)(base + o_cs);
    int32_t *bits = (int32_t *)(base + o_bits), *list = (int32_t *)(base + o_list);
    unsigned int *ctr = (unsigned int *)(base + o_ctr);
    const GrOut out{ssr_r, ssr_u, tss, rank, status};
    PCG_HIP(h, hipMemsetAsync(ctr, 0, 4, h->stream));
    hipLaunchKernelGGL(k_granger_cols, dim3((unsigned)n), dim3(GR_BLOCK), 0, h->stream, X, T, (int)n, ldx, Zt, cs, bits);
    PCG_HIP(h, hipGetLastError());
    // blockIdx.y splits a caused column's causing columns over more blocks when n alone leaves
    // CUs idle (about 4 blocks per CU of a 256-CU part)
    const int64_t per_col = (n + GR_WAVES - 1) / GR_WAVES;
    const unsigned gy = (unsigned)std::max<int64_t>(1, std::min<int64_t>(per_col, 1024 / n));
    hipLaunchKernelGGL(k_granger_pairs, dim3((unsigned)n, gy), dim3(GR_BLOCK), 0, h->stream, (const double *)Zt, T, (int)n,
                       maxlag, (const double *)cs, (const int32_t *)bits, out, list, ctr);
    PCG_HIP(h, hipGetLastError());
    int64_t marked = 0;
    if (int rc = pcg_read_counter(h, "pcg_granger", ctr, items, &marked)) return rc;
    if (marked) {
        const int64_t slot = 7 * T;            // doubles per block: M <= 7 columns of nobs < T rows
        const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>({marked, 2048, GR_WS_BYTES / (slot * 8)}));
        if (!pcg_ensure(h, h->granger_work, (size_t)(blocks * slot * 8)))
            return pcg_fail(h, PCG_ERR_OOM, "pcg_granger: exact workspace (%lld B)", (long long)(blocks * slot * 8));
        hipLaunchKernelGGL(k_granger_exact, dim3((unsigned)blocks), dim3(GR_BLOCK), 0, h->stream, (const double *)Zt, T,
                           (int)n, maxlag, (const int32_t *)list, marked, (double *)h->granger_work.p, slot, out);
        PCG_HIP(h, hipGetLastError());
        PCG_HIP(h, hipStreamSynchronize(h->stream));
    }
    if (exact_items) *exact_items = marked;
    return PCG_OK;
}
