// cmlp.hip — full-batch ISTA training of RCAEval's cMLP neural Granger learner.
//
// Replaces the training loop of RCAEval/graph_construction/cmlp.py:478-540 (`train_model_ista`,
// penalty "H") for the model `cmlp()` builds (:591-618): p networks Conv1d(p, hidden, lag) -> ReLU ->
// Conv1d(hidden, 1, 1), all fp32. With N = T - lag samples and K = lag * p inputs, every network
// reads the same lag-expanded matrix A (N x K, A[n, c * lag + k] = X[n + k, c]), and torch's
// W1[hidden][p][lag] is already the row-major hidden x K matrix that multiplies it.
//
// Kernels ("cMLP"):
//   k_cmlp_lag    A, zero-padded to Npad x Kpad, once per call.
//   k_cmlp_fwd    block (row tile of 64, network i): Z = A W1_i^T on v_mfma_f32_16x16x4_f32, then
//                 in registers b1, ReLU, the w2 dot product (16-lane shuffle), the residual and
//                 g = 2 r / N. Out: dZ = g w2 [Z > 0] (Npad x HP per network, zero in the padding)
//                 and the tile's fp64 sums over its samples of dZ, g relu(Z), g and r^2.
//   k_cmlp_bwd    block (16 input series, network i): dW1 = dZ^T A for all hidden rows of its
//                 16 * lag columns on the same MFMA; the epilogue takes the gradient step into an
//                 LDS tile, runs the lag stages of the hierarchical prox on it (16 lanes per
//                 (network, series) group) and writes W1 back. Block 0 of a network also adds up
//                 the tile sums (db1, dw2 + ridge, db2) in tile order and steps b1, w2, b2. No
//                 block reads what another block of the launch writes.
//   k_cmlp_check  per network: MSE from the tile sums, the ridge term and the hierarchical penalty
//   k_cmlp_total  their sum over networks / p: the scalar the host reads at a check.
// Every sum has a fixed order (k-ordered MFMA chains, shuffles, serial tile sums), there are no
// atomics, and an iteration is two launches; the host reads one double per check.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "dense_dev.h"
#include "handle.h"

namespace {

constexpr int CM_BLOCK = 256;
constexpr int CM_MAX_HIDDEN = 128, CM_MAX_LAG = 8, CM_MAX_P = 1024;
constexpr int CM_TM = 64;                 // forward: samples per block (16 per wave)
constexpr int CM_KC = 32;                 // forward: inputs staged per step
constexpr int CM_FS = 36;                 // forward: LDS row stride (floats); 36 r + c hits 64 banks once
constexpr int CM_CT = 16;                 // backward: input series per block (16 * lag columns)
constexpr int CM_NC = 32;                 // backward: samples staged per step
constexpr int CM_BS = 144;                // backward: LDS row stride (floats), 144 mod 64 = 16

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct CmShape {
    int p, lag, hidden, HP, K, Kf, Kpad, tiles;   // HP: hidden rounded up to 16; Kf: K rounded up to CM_KC
    int64_t N, Npad, pstride;                     // pstride: floats per network in `params`
};

__host__ __device__ inline int64_t cm_off_b1(const CmShape &s) { return (int64_t)s.hidden * s.K; }
// doubles per (network, row tile) of the forward pass's sums: db1[HP], dw2[HP], sum g, sum r^2
__host__ __device__ inline int cm_tstride(const CmShape &s) { return 2 * s.HP + 2; }

__global__ __launch_bounds__(CM_BLOCK) void k_cmlp_lag(const float *X, int64_t ldx, CmShape s, float *A) {
    const int64_t total = s.Npad * s.Kpad;
    for (int64_t q = (int64_t)blockIdx.x * CM_BLOCK + threadIdx.x; q < total; q += (int64_t)gridDim.x * CM_BLOCK) {
        const int64_t n = q / s.Kpad;
        const int j = (int)(q - n * s.Kpad), c = j / s.lag, k = j - c * s.lag;
        A[q] = (n < s.N && c < s.p) ? X[(n + k) * ldx + c] : 0.f;
    }
}

// ---- forward -----------------------------------------------------------------------------------
// NCT: HP / 16, a template parameter so that every MFMA and its accumulator are unconditional
template <int NCT>
__global__ __launch_bounds__(CM_BLOCK) void k_cmlp_fwd(const float *A, const float *X, int64_t ldx, CmShape s,
                                                       const float *params, float *dZ, double *tparts) {
    __shared__ __attribute__((aligned(16))) float As[CM_TM * CM_FS];
    __shared__ __attribute__((aligned(16))) float Ws[CM_MAX_HIDDEN * CM_FS];
    __shared__ double red[2 * CM_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr16 = lane & 15, lq = lane >> 4;
    const int i = blockIdx.y, tile = blockIdx.x;
    const int64_t n0 = (int64_t)tile * CM_TM;
    const float *W1 = params + (int64_t)i * s.pstride, *b1 = W1 + cm_off_b1(s), *w2 = b1 + s.hidden, *b2 = w2 + s.hidden;
    f32x4 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the next step's A and W1 pieces travel in registers while this step's MFMAs run; W1 is read
    // at clamped addresses and zeroed by select, so the 16 loads issue back to back
    f32x4 av[2];
    float wv[16];
#define CM_FWD_FETCH(k0_)                                                                       \
    do {                                                                                        \
        _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                         \
            const int q = tid + u * CM_BLOCK, r = q >> 3, c4 = (q & 7) * 4;                     \
            av[u] = *(const f32x4 *)&A[(n0 + r) * s.Kpad + (k0_) + c4];                        \
        }                                                                                       \
        _Pragma("unroll") for (int u = 0; u < 16; ++u) {                                        \
            const int q = tid + u * CM_BLOCK, hh = q >> 5, j = (k0_) + (q & 31);                \
            const float v = W1[(int64_t)min(hh, s.hidden - 1) * s.K + min(j, s.K - 1)];         \
            wv[u] = (hh < s.hidden && j < s.K) ? v : 0.f;                                       \
        }                                                                                       \
    } while (0)
    CM_FWD_FETCH(0);
    for (int k0 = 0; k0 < s.Kf; k0 += CM_KC) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int q = tid + u * CM_BLOCK, r = q >> 3, c4 = (q & 7) * 4;
            *(f32x4 *)&As[r * CM_FS + c4] = av[u];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int q = tid + u * CM_BLOCK;
            Ws[(q >> 5) * CM_FS + (q & 31)] = wv[u];
        }
        __syncthreads();
        if (k0 + CM_KC < s.Kf) CM_FWD_FETCH(k0 + CM_KC);
#pragma unroll
        for (int ks = 0; ks < CM_KC / 4; ++ks) {
            const float a = As[(wave * 16 + lr16) * CM_FS + ks * 4 + lq];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const float b = Ws[(ct * 16 + lr16) * CM_FS + ks * 4 + lq];
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[ct], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // acc[ct][reg]: sample n0 + wave * 16 + lq * 4 + reg, hidden unit ct * 16 + lr16
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const int hh = ct * 16 + lr16;
        const float bb = hh < s.hidden ? b1[hh] : 0.f, ww = hh < s.hidden ? w2[hh] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float z = acc[ct][r] + bb;
            acc[ct][r] = z;
            o[r] = fmaf(fmaxf(z, 0.f), ww, o[r]);
        }
    }
    const float bias2 = b2[0], scale = 2.f / (float)s.N;
    float g[4];
    double l2 = 0.0, gs = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float v = o[r];
        for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 64);
        const int64_t n = n0 + wave * 16 + lq * 4 + r;
        const float res = n < s.N ? (v + bias2) - X[(n + s.lag) * ldx + i] : 0.f;
        g[r] = scale * res;
        l2 += (double)res * (double)res;
        gs += (double)g[r];
    }
    // dZ out, and the tile's sums over its samples of dZ (db1), g relu(Z) (dw2), g (db2) and r^2:
    // registers, then the lane groups of a wave, then the waves through LDS (Ws is free)
    float *dZi = dZ + (int64_t)i * s.Npad * s.HP;
    double *wred = (double *)Ws;                  // [wave][2 HP]
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const int hh = ct * 16 + lr16;
        const float ww = hh < s.hidden ? w2[hh] : 0.f;
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t n = n0 + wave * 16 + lq * 4 + r;
            const float z = acc[ct][r], dz = z > 0.f ? g[r] * ww : 0.f;
            dZi[n * s.HP + hh] = dz;
            s1 += (double)dz;
            s2 += (double)(g[r] * fmaxf(z, 0.f));
        }
        s1 += __shfl_xor(s1, 16, 64);
        s1 += __shfl_xor(s1, 32, 64);
        s2 += __shfl_xor(s2, 16, 64);
        s2 += __shfl_xor(s2, 32, 64);
        if (lq == 0) {
            wred[wave * 2 * s.HP + hh] = s1;
            wred[wave * 2 * s.HP + s.HP + hh] = s2;
        }
    }
    l2 = wave_sum(lr16 == 0 ? l2 : 0.0);
    gs = wave_sum(lr16 == 0 ? gs : 0.0);
    if (lane == 0) {
        red[wave] = l2;
        red[CM_BLOCK / 64 + wave] = gs;
    }
    __syncthreads();
    double *tp = tparts + ((int64_t)i * s.tiles + tile) * cm_tstride(s);
    for (int q = tid; q < 2 * s.HP; q += CM_BLOCK)
        tp[q] = ((wred[q] + wred[2 * s.HP + q]) + wred[4 * s.HP + q]) + wred[6 * s.HP + q];
    if (tid == 0) {
        tp[2 * s.HP] = ((red[4] + red[5]) + red[6]) + red[7];
        tp[2 * s.HP + 1] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

// ---- backward, step and prox -------------------------------------------------------------------
// LAG: the lag, a template parameter for the same reason
template <int LAG>
__global__ __launch_bounds__(CM_BLOCK) void k_cmlp_bwd(const float *A, CmShape s, float *params, const float *dZ,
                                                       const double *tparts, float lr, float thr, int prox,
                                                       float lam_ridge) {
    extern __shared__ float4 cm_smem[];
    float *sm = (float *)cm_smem;
    float *Ds = sm, *Bs = sm + CM_NC * CM_BS;     // main loop: dZ and A chunks
    float *Wt = sm;                               // epilogue: HP x W tile of the stepped W1 (aliases them)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr16 = lane & 15, lq = lane >> 4;
    constexpr int W = CM_CT * LAG;
    const int i = blockIdx.y, j0 = blockIdx.x * W;
    const int nrt = s.HP / 16, hp4 = s.HP / 4, w4 = W / 4;
    float *W1 = params + (int64_t)i * s.pstride;
    const float *dZi = dZ + (int64_t)i * s.Npad * s.HP;
    f32x4 acc[2][LAG];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int ct = 0; ct < LAG; ++ct) acc[r][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool on0 = wave < nrt, on1 = wave + 4 < nrt;
    // each thread's (up to) four float4 pieces of a dZ chunk and of an A chunk: offsets once, then
    // the next chunk travels in registers while this chunk's MFMAs run
    int dsrc[4], ddst[4], bsrc[4], bdst[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int q = tid + u * CM_BLOCK;
        const int rd = q / hp4, cd = (q - rd * hp4) * 4, rb = q / w4, cb = (q - rb * w4) * 4;
        dsrc[u] = rd < CM_NC ? rd * s.HP + cd : -1;
        ddst[u] = rd * CM_BS + cd;
        bsrc[u] = rb < CM_NC ? rb * s.Kpad + j0 + cb : -1;
        bdst[u] = rb * CM_BS + cb;
    }
    f32x4 dv[4], bv[4];
#define CM_BWD_FETCH(n0_)                                                                       \
    do {                                                                                        \
        _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                         \
            dv[u] = *(const f32x4 *)&dZi[(n0_) * s.HP + max(dsrc[u], 0)];                      \
            bv[u] = *(const f32x4 *)&A[(n0_) * s.Kpad + max(bsrc[u], j0)];                     \
        }                                                                                       \
    } while (0)
    CM_BWD_FETCH((int64_t)0);
    for (int64_t n0 = 0; n0 < s.Npad; n0 += CM_NC) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (dsrc[u] >= 0) *(f32x4 *)&Ds[ddst[u]] = dv[u];
            if (bsrc[u] >= 0) *(f32x4 *)&Bs[bdst[u]] = bv[u];
        }
        __syncthreads();
        if (n0 + CM_NC < s.Npad) CM_BWD_FETCH(n0 + CM_NC);
        // a wave without a row tile multiplies zeros: no branch around an MFMA
#pragma unroll
        for (int ks = 0; ks < CM_NC / 4; ++ks) {
            const int kk = ks * 4 + lq;
            const float a0 = on0 ? Ds[kk * CM_BS + wave * 16 + lr16] : 0.f;
            const float a1 = on1 ? Ds[kk * CM_BS + (wave + 4) * 16 + lr16] : 0.f;
#pragma unroll
            for (int ct = 0; ct < LAG; ++ct) {
                const float b = Bs[kk * CM_BS + ct * 16 + lr16];
                acc[0][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b, acc[0][ct], 0, 0, 0);
                acc[1][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b, acc[1][ct], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // gradient step into the LDS tile: acc[r][ct][reg] is hidden (wave + 4 r) * 16 + lq * 4 + reg,
    // column j0 + ct * 16 + lr16
#pragma unroll
    for (int r = 0; r < 2; ++r)
        if (r == 0 ? on0 : on1) {
#pragma unroll
            for (int ct = 0; ct < LAG; ++ct) {
                const int jl = ct * 16 + lr16, j = j0 + jl;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int hh = (wave + 4 * r) * 16 + lq * 4 + e;
                    float v = 0.f;
                    if (hh < s.hidden && j < s.K)
                        v = __fsub_rn(W1[(int64_t)hh * s.K + j], __fmul_rn(lr, acc[r][ct][e]));
                    Wt[hh * W + jl] = v;
                }
            }
        }
    __syncthreads();
    if (prox) {
        // 16 lanes per (network, series) group; a lane keeps the hidden rows t, t + 16, .. through
        // all stages, so the stages need no barrier between them
        const int cl = tid >> 4, t = tid & 15;
        for (int kk = 0; kk < LAG; ++kk) {
            double ss = 0.0;
            for (int hh = t; hh < s.hidden; hh += 16)
                for (int k = 0; k <= kk; ++k) {
                    const double v = (double)Wt[hh * W + cl * LAG + k];
                    ss = fma(v, v, ss);
                }
            for (int m = 1; m < 16; m <<= 1) ss += __shfl_xor(ss, m, 64);
            const float nrm = (float)sqrt(ss);
            const float den = fmaxf(nrm, thr), num = fmaxf(__fsub_rn(nrm, thr), 0.f);
            for (int hh = t; hh < s.hidden; hh += 16)
                for (int k = 0; k <= kk; ++k) {
                    float *w = &Wt[hh * W + cl * LAG + k];
                    *w = __fmul_rn(__fdiv_rn(*w, den), num);
                }
        }
        __syncthreads();
    }
    for (int q = tid; q < s.hidden * W; q += CM_BLOCK) {
        const int hh = q / W, jl = q - hh * W, j = j0 + jl;
        if (j < s.K) W1[(int64_t)hh * s.K + j] = Wt[hh * W + jl];
    }
    if (blockIdx.x != 0) return;
    // b1, w2, b2 of network i: the forward pass's tile sums in tile order
    float *b1 = W1 + cm_off_b1(s), *w2 = b1 + s.hidden, *b2 = w2 + s.hidden;
    const int ts = cm_tstride(s);
    const double *tp = tparts + (int64_t)i * s.tiles * ts;
    const int hh = tid & 127;
    if (hh < s.hidden) {
        const double *src = tp + (tid < 128 ? 0 : s.HP) + hh;
        double sum = 0.0;
        for (int t = 0; t < s.tiles; ++t) sum += src[(int64_t)t * ts];
        if (tid < 128) b1[hh] = __fsub_rn(b1[hh], __fmul_rn(lr, (float)sum));
        else {
            const float w = w2[hh], grad = __fadd_rn((float)sum, __fmul_rn(__fmul_rn(w, 2.f), lam_ridge));
            w2[hh] = __fsub_rn(w, __fmul_rn(lr, grad));
        }
    }
    if (tid == 0) {
        double sg = 0.0;
        for (int t = 0; t < s.tiles; ++t) sg += tp[(int64_t)t * ts + 2 * s.HP];
        b2[0] = __fsub_rn(b2[0], __fmul_rn(lr, (float)sg));
    }
}

// ---- the check's loss --------------------------------------------------------------------------
// part[i] = mse_i + lam_ridge |w2_i|^2 + lam sum_c sum_k |W1_i[:, c, :k+1]|; mse[i] alone as well
__global__ __launch_bounds__(CM_BLOCK) void k_cmlp_check(CmShape s, const float *params, const double *tparts,
                                                         double lam, double lam_ridge, double *part, double *mse) {
    __shared__ double red[CM_BLOCK / 64];
    const int i = blockIdx.x, tid = threadIdx.x;
    const float *W1 = params + (int64_t)i * s.pstride, *w2 = W1 + cm_off_b1(s) + s.hidden;
    double pen = 0.0;
    for (int c = tid; c < s.p; c += CM_BLOCK) {
        double q[CM_MAX_LAG];
#pragma unroll
        for (int k = 0; k < CM_MAX_LAG; ++k) q[k] = 0.0;
        for (int hh = 0; hh < s.hidden; ++hh) {
            const float *w = W1 + (int64_t)hh * s.K + (int64_t)c * s.lag;
#pragma unroll
            for (int k = 0; k < CM_MAX_LAG; ++k)
                if (k < s.lag) {
                    const double v = (double)w[k];
                    q[k] = fma(v, v, q[k]);
                }
        }
        double cum = 0.0;
#pragma unroll
        for (int k = 0; k < CM_MAX_LAG; ++k)
            if (k < s.lag) {
                cum += q[k];
                pen += sqrt(cum);
            }
    }
    pen = block_sum<CM_BLOCK>(pen, red);
    double r2 = 0.0;
    for (int hh = tid; hh < s.hidden; hh += CM_BLOCK) r2 = fma((double)w2[hh], (double)w2[hh], r2);
    r2 = block_sum<CM_BLOCK>(r2, red);
    if (tid == 0) {
        double l2 = 0.0;
        for (int t = 0; t < s.tiles; ++t) l2 += tparts[((int64_t)i * s.tiles + t) * cm_tstride(s) + 2 * s.HP + 1];
        const double m = l2 / (double)s.N;
        mse[i] = m;
        part[i] = m + lam_ridge * r2 + lam * pen;
    }
}

__global__ __launch_bounds__(CM_BLOCK) void k_cmlp_total(int p, const double *part, double *out) {
    __shared__ double red[CM_BLOCK / 64];
    double v = 0.0;
    for (int i = threadIdx.x; i < p; i += CM_BLOCK) v += part[i];
    v = block_sum<CM_BLOCK>(v, red);
    if (threadIdx.x == 0) out[0] = v / (double)p;
}

// ---- host --------------------------------------------------------------------------------------
struct CmRun {
    CmShape s;
    const float *X;
    int64_t ldx;
    float *params, *A, *dZ, *best;
    double *tparts, *part, *mse, *total;
    float lr, thr, lam_ridge;
    int prox;
    double lam, lam_ridge_d;
    size_t lds;
};

// argument checks of both entry points: nothing is launched or allocated before they pass
int cm_validate(pcg_handle *h, const char *who, const float *X, int64_t T, int64_t p, int64_t ldx, int lag, int hidden,
                const float *params, double lr, double lam, double lam_ridge) {
    if (lag < 1 || lag > CM_MAX_LAG || hidden < 1 || hidden > CM_MAX_HIDDEN)
        return pcg_fail(h, PCG_ERR_INVALID, "%s: lag %d outside 1..%d or hidden %d outside 1..%d", who, lag, CM_MAX_LAG,
                        hidden, CM_MAX_HIDDEN);
    if (p < 1 || p > CM_MAX_P || ldx < p || T < 1 || T > ((int64_t)1 << 24))
        return pcg_fail(h, PCG_ERR_INVALID, "%s: bad shape (T=%lld p=%lld ldx=%lld)", who, (long long)T, (long long)p,
                        (long long)ldx);
    if (!X || !params) return pcg_fail(h, PCG_ERR_INVALID, "%s: null pointer", who);
    if (!(lr > 0.0) || !(lam >= 0.0) || !(lam_ridge >= 0.0) || !std::isfinite(lr) || !std::isfinite(lam) ||
        !std::isfinite(lam_ridge))
        return pcg_fail(h, PCG_ERR_INVALID, "%s: lr must be positive and finite, lam and lam_ridge non-negative", who);
    if (T <= lag)
        return pcg_fail(h, PCG_ERR_DOMAIN, "%s: no sample to fit (T=%lld <= lag=%d)", who, (long long)T, lag);
    return PCG_OK;
}

// scratch, the launch constants and the lag-expanded A
int cm_setup(pcg_handle *h, const char *who, const float *X, int64_t T, int64_t p, int64_t ldx, int lag, int hidden,
             float *params, double lr, double lam, double lam_ridge, bool want_best, CmRun &r) {
    CmShape &s = r.s;
    s.p = (int)p;
    s.lag = lag;
    s.hidden = hidden;
    s.HP = (hidden + 15) / 16 * 16;
    s.K = lag * (int)p;
    s.Kf = (s.K + CM_KC - 1) / CM_KC * CM_KC;
    const int wcols = (int)((p + CM_CT - 1) / CM_CT) * CM_CT * lag;      // the backward blocks' columns
    s.Kpad = (std::max(s.Kf, wcols) + 31) / 32 * 32;
    s.N = T - lag;
    s.Npad = (s.N + CM_TM - 1) / CM_TM * CM_TM;
    s.tiles = (int)(s.Npad / CM_TM);
    s.pstride = (int64_t)hidden * s.K + 2 * hidden + 1;
    Carve cv;
    const size_t act = (size_t)p * s.Npad * s.HP * 4;
    const size_t o_a = cv.take((size_t)s.Npad * s.Kpad * 4), o_dz = cv.take(act),
                 o_tp = cv.take((size_t)p * s.tiles * cm_tstride(s) * 8), o_part = cv.take((size_t)p * 8), o_mse = cv.take((size_t)p * 8), o_tot = cv.take(8);
    if (!pcg_ensure(h, h->cmlp_scratch, cv.total))
        return pcg_fail(h, PCG_ERR_OOM, "%s: scratch (%lld B)", who, (long long)cv.total);
    if (want_best && !pcg_ensure(h, h->cmlp_best, (size_t)p * s.pstride * 4))
        return pcg_fail(h, PCG_ERR_OOM, "%s: snapshot (%lld B)", who, (long long)(p * s.pstride * 4));
    char *base = (char *)h->cmlp_scratch.p;
    r.X = X;
    r.ldx = ldx;
    r.params = params;
    r.A = (float *)(base + o_a);
    r.dZ = (float *)(base + o_dz);
    r.tparts = (double *)(base + o_tp);
    r.part = (double *)(base + o_part);
    r.mse = (double *)(base + o_mse);
    r.total = (double *)(base + o_tot);
    r.best = want_best ? (float *)h->cmlp_best.p : nullptr;
    r.lr = (float)lr;
    r.thr = (float)(lr * lam);
    r.prox = lam > 0.0;
    r.lam_ridge = (float)lam_ridge;
    r.lam = lam;
    r.lam_ridge_d = lam_ridge;
    r.lds = std::max((size_t)2 * CM_NC * CM_BS, (size_t)s.HP * CM_CT * lag) * sizeof(float);
    PCG_HIP(h, hipSetDevice(h->device));
    const int64_t cells = s.Npad * s.Kpad;
    hipLaunchKernelGGL(k_cmlp_lag, dim3((unsigned)std::min<int64_t>((cells + CM_BLOCK - 1) / CM_BLOCK, 4096)),
                       dim3(CM_BLOCK), 0, h->stream, X, ldx, s, r.A);
    PCG_HIP(h, hipGetLastError());
    return PCG_OK;
}

int cm_forward(pcg_handle *h, const CmRun &r) {
    const dim3 grid((unsigned)r.s.tiles, (unsigned)r.s.p);
#define CM_FWD(NCT)                                                                                        \
    case NCT:                                                                                              \
        hipLaunchKernelGGL(k_cmlp_fwd<NCT>, grid, dim3(CM_BLOCK), 0, h->stream, (const float *)r.A, r.X, r.ldx, r.s, \
                           (const float *)r.params, r.dZ, r.tparts);                                       \
        break
    switch (r.s.HP / 16) {
        CM_FWD(1); CM_FWD(2); CM_FWD(3); CM_FWD(4); CM_FWD(5); CM_FWD(6); CM_FWD(7); CM_FWD(8);
    }
#undef CM_FWD
    PCG_HIP(h, hipGetLastError());
    return PCG_OK;
}

int cm_backward(pcg_handle *h, const CmRun &r) {
    const dim3 grid((unsigned)((r.s.p + CM_CT - 1) / CM_CT), (unsigned)r.s.p);
#define CM_BWD(LAG)                                                                                        \
    case LAG:                                                                                              \
        hipLaunchKernelGGL(k_cmlp_bwd<LAG>, grid, dim3(CM_BLOCK), r.lds, h->stream, (const float *)r.A, r.s, r.params, \
                           (const float *)r.dZ, (const double *)r.tparts, r.lr, r.thr, r.prox, r.lam_ridge); \
        break
    switch (r.s.lag) {
        CM_BWD(1); CM_BWD(2); CM_BWD(3); CM_BWD(4); CM_BWD(5); CM_BWD(6); CM_BWD(7); CM_BWD(8);
    }
#undef CM_BWD
    PCG_HIP(h, hipGetLastError());
    return PCG_OK;
}

// the losses of the forward pass last enqueued
int cm_losses(pcg_handle *h, const CmRun &r) {
    hipLaunchKernelGGL(k_cmlp_check, dim3((unsigned)r.s.p), dim3(CM_BLOCK), 0, h->stream, r.s, (const float *)r.params,
                       (const double *)r.tparts, r.lam, r.lam_ridge_d, r.part, r.mse);
    PCG_HIP(h, hipGetLastError());
    hipLaunchKernelGGL(k_cmlp_total, dim3(1), dim3(CM_BLOCK), 0, h->stream, r.s.p, (const double *)r.part, r.total);
    PCG_HIP(h, hipGetLastError());
    return PCG_OK;
}

}  // namespace

extern "C" int pcg_cmlp_limits(int32_t *max_hidden, int32_t *max_lag, int32_t *max_p) {
    if (max_hidden) *max_hidden = CM_MAX_HIDDEN;
    if (max_lag) *max_lag = CM_MAX_LAG;
    if (max_p) *max_p = CM_MAX_P;
    return PCG_OK;
}

extern "C" int pcg_cmlp_steps(pcg_handle *h, const float *X, int64_t T, int64_t p, int64_t ldx, int lag, int hidden,
                              float *params, double lr, double lam, double lam_ridge, int64_t k, double *smooth) {
    if (!h) return PCG_ERR_INVALID;
    if (k < 0) return pcg_fail(h, PCG_ERR_INVALID, "pcg_cmlp_steps: k = %lld", (long long)k);
    if (int rc = cm_validate(h, "pcg_cmlp_steps", X, T, p, ldx, lag, hidden, params, lr, lam, lam_ridge)) return rc;
    CmRun r;
    if (int rc = cm_setup(h, "pcg_cmlp_steps", X, T, p, ldx, lag, hidden, params, lr, lam, lam_ridge, false, r)) return rc;
    for (int64_t it = 0; it < k; ++it) {
        if (int rc = cm_forward(h, r)) return rc;
        if (int rc = cm_backward(h, r)) return rc;
    }
    if (smooth) {
        if (int rc = cm_forward(h, r)) return rc;
        if (int rc = cm_losses(h, r)) return rc;
        PCG_HIP(h, hipMemcpyAsync(smooth, r.mse, (size_t)p * 8, hipMemcpyDeviceToHost, h->stream));
    }
    PCG_HIP(h, hipStreamSynchronize(h->stream));
    return PCG_OK;
}

extern "C" int pcg_cmlp_train(pcg_handle *h, const float *X, int64_t T, int64_t p, int64_t ldx, int lag, int hidden,
                              float *params, double lr, double lam, double lam_ridge, int64_t max_iter,
                              int64_t check_every, int64_t lookback, double *losses, int64_t *n_checks,
                              int64_t *best_it, int64_t *last_it) {
    if (!h) return PCG_ERR_INVALID;
    if (max_iter < 0 || check_every < 1 || lookback < 0 || !losses)
        return pcg_fail(h, PCG_ERR_INVALID, "pcg_cmlp_train: max_iter=%lld check_every=%lld lookback=%lld or losses null",
                        (long long)max_iter, (long long)check_every, (long long)lookback);
    if (int rc = cm_validate(h, "pcg_cmlp_train", X, T, p, ldx, lag, hidden, params, lr, lam, lam_ridge)) return rc;
    if (max_iter < check_every)                   // the reference has no model to restore
        return pcg_fail(h, PCG_ERR_DOMAIN, "pcg_cmlp_train: no check runs (max_iter=%lld < check_every=%lld)",
                        (long long)max_iter, (long long)check_every);
    CmRun r;
    if (int rc = cm_setup(h, "pcg_cmlp_train", X, T, p, ldx, lag, hidden, params, lr, lam, lam_ridge, true, r)) return rc;
    const size_t pbytes = (size_t)p * r.s.pstride * 4;
    int64_t checks = 0, best = -1, last = max_iter - 1;
    double best_loss = std::numeric_limits<double>::infinity();
    bool have_fwd = false;                        // the forward pass of the current parameters is on the stream
    for (int64_t it = 0; it < max_iter; ++it) {
        if (!have_fwd)
            if (int rc = cm_forward(h, r)) return rc;
        if (int rc = cm_backward(h, r)) return rc;
        have_fwd = false;
        if ((it + 1) % check_every != 0) continue;
        if (int rc = cm_forward(h, r)) return rc;
        have_fwd = true;
        if (int rc = cm_losses(h, r)) return rc;
        double mean_loss = 0.0;
        PCG_HIP(h, hipMemcpyAsync(&mean_loss, r.total, 8, hipMemcpyDeviceToHost, h->stream));
        PCG_HIP(h, hipStreamSynchronize(h->stream));
        losses[checks++] = mean_loss;
        if (mean_loss < best_loss) {
            best_loss = mean_loss;
            best = it;
            PCG_HIP(h, hipMemcpyAsync(r.best, params, pbytes, hipMemcpyDeviceToDevice, h->stream));
        } else if (best < 0) {
            if (n_checks) *n_checks = checks;
            return pcg_fail(h, PCG_ERR_DOMAIN, "pcg_cmlp_train: the first check's loss is not finite (%g)", mean_loss);
        } else if (it - best == lookback * check_every) {
            last = it;
            break;
        }
    }
    PCG_HIP(h, hipMemcpyAsync(params, r.best, pbytes, hipMemcpyDeviceToDevice, h->stream));
    PCG_HIP(h, hipStreamSynchronize(h->stream));
    if (n_checks) *n_checks = checks;
    if (best_it) *best_it = best;
    if (last_it) *last_it = last;
    return PCG_OK;
}
