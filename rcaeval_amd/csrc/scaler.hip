// scaler.hip — per-column scalers of a normal window and the largest scaled value of the anomalous
// window, batched over columns and cases (baro = robust_scaler, nsigma).
//
// Replaces the loop of RCAEval/e2e/__init__.py:83-170: per metric column one sklearn fit on the
// normal rows a (RobustScaler: median and 25-75 inter-quartile range; StandardScaler: mean and
// standard deviation), transform of the anomalous rows b, score = max. The arithmetic is restated
// operation for operation (include/pcgpu.h has the formulas; tests/baro_ref.py pins them to
// sklearn), under contract(off) so no product is fused into the sum behind it: center, scale and
// score are bit for bit the reference's.
//
// Layout: the input is row-major (N x n, row stride lda), so a column is strided. The robust
// kernels give one 256-thread block a tile of SC_TC = 8 adjacent columns and read it row by row:
// 8 lanes take the 64 contiguous bytes of a row, a wave takes 8 rows. The order statistics are
// exact, selected on order-preserving uint64 keys (sign bit flipped for non-negatives, all bits
// for negatives):
//   k_sc_sort    N <= SC_LDS_ROWS: the tile's key columns are sorted in LDS (bitonic, padded to a
//                power of two P with the largest key). A column starts at c * (P + 4) words, so the
//                4 rows x 8 columns a half-wave stores fall into 64 distinct banks. The dynamic LDS
//                is 64 (P + 4) bytes: 128 KiB at P = 2048 (one block per CU of 160 KiB), four
//                blocks per CU at the P = 512 of an RQ2 case.
//   k_sc_select  longer columns: 8-bit MSB radix select over the column in global memory (L2), all
//                six ranks of all 8 columns in the same 8 passes; 256-bin histograms in LDS, one
//                per (column, rank), ranks whose prefixes still agree sharing one.
// k_sc_standard runs one thread per column (adjacent lanes read adjacent columns, so coalesced)
// with numpy's summation order (dense_dev.h: pairwise inside blocks of 8192), which a block-wide reduction would not keep.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <vector>

#include "dense_dev.h"
#include "handle.h"

#pragma clang fp contract(off)

namespace {

constexpr int SC_BLOCK = 256;
constexpr int SC_TC = 8;                       // adjacent columns per tile
constexpr int SC_RPP = SC_BLOCK / SC_TC;       // rows per pass of the block
constexpr int SC_LDS_ROWS = 2048;              // largest N of the in-LDS sort
constexpr int SC_PAD = 4;                      // words between the key columns (bank spread)
constexpr int SC_RANKS = 6;                    // q25 lo / hi, median lo / hi, q75 lo / hi
constexpr int SC_HSTRIDE = 257;                // histogram stride: the 48 scans hit distinct banks
constexpr int SC_STD_BLOCK = 64;               // standard mode: columns per block, one thread each
constexpr int64_t SC_MAX_ROWS = INT32_MAX;     // the radix select counts in 32 bits
constexpr uint64_t SC_MSB = 0x8000000000000000ull;

struct ScTile {
    int32_t cas, c0;                           // case index, first column of the tile
};

struct ScOut {
    double *center, *scale, *score;
    int32_t *status;
};

__device__ inline uint64_t sc_key(double x) {
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | SC_MSB);
}

__device__ inline double sc_val(uint64_t k) {
    return __longlong_as_double((long long)((k >> 63) ? (k ^ SC_MSB) : ~k));
}

__device__ inline bool sc_finite(double x) {
    return (((uint64_t)__double_as_longlong(x) >> 52) & 0x7ff) != 0x7ff;
}

// The ranks of the six order statistics (rk[0..1] q25 lo / hi, rk[2..3] the median's, rk[4..5] q75
// lo / hi) and the two interpolation fractions: numpy's virtual index of method "linear"
__device__ inline void sc_ranks(int64_t N, int64_t *rk, double *t) {
    const double ps[2] = {0.25, 0.75};
    for (int q = 0; q < 2; ++q) {
        const double p = ps[q];
        const double v = (double)N * p + (1.0 + p * (1.0 - 1.0 - 1.0)) - 1.0;
        const double fl = floor(v);
        const int64_t lo = (int64_t)fl;
        t[q] = v - fl;
        rk[q * 4] = lo;
        rk[q * 4 + 1] = lo + 1 < N - 1 ? lo + 1 : N - 1;
    }
    rk[2] = (N - 1) / 2;
    rk[3] = N / 2;
}

// center and scale of the robust scaler from the six order statistics s (in sc_ranks' order)
__device__ inline void sc_robust(const double *s, const double *t, int64_t N, double &mid, double &scale) {
    mid = (N & 1) ? s[2] : (s[2] + s[3]) / 2.0;
    double q[2];
    for (int k = 0; k < 2; ++k) {
        const double lo = s[k * 4], hi = s[k * 4 + 1], d = hi - lo;
        q[k] = t[k] < 0.5 ? lo + d * t[k] : hi - d * (1.0 - t[k]);
    }
    scale = q[1] - q[0];
    if (scale < 10.0 * DBL_EPSILON) scale = 1.0;
}

// The tile's scores and its four outputs, from the centers / scales in shc / shs. bad[c] != 0: a
// non-finite value was met in column c of A. Every thread of the block calls it
__device__ inline void sc_score(const pcg_scaler_case_t &cs, int c0, const double *shc, const double *shs, int *bad,
                                double *red, const ScOut &out) {
    const int tid = threadIdx.x, c = tid % SC_TC;
    const int64_t col = (int64_t)c0 + c;
    double m = -HUGE_VAL;
    if (col < cs.n) {
        const double ce = shc[c], sc = shs[c];
        for (int64_t r = tid / SC_TC; r < cs.M; r += SC_RPP) {
            const double b = cs.B[r * cs.ldb + col];
            if (!sc_finite(b)) bad[c] = 1;
            const double z = (b - ce) / sc;
            m = z > m ? z : m;
        }
    }
    red[tid] = m;
    __syncthreads();
    if (tid < SC_TC && col < cs.n) {
        double best = red[tid];
        for (int k = 1; k < SC_RPP; ++k) {
            const double v = red[tid + k * SC_TC];
            best = v > best ? v : best;
        }
        const int64_t slot = cs.out_off + col;
        out.center[slot] = shc[c];
        out.scale[slot] = shs[c];
        out.score[slot] = best;
        // a center or scale that overflowed on finite input makes z NaN, and the reference's max then
        // depends on the row order: such a column is flagged like a non-finite one
        out.status[slot] = (bad[c] || !sc_finite(shc[c]) || !sc_finite(shs[c])) ? 1 : 0;
    }
}

__global__ __launch_bounds__(SC_BLOCK) void k_sc_sort(const pcg_scaler_case_t *cases, const ScTile *tiles, ScOut out) {
    extern __shared__ uint64_t keys[];
    __shared__ double shc[SC_TC], shs[SC_TC], red[SC_BLOCK];
    __shared__ int bad[SC_TC];
    const ScTile tl = tiles[blockIdx.x];
    const pcg_scaler_case_t cs = cases[tl.cas];
    const int tid = threadIdx.x, N = (int)cs.N;
    int P = 1, lg = 0;                           // P = 2^lg >= N
    while (P < N) {
        P <<= 1;
        ++lg;
    }
    const int ld = P + SC_PAD;
    if (tid < SC_TC) bad[tid] = 0;
    __syncthreads();
    for (int idx = tid; idx < P * SC_TC; idx += SC_BLOCK) {
        const int r = idx / SC_TC, c = idx % SC_TC;
        uint64_t k = ~0ull;                      // padding sorts behind every finite value
        if (r < N && (int64_t)tl.c0 + c < cs.n) {
            const double x = cs.A[(int64_t)r * cs.lda + tl.c0 + c];
            if (!sc_finite(x)) bad[c] = 1;
            k = sc_key(x);
        }
        keys[c * ld + r] = k;
    }
    __syncthreads();
    // bitonic sort of every column, ascending: P / 2 compare-exchanges per column and step
    const int half = P >> 1;
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int idx = tid; idx < half * SC_TC; idx += SC_BLOCK) {
                const int c = idx >> (lg - 1), i = idx & (half - 1);
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                uint64_t *colk = keys + c * ld;
                const uint64_t a = colk[lo], b = colk[hi];
                if ((a > b) == ((lo & k) == 0)) {
                    colk[lo] = b;
                    colk[hi] = a;
                }
            }
            __syncthreads();
        }
    if (tid < SC_TC && (int64_t)tl.c0 + tid < cs.n) {
        int64_t rk[SC_RANKS];
        double t[2], s[SC_RANKS];
        sc_ranks(cs.N, rk, t);
        for (int k = 0; k < SC_RANKS; ++k) s[k] = sc_val(keys[tid * ld + (int)rk[k]]);
        sc_robust(s, t, cs.N, shc[tid], shs[tid]);
    }
    __syncthreads();
    sc_score(cs, tl.c0, shc, shs, bad, red, out);
}

__global__ __launch_bounds__(SC_BLOCK) void k_sc_select(const pcg_scaler_case_t *cases, const ScTile *tiles, ScOut out) {
    __shared__ unsigned int hist[SC_TC * SC_RANKS * SC_HSTRIDE];
    __shared__ uint64_t prefix[SC_TC][SC_RANKS];     // the key bits above the current digit
    __shared__ unsigned int rem[SC_TC][SC_RANKS];    // the rank among the keys with that prefix
    __shared__ int lead[SC_TC][SC_RANKS];            // the first rank with the same prefix: its histogram serves both
    __shared__ double shc[SC_TC], shs[SC_TC], red[SC_BLOCK];
    __shared__ int bad[SC_TC];
    const ScTile tl = tiles[blockIdx.x];
    const pcg_scaler_case_t cs = cases[tl.cas];
    const int tid = threadIdx.x, c = tid % SC_TC;
    const int64_t col = (int64_t)tl.c0 + c;
    const bool live = col < cs.n;
    const int sc_c = tid / SC_RANKS, sc_k = tid % SC_RANKS;       // the (column, rank) a scanning thread owns
    const bool scans = tid < SC_TC * SC_RANKS && (int64_t)tl.c0 + sc_c < cs.n;
    if (tid < SC_TC) bad[tid] = 0;
    if (tid < SC_TC * SC_RANKS) {
        int64_t rk[SC_RANKS];
        double t[2];
        sc_ranks(cs.N, rk, t);
        prefix[sc_c][sc_k] = 0;
        rem[sc_c][sc_k] = (unsigned int)rk[sc_k];
        lead[sc_c][sc_k] = 0;
    }
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int e = tid; e < SC_TC * SC_RANKS * SC_HSTRIDE; e += SC_BLOCK) hist[e] = 0;
        __syncthreads();
        if (live) {
            uint64_t lp[SC_RANKS];
            bool act[SC_RANKS];
#pragma unroll
            for (int k = 0; k < SC_RANKS; ++k) {
                lp[k] = prefix[c][k];
                act[k] = lead[c][k] == k;
            }
            for (int64_t r = tid / SC_TC; r < cs.N; r += SC_RPP) {
                const double x = cs.A[r * cs.lda + col];
                if (shift == 56 && !sc_finite(x)) bad[c] = 1;
                const uint64_t key = sc_key(x);
                const uint64_t above = shift == 56 ? 0 : key >> (shift + 8);
                const unsigned int d = (unsigned int)(key >> shift) & 255u;
#pragma unroll
                for (int k = 0; k < SC_RANKS; ++k)
                    if (act[k] && above == lp[k]) atomicAdd(&hist[(c * SC_RANKS + k) * SC_HSTRIDE + d], 1u);
            }
        }
        __syncthreads();
        if (scans) {                               // the digit holding this rank
            const unsigned int *hh = hist + (sc_c * SC_RANKS + lead[sc_c][sc_k]) * SC_HSTRIDE;
            const unsigned int want = rem[sc_c][sc_k];
            unsigned int cum = 0;
            int d = 0;
            for (; d < 255; ++d) {
                const unsigned int n_d = hh[d];
                if (want < cum + n_d) break;
                cum += n_d;
            }
            rem[sc_c][sc_k] = want - cum;
            prefix[sc_c][sc_k] = (prefix[sc_c][sc_k] << 8) | (uint64_t)d;
        }
        __syncthreads();
        if (scans) {
            int l = sc_k;
            for (int j = sc_k - 1; j >= 0; --j)
                if (prefix[sc_c][j] == prefix[sc_c][sc_k]) l = j;
            lead[sc_c][sc_k] = l;
        }
        __syncthreads();
    }
    if (tid < SC_TC && (int64_t)tl.c0 + tid < cs.n) {
        int64_t rk[SC_RANKS];
        double t[2], s[SC_RANKS];
        sc_ranks(cs.N, rk, t);
        for (int k = 0; k < SC_RANKS; ++k) s[k] = sc_val(prefix[tid][k]);
        sc_robust(s, t, cs.N, shc[tid], shs[tid]);
    }
    __syncthreads();
    sc_score(cs, tl.c0, shc, shs, bad, red, out);
}

__global__ __launch_bounds__(SC_STD_BLOCK) void k_sc_standard(const pcg_scaler_case_t *cases, const ScTile *tiles,
                                                              ScOut out) {
    const ScTile tl = tiles[blockIdx.x];
    const pcg_scaler_case_t cs = cases[tl.cas];
    const int64_t col = (int64_t)tl.c0 + threadIdx.x;
    if (col >= cs.n) return;
    const double *a = cs.A + col;
    const int64_t lda = cs.lda;
    const double cnt = (double)cs.N;
    int bad = 0;
    const double S = np_sum_at([&](int64_t i) {
        const double x = a[i * lda];
        bad |= !sc_finite(x);
        return x;
    }, cs.N);
    const double mean = S / cnt;
    const double corr = np_sum_at([=](int64_t i) { return a[i * lda] - mean; }, cs.N);
    double u = np_sum_at([=](int64_t i) {
        const double tmp = a[i * lda] - mean;
        return tmp * tmp;
    }, cs.N);
    u = u - corr * corr / cnt;
    const double var = u / cnt;
    double scale = sqrt(var);
    // sklearn's _is_constant_feature: the variance is within the two-pass algorithm's error bound
    const double nme = cnt * mean * DBL_EPSILON;
    if (var <= cnt * DBL_EPSILON * var + nme * nme) scale = 1.0;
    // Python's max: the first z, replaced by a later one that compares greater (a variance that
    // overflowed makes z NaN on finite input, and the reference's answer then depends on this)
    double m = 0.0;
    for (int64_t r = 0; r < cs.M; ++r) {
        const double b = cs.B[r * cs.ldb + col];
        bad |= !sc_finite(b);
        const double z = (b - mean) / scale;
        m = (r == 0 || z > m) ? z : m;
    }
    const int64_t slot = cs.out_off + col;
    out.center[slot] = mean;
    out.scale[slot] = scale;
    out.score[slot] = m;
    out.status[slot] = bad;
}

}  // namespace

extern "C" int pcg_scaler_abi_info(int64_t *case_bytes) {
    if (case_bytes) *case_bytes = (int64_t)sizeof(pcg_scaler_case_t);
    return PCG_OK;
}

extern "C" int pcg_scaler_limits(int64_t *lds_rows) {
    if (lds_rows) *lds_rows = SC_LDS_ROWS;
    return PCG_OK;
}

extern "C" int pcg_scaler_batch(pcg_handle *h, const pcg_scaler_case_t *cases, int64_t count, int mode, double *center,
                                double *scale, double *score, int32_t *status) {
    if (!h) return PCG_ERR_INVALID;
    if (count < 0 || count > INT32_MAX || (mode != 0 && mode != 1))
        return pcg_fail(h, PCG_ERR_INVALID, "pcg_scaler_batch: bad count or mode (count=%lld mode=%d)", (long long)count, mode);
    if (count == 0) return PCG_OK;
    if (!cases) return pcg_fail(h, PCG_ERR_INVALID, "pcg_scaler_batch: null pointer");
    // tiles of the three kernels: [0] in-LDS sort, [1] radix select, [2] standard
    std::vector<ScTile> tiles[3];
    int p_max = 1;
    for (int64_t i = 0; i < count; ++i) {
        const pcg_scaler_case_t &c = cases[i];
        if (c.N < 1 || c.M < 1 || c.N > SC_MAX_ROWS || c.M > SC_MAX_ROWS || c.n < 0 || c.n > INT32_MAX || c.lda < c.n ||
            c.ldb < c.n || c.out_off < 0)
            return pcg_fail(h, PCG_ERR_INVALID,
                            "pcg_scaler_batch: case %lld: bad shape (N=%lld M=%lld n=%lld lda=%lld ldb=%lld out_off=%lld: "
                            "1 <= N, M <= %lld, lda, ldb >= n)",
                            (long long)i, (long long)c.N, (long long)c.M, (long long)c.n, (long long)c.lda,
                            (long long)c.ldb, (long long)c.out_off, (long long)SC_MAX_ROWS);
        if (c.n == 0) continue;
        if (!c.A || !c.B) return pcg_fail(h, PCG_ERR_INVALID, "pcg_scaler_batch: case %lld: null pointer", (long long)i);
        const int kind = mode == 1 ? 2 : (c.N <= SC_LDS_ROWS ? 0 : 1);
        const int width = mode == 1 ? SC_STD_BLOCK : SC_TC;
        for (int64_t c0 = 0; c0 < c.n; c0 += width) tiles[kind].push_back({(int32_t)i, (int32_t)c0});
        if (kind == 0)
            while (p_max < c.N) p_max <<= 1;
    }
    const size_t n_tiles = tiles[0].size() + tiles[1].size() + tiles[2].size();
    if (n_tiles == 0) return PCG_OK;
    if (n_tiles > (size_t)INT32_MAX) return pcg_fail(h, PCG_ERR_INVALID, "pcg_scaler_batch: too many column tiles");
    if (!center || !scale || !score || !status) return pcg_fail(h, PCG_ERR_INVALID, "pcg_scaler_batch: null pointer");
    PCG_HIP(h, hipSetDevice(h->device));
    Carve cv;
    const size_t o_cases = cv.take((size_t)count * sizeof(pcg_scaler_case_t));
    size_t o_tiles[3];
    for (int k = 0; k < 3; ++k) o_tiles[k] = cv.take(tiles[k].size() * sizeof(ScTile));
    if (!pcg_ensure(h, h->scaler_up, cv.total))
        return pcg_fail(h, PCG_ERR_OOM, "pcg_scaler_batch: scratch (%lld B)", (long long)cv.total);
    std::vector<char> up(cv.total, 0);
    memcpy(up.data() + o_cases, cases, (size_t)count * sizeof(pcg_scaler_case_t));
    for (int k = 0; k < 3; ++k)
        if (!tiles[k].empty()) memcpy(up.data() + o_tiles[k], tiles[k].data(), tiles[k].size() * sizeof(ScTile));
    char *dev = (char *)h->scaler_up.p;
    // a few KB from pageable memory: copied before the call goes on, so no error path below can
    // leave a transfer reading `up` behind (the previous call's kernels ended with its stream sync)
    PCG_HIP(h, hipMemcpy(dev, up.data(), cv.total, hipMemcpyHostToDevice));
    const pcg_scaler_case_t *dcases = (const pcg_scaler_case_t *)(dev + o_cases);
    const ScOut out{center, scale, score, status};
    if (!tiles[0].empty()) {
        const size_t lds = (size_t)SC_TC * (size_t)(p_max + SC_PAD) * sizeof(uint64_t);
        if (!h->scaler_lds_set) {                  // once per handle, for the largest P
            const size_t lds_max = (size_t)SC_TC * (size_t)(SC_LDS_ROWS + SC_PAD) * sizeof(uint64_t);
            PCG_HIP(h, hipFuncSetAttribute((const void *)k_sc_sort, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
            h->scaler_lds_set = true;
        }
        hipLaunchKernelGGL(k_sc_sort, dim3((unsigned)tiles[0].size()), dim3(SC_BLOCK), lds, h->stream, dcases,
                           (const ScTile *)(dev + o_tiles[0]), out);
        PCG_HIP(h, hipGetLastError());
    }
    if (!tiles[1].empty()) {
        hipLaunchKernelGGL(k_sc_select, dim3((unsigned)tiles[1].size()), dim3(SC_BLOCK), 0, h->stream, dcases,
                           (const ScTile *)(dev + o_tiles[1]), out);
        PCG_HIP(h, hipGetLastError());
    }
    if (!tiles[2].empty()) {
        hipLaunchKernelGGL(k_sc_standard, dim3((unsigned)tiles[2].size()), dim3(SC_STD_BLOCK), 0, h->stream, dcases,
                           (const ScTile *)(dev + o_tiles[2]), out);
        PCG_HIP(h, hipGetLastError());
    }
    PCG_HIP(h, hipStreamSynchronize(h->stream));
    return PCG_OK;
}

extern "C" int pcg_scaler_case(pcg_handle *h, const double *A, int64_t lda, const double *B, int64_t ldb, int64_t N,
                               int64_t M, int64_t n, int64_t out_off, int mode, double *center, double *scale,
                               double *score, int32_t *status) {
    const pcg_scaler_case_t c{A, B, N, M, n, lda, ldb, out_off};
    return pcg_scaler_batch(h, &c, 1, mode, center, scale, score, status);
}
