// dense_dev.h — the block-wide reductions and the two small dense factorisations shared by the side
// engines (granger.hip, lingam.hip, pcmci.hip, fges.hip), and numpy's pairwise summation order
// (chisq.hip, scaler.hip). Device code only; NT is the block size.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

__device__ inline double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum over the block's NT threads; every thread gets the total. red: NT / 64 doubles of LDS
template <int NT>
__device__ inline double block_sum(double v, double *red) {
    v = wave_sum(v);
    if (NT == 64) return v;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < NT / 64; ++w) s += red[w];
    __syncthreads();
    return s;
}

// sum of K per-thread values over the block; every thread gets the same totals. red: K * NT / 64
template <int NT, int K>
__device__ inline void block_sum(double (&v)[K], double *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) red[k * (NT / 64) + wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
        for (int w = 0; w < NT / 64; ++w) s += red[k * (NT / 64) + w];
        v[k] = s;
    }
    __syncthreads();
}

// min and max over the block; every thread gets both. red: 2 * NT / 64
template <int NT>
__device__ inline void block_minmax(double &lo, double &hi, double *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 32; o > 0; o >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, o, 64));
        hi = fmax(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) {
        red[wave] = lo;
        red[NT / 64 + wave] = hi;
    }
    __syncthreads();
    for (int w = 0; w < NT / 64; ++w) {
        lo = fmin(lo, red[w]);
        hi = fmax(hi, red[NT / 64 + w]);
    }
    __syncthreads();
}

// Class of a column from each thread's min and max over its finite values and bad = 1.0 where it
// met a non-finite one: 2 non-finite, 1 constant, 0 neither (block-uniform). red: 3 * NT / 64, not
// read again here, so there is no barrier behind the last read
template <int NT>
__device__ inline int column_class(double lo, double hi, double bad, double *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 32; o > 0; o >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, o, 64));
        hi = fmax(hi, __shfl_xor(hi, o, 64));
        bad = fmax(bad, __shfl_xor(bad, o, 64));
    }
    if (lane == 0) {
        red[wave * 3] = lo;
        red[wave * 3 + 1] = hi;
        red[wave * 3 + 2] = bad;
    }
    __syncthreads();
    for (int w = 0; w < NT / 64; ++w) {
        lo = fmin(lo, red[w * 3]);
        hi = fmax(hi, red[w * 3 + 1]);
        bad = fmax(bad, red[w * 3 + 2]);
    }
    return bad > 0.0 ? 2 : (lo == hi ? 1 : 0);
}

// numpy's pairwise_sum over at(0) .. at(n - 1), one thread: leaves of <= 128 elements (8
// accumulators), halves rounded down to a multiple of 8 — post-order over an explicit stack
// (thread-local). at(i) is element i: a pointer read, or a strided / transformed one
template <class At>
__device__ inline double np_pairwise_leaf(At at, int64_t s, int64_t n) {
#pragma clang fp contract(off)      // at() may end in a product: it is rounded before it is added
    if (n < 8) {
        double res = 0.0;
        for (int64_t i = 0; i < n; ++i) res += at(s + i);
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = at(s + j);
    int64_t i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += at(s + i + j);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += at(s + i);
    return res;
}

template <class At>
__device__ inline double np_pairwise_sum_at(At at, int64_t n) {
    struct Frame { int64_t s, n; int state; double left; };
    Frame st[64];
    int sp = 1;
    st[0] = {0, n, 0, 0.0};
    double result = 0.0;      // value of the frame that finished last
    while (sp) {
        Frame &f = st[sp - 1];
        if (f.n <= 128) {
            result = np_pairwise_leaf(at, f.s, f.n);
            --sp;
            continue;
        }
        int64_t n2 = f.n / 2;
        n2 -= n2 % 8;
        if (f.state == 0) {
            f.state = 1;
            st[sp++] = {f.s, n2, 0, 0.0};
        } else if (f.state == 1) {
            f.left = result;
            f.state = 2;
            st[sp++] = {f.s + n2, f.n - n2, 0, 0.0};
        } else {
            result = f.left + result;
            --sp;
        }
    }
    return result;
}

__device__ inline double np_pairwise_sum(const double *a, int64_t n) {
    return np_pairwise_sum_at([a](int64_t i) { return a[i]; }, n);
}

// numpy's sum of n contiguous doubles: the reduction runs in buffer-sized blocks of 8192 elements,
// pairwise inside a block, the blocks accumulated in order onto 0.0
template <class At>
__device__ inline double np_sum_at(At at, int64_t n) {
    double v = 0.0;
    for (int64_t b0 = 0; b0 < n; b0 += 8192)
        v += np_pairwise_sum_at([=](int64_t i) { return at(b0 + i); }, n - b0 < 8192 ? n - b0 : (int64_t)8192);
    return v;
}

// Gather the lower triangle of R[cols, cols] (m x m, unit diagonal; R has leading dimension ldr)
// into A (row stride LD) and eliminate its first d columns (right-looking Cholesky). On return
// rows >= d hold, in columns < d, their rows of the factor, and in columns >= d the Schur
// complement given cols[0..d). False (block-uniform) when a pivot is below tau. Starts with a
// barrier: A and cols may have just been written / read.
template <int NT, int LD>
__device__ bool chol_eliminate(const double *R, int64_t ldr, const int *cols, int m, int d, double *A, double tau) {
    const int tid = threadIdx.x;
    __syncthreads();
    for (int idx = tid; idx < m * m; idx += NT) {
        const int r = idx / m, c = idx % m;
        if (c <= r) A[r * LD + c] = r == c ? 1.0 : R[(int64_t)cols[r] * ldr + cols[c]];
    }
    bool ok = true;
    for (int k = 0; k < d; ++k) {
        __syncthreads();
        const double piv = A[k * LD + k];
        if (!(piv >= tau)) {                   // block-uniform
            ok = false;
            break;
        }
        const double lkk = sqrt(piv), ik = 1.0 / lkk;
        __syncthreads();                       // everyone has read the pivot
        for (int r = k + 1 + tid; r < m; r += NT) A[r * LD + k] *= ik;
        if (tid == 0) A[k * LD + k] = lkk;
        __syncthreads();
        const int w = m - k - 1;
        for (int idx = tid; idx < w * w; idx += NT) {
            const int r = k + 1 + idx / w, c = k + 1 + idx % w;
            if (c <= r) A[r * LD + c] -= A[r * LD + k] * A[c * LD + k];
        }
    }
    __syncthreads();
    return ok;
}

// Householder QR steps over the columns k_lo..k_hi-1 of the column-major m x T design Aw, applied
// to every later column, with block-wide reductions (red: NT / 64). rdone reflectors were applied
// before; returns the count after. A column whose remaining norm is below the rank tolerance tol
// (lstsq's max(T, m) eps) is skipped, which gives the minimum-norm least-squares residual. Each
// thread owns the rows r = tid, tid + NT, .. for the whole factorisation, so no thread ever reads
// a row another thread wrote.
template <int NT>
__device__ inline int64_t qr_eliminate(double *Aw, int64_t T, int m, int k_lo, int k_hi, int64_t rdone, double tol,
                                       double *red) {
    const int tid = threadIdx.x;
    for (int k = k_lo; k < k_hi; ++k) {
        const double *ak = Aw + (int64_t)k * T;
        double n0 = 0.0, n1 = 0.0;
        for (int64_t r = tid; r < T; r += NT)
            if (r >= rdone) {
                const double v = ak[r];
                n0 = fma(v, v, n0);
                if (r == rdone) n1 = v;
            }
        n0 = block_sum<NT>(n0, red);
        n1 = block_sum<NT>(n1, red);
        if (!(n0 > tol * tol * (double)T)) continue;               // block-uniform: dependent column
        const double alpha = -copysign(sqrt(n0), n1), vr = n1 - alpha, vn2 = 2.0 * (n0 - n1 * alpha);
        for (int u = k + 1; u < m; ++u) {
            double *au = Aw + (int64_t)u * T;
            double dot = 0.0;
            for (int64_t r = tid; r < T; r += NT)
                if (r >= rdone) dot = fma(r == rdone ? vr : ak[r], au[r], dot);
            const double f = 2.0 * block_sum<NT>(dot, red) / vn2;
            for (int64_t r = tid; r < T; r += NT)
                if (r >= rdone) au[r] -= f * (r == rdone ? vr : ak[r]);
        }
        ++rdone;
    }
    return rdone;
}
