// Row helpers shared by the kernels that keep one bf16 row per thread in fp32 registers (biased, window and class attention,
// the PatchConvNet and batch-norm elementwise kernels): bf16 row <-> fp32 registers, Hardswish, the fixed-order 256-thread
// LDS tree, the kernel that sums the partials of a table gradient, the three fixed-order reducers of partial rows that finish
// every deterministic gradient, and the host's grid size.  The MFMA fragment helpers of the ViT attention kernels live in
// nrv_attn_common.hpp.  Everything here has internal linkage: nothing is an exported symbol.
#pragma once
#include "nrv_common.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
// N consecutive bf16 (global or LDS) <-> fp32 registers: 16-byte accesses for N % 8 == 0, one 8-byte access for N == 4
// ---------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void load_row(const bf16_t* src, float (&r)[N], bool ok = true) {
    static_assert(N == 4 || N % 8 == 0, "a row is 4 or a multiple of 8 elements");
    if constexpr (N == 4) {
        const u32x2_t v = ok ? *reinterpret_cast<const u32x2_t*>(src) : u32x2_t{0u, 0u};
        r[0] = bf16lo_to_f32(v[0]); r[1] = bf16hi_to_f32(v[0]); r[2] = bf16lo_to_f32(v[1]); r[3] = bf16hi_to_f32(v[1]);
    } else {
#pragma unroll
        for (int c = 0; c < N / 8; ++c) {
            const u32x4_t v = ok ? *reinterpret_cast<const u32x4_t*>(src + c * 8) : u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                r[c * 8 + 2 * e] = bf16lo_to_f32(v[e]);
                r[c * 8 + 2 * e + 1] = bf16hi_to_f32(v[e]);
            }
        }
    }
}

// sum_d a[d] * row[d], d ascending
template <int N>
__device__ __forceinline__ float dot_row(const float (&a)[N], const bf16_t* row) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < N / 8; ++c) {
        const u32x4_t v = *reinterpret_cast<const u32x4_t*>(row + c * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc = fmaf(a[c * 8 + 2 * e], bf16lo_to_f32(v[e]), acc);
            acc = fmaf(a[c * 8 + 2 * e + 1], bf16hi_to_f32(v[e]), acc);
        }
    }
    return acc;
}

// acc += w * row
template <int N>
__device__ __forceinline__ void axpy_row(float w, const bf16_t* row, float (&acc)[N]) {
#pragma unroll
    for (int c = 0; c < N / 8; ++c) {
        const u32x4_t v = *reinterpret_cast<const u32x4_t*>(row + c * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[c * 8 + 2 * e] = fmaf(w, bf16lo_to_f32(v[e]), acc[c * 8 + 2 * e]);
            acc[c * 8 + 2 * e + 1] = fmaf(w, bf16hi_to_f32(v[e]), acc[c * 8 + 2 * e + 1]);
        }
    }
}

// dst = bf16(r * mul), packed
template <int N>
__device__ __forceinline__ void store_row(bf16_t* dst, const float (&r)[N], float mul = 1.f) {
    static_assert(N == 4 || N % 8 == 0, "a row is 4 or a multiple of 8 elements");
    if constexpr (N == 4) {
        *reinterpret_cast<u32x2_t*>(dst) = u32x2_t{pack_bf16x2(r[0] * mul, r[1] * mul), pack_bf16x2(r[2] * mul, r[3] * mul)};
    } else {
#pragma unroll
        for (int c = 0; c < N / 8; ++c) {
            u32x4_t v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = pack_bf16x2(r[c * 8 + 2 * e] * mul, r[c * 8 + 2 * e + 1] * mul);
            *reinterpret_cast<u32x4_t*>(dst + c * 8) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Hardswish (levit.py:229-232) and torch's hardswish_backward boundaries: 0 below -3, x / 3 + 1/2 on [-3, 3], 1 above
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float hardswish(float x) { return x * fminf(fmaxf(x + 3.f, 0.f), 6.f) / 6.f; }
__device__ __forceinline__ float hardswish_grad(float x) { return x < -3.f ? 0.f : (x <= 3.f ? x / 3.f + 0.5f : 1.f); }

// ---------------------------------------------------------------------------------------------
// fixed-order reductions over a workgroup of 256 threads: a tree in LDS (buf: 256 floats), the result in every thread
// ---------------------------------------------------------------------------------------------
template <bool MAX>
__device__ __forceinline__ float block_reduce_256(float v, float* buf) {
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            if (MAX) buf[threadIdx.x] = fmaxf(buf[threadIdx.x], buf[threadIdx.x + o]);
            else buf[threadIdx.x] += buf[threadIdx.x + o];
        }
        __syncthreads();
    }
    const float r = buf[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ float block_max_256(float v, float* buf) { return block_reduce_256<true>(v, buf); }
__device__ __forceinline__ float block_sum_256(float v, float* buf) { return block_reduce_256<false>(v, buf); }

// The partials of one table-gradient entry, summed in a fixed order: workgroup (x, y) owns entry e = y * gridDim.x + x, whose n
// partials are part[e * n .. e * n + n - 1]; thread k adds partials k, k + 256, ... in order, then the tree; one store to
// out[x * sx + y * sy].  No atomics: reruns are bit-identical.  A template so that only the translation units that launch it
// get a copy (THREADS is always 256, the width of the tree).
template <int THREADS>
__global__ __launch_bounds__(THREADS) void reduce_partials_kernel(const float* __restrict__ part, float* __restrict__ out, int n,
                                                                  long long sx, long long sy) {
    static_assert(THREADS == 256, "block_sum_256 is a 256-thread tree");
    __shared__ float red[256];
    const float* src = part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * n;
    float acc = 0.f;
    for (int c = threadIdx.x; c < n; c += 256) acc += src[c];
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) out[blockIdx.x * sx + blockIdx.y * sy] = acc;
}

// ---------------------------------------------------------------------------------------------
// The second step of every deterministic gradient: P fp32 partial rows [P, ncols], written by a first kernel, added in one fixed
// order.  All three are templates for the reason above (THREADS is the workgroup size, fixed per kernel).  The stores share one
// form: column c goes to out0[c] below `split` and to out1[c - split] from it on, as beta * old + sum when beta != 0.
// ---------------------------------------------------------------------------------------------
// out[c] = beta * out[c] + sum_p partial[p][c]  (fixed summation order; tests/norm_ref.py::reduce_rows emulates it)
// 16 columns x 64 row-lanes per workgroup: lane r adds rows r, r + 64, ... in order, then lane 0 adds the 64 lane sums in order.
// With ~1000 partial rows and ~1500 columns this gives ~100 workgroups and 16 loads per thread (a 64-column x 16-lane layout
// left the kernel on 24 CUs with 64 dependent loads per thread: 20 us).  Grid: cdiv(ncols, RR_COLS).
constexpr int RR_COLS = 16, RR_LANES = 64;
template <int THREADS>
__global__ __launch_bounds__(THREADS) void reduce_rows_kernel(const float* __restrict__ partial, int P, int ncols,
                                                              float* __restrict__ out0, float* __restrict__ out1,
                                                              int split_col, float beta) {
    static_assert(THREADS == RR_COLS * RR_LANES, "16 columns x 64 row lanes");
    __shared__ float red[RR_LANES][RR_COLS + 1];
    const int cl = threadIdx.x % RR_COLS, rl = threadIdx.x / RR_COLS;
    const int c = blockIdx.x * RR_COLS + cl;
    float s = 0.f;
    if (c < ncols)
        for (int p = rl; p < P; p += RR_LANES) s += partial[(long long)p * ncols + c];
    red[rl][cl] = s;
    __syncthreads();
    if (rl == 0 && c < ncols) {
        float t = 0.f;
#pragma unroll 8
        for (int k = 0; k < RR_LANES; ++k) t += red[k][cl];
        float* dst = c < split_col ? out0 + c : out1 + (c - split_col);
        *dst = beta != 0.f ? beta * (*dst) + t : t;
    }
}

// The serial form, for few partial rows: one thread per column adds its P partials p = 0 .. P - 1 in index order.
// Grid: cdiv(ncols, 256), exact.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void sum_rows_kernel(const float* __restrict__ part, int P, int ncols, float* __restrict__ out0,
                                                           float* __restrict__ out1, int split, float beta) {
    const long long c = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (c >= ncols) return;
    float v = 0.f;
    for (int p = 0; p < P; ++p) v += part[(long long)p * ncols + c];
    float* dst = c < split ? out0 + c : out1 + (c - split);
    *dst = beta != 0.f ? beta * (*dst) + v : v;
}

// Tap gradients of a depthwise convolution: per-sample partials [B][KK + 1][C] (tap t < KK, the bias at t = KK; c fastest), one
// thread per (t, c) adds the samples b = 0 .. B - 1 in index order; dw [C, KK] and dbias [C].  Grid: cdiv((KK + 1) C, 256), exact.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void tap_wred_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                           float* __restrict__ dbias, int B, int C, int KK) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    const long long n = (long long)(KK + 1) * C;
    if (i >= n) return;
    float v = 0.f;
    for (int b = 0; b < B; ++b) v += part[b * n + i];
    const int t = (int)(i / C), c = (int)(i - (long long)t * C);
    if (t < KK) dw[(long long)c * KK + t] = v;
    else dbias[c] = v;
}

// workgroups for `items` work items at `block` per workgroup, at most `cap` (the grid-stride loops take the rest), at least 1
inline int grid_for(long long items, int block, int cap) {
    const long long g = (items + block - 1) / block;
    return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

}  // namespace
