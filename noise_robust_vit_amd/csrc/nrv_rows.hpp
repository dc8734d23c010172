// Row helpers shared by the kernels that keep one bf16 row per thread in fp32 registers (biased, window and class attention,
// the PatchConvNet and batch-norm elementwise kernels): bf16 row <-> fp32 registers, Hardswish, the fixed-order 256-thread
// LDS tree, the kernel that sums the partials of a table gradient, and the host's grid size.  The MFMA fragment helpers of the
// ViT attention kernels live in nrv_attn_common.hpp.  Everything here has internal linkage: nothing is an exported symbol.
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

// workgroups for `items` work items at `block` per workgroup, at most `cap` (the grid-stride loops take the rest), at least 1
inline int grid_for(long long items, int block, int cap) {
    const long long g = (items + block - 1) / block;
    return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

}  // namespace
