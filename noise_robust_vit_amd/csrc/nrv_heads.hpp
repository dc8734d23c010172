// Helpers of the kernels that own all heads of a materialised [B, H, Nq, Nk] matrix at once (gfx950): talking heads
// (nrv_talking_heads.hip) and re-attention (nrv_reattn.hip).  A workgroup of TH_THREADS threads holds H rows of np positions in
// LDS (row stride th_ld(np)); the H x H matrices are read with wave-uniform indices (scalar loads).
#pragma once
#include "nrv_common.hpp"

namespace {

constexpr int TH_MAXH = 16, TH_MAXNK = 1025, TH_THREADS = 256, TH_TILE = 512, TH_PARTS = 1024;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// LDS row stride of an image with np positions per head: a multiple of 4 (16-byte reads) that is not a multiple of 64 banks
__host__ __device__ __forceinline__ int th_ld(int np) {
    const int l = ((np + 3) & ~3) + 4;
    return (l & 63) ? l : l + 4;
}

template <int V>
__device__ __forceinline__ void ldv(const float* p, float (&v)[V]) {
    if constexpr (V == 4) {
        const f32x4_t t = *reinterpret_cast<const f32x4_t*>(p);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
        v[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void stv(float* p, const float (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<f32x4_t*>(p) = f32x4_t{v[0], v[1], v[2], v[3]};
    else *p = v[0];
}
template <int V>
__device__ __forceinline__ void stv(bf16_t* p, const float (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<u32x2_t*>(p) = u32x2_t{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
    else *p = f32_to_bf16(v[0]);
}

// s[h][0 .. np) = g[h * hstride + 0 .. np) for h < H; positions np .. round-up-to-4 are zeroed (V == 4 has none)
template <int V>
__device__ __forceinline__ void th_load(float* __restrict__ s, int ld, const float* __restrict__ g, long long hstride, int H, int np) {
    const int q = (np + 3) >> 2;                               // 4-position groups per head
    if constexpr (V == 4) {
        for (int idx = threadIdx.x; idx < H * q; idx += TH_THREADS) {
            const int h = idx / q, c = idx - h * q;
            *reinterpret_cast<f32x4_t*>(s + h * ld + 4 * c) = *reinterpret_cast<const f32x4_t*>(g + h * hstride + 4 * c);
        }
    } else {
        const int n4 = 4 * q;
        for (int idx = threadIdx.x; idx < H * n4; idx += TH_THREADS) {
            const int h = idx / n4, p = idx - h * n4;
            s[h * ld + p] = p < np ? g[h * hstride + p] : 0.f;
        }
    }
}

// out[o] = sum_i M(o, i) x[i] at every position of an LDS image x[H][np]; M(o, i) = W[i * H + o] (TR = false: the forward mixing
// out[g] = sum_h W[h, g] x[h]) or W[o * H + i] (TR = true: its transpose, the gradient).  `seen(i, p, x_i)` gets every input
// and `put(o, p, out_o)` every result of V consecutive positions; a thread reads its positions before it writes any of them, so
// `put` may overwrite the image.
template <int V, bool TR, class Seen, class Put>
__device__ __forceinline__ void th_mix(const float* s, int ld, const float* __restrict__ W, int H, int np, Seen seen, Put put) {
    for (int p = threadIdx.x * V; p < np; p += TH_THREADS * V) {
        float x[TH_MAXH][V];
#pragma unroll
        for (int i = 0; i < TH_MAXH; ++i)
            if (i < H) {
                ldv<V>(s + i * ld + p, x[i]);
                seen(i, p, x[i]);
            }
        for (int o = 0; o < H; ++o) {
            float acc[V];
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = 0.f;
#pragma unroll
            for (int i = 0; i < TH_MAXH; ++i)
                if (i < H) {
                    const float w = TR ? W[o * H + i] : W[i * H + o];
#pragma unroll
                    for (int v = 0; v < V; ++v) acc[v] = fmaf(w, x[i][v], acc[v]);
                }
            put(o, p, acc);
        }
    }
}

// thread t = split * H*H + h * H + g: sum_p x[h][p] y[g][p] over the 4-position groups split, split + nsplit, ... of one image
// (four fp32 chains of at most 257 terms); the caller adds the images' sums in double, so that a gradient summed over 10^7
// elements keeps fp32 accuracy
__device__ __forceinline__ float th_pairs(const float* x, const float* y, int ld, int H, int np) {
    const int pairs = H * H, nsplit = TH_THREADS / pairs;
    const int split = threadIdx.x / pairs, pair = threadIdx.x - split * pairs;
    if (split >= nsplit) return 0.f;
    const float* xr = x + (pair / H) * ld;
    const float* yr = y + (pair % H) * ld;
    const int n4 = (np + 3) & ~3;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    for (int p = 4 * split; p < n4; p += 4 * nsplit) {
        const f32x4_t a = *reinterpret_cast<const f32x4_t*>(xr + p), b = *reinterpret_cast<const f32x4_t*>(yr + p);
        acc[0] = fmaf(a[0], b[0], acc[0]); acc[1] = fmaf(a[1], b[1], acc[1]);
        acc[2] = fmaf(a[2], b[2], acc[2]); acc[3] = fmaf(a[3], b[3], acc[3]);
    }
    return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

// the workgroup's H*H sums from its threads' split sums, in split order; red: TH_THREADS doubles of LDS
__device__ __forceinline__ void th_pairs_out(double* red, double acc, int H, double* __restrict__ out) {
    const int pairs = H * H, nsplit = TH_THREADS / pairs;
    __syncthreads();
    red[threadIdx.x] = acc;
    __syncthreads();
    if ((int)threadIdx.x < pairs) {
        double s = 0.0;
        for (int k = 0; k < nsplit; ++k) s += red[k * pairs + threadIdx.x];
        out[threadIdx.x] = s;
    }
}

extern __shared__ __attribute__((aligned(16))) float th_smem[];

// out[k] = sum over the parts, in part order; k < n0 goes to out0, the rest to out1
__global__ void th_reduce_kernel(const double* __restrict__ part, int nparts, int n, int n0, float* __restrict__ out0,
                                 float* __restrict__ out1) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    double s = 0.0;
#pragma unroll 8
    for (int q = 0; q < nparts; ++q) s += part[(long long)q * n + k];
    if (k < n0) out0[k] = (float)s;
    else out1[k - n0] = (float)s;
}

bool th_shape_ok(int B, int H, int Nq, int Nk) {
    return B >= 1 && H >= 1 && H <= TH_MAXH && Nq >= 1 && Nk >= 1 && Nk <= TH_MAXNK && (long long)B * Nq <= 0x7fffffffll &&
           (long long)B * H * Nq * Nk < (1ll << 40);
}

int th_parts(long long work) { return (int)(work < TH_PARTS ? work : TH_PARTS); }

template <class K>
int th_lds_attr(K kernel, size_t bytes) {
    return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

constexpr size_t TH_LDS_MAX = ((size_t)2 * TH_MAXH * (((TH_MAXNK + 3) & ~3) + 8) + 2 * TH_THREADS) * 4;      // 134 KB of the CU's 160

}  // namespace
