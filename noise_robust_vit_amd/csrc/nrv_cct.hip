// CCT kernels (gfx950): what the Compact Convolutional Transformer (cct.py) needs beside the encoder's GEMMs and attention.
//   * ReLU + MaxPool2d fused on the NHWC token rows a convolution's GEMM wrote, with the argmax tap kept for the backward, and
//     the backward in gather form (cct.py:182-191);
//   * LayerNorm whose OUTPUT is the fp32 residual stream (the post-norm `src = norm1(src)`, cct.py:139): fp32 in, fp32 out,
//     and a backward that takes an fp32 gradient;
//   * sequence pooling, softmax_n(y a + bias) . y (cct.py:286-288), forward and backward.
// All of it is memory-bound: 16-byte accesses, fp32 arithmetic in registers, every sum in a fixed order (no atomics), so reruns
// are bit-identical: the per-workgroup partials of dgamma / dbeta and the per-sample partials of the pooling's da / dbias are
// added by reduce_rows_kernel (nrv_rows.hpp).  Grids are exact (one work item per thread, wave or workgroup; no capped
// grid-stride loop).
#include "nrv_rows.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
// ReLU + max pool
// ---------------------------------------------------------------------------------------------
template <bool F32>
__device__ __forceinline__ void load8(const void* base, long long idx, float (&r)[8]) {
    if (F32) {
        const f32x4_t a = *reinterpret_cast<const f32x4_t*>(reinterpret_cast<const float*>(base) + idx);
        const f32x4_t b = *reinterpret_cast<const f32x4_t*>(reinterpret_cast<const float*>(base) + idx + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { r[e] = a[e]; r[4 + e] = b[e]; }
    } else {
        load_row(reinterpret_cast<const bf16_t*>(base) + idx, r);
    }
}

// one thread = (output token, 8 channels).  best = the first maximum among the in-bounds taps, ky then kx ascending (a later
// tap replaces it only when strictly larger); with relu a maximum <= 0 stores 0 and the mark 255.  Values are copied.
template <bool F32>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const void* __restrict__ y, float* __restrict__ out_f32, bf16_t* __restrict__ out_bf16,
                                                          unsigned char* __restrict__ idx, long long items, int H, int W, int Ho, int Wo,
                                                          int C, int pk, int ps, int pp, int relu) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int c8 = C >> 3;
    const long long tok = i / c8;
    const int c = (int)(i - tok * c8) * 8;
    const long long b = tok / ((long long)Ho * Wo);
    const int rem = (int)(tok - b * Ho * Wo);
    const int oy = rem / Wo, ox = rem - oy * Wo;
    const long long base = b * H * W;
    float best[8];
    unsigned tap[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { best[j] = 0.f; tap[j] = 0u; }
    bool first = true;
    for (int ky = 0; ky < pk; ++ky) {
        const int iy = oy * ps - pp + ky;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < pk; ++kx) {
            const int ix = ox * ps - pp + kx;
            if (ix < 0 || ix >= W) continue;
            float v[8];
            load8<F32>(y, (base + (long long)iy * W + ix) * C + c, v);
            const unsigned t = (unsigned)(ky * pk + kx);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (first || v[j] > best[j]) { best[j] = v[j]; tap[j] = t; }
            }
            first = false;
        }
    }
    if (relu) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (!(best[j] > 0.f)) { best[j] = 0.f; tap[j] = 255u; }
    }
    const long long o = tok * C + c;
    if (out_f32 != nullptr) {
        *reinterpret_cast<f32x4_t*>(out_f32 + o) = f32x4_t{best[0], best[1], best[2], best[3]};
        *reinterpret_cast<f32x4_t*>(out_f32 + o + 4) = f32x4_t{best[4], best[5], best[6], best[7]};
    }
    if (out_bf16 != nullptr) store_row(out_bf16 + o, best);
    u32x2_t pk8;
    pk8[0] = tap[0] | (tap[1] << 8) | (tap[2] << 16) | (tap[3] << 24);
    pk8[1] = tap[4] | (tap[5] << 8) | (tap[6] << 16) | (tap[7] << 24);
    *reinterpret_cast<u32x2_t*>(idx + o) = pk8;
}

// one thread = (input token, 8 channels): input (y, x) is tap (ky, kx) of window (oy, ox) when oy ps - pp + ky = y and
// ox ps - pp + kx = x; the windows are visited oy then ox ascending and add their dout where idx names the tap.
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ dout, const unsigned char* __restrict__ idx,
                                                          bf16_t* __restrict__ dy, long long items, int H, int W, int Ho, int Wo, int C,
                                                          int pk, int ps, int pp) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int c8 = C >> 3;
    const long long tok = i / c8;
    const int c = (int)(i - tok * c8) * 8;
    const long long b = tok / ((long long)H * W);
    const int rem = (int)(tok - b * H * W);
    const int yy = rem / W, xx = rem - yy * W;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    const int ty = yy + pp - pk + 1, tx = xx + pp - pk + 1;
    const int oy0 = ty <= 0 ? 0 : (ty + ps - 1) / ps, ox0 = tx <= 0 ? 0 : (tx + ps - 1) / ps;
    int oy1 = (yy + pp) / ps, ox1 = (xx + pp) / ps;
    if (oy1 > Ho - 1) oy1 = Ho - 1;
    if (ox1 > Wo - 1) ox1 = Wo - 1;
    for (int oy = oy0; oy <= oy1; ++oy) {
        const int ky = yy + pp - oy * ps;
        for (int ox = ox0; ox <= ox1; ++ox) {
            const unsigned t = (unsigned)(ky * pk + (xx + pp - ox * ps));
            const long long o = ((b * Ho + oy) * Wo + ox) * C + c;
            const u32x2_t m = *reinterpret_cast<const u32x2_t*>(idx + o);
            const f32x4_t d0 = *reinterpret_cast<const f32x4_t*>(dout + o), d1 = *reinterpret_cast<const f32x4_t*>(dout + o + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (((m[0] >> (8 * j)) & 255u) == t) acc[j] += d0[j];
                if (((m[1] >> (8 * j)) & 255u) == t) acc[4 + j] += d1[j];
            }
        }
    }
    store_row(dy + tok * C + c, acc);
}

bool maxpool_shape_ok(int B, int H, int W, int C, int pk, int ps, int pp) {
    if (!(pk == 2 || pk == 3) || ps < 1 || ps > pk || pp < 0 || pp > pk / 2) return false;
    if (!(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && C <= (1 << 20) && (long long)H * W <= (1ll << 24))) return false;
    if (H + 2 * pp < pk || W + 2 * pp < pk) return false;
    const long long rows = (long long)B * H * W;
    return rows * C <= (1ll << 40) && nrv_cdiv(rows * (C / 8), 256) <= NRV_MAX_BLOCKS;
}

// ---------------------------------------------------------------------------------------------
// LayerNorm on the fp32 stream: one wave per row, lane l holds the 4-element chunks l, l + 64, ... of its row
// ---------------------------------------------------------------------------------------------
constexpr int LNF_ROWS_PER_WAVE = 8;             // rows one wave of the backward walks, at least (lnf_rpw)

template <int MAXJ>
__global__ __launch_bounds__(256) void lnf_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float* __restrict__ y32, bf16_t* __restrict__ y16,
                                                      float* __restrict__ mean, float* __restrict__ rstd, long long rows, int dim,
                                                      float eps) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float inv_dim = 1.0f / (float)dim;
    f32x4_t v[MAXJ];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        const int c = (lane + 64 * j) * 4;
        if (c < dim) {
            v[j] = *reinterpret_cast<const f32x4_t*>(x + row * dim + c);
            s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
        } else {
            v[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
    }
    const float mu = wave_sum(s) * inv_dim;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        const int c = (lane + 64 * j) * 4;
        if (c < dim) {
            const f32x4_t d = v[j] - mu;
            const f32x4_t d2 = d * d;
            q += (d2[0] + d2[1]) + (d2[2] + d2[3]);
        }
    }
    const float rs = 1.0f / sqrtf(wave_sum(q) * inv_dim + eps);
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        const int c = (lane + 64 * j) * 4;
        if (c < dim) {
            const f32x4_t g = *reinterpret_cast<const f32x4_t*>(gamma + c), b = *reinterpret_cast<const f32x4_t*>(beta + c);
            const f32x4_t o = (v[j] - mu) * rs * g + b;
            *reinterpret_cast<f32x4_t*>(y32 + row * dim + c) = o;
            if (y16 != nullptr)
                *reinterpret_cast<u32x2_t*>(y16 + row * dim + c) = u32x2_t{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
        }
    }
    if (lane == 0) {
        mean[row] = mu;
        rstd[row] = rs;
    }
}

// wave w of the launch walks rows rpw w .. rpw w + rpw - 1 in order: dx = (g - mean(g) - xh mean(g xh)) rstd with g = dy gamma,
// xh = (x - mean) rstd.  Its column partials sum(dy xh) and sum(dy) meet those of the workgroup's other three waves in LDS
// ([4][dim] floats, added in wave order) and go to partial[workgroup][0 / 1][dim].
template <int MAXJ>
__global__ __launch_bounds__(256) void lnf_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                      const float* __restrict__ gamma, const float* __restrict__ mean,
                                                      const float* __restrict__ rstd, float* __restrict__ dx32, bf16_t* __restrict__ dx16,
                                                      float* __restrict__ partial, long long rows, int dim, int rpw) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* red = reinterpret_cast<float*>(smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r0 = ((long long)blockIdx.x * 4 + wave) * rpw;
    const float inv_dim = 1.0f / (float)dim;
    f32x4_t adg[MAXJ], adb[MAXJ];
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        adg[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        adb[j] = adg[j];
    }
    for (int r = 0; r < rpw; ++r) {
        const long long row = r0 + r;
        if (row >= rows) break;
        const float mu = mean[row], rs = rstd[row];
        f32x4_t xh[MAXJ], g[MAXJ];
        float c1 = 0.f, c2 = 0.f;
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) {
            const int c = (lane + 64 * j) * 4;
            if (c < dim) {
                const f32x4_t d = *reinterpret_cast<const f32x4_t*>(dy + row * dim + c);
                xh[j] = (*reinterpret_cast<const f32x4_t*>(x + row * dim + c) - mu) * rs;
                g[j] = d * *reinterpret_cast<const f32x4_t*>(gamma + c);
                const f32x4_t p = g[j] * xh[j];
                c1 += (p[0] + p[1]) + (p[2] + p[3]);
                c2 += (g[j][0] + g[j][1]) + (g[j][2] + g[j][3]);
                adg[j] += d * xh[j];
                adb[j] += d;
            } else {
                xh[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                g[j] = xh[j];
            }
        }
        c1 = wave_sum(c1) * inv_dim;
        c2 = wave_sum(c2) * inv_dim;
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) {
            const int c = (lane + 64 * j) * 4;
            if (c < dim) {
                const f32x4_t d = (g[j] - c2 - xh[j] * c1) * rs;
                *reinterpret_cast<f32x4_t*>(dx32 + row * dim + c) = d;
                if (dx16 != nullptr)
                    *reinterpret_cast<u32x2_t*>(dx16 + row * dim + c) = u32x2_t{pack_bf16x2(d[0], d[1]), pack_bf16x2(d[2], d[3])};
            }
        }
    }
    for (int pass = 0; pass < 2; ++pass) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) {
            const int c = (lane + 64 * j) * 4;
            if (c < dim) *reinterpret_cast<f32x4_t*>(red + wave * dim + c) = pass == 0 ? adg[j] : adb[j];
        }
        __syncthreads();
        for (int c = threadIdx.x * 4; c < dim; c += 1024) {
            f32x4_t s = *reinterpret_cast<const f32x4_t*>(red + c);
#pragma unroll
            for (int k = 1; k < 4; ++k) s += *reinterpret_cast<const f32x4_t*>(red + k * dim + c);
            *reinterpret_cast<f32x4_t*>(partial + ((long long)blockIdx.x * 2 + pass) * dim + c) = s;
        }
    }
}

// rows one wave of the backward walks: 8, or more so that the launch has at most 4096 waves (1024 workgroups: that many
// partial rows of dgamma / dbeta, an int for reduce_rows_kernel)
int lnf_rpw(long long rows) {
    const long long r = nrv_cdiv(rows, 4096);
    return (int)(r < LNF_ROWS_PER_WAVE ? LNF_ROWS_PER_WAVE : (r > 0x7fffffff ? 0x7fffffff : r));
}
int lnf_bwd_blocks(long long rows) { return (int)nrv_cdiv(nrv_cdiv(rows, lnf_rpw(rows)), 4); }

bool lnf_shape_ok(long long rows, int dim) {
    return rows >= 1 && dim >= 8 && dim % 8 == 0 && dim <= 4096 && rows <= (1ll << 40) / dim && nrv_cdiv(rows, 4) <= NRV_MAX_BLOCKS;
}
int lnf_maxj(int dim) {
    const int chunks = (dim / 4 + 63) / 64;
    return chunks <= 1 ? 1 : chunks <= 2 ? 2 : chunks <= 4 ? 4 : chunks <= 8 ? 8 : 16;
}

// ---------------------------------------------------------------------------------------------
// sequence pooling: one workgroup per sample
// ---------------------------------------------------------------------------------------------
constexpr int SP_MAX_N = 4096;

// dot[t] = y_t . v for the sample's n tokens: wave k takes tokens k, k + 4, ...; columns in 4-element chunks over the lanes
__device__ __forceinline__ void seqpool_dots(const float* __restrict__ yb, const float* __restrict__ v, float* dot, int n, int D, float add) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = wave; t < n; t += 4) {
        float s = 0.f;
        for (int c = lane * 4; c < D; c += 256) {
            const f32x4_t a = *reinterpret_cast<const f32x4_t*>(yb + (long long)t * D + c), b = *reinterpret_cast<const f32x4_t*>(v + c);
            s = fmaf(a[0], b[0], s); s = fmaf(a[1], b[1], s); s = fmaf(a[2], b[2], s); s = fmaf(a[3], b[3], s);
        }
        s = wave_sum(s);
        if (lane == 0) dot[t] = s + add;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void seqpool_fwd_kernel(const float* __restrict__ y, const float* __restrict__ a, const float* __restrict__ bias,
                                                          float* __restrict__ w, float* __restrict__ out, int n, int D) {
    __shared__ float sw[SP_MAX_N];
    __shared__ float red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* yb = y + (long long)b * n * D;
    seqpool_dots(yb, a, sw, n, D, bias[0]);
    float m = -INFINITY;
    for (int t = tid; t < n; t += 256) m = fmaxf(m, sw[t]);
    m = block_max_256(m, red);
    float s = 0.f;
    for (int t = tid; t < n; t += 256) {
        const float e = expf(sw[t] - m);
        sw[t] = e;
        s += e;
    }
    s = block_sum_256(s, red);
    for (int t = tid; t < n; t += 256) {
        const float p = sw[t] / s;
        sw[t] = p;
        w[(long long)b * n + t] = p;
    }
    __syncthreads();
    for (int c = tid; c < D; c += 256) {
        float acc = 0.f;
#pragma unroll 4
        for (int t = 0; t < n; ++t) acc = fmaf(sw[t], yb[(long long)t * D + c], acc);
        out[(long long)b * D + c] = acc;
    }
}

// part[b][0 .. D-1] = sum_n dl_n y_n (n ascending), part[B * D + b] = sum_n dl_n
__global__ __launch_bounds__(256) void seqpool_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ y, const float* __restrict__ a,
                                                          const float* __restrict__ w, float* __restrict__ dy, float* __restrict__ part,
                                                          int B, int n, int D) {
    __shared__ float sw[SP_MAX_N];
    __shared__ float sl[SP_MAX_N];
    __shared__ float red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* yb = y + (long long)b * n * D;
    const float* db = dout + (long long)b * D;
    seqpool_dots(yb, db, sl, n, D, 0.f);                                   // t_n
    float s = 0.f;
    for (int t = tid; t < n; t += 256) {
        const float p = w[(long long)b * n + t];
        sw[t] = p;
        s = fmaf(p, sl[t], s);
    }
    s = block_sum_256(s, red);
    float sd = 0.f;
    for (int t = tid; t < n; t += 256) {
        const float dl = sw[t] * (sl[t] - s);
        sl[t] = dl;
        sd += dl;
    }
    sd = block_sum_256(sd, red);                                           // ends with a barrier: sl is complete
    if (tid == 0) part[(long long)B * D + b] = sd;
    for (int c = tid; c < D; c += 256) {
        const float dc = db[c], ac = a[c];
        float acc = 0.f;
#pragma unroll 4
        for (int t = 0; t < n; ++t) {
            const float dl = sl[t];
            const long long o = ((long long)b * n + t) * D + c;
            acc = fmaf(dl, y[o], acc);
            dy[o] = fmaf(dl, ac, sw[t] * dc);
        }
        part[(long long)b * D + c] = acc;
    }
}

bool seqpool_shape_ok(int B, int n, int D) {
    return B >= 1 && B <= (1 << 24) && n >= 1 && n <= SP_MAX_N && D >= 8 && D % 8 == 0 && D <= 4096 && (long long)B * n * D <= (1ll << 40);
}

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" int nrv_relu_maxpool_fwd(const void* y, int y_dtype, int relu, float* out_f32, void* out_bf16, void* idx_u8, int B, int H, int W,
                                    int C, int pk, int ps, int pp, void* stream) {
    if (!maxpool_shape_ok(B, H, W, C, pk, ps, pp)) return NRV_ERR_SHAPE;
    if (!y || !idx_u8 || (!out_f32 && !out_bf16)) return NRV_ERR_NULL;
    if (y_dtype != NRV_F32 && y_dtype != NRV_BF16) return NRV_ERR_DTYPE;
    if (!nrv_aligned16(y) || !nrv_aligned16(out_f32) || !nrv_aligned16(out_bf16) || !nrv_aligned16(idx_u8)) return NRV_ERR_ALIGN;
    const int Ho = (H + 2 * pp - pk) / ps + 1, Wo = (W + 2 * pp - pk) / ps + 1;
    const long long items = (long long)B * Ho * Wo * (C / 8);
    const dim3 grid((unsigned)nrv_cdiv(items, 256));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (y_dtype == NRV_F32)
        hipLaunchKernelGGL(maxpool_fwd_kernel<true>, grid, dim3(256), 0, st, y, out_f32, static_cast<bf16_t*>(out_bf16),
                           static_cast<unsigned char*>(idx_u8), items, H, W, Ho, Wo, C, pk, ps, pp, relu != 0);
    else
        hipLaunchKernelGGL(maxpool_fwd_kernel<false>, grid, dim3(256), 0, st, y, out_f32, static_cast<bf16_t*>(out_bf16),
                           static_cast<unsigned char*>(idx_u8), items, H, W, Ho, Wo, C, pk, ps, pp, relu != 0);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nrv_relu_maxpool_bwd(const float* dout, const void* idx_u8, void* dy_bf16, int B, int H, int W, int C, int pk, int ps, int pp,
                                    void* stream) {
    if (!maxpool_shape_ok(B, H, W, C, pk, ps, pp)) return NRV_ERR_SHAPE;
    if (!dout || !idx_u8 || !dy_bf16) return NRV_ERR_NULL;
    if (!nrv_aligned16(dout) || !nrv_aligned16(idx_u8) || !nrv_aligned16(dy_bf16)) return NRV_ERR_ALIGN;
    const int Ho = (H + 2 * pp - pk) / ps + 1, Wo = (W + 2 * pp - pk) / ps + 1;
    const long long items = (long long)B * H * W * (C / 8);
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3((unsigned)nrv_cdiv(items, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), dout,
                       static_cast<const unsigned char*>(idx_u8), static_cast<bf16_t*>(dy_bf16), items, H, W, Ho, Wo, C, pk, ps, pp);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nrv_layernorm_f32_fwd(const float* x, const float* gamma, const float* beta, float* y_f32, void* y_bf16, float* mean,
                                     float* rstd, int64_t rows, int dim, float eps, void* stream) {
    if (!lnf_shape_ok(rows, dim)) return NRV_ERR_SHAPE;
    if (!x || !gamma || !beta || !y_f32 || !mean || !rstd) return NRV_ERR_NULL;
    if (!nrv_aligned16(x) || !nrv_aligned16(gamma) || !nrv_aligned16(beta) || !nrv_aligned16(y_f32) || !nrv_aligned16(y_bf16))
        return NRV_ERR_ALIGN;
    const dim3 grid((unsigned)nrv_cdiv(rows, 4));
    hipStream_t st = static_cast<hipStream_t>(stream);
    bf16_t* y16 = static_cast<bf16_t*>(y_bf16);
    switch (lnf_maxj(dim)) {
        case 1: hipLaunchKernelGGL(lnf_fwd_kernel<1>, grid, dim3(256), 0, st, x, gamma, beta, y_f32, y16, mean, rstd, rows, dim, eps); break;
        case 2: hipLaunchKernelGGL(lnf_fwd_kernel<2>, grid, dim3(256), 0, st, x, gamma, beta, y_f32, y16, mean, rstd, rows, dim, eps); break;
        case 4: hipLaunchKernelGGL(lnf_fwd_kernel<4>, grid, dim3(256), 0, st, x, gamma, beta, y_f32, y16, mean, rstd, rows, dim, eps); break;
        case 8: hipLaunchKernelGGL(lnf_fwd_kernel<8>, grid, dim3(256), 0, st, x, gamma, beta, y_f32, y16, mean, rstd, rows, dim, eps); break;
        default: hipLaunchKernelGGL(lnf_fwd_kernel<16>, grid, dim3(256), 0, st, x, gamma, beta, y_f32, y16, mean, rstd, rows, dim, eps); break;
    }
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t nrv_layernorm_f32_bwd_workspace(int64_t rows, int dim) {
    if (!lnf_shape_ok(rows, dim)) return 0;
    return (size_t)lnf_bwd_blocks(rows) * 2 * dim * 4;
}

extern "C" int nrv_layernorm_f32_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                                     float* dx_f32, void* dx_bf16, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                                     int64_t rows, int dim, void* stream) {
    if (!lnf_shape_ok(rows, dim)) return NRV_ERR_SHAPE;
    if (!dy || !x || !gamma || !mean || !rstd || !dx_f32 || !dgamma || !dbeta || !workspace) return NRV_ERR_NULL;
    if (workspace_bytes < nrv_layernorm_f32_bwd_workspace(rows, dim)) return NRV_ERR_WORKSPACE;
    if (!nrv_aligned16(dy) || !nrv_aligned16(x) || !nrv_aligned16(gamma) || !nrv_aligned16(dx_f32) || !nrv_aligned16(dx_bf16) ||
        !nrv_aligned16(workspace))
        return NRV_ERR_ALIGN;
    const int rpw = lnf_rpw(rows);
    const int blocks = lnf_bwd_blocks(rows);
    const dim3 grid((unsigned)blocks);
    const size_t lds = (size_t)4 * dim * 4;
    hipStream_t st = static_cast<hipStream_t>(stream);
    bf16_t* dx16 = static_cast<bf16_t*>(dx_bf16);
    float* part = static_cast<float*>(workspace);
    switch (lnf_maxj(dim)) {
        case 1: hipLaunchKernelGGL(lnf_bwd_kernel<1>, grid, dim3(256), lds, st, dy, x, gamma, mean, rstd, dx_f32, dx16, part, rows, dim, rpw); break;
        case 2: hipLaunchKernelGGL(lnf_bwd_kernel<2>, grid, dim3(256), lds, st, dy, x, gamma, mean, rstd, dx_f32, dx16, part, rows, dim, rpw); break;
        case 4: hipLaunchKernelGGL(lnf_bwd_kernel<4>, grid, dim3(256), lds, st, dy, x, gamma, mean, rstd, dx_f32, dx16, part, rows, dim, rpw); break;
        case 8: hipLaunchKernelGGL(lnf_bwd_kernel<8>, grid, dim3(256), lds, st, dy, x, gamma, mean, rstd, dx_f32, dx16, part, rows, dim, rpw); break;
        default: hipLaunchKernelGGL(lnf_bwd_kernel<16>, grid, dim3(256), lds, st, dy, x, gamma, mean, rstd, dx_f32, dx16, part, rows, dim, rpw); break;
    }
    NRV_CHECK_LAUNCH();
    hipLaunchKernelGGL(reduce_rows_kernel<RR_COLS * RR_LANES>, dim3((unsigned)nrv_cdiv(2 * dim, RR_COLS)), dim3(RR_COLS * RR_LANES), 0, st, part,
                       blocks, 2 * dim, dgamma, dbeta, dim, 0.f);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nrv_seqpool_fwd(const float* y, const float* a, const float* bias, float* w, float* out, int B, int n, int D, void* stream) {
    if (!seqpool_shape_ok(B, n, D)) return NRV_ERR_SHAPE;
    if (!y || !a || !bias || !w || !out) return NRV_ERR_NULL;
    if (!nrv_aligned16(y) || !nrv_aligned16(a)) return NRV_ERR_ALIGN;
    hipLaunchKernelGGL(seqpool_fwd_kernel, dim3((unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream), y, a, bias, w, out, n, D);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t nrv_seqpool_bwd_workspace(int B, int D) {
    if (!seqpool_shape_ok(B, 1, D)) return 0;
    return ((size_t)B * D + B) * 4;
}

extern "C" int nrv_seqpool_bwd(const float* dout, const float* y, const float* a, const float* w, float* dy, float* da, float* dbias,
                               void* workspace, size_t workspace_bytes, int B, int n, int D, void* stream) {
    if (!seqpool_shape_ok(B, n, D)) return NRV_ERR_SHAPE;
    if (!dout || !y || !a || !w || !dy || !da || !dbias || !workspace) return NRV_ERR_NULL;
    if (workspace_bytes < nrv_seqpool_bwd_workspace(B, D)) return NRV_ERR_WORKSPACE;
    if (!nrv_aligned16(dout) || !nrv_aligned16(y)) return NRV_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(seqpool_bwd_kernel, dim3((unsigned)B), dim3(256), 0, st, dout, y, a, w, dy, part, B, n, D);
    NRV_CHECK_LAUNCH();
    // da[c] = sum_b part[b][c], dbias = sum_b part[B * D + b]: lane r of 64 adds samples r, r + 64, ..., then the lanes in order
    hipLaunchKernelGGL(reduce_rows_kernel<RR_COLS * RR_LANES>, dim3((unsigned)nrv_cdiv(D, RR_COLS)), dim3(RR_COLS * RR_LANES), 0, st, part, B, D, da,
                       da, D, 0.f);
    NRV_CHECK_LAUNCH();
    hipLaunchKernelGGL(reduce_rows_kernel<RR_COLS * RR_LANES>, dim3(1), dim3(RR_COLS * RR_LANES), 0, st, part + (long long)B * D, B, 1, dbias, dbias,
                       1, 0.f);
    NRV_CHECK_LAUNCH();
    return 0;
}
