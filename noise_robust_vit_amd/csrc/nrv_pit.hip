// PiT kernels (gfx950): the Pool layer's depthwise convolution, Conv2d(C, 2C, 3, stride 2, padding 1, groups = C, bias), on
// token-major rows of the fp32 residual stream with lead class rows in front of every sample's plane (pit.py:90-117).  Output
// channel o reads input channel o / 2.  Memory-bound: a lane owns 4 input channels (one 16-byte fp32 access) and their 8
// output channels (one 16-byte bf16 access); the arithmetic is fp32 in registers with one bf16 rounding on the forward's store.
// Nothing is staged in LDS: every input is read by 2.25 windows on average, the windows that share it sit in neighbouring
// lanes of the same or the next workgroup, and a stride-2 tile of T x T outputs would stage (2T + 1)^2 inputs to save those
// re-reads from the caches.  Every sum runs in a fixed order (no atomics): reruns are bit-identical; the per-sample
// partials of dw / dbias are added by tap_wred_kernel (nrv_rows.hpp).  Grids are exact (one work item per thread, no capped
// grid-stride loop).
#include "nrv_rows.hpp"

namespace {

// the 72 taps [8, 9] of the 8 output channels of input channels c .. c + 3: consecutive floats, 288 bytes from a 16-byte
// aligned base
__device__ __forceinline__ void pool_taps(const float* __restrict__ w, int c, float (&wr)[72]) {
    const f32x4_t* wp = reinterpret_cast<const f32x4_t*>(w + (long long)c * 18);
#pragma unroll
    for (int i = 0; i < 18; ++i) {
        const f32x4_t v = wp[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) wr[4 * i + e] = v[e];
    }
}

// one thread = (output token, 4 input channels): acc[j] = bias[o] + sum_t w[o, t] x(2 oy - 1 + ky, 2 ox - 1 + kx, o / 2),
// o = 2c + j, t = 3 ky + kx ascending; taps outside the plane are skipped
__global__ __launch_bounds__(256) void pool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                       bf16_t* __restrict__ out, long long items, int H, int W, int Ho, int Wo, int lead,
                                                       int C) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int c4 = C >> 2;
    const long long tok = i / c4;
    const int c = (int)(i - tok * c4) * 4;
    const long long b = tok / ((long long)Ho * Wo);
    const int rem = (int)(tok - b * Ho * Wo);
    const int oy = rem / Wo, ox = rem - oy * Wo;
    const float* xb = x + (b * (lead + (long long)H * W) + lead) * C + c;
    float wr[72], acc[8];
    pool_taps(w, c, wr);
    const f32x4_t b0 = *reinterpret_cast<const f32x4_t*>(bias + 2 * c), b1 = *reinterpret_cast<const f32x4_t*>(bias + 2 * c + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { acc[j] = b0[j]; acc[4 + j] = b1[j]; }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy - 1 + ky;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox - 1 + kx;
            if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
            const f32x4_t xv = *reinterpret_cast<const f32x4_t*>(xb + ((long long)iy * W + ix) * C);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = fmaf(wr[j * 9 + ky * 3 + kx], xv[j >> 1], acc[j]);
        }
    }
    store_row(out + tok * 2 * C + 2 * c, acc);
}

// one thread = (row of dx, 4 input channels).  Input (y, x) is tap (ky, kx) of window (oy, ox) when 2 oy - 1 + ky = y and
// 2 ox - 1 + kx = x: at most two ky and two kx.  ky, then kx, then o = 2c, 2c + 1 ascending.  Class rows are zeros.
__global__ __launch_bounds__(256) void pool_dx_kernel(const float* __restrict__ w, const bf16_t* __restrict__ dout, float* __restrict__ dx,
                                                      long long items, int H, int W, int Ho, int Wo, int lead, int C) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int c4 = C >> 2, N = lead + H * W;
    const long long row = i / c4;
    const int c = (int)(i - row * c4) * 4;
    const long long b = row / N;
    const int t = (int)(row - b * N) - lead;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    if (t >= 0) {
        const int y = t / W, xx = t - y * W;
        float wr[72];
        pool_taps(w, c, wr);
        const bf16_t* db = dout + b * Ho * Wo * 2 * C + 2 * c;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int ny = y + 1 - ky;
            if (ny < 0 || (ny & 1) || (ny >> 1) >= Ho) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int nx = xx + 1 - kx;
                if (nx < 0 || (nx & 1) || (nx >> 1) >= Wo) continue;
                float g[8];
                load_row(db + ((long long)(ny >> 1) * Wo + (nx >> 1)) * 2 * C, g);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j >> 1] = fmaf(wr[j * 9 + ky * 3 + kx], g[j], acc[j >> 1]);
            }
        }
    }
    *reinterpret_cast<f32x4_t*>(dx + row * C + c) = acc;
}

// per-sample partials: part[(b*10 + t) * 2C + o] = sum over the output tokens in row-major order of dout(b, p, o) times
// x(tap t of p, o / 2) for t < 9, of dout(b, p, o) for t = 9 (the bias).  One thread = one partial; o is the fastest index,
// so a wave reads 64 consecutive bf16 of dout and 32 consecutive floats of x.
__global__ __launch_bounds__(256) void pool_dw_kernel(const float* __restrict__ x, const bf16_t* __restrict__ dout, float* __restrict__ part,
                                                      long long items, int H, int W, int Ho, int Wo, int lead, int C) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int C2 = 2 * C;
    const int o = (int)(i % C2);
    const long long r = i / C2;
    const int t = (int)(r % 10);
    const long long b = r / 10;
    const int ky = t / 3, kx = t - ky * 3;
    const float* xb = x + (b * (lead + (long long)H * W) + lead) * C + (o >> 1);
    const bf16_t* db = dout + b * Ho * Wo * C2 + o;
    float acc = 0.f;
    for (int oy = 0; oy < Ho; ++oy) {
        const int iy = 2 * oy - 1 + ky;
        if (t < 9 && (iy < 0 || iy >= H)) continue;
        for (int ox = 0; ox < Wo; ++ox) {
            const float g = bf16_to_f32(db[((long long)oy * Wo + ox) * C2]);
            if (t == 9) { acc += g; continue; }
            const int ix = 2 * ox - 1 + kx;
            if (ix < 0 || ix >= W) continue;
            acc = fmaf(g, xb[((long long)iy * W + ix) * C], acc);
        }
    }
    part[i] = acc;
}

bool pool_shape_ok(int B, int H, int W, int lead, int C) {
    if (!(B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W <= (1ll << 24) && (lead == 0 || lead == 1) && C > 0 && C % 8 == 0 &&
          C <= (1 << 20)))
        return false;
    const long long rows = (long long)B * (lead + (long long)H * W);
    return rows * C <= (1ll << 40) && nrv_cdiv(rows * (C / 4), 256) <= NRV_MAX_BLOCKS && nrv_cdiv((long long)B * 20 * C, 256) <= NRV_MAX_BLOCKS;
}

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" int nrv_pool_dwconv_fwd(const float* x_f32, const float* w, const float* bias, void* out_bf16, int B, int H, int W, int lead,
                                   int C, void* stream) {
    if (!pool_shape_ok(B, H, W, lead, C)) return NRV_ERR_SHAPE;
    if (!x_f32 || !w || !bias || !out_bf16) return NRV_ERR_NULL;
    if (!nrv_aligned16(x_f32) || !nrv_aligned16(w) || !nrv_aligned16(bias) || !nrv_aligned16(out_bf16)) return NRV_ERR_ALIGN;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long long items = (long long)B * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(pool_fwd_kernel, dim3((unsigned)nrv_cdiv(items, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x_f32, w, bias,
                       static_cast<bf16_t*>(out_bf16), items, H, W, Ho, Wo, lead, C);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t nrv_pool_dwconv_bwd_workspace(int B, int H, int W, int C) {
    if (!pool_shape_ok(B, H, W, 0, C)) return 0;
    return (size_t)B * 20 * C * 4;
}

extern "C" int nrv_pool_dwconv_bwd(const float* x_f32, const float* w, const void* dout_bf16, float* dx_f32, float* dw, float* dbias,
                                   void* workspace, size_t workspace_bytes, int B, int H, int W, int lead, int C, void* stream) {
    if (!pool_shape_ok(B, H, W, lead, C)) return NRV_ERR_SHAPE;
    if (!x_f32 || !w || !dout_bf16 || !dx_f32 || !dw || !dbias || !workspace) return NRV_ERR_NULL;
    if (workspace_bytes < nrv_pool_dwconv_bwd_workspace(B, H, W, C)) return NRV_ERR_WORKSPACE;
    if (!nrv_aligned16(x_f32) || !nrv_aligned16(w) || !nrv_aligned16(dout_bf16) || !nrv_aligned16(dx_f32) || !nrv_aligned16(workspace))
        return NRV_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const bf16_t* dout = static_cast<const bf16_t*>(dout_bf16);
    float* part = static_cast<float*>(workspace);
    const long long rows = (long long)B * (lead + (long long)H * W), items = rows * (C / 4);
    hipLaunchKernelGGL(pool_dx_kernel, dim3((unsigned)nrv_cdiv(items, 256)), dim3(256), 0, st, w, dout, dx_f32, items, H, W, Ho, Wo, lead, C);
    NRV_CHECK_LAUNCH();
    const long long parts = (long long)B * 20 * C;
    hipLaunchKernelGGL(pool_dw_kernel, dim3((unsigned)nrv_cdiv(parts, 256)), dim3(256), 0, st, x_f32, dout, part, parts, H, W, Ho, Wo, lead, C);
    NRV_CHECK_LAUNCH();
    // dw [2C, 9] and dbias [2C] = the per-sample partials summed over the samples in index order
    hipLaunchKernelGGL(tap_wred_kernel<256>, dim3((unsigned)nrv_cdiv(20ll * C, 256)), dim3(256), 0, st, part, dw, dbias, B, 2 * C, 9);
    NRV_CHECK_LAUNCH();
    return 0;
}
