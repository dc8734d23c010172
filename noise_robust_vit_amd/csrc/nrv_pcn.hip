// PatchConvNet kernels (gfx950): depthwise 3x3 convolution with GELU and the squeeze as a by-product, squeeze-and-excitation,
// LayerScale residuals with row-mode drop path, the GELU' multiply of the stem, and class attention (one query per sample).
// Token-major rows [B*H*W, C] throughout: row b*H*W + y*W + x is the reference's x.transpose(-1, -2).reshape(B, C, H, W)
// (patch_convnet.py:239-243).  Every reduction runs in a fixed order (no atomics): reruns are bit-identical.  The 4- and 8-element
// bf16 <-> fp32 row accesses (load_row / store_row) and the 256-thread LDS tree (block_sum_256 / block_max_256) are those of
// nrv_rows.hpp.
#include "nrv_rows.hpp"

namespace {

constexpr int PCN_GRID_CAP = 65535 * 8;     // workgroups of the grid-stride elementwise kernels, at most

// gelu' of element (m, n) from a saved stream: bf16 [rows, ld], or the 8-bit stream of NRV_EPI_BIAS_GELU_Q8 stored in row pairs,
// byte (m, n) at (m >> 1) * 2 ld + (n >> 6) * 128 + (m & 1) * 64 + (n & 63) (include/nrv.h).  Four columns n .. n + 3, n % 4 == 0.
__device__ __forceinline__ void dgelu4(const void* g, int dtype, long long m, int n, int ld, float (&out)[4]) {
    if (dtype == NRV_BF16) {
        load_row(static_cast<const bf16_t*>(g) + m * ld + n, out);
        return;
    }
    const unsigned char* q = static_cast<const unsigned char*>(g) + (m >> 1) * 2 * (long long)ld + (n >> 6) * 128 + (m & 1) * 64 + (n & 63);
    const unsigned d = *reinterpret_cast<const unsigned*>(q);
    constexpr float c = 1.0f / 202.0f, z = -26.0f / 202.0f;       // the NRV_EPI_DGELU_Q8 decode
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = fmaf((float)((d >> (8 * j)) & 0xffu), c, z);
}

// ---------------------------------------------------------------------------------------------
// depthwise 3x3 (zero padding), one workgroup per (64-channel block, sample): 16 lanes x 4 channels per row, 16 rows in flight.
// The per-(sample, channel) sums are reduced over the 16 row groups in order.
// ---------------------------------------------------------------------------------------------
constexpr int DW_CB = 64, DW_RG = 16;

__device__ __forceinline__ void dw_taps(const bf16_t* __restrict__ a, long long row0, int y, int x, int H, int W, int C, int c0,
                                        float (&tap)[9][4]) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
            load_row(a + (row0 + yy * W + xx) * C + c0, tap[t]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) tap[t][j] = 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void dw_fwd_kernel(const bf16_t* __restrict__ a, const float* __restrict__ w, const float* __restrict__ bias,
                                                     bf16_t* __restrict__ d, float* __restrict__ sq, int H, int W, int C) {
    __shared__ float red[DW_RG][DW_CB];
    const int b = blockIdx.y, lc = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int c0 = blockIdx.x * DW_CB + lc * 4;
    const bool cok = c0 < C;
    const int HW = H * W;
    const long long row0 = (long long)b * HW;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (cok) {
        float wr[4][9], bs[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bs[j] = bias[c0 + j];
#pragma unroll
            for (int t = 0; t < 9; ++t) wr[j][t] = w[(c0 + j) * 9 + t];
        }
        for (int p = rg; p < HW; p += DW_RG) {
            const int y = p / W, x = p - y * W;
            float tap[9][4];
            dw_taps(a, row0, y, x, H, W, C, c0, tap);
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float u = bs[j];
#pragma unroll
                for (int t = 0; t < 9; ++t) u = fmaf(wr[j][t], tap[t][j], u);
                o[j] = gelu_fwd(u);
                acc[j] += o[j];
            }
            store_row(d + (row0 + p) * C + c0, o);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) red[rg][lc * 4 + j] = acc[j];
    __syncthreads();
    if (threadIdx.x < DW_CB && blockIdx.x * DW_CB + (int)threadIdx.x < C) {
        float s = 0.f;
        for (int r = 0; r < DW_RG; ++r) s += red[r][threadIdx.x];
        sq[(long long)b * C + blockIdx.x * DW_CB + threadIdx.x] = s;
    }
}

// backward, pass 1: dd = (dg s[b] + dmean[b] / HW) gelu'(pre), pre recomputed from a; fp32 dd to the workspace; per-(sample,
// channel) partials of dW (9 taps) and db, reduced over the row groups in order: part[(b * 10 + t) * C + c], db at t = 9.
__global__ __launch_bounds__(256) void dw_bwd_dd_kernel(const bf16_t* __restrict__ a, const float* __restrict__ w, const float* __restrict__ bias,
                                                        const bf16_t* __restrict__ dg, const float* __restrict__ s, const float* __restrict__ dmean,
                                                        float inv_hw, float* __restrict__ dd, float* __restrict__ part, int H, int W, int C) {
    __shared__ float red[DW_RG][DW_CB];
    const int b = blockIdx.y, lc = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int c0 = blockIdx.x * DW_CB + lc * 4;
    const bool cok = c0 < C;
    const int HW = H * W;
    const long long row0 = (long long)b * HW;
    float adw[10][4];
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) adw[t][j] = 0.f;
    if (cok) {
        float wr[4][9], bs[4], sc[4], dm[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bs[j] = bias[c0 + j];
            sc[j] = s[(long long)b * C + c0 + j];
            dm[j] = dmean[(long long)b * C + c0 + j] * inv_hw;
#pragma unroll
            for (int t = 0; t < 9; ++t) wr[j][t] = w[(c0 + j) * 9 + t];
        }
        for (int p = rg; p < HW; p += DW_RG) {
            const int y = p / W, x = p - y * W;
            float tap[9][4], g[4];
            dw_taps(a, row0, y, x, H, W, C, c0, tap);
            load_row(dg + (row0 + p) * C + c0, g);
            f32x4_t o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float u = bs[j];
#pragma unroll
                for (int t = 0; t < 9; ++t) u = fmaf(wr[j][t], tap[t][j], u);
                const float v = fmaf(g[j], sc[j], dm[j]) * gelu_grad(u);
                o[j] = v;
#pragma unroll
                for (int t = 0; t < 9; ++t) adw[t][j] = fmaf(v, tap[t][j], adw[t][j]);
                adw[9][j] += v;
            }
            *reinterpret_cast<f32x4_t*>(dd + (row0 + p) * C + c0) = o;
        }
    }
#pragma unroll
    for (int t = 0; t < 10; ++t) {
#pragma unroll
        for (int j = 0; j < 4; ++j) red[rg][lc * 4 + j] = adw[t][j];
        __syncthreads();
        if (threadIdx.x < DW_CB && blockIdx.x * DW_CB + (int)threadIdx.x < C) {
            float v = 0.f;
            for (int r = 0; r < DW_RG; ++r) v += red[r][threadIdx.x];
            part[((long long)b * 10 + t) * C + blockIdx.x * DW_CB + threadIdx.x] = v;
        }
        __syncthreads();
    }
}

// backward, pass 2: da(p) = sum_t w[t] dd(p - off_t) in tap order, times the 1x1 conv's gelu' when a stream is given
__global__ __launch_bounds__(256) void dw_bwd_da_kernel(const float* __restrict__ dd, const float* __restrict__ w, const void* __restrict__ gs,
                                                        int gdtype, bf16_t* __restrict__ da, long long n4, int H, int W, int C) {
    const int C4 = C >> 2, HW = H * W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / C4;
        const int c0 = (int)(i - r * C4) * 4;
        const long long b = r / HW;
        const int p = (int)(r - b * HW), y = p / W, x = p - y * W;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = y - (t / 3 - 1), xx = x - (t % 3 - 1);     // the output this input reached through tap t
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                const f32x4_t v = *reinterpret_cast<const f32x4_t*>(dd + (b * HW + yy * W + xx) * C + c0);
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = fmaf(w[(c0 + j) * 9 + t], v[j], o[j]);
            }
        }
        if (gs) {
            float g[4];
            dgelu4(gs, gdtype, r, c0, C, g);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] *= g[j];
        }
        store_row(da + r * C + c0, o);
    }
}

// backward, pass 3: dW [C, 9] and db [C] = the per-sample partials summed over the batch in order (tap_wred_kernel, nrv_rows.hpp)

// ---------------------------------------------------------------------------------------------
// squeeze-and-excitation (utils.py:1148-1184)
// ---------------------------------------------------------------------------------------------
constexpr int SE_CMAX = 4096, SE_RDMAX = 1024;

__global__ __launch_bounds__(256) void se_fwd_kernel(const float* __restrict__ sq, float inv_hw, const float* __restrict__ wr,
                                                     const float* __restrict__ br, const float* __restrict__ we, const float* __restrict__ be,
                                                     float* __restrict__ hid, float* __restrict__ s, int C, int rd) {
    __shared__ float m[SE_CMAX];
    __shared__ float hs[SE_RDMAX];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int c = threadIdx.x; c < C; c += 256) m[c] = sq[(long long)b * C + c] * inv_hw;
    __syncthreads();
    for (int j = wv; j < rd; j += 4) {
        float v = 0.f;
        for (int c = lane; c < C; c += 64) v = fmaf(wr[(long long)j * C + c], m[c], v);
        v = wave_sum(v) + br[j];
        v = v > 0.f ? v : 0.f;
        if (lane == 0) {
            hs[j] = v;
            hid[(long long)b * rd + j] = v;
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float z = be[c];
        for (int j = 0; j < rd; ++j) z = fmaf(we[(long long)c * rd + j], hs[j], z);
        s[(long long)b * C + c] = 1.0f / (1.0f + __expf(-z));
    }
}

__global__ __launch_bounds__(256) void se_apply_kernel(const bf16_t* __restrict__ d, const float* __restrict__ s, bf16_t* __restrict__ g,
                                                       long long n4, int HW, int C) {
    const int C4 = C >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / C4;
        const int c0 = (int)(i - r * C4) * 4;
        const long long b = r / HW;
        float v[4];
        load_row(d + r * C + c0, v);
        const f32x4_t sc = *reinterpret_cast<const f32x4_t*>(s + b * C + c0);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] *= sc[j];
        store_row(g + r * C + c0, v);
    }
}

// ds[b, c] = sum_hw dg d, one workgroup per (64-channel block, sample), row groups reduced in order
__global__ __launch_bounds__(256) void se_dsum_kernel(const bf16_t* __restrict__ dg, const bf16_t* __restrict__ d, float* __restrict__ ds,
                                                      int HW, int C) {
    __shared__ float red[DW_RG][DW_CB];
    const int b = blockIdx.y, lc = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int c0 = blockIdx.x * DW_CB + lc * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (c0 < C) {
        for (int p = rg; p < HW; p += DW_RG) {
            float x[4], y[4];
            load_row(dg + ((long long)b * HW + p) * C + c0, x);
            load_row(d + ((long long)b * HW + p) * C + c0, y);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(x[j], y[j], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) red[rg][lc * 4 + j] = acc[j];
    __syncthreads();
    if (threadIdx.x < DW_CB && blockIdx.x * DW_CB + (int)threadIdx.x < C) {
        float v = 0.f;
        for (int r = 0; r < DW_RG; ++r) v += red[r][threadIdx.x];
        ds[(long long)b * C + blockIdx.x * DW_CB + threadIdx.x] = v;
    }
}

// per sample: dz = ds s (1 - s) (sigmoid'), dp = relu'(h) W_e^T dz, dmean = W_r^T dp
__global__ __launch_bounds__(256) void se_bwd_sample_kernel(const float* __restrict__ ds, const float* __restrict__ s, const float* __restrict__ hid,
                                                            const float* __restrict__ wr, const float* __restrict__ we,
                                                            float* __restrict__ dz, float* __restrict__ dp, float* __restrict__ dmean, int C, int rd) {
    __shared__ float z[SE_CMAX];
    __shared__ float p[SE_RDMAX];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float sv = s[(long long)b * C + c];
        const float v = ds[(long long)b * C + c] * sv * (1.0f - sv);
        z[c] = v;
        dz[(long long)b * C + c] = v;
    }
    __syncthreads();
    for (int j = wv; j < rd; j += 4) {
        float v = 0.f;
        for (int c = lane; c < C; c += 64) v = fmaf(we[(long long)c * rd + j], z[c], v);
        v = wave_sum(v);
        v = hid[(long long)b * rd + j] > 0.f ? v : 0.f;
        if (lane == 0) {
            p[j] = v;
            dp[(long long)b * rd + j] = v;
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float v = 0.f;
        for (int j = 0; j < rd; ++j) v = fmaf(wr[(long long)j * C + c], p[j], v);
        dmean[(long long)b * C + c] = v;
    }
}

// the FC weight gradients, each a sum over the batch in sample order
__global__ __launch_bounds__(256) void se_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ dp, const float* __restrict__ hid,
                                                       const float* __restrict__ sq, float inv_hw, float* __restrict__ dwr, float* __restrict__ dbr,
                                                       float* __restrict__ dwe, float* __restrict__ dbe, int B, int C, int rd) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long n = (long long)C * rd;
    if (i < n) {                                   // dW_e [C, rd]
        const int c = (int)(i / rd), j = (int)(i - (long long)c * rd);
        float v = 0.f;
        for (int b = 0; b < B; ++b) v = fmaf(dz[(long long)b * C + c], hid[(long long)b * rd + j], v);
        dwe[i] = v;
    } else if (i < 2 * n) {                        // dW_r [rd, C]
        const long long k = i - n;
        const int j = (int)(k / C), c = (int)(k - (long long)j * C);
        float v = 0.f;
        for (int b = 0; b < B; ++b) v = fmaf(dp[(long long)b * rd + j], sq[(long long)b * C + c] * inv_hw, v);
        dwr[k] = v;
    } else if (i < 2 * n + C) {
        const int c = (int)(i - 2 * n);
        float v = 0.f;
        for (int b = 0; b < B; ++b) v += dz[(long long)b * C + c];
        dbe[c] = v;
    } else if (i < 2 * n + C + rd) {
        const int j = (int)(i - 2 * n - C);
        float v = 0.f;
        for (int b = 0; b < B; ++b) v += dp[(long long)b * rd + j];
        dbr[j] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// LayerScale residual with row-mode drop path: out = x + f gamma y, f = keep[r / rows_per_sample] / survival (or 1)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ls_add_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ gamma,
                                                     const float* __restrict__ keep, float inv_surv, float* __restrict__ out,
                                                     long long n4, long long rps, int C) {
    const int C4 = C >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / C4;
        const int c0 = (int)(i - r * C4) * 4;
        const float f = keep ? keep[r / rps] * inv_surv : 1.0f;
        const f32x4_t xv = *reinterpret_cast<const f32x4_t*>(x + r * C + c0);
        const f32x4_t yv = *reinterpret_cast<const f32x4_t*>(y + r * C + c0);
        const f32x4_t gv = *reinterpret_cast<const f32x4_t*>(gamma + c0);
        f32x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaf(f * gv[j], yv[j], xv[j]);
        *reinterpret_cast<f32x4_t*>(out + r * C + c0) = o;
    }
}

constexpr int LS_ROWS = 128;     // rows per partial

// dz = bf16(dy f gamma); partial[chunk, c] = sum over the chunk's rows of dy f y, 4 row lanes reduced in order; dgamma = the
// chunks added in index order (sum_rows_kernel, nrv_rows.hpp)
__global__ __launch_bounds__(256) void ls_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ gamma,
                                                     const float* __restrict__ keep, float inv_surv, bf16_t* __restrict__ dz,
                                                     float* __restrict__ part, long long rows, long long rps, int C) {
    __shared__ float red[4][64];
    const int lc = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lc;
    const long long r0 = (long long)blockIdx.y * LS_ROWS;
    float acc = 0.f;
    if (c < C) {
        const float g = gamma[c];
        for (int k = rl; k < LS_ROWS; k += 4) {
            const long long r = r0 + k;
            if (r >= rows) break;
            const float f = keep ? keep[r / rps] * inv_surv : 1.0f;
            const float v = dy[r * C + c] * f;
            dz[r * C + c] = f32_to_bf16(v * g);
            acc = fmaf(v, y[r * C + c], acc);
        }
    }
    red[rl][lc] = acc;
    __syncthreads();
    if (threadIdx.x < 64 && c < C) part[(long long)blockIdx.y * C + c] = ((red[0][lc] + red[1][lc]) + red[2][lc]) + red[3][lc];
}

// out = bf16(dx gelu'(stream))
__global__ __launch_bounds__(256) void dgelu_rows_kernel(const float* __restrict__ dx, const void* __restrict__ gs, int gdtype,
                                                         bf16_t* __restrict__ out, long long n4, int C) {
    const int C4 = C >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / C4;
        const int c0 = (int)(i - r * C4) * 4;
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(dx + r * C + c0);
        float g[4], o[4];
        dgelu4(gs, gdtype, r, c0, C, g);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = v[j] * g[j];
        store_row(out + r * C + c0, o);
    }
}

// ---------------------------------------------------------------------------------------------
// class attention (patch_convnet.py:88-101): per (sample, head) one query against Nk = 1 + Np keys, key 0 from the class
// source (kc / vc: one row per sample), keys 1 .. Np from the patch source (kp / vp: Np rows per sample).  dh % 8 == 0,
// dh <= 1024, Nk <= 4096.  Scores: one wave per key, lanes over dh (8 elements each, two passes at most); P V and dq: groups
// of dh / 8 lanes per key, group partials reduced in order.
// ---------------------------------------------------------------------------------------------
constexpr int CA_NMAX = 4096, CA_DMAX = 1024;

struct ClsArgs {
    const bf16_t *q, *kc, *kp, *vc, *vp;
    long long ldq, ldkc, ldkp, ldvc, ldvp;
    int B, H, Np, dh;
    float scale;
};

__device__ __forceinline__ const bf16_t* ca_row(const bf16_t* c, long long ldc, const bf16_t* p, long long ldp, int b, int Np, int j, int hoff) {
    return j == 0 ? c + (long long)b * ldc + hoff : p + ((long long)b * Np + j - 1) * ldp + hoff;
}

// o[e] = sum_j w[j] x_j[e] for the dh elements of one head (x = v or k rows), groups of dh/8 lanes, partials summed in order
__device__ __forceinline__ void ca_weighted_rows(const float* w, const bf16_t* c, long long ldc, const bf16_t* p, long long ldp, int b, int Np,
                                                 int Nk, int hoff, int dh, float mul, float* part, bf16_t* out) {
    const int G = dh >> 3, ng = 256 / G;
    const int g = threadIdx.x / G, e0 = (threadIdx.x - g * G) * 8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (g < ng) {
        for (int j = g; j < Nk; j += ng) {
            float x[8];
            load_row(ca_row(c, ldc, p, ldp, b, Np, j, hoff) + e0, x);
            const float wj = w[j];
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] = fmaf(wj, x[k], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) part[g * dh + e0 + k] = acc[k];
    }
    __syncthreads();
    if ((int)threadIdx.x < G) {
        float o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float v = 0.f;
            for (int r = 0; r < ng; ++r) v += part[r * dh + threadIdx.x * 8 + k];
            o[k] = v * mul;
        }
        store_row(out + threadIdx.x * 8, o);
    }
}

__global__ __launch_bounds__(256) void cls_attn_fwd_kernel(ClsArgs A, bf16_t* __restrict__ o, long long ldo, float* __restrict__ lse) {
    __shared__ float S[CA_NMAX];
    __shared__ float part[2048];
    __shared__ float buf[256];
    const int bh = blockIdx.x, b = bh / A.H, h = bh - b * A.H;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int Nk = A.Np + 1, dh = A.dh, hoff = h * dh;
    float qv[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = lane * 8 + 512 * i;
        if (e < dh) load_row(A.q + (long long)b * A.ldq + hoff + e, qv[i]);
    }
    for (int j = wv; j < Nk; j += 4) {
        const bf16_t* kr = ca_row(A.kc, A.ldkc, A.kp, A.ldkp, b, A.Np, j, hoff);
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = lane * 8 + 512 * i;
            if (e < dh) {
                float k[8];
                load_row(kr + e, k);
#pragma unroll
                for (int t = 0; t < 8; ++t) v = fmaf(qv[i][t], k[t], v);
            }
        }
        v = wave_sum(v);
        if (lane == 0) S[j] = v * A.scale;
    }
    __syncthreads();
    float m = -INFINITY;
    for (int j = threadIdx.x; j < Nk; j += 256) m = fmaxf(m, S[j]);
    m = block_max_256(m, buf);
    float l = 0.f;
    for (int j = threadIdx.x; j < Nk; j += 256) l += __expf(S[j] - m);
    l = block_sum_256(l, buf);
    const float L = m + __logf(l);
    for (int j = threadIdx.x; j < Nk; j += 256) S[j] = __expf(S[j] - L);
    if (threadIdx.x == 0) lse[bh] = L;
    __syncthreads();
    ca_weighted_rows(S, A.vc, A.ldvc, A.vp, A.ldvp, b, A.Np, Nk, hoff, dh, 1.0f, part, o + (long long)b * ldo + hoff);
}

__global__ __launch_bounds__(256) void cls_attn_bwd_kernel(ClsArgs A, const bf16_t* __restrict__ dout, long long ldo, const float* __restrict__ lse,
                                                           bf16_t* __restrict__ dq, bf16_t* __restrict__ dkc, bf16_t* __restrict__ dkp,
                                                           bf16_t* __restrict__ dvc, bf16_t* __restrict__ dvp) {
    __shared__ float P[CA_NMAX];
    __shared__ float dS[CA_NMAX];
    __shared__ float part[2048];
    __shared__ float buf[256];
    const int bh = blockIdx.x, b = bh / A.H, h = bh - b * A.H;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int Nk = A.Np + 1, dh = A.dh, hoff = h * dh;
    const float L = lse[bh];
    float qv[2][8], gv[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = lane * 8 + 512 * i;
        if (e < dh) {
            load_row(A.q + (long long)b * A.ldq + hoff + e, qv[i]);
            load_row(dout + (long long)b * ldo + hoff + e, gv[i]);
        }
    }
    // P_j (recomputed from the saved lse) and dP_j = do . v_j
    for (int j = wv; j < Nk; j += 4) {
        const bf16_t* kr = ca_row(A.kc, A.ldkc, A.kp, A.ldkp, b, A.Np, j, hoff);
        const bf16_t* vr = ca_row(A.vc, A.ldvc, A.vp, A.ldvp, b, A.Np, j, hoff);
        float s = 0.f, d = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = lane * 8 + 512 * i;
            if (e < dh) {
                float k[8], v[8];
                load_row(kr + e, k);
                load_row(vr + e, v);
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    s = fmaf(qv[i][t], k[t], s);
                    d = fmaf(gv[i][t], v[t], d);
                }
            }
        }
        s = wave_sum(s);
        d = wave_sum(d);
        if (lane == 0) {
            P[j] = __expf(s * A.scale - L);
            dS[j] = d;
        }
    }
    __syncthreads();
    float D = 0.f;
    for (int j = threadIdx.x; j < Nk; j += 256) D = fmaf(P[j], dS[j], D);
    D = block_sum_256(D, buf);
    for (int j = threadIdx.x; j < Nk; j += 256) dS[j] = P[j] * (dS[j] - D);
    __syncthreads();
    // dk_j = scale dS_j q, dv_j = P_j do
    for (int j = wv; j < Nk; j += 4) {
        bf16_t* kr = const_cast<bf16_t*>(ca_row(dkc, A.ldkc, dkp, A.ldkp, b, A.Np, j, hoff));
        bf16_t* vr = const_cast<bf16_t*>(ca_row(dvc, A.ldvc, dvp, A.ldvp, b, A.Np, j, hoff));
        const float ks = dS[j] * A.scale, pj = P[j];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = lane * 8 + 512 * i;
            if (e < dh) {
                float k[8], v[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    k[t] = ks * qv[i][t];
                    v[t] = pj * gv[i][t];
                }
                store_row(kr + e, k);
                store_row(vr + e, v);
            }
        }
    }
    // dq = scale sum_j dS_j k_j
    ca_weighted_rows(dS, A.kc, A.ldkc, A.kp, A.ldkp, b, A.Np, Nk, hoff, dh, A.scale, part, dq + (long long)b * A.ldq + hoff);
}

bool ca_shape_ok(int B, int H, int Np, int dh) {
    return B > 0 && H > 0 && Np >= 0 && Np + 1 <= CA_NMAX && dh > 0 && dh % 8 == 0 && dh <= CA_DMAX;
}

bool ld_ok(long long ld, int H, int dh) { return ld >= (long long)H * dh && ld % 8 == 0; }

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
static inline bool dw_shape_ok(int B, int H, int W, int C) {
    return B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && B <= 65535 && (long long)H * W <= (1ll << 24);
}

extern "C" int nrv_dwconv3x3_fwd(const void* a, const float* w, const float* bias, void* d_bf16, float* sq,
                                 int B, int H, int W, int C, void* stream) {
    if (!a || !w || !bias || !d_bf16 || !sq) return NRV_ERR_NULL;
    if (!dw_shape_ok(B, H, W, C)) return NRV_ERR_SHAPE;
    if (!nrv_aligned16(a) || !nrv_aligned16(d_bf16)) return NRV_ERR_ALIGN;
    hipLaunchKernelGGL(dw_fwd_kernel, dim3((unsigned)nrv_cdiv(C, DW_CB), B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const bf16_t*>(a), w, bias, static_cast<bf16_t*>(d_bf16), sq, H, W, C);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t nrv_dwconv3x3_bwd_workspace(int B, int H, int W, int C) {
    if (!dw_shape_ok(B, H, W, C)) return 0;
    return (size_t)B * H * W * C * 4 + (size_t)B * C * 10 * 4;
}

extern "C" int nrv_dwconv3x3_bwd(const void* a, const float* w, const float* bias, const void* dg, const float* s, const float* dmean,
                                 const void* gelu_stream, int gelu_dtype, void* da_bf16, float* dw, float* db,
                                 void* workspace, size_t workspace_bytes, int B, int H, int W, int C, void* stream) {
    if (!a || !w || !bias || !dg || !s || !dmean || !da_bf16 || !dw || !db || !workspace) return NRV_ERR_NULL;
    if (!dw_shape_ok(B, H, W, C)) return NRV_ERR_SHAPE;
    if (gelu_stream && gelu_dtype != NRV_BF16 && gelu_dtype != NRV_U8) return NRV_ERR_DTYPE;
    if (gelu_stream && gelu_dtype == NRV_U8 && C % 64) return NRV_ERR_SHAPE;
    if (workspace_bytes < nrv_dwconv3x3_bwd_workspace(B, H, W, C)) return NRV_ERR_WORKSPACE;
    if (!nrv_aligned16(a) || !nrv_aligned16(dg) || !nrv_aligned16(da_bf16) || !nrv_aligned16(workspace) ||
        (gelu_stream && !nrv_aligned16(gelu_stream)))
        return NRV_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* dd = static_cast<float*>(workspace);
    float* part = dd + (size_t)B * H * W * C;
    hipLaunchKernelGGL(dw_bwd_dd_kernel, dim3((unsigned)nrv_cdiv(C, DW_CB), B), dim3(256), 0, st, static_cast<const bf16_t*>(a), w, bias,
                       static_cast<const bf16_t*>(dg), s, dmean, 1.0f / (float)(H * W), dd, part, H, W, C);
    NRV_CHECK_LAUNCH();
    const long long n4 = (long long)B * H * W * C / 4;
    hipLaunchKernelGGL(dw_bwd_da_kernel, dim3(grid_for(n4, 256, PCN_GRID_CAP)), dim3(256), 0, st, dd, w, gelu_stream, gelu_dtype,
                       static_cast<bf16_t*>(da_bf16), n4, H, W, C);
    NRV_CHECK_LAUNCH();
    // an exact grid: the reducer has no stride loop and dw_shape_ok does not bound C (10 C / 256 fits gridDim.x for any int C)
    hipLaunchKernelGGL(tap_wred_kernel<256>, dim3((unsigned)nrv_cdiv(10ll * C, 256)), dim3(256), 0, st, part, dw, db, B, C, 9);
    NRV_CHECK_LAUNCH();
    return 0;
}

static inline bool se_shape_ok(int B, int C, int rd) {
    return B > 0 && B <= 65535 && C > 0 && C % 8 == 0 && C <= SE_CMAX && rd > 0 && rd <= SE_RDMAX;
}

extern "C" int nrv_se_fwd(const float* sq, int HW, const float* wr, const float* br, const float* we, const float* be,
                          float* hid, float* s, int B, int C, int rd, void* stream) {
    if (!sq || !wr || !br || !we || !be || !hid || !s) return NRV_ERR_NULL;
    if (!se_shape_ok(B, C, rd) || HW <= 0) return NRV_ERR_SHAPE;
    hipLaunchKernelGGL(se_fwd_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), sq, 1.0f / (float)HW, wr, br, we, be, hid, s, C, rd);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nrv_se_apply(const void* d, const float* s, void* g_bf16, int B, int HW, int C, void* stream) {
    if (!d || !s || !g_bf16) return NRV_ERR_NULL;
    if (B <= 0 || HW <= 0 || C <= 0 || C % 8) return NRV_ERR_SHAPE;
    if (!nrv_aligned16(d) || !nrv_aligned16(s) || !nrv_aligned16(g_bf16)) return NRV_ERR_ALIGN;
    const long long n4 = (long long)B * HW * C / 4;
    hipLaunchKernelGGL(se_apply_kernel, dim3(grid_for(n4, 256, PCN_GRID_CAP)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const bf16_t*>(d), s, static_cast<bf16_t*>(g_bf16), n4, HW, C);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t nrv_se_bwd_workspace(int B, int C, int rd) {
    if (!se_shape_ok(B, C, rd)) return 0;
    return ((size_t)2 * B * C + (size_t)B * rd) * 4;
}

extern "C" int nrv_se_bwd(const void* dg, const void* d, const float* sq, int HW, const float* s, const float* hid,
                          const float* wr, const float* we, float* dmean, float* dwr, float* dbr, float* dwe, float* dbe,
                          void* workspace, size_t workspace_bytes, int B, int C, int rd, void* stream) {
    if (!dg || !d || !sq || !s || !hid || !wr || !we || !dmean || !dwr || !dbr || !dwe || !dbe || !workspace) return NRV_ERR_NULL;
    if (!se_shape_ok(B, C, rd) || HW <= 0) return NRV_ERR_SHAPE;
    if (workspace_bytes < nrv_se_bwd_workspace(B, C, rd)) return NRV_ERR_WORKSPACE;
    if (!nrv_aligned16(dg) || !nrv_aligned16(d)) return NRV_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* ds = static_cast<float*>(workspace);
    float* dz = ds + (size_t)B * C;
    float* dp = dz + (size_t)B * C;
    hipLaunchKernelGGL(se_dsum_kernel, dim3((unsigned)nrv_cdiv(C, DW_CB), B), dim3(256), 0, st, static_cast<const bf16_t*>(dg),
                       static_cast<const bf16_t*>(d), ds, HW, C);
    NRV_CHECK_LAUNCH();
    hipLaunchKernelGGL(se_bwd_sample_kernel, dim3(B), dim3(256), 0, st, ds, s, hid, wr, we, dz, dp, dmean, C, rd);
    NRV_CHECK_LAUNCH();
    const long long n = 2ll * C * rd + C + rd;
    hipLaunchKernelGGL(se_wgrad_kernel, dim3((unsigned)nrv_cdiv(n, 256)), dim3(256), 0, st, dz, dp, hid, sq, 1.0f / (float)HW,
                       dwr, dbr, dwe, dbe, B, C, rd);
    NRV_CHECK_LAUNCH();
    return 0;
}

static inline int ls_check(int64_t rows, int64_t rps, int C, const float* keep, float survival) {
    if (rows <= 0 || C <= 0 || C % 4 || (keep && (rps <= 0 || rows % rps || !(survival > 0.f)))) return NRV_ERR_SHAPE;
    return 0;
}

extern "C" int nrv_ls_add_f32(const float* x, const float* y, const float* gamma, const float* keep, float survival, float* out,
                              int64_t rows, int64_t rows_per_sample, int C, void* stream) {
    if (!x || !y || !gamma || !out) return NRV_ERR_NULL;
    if (int e = ls_check(rows, rows_per_sample, C, keep, survival)) return e;
    if (!nrv_aligned16(x) || !nrv_aligned16(y) || !nrv_aligned16(gamma) || !nrv_aligned16(out)) return NRV_ERR_ALIGN;
    const long long n4 = rows * (long long)C / 4;
    hipLaunchKernelGGL(ls_add_kernel, dim3(grid_for(n4, 256, PCN_GRID_CAP)), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, gamma, keep,
                       keep ? 1.0f / survival : 1.0f, out, n4, keep ? (long long)rows_per_sample : 1ll, C);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t nrv_ls_bwd_workspace(int64_t rows, int C) {
    if (rows <= 0 || C <= 0) return 0;
    return (size_t)nrv_cdiv(rows, LS_ROWS) * C * 4;
}

extern "C" int nrv_ls_bwd(const float* dy, const float* y, const float* gamma, const float* keep, float survival, void* dz_bf16,
                          float* dgamma, void* workspace, size_t workspace_bytes, int64_t rows, int64_t rows_per_sample, int C,
                          void* stream) {
    if (!dy || !y || !gamma || !dz_bf16 || !dgamma || !workspace) return NRV_ERR_NULL;
    if (int e = ls_check(rows, rows_per_sample, C, keep, survival)) return e;
    if (nrv_cdiv(rows, LS_ROWS) > 65535) return NRV_ERR_SHAPE;
    if (workspace_bytes < nrv_ls_bwd_workspace(rows, C)) return NRV_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int chunks = (int)nrv_cdiv(rows, LS_ROWS);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(ls_bwd_kernel, dim3((unsigned)nrv_cdiv(C, 64), chunks), dim3(256), 0, st, dy, y, gamma, keep,
                       keep ? 1.0f / survival : 1.0f, static_cast<bf16_t*>(dz_bf16), part, (long long)rows,
                       keep ? (long long)rows_per_sample : 1ll, C);
    NRV_CHECK_LAUNCH();
    hipLaunchKernelGGL(sum_rows_kernel<256>, dim3((unsigned)nrv_cdiv(C, 256)), dim3(256), 0, st, part, chunks, C, dgamma, dgamma, C, 0.f);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nrv_dgelu_rows(const float* dx, const void* gelu_stream, int gelu_dtype, void* out_bf16, int64_t rows, int C, void* stream) {
    if (!dx || !gelu_stream || !out_bf16) return NRV_ERR_NULL;
    if (gelu_dtype != NRV_BF16 && gelu_dtype != NRV_U8) return NRV_ERR_DTYPE;
    if (rows <= 0 || C <= 0 || C % 8 || (gelu_dtype == NRV_U8 && C % 64)) return NRV_ERR_SHAPE;
    if (!nrv_aligned16(dx) || !nrv_aligned16(gelu_stream) || !nrv_aligned16(out_bf16)) return NRV_ERR_ALIGN;
    const long long n4 = rows * (long long)C / 4;
    hipLaunchKernelGGL(dgelu_rows_kernel, dim3(grid_for(n4, 256, PCN_GRID_CAP)), dim3(256), 0, static_cast<hipStream_t>(stream), dx, gelu_stream,
                       gelu_dtype, static_cast<bf16_t*>(out_bf16), n4, C);
    NRV_CHECK_LAUNCH();
    return 0;
}

static inline int ca_check(const void* q, int64_t ldq, const void* kc, int64_t ldkc, const void* kp, int64_t ldkp,
                           const void* vc, int64_t ldvc, const void* vp, int64_t ldvp, int B, int heads, int Np, int dh) {
    if (!q || !kc || !vc || (Np > 0 && (!kp || !vp))) return NRV_ERR_NULL;
    if (!ca_shape_ok(B, heads, Np, dh)) return NRV_ERR_SHAPE;
    if (!ld_ok(ldq, heads, dh) || !ld_ok(ldkc, heads, dh) || !ld_ok(ldvc, heads, dh) ||
        (Np > 0 && (!ld_ok(ldkp, heads, dh) || !ld_ok(ldvp, heads, dh))))
        return NRV_ERR_SHAPE;
    if (!nrv_aligned16(q) || !nrv_aligned16(kc) || !nrv_aligned16(vc) || (Np > 0 && (!nrv_aligned16(kp) || !nrv_aligned16(vp))))
        return NRV_ERR_ALIGN;
    return 0;
}

extern "C" int nrv_cls_attn_fwd(const void* q, int64_t ldq, const void* kc, int64_t ldkc, const void* kp, int64_t ldkp,
                                const void* vc, int64_t ldvc, const void* vp, int64_t ldvp, void* out_bf16, int64_t ldo, float* lse,
                                int B, int heads, int Np, int dh, float scale, void* stream) {
    if (int e = ca_check(q, ldq, kc, ldkc, kp, ldkp, vc, ldvc, vp, ldvp, B, heads, Np, dh)) return e;
    if (!out_bf16 || !lse) return NRV_ERR_NULL;
    if (!ld_ok(ldo, heads, dh)) return NRV_ERR_SHAPE;
    if (!nrv_aligned16(out_bf16)) return NRV_ERR_ALIGN;
    ClsArgs A{static_cast<const bf16_t*>(q), static_cast<const bf16_t*>(kc), static_cast<const bf16_t*>(kp), static_cast<const bf16_t*>(vc),
              static_cast<const bf16_t*>(vp), ldq, ldkc, ldkp, ldvc, ldvp, B, heads, Np, dh, scale};
    hipLaunchKernelGGL(cls_attn_fwd_kernel, dim3((unsigned)(B * heads)), dim3(256), 0, static_cast<hipStream_t>(stream), A,
                       static_cast<bf16_t*>(out_bf16), (long long)ldo, lse);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nrv_cls_attn_bwd(const void* q, int64_t ldq, const void* kc, int64_t ldkc, const void* kp, int64_t ldkp,
                                const void* vc, int64_t ldvc, const void* vp, int64_t ldvp, const void* dout_bf16, int64_t ldo,
                                const float* lse, void* dq, void* dkc, void* dkp, void* dvc, void* dvp,
                                int B, int heads, int Np, int dh, float scale, void* stream) {
    if (int e = ca_check(q, ldq, kc, ldkc, kp, ldkp, vc, ldvc, vp, ldvp, B, heads, Np, dh)) return e;
    if (!dout_bf16 || !lse || !dq || !dkc || !dvc || (Np > 0 && (!dkp || !dvp))) return NRV_ERR_NULL;
    if (!ld_ok(ldo, heads, dh)) return NRV_ERR_SHAPE;
    if (!nrv_aligned16(dout_bf16) || !nrv_aligned16(dq) || !nrv_aligned16(dkc) || !nrv_aligned16(dvc) ||
        (Np > 0 && (!nrv_aligned16(dkp) || !nrv_aligned16(dvp))))
        return NRV_ERR_ALIGN;
    ClsArgs A{static_cast<const bf16_t*>(q), static_cast<const bf16_t*>(kc), static_cast<const bf16_t*>(kp), static_cast<const bf16_t*>(vc),
              static_cast<const bf16_t*>(vp), ldq, ldkc, ldkp, ldvc, ldvp, B, heads, Np, dh, scale};
    hipLaunchKernelGGL(cls_attn_bwd_kernel, dim3((unsigned)(B * heads)), dim3(256), 0, static_cast<hipStream_t>(stream), A,
                       static_cast<const bf16_t*>(dout_bf16), (long long)ldo, lse, static_cast<bf16_t*>(dq), static_cast<bf16_t*>(dkc),
                       static_cast<bf16_t*>(dkp), static_cast<bf16_t*>(dvc), static_cast<bf16_t*>(dvp));
    NRV_CHECK_LAUNCH();
    return 0;
}
