// Tokens-to-token (T2T-ViT, t2t.py:58-93) pieces that the ViT kernels do not cover:
//   soft split : nn.Unfold(ks, stride, pad) on token-major rows and its backward are the channel-major instantiation of the
//                unfold / fold kernel pair of nrv_misc.hip (nrv_soft_split_fwd / nrv_soft_split_bwd live there).
//   LayerNorm over the true width n of rows stored with a stride ld >= n (n = 147, 1323: ks*ks*C is no multiple of 8, the
//                GEMMs need K % 8 == 0, so the residual stream keeps zero pad columns): statistics over n, pad columns of
//                y / dx written as zeros.  One wave per row, two passes over the row for mean and centred variance (the
//                second pass hits L1 / L2).  dgamma / dbeta: per-slab column sums, then sum_rows_kernel (nrv_rows.hpp) in slab order.
#include "nrv_rows.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
// LayerNorm over n of ld columns
// ---------------------------------------------------------------------------------------------
constexpr int LNP_THREADS = 256;
constexpr int LNP_WAVES = LNP_THREADS / 64;
constexpr int LNP_MAX_N = 4096;
constexpr int LNP_MAX_SLABS = 128;
constexpr int LNP_SLAB_ROWS = 128;       // a slab holds at least this many rows (fewer slabs on short inputs)

template <bool F32>
__device__ __forceinline__ float ld1(const void* base, long long idx) {
    if (F32) return reinterpret_cast<const float*>(base)[idx];
    return bf16_to_f32(reinterpret_cast<const bf16_t*>(base)[idx]);
}

template <bool X_F32>
__global__ __launch_bounds__(LNP_THREADS) void ln_pad_fwd_kernel(const void* __restrict__ x, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, bf16_t* __restrict__ y,
                                                                 float* __restrict__ mean, float* __restrict__ rstd,
                                                                 long long rows, int n, int ld, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv_n = 1.0f / (float)n;
    for (long long r = (long long)blockIdx.x * LNP_WAVES + wave; r < rows; r += (long long)gridDim.x * LNP_WAVES) {
        const long long base = r * ld;
        float s = 0.f;
        for (int j = lane; j < n; j += 64) s += ld1<X_F32>(x, base + j);
        const float mu = wave_sum(s) * inv_n;
        float q = 0.f;
        for (int j = lane; j < n; j += 64) {
            const float d = ld1<X_F32>(x, base + j) - mu;
            q = fmaf(d, d, q);
        }
        const float rs = rsqrtf(wave_sum(q) * inv_n + eps);
        for (int j = lane; j < ld; j += 64)
            y[base + j] = j < n ? f32_to_bf16(fmaf((ld1<X_F32>(x, base + j) - mu) * rs, gamma[j], beta[j])) : (bf16_t)0;
        if (lane == 0) {
            mean[r] = mu;
            rstd[r] = rs;
        }
    }
}

// dx = dres + rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * gamma, means over the n true columns
template <bool X_F32, bool R_F32>
__global__ __launch_bounds__(LNP_THREADS) void ln_pad_bwd_kernel(const bf16_t* __restrict__ dy, const void* __restrict__ x,
                                                                 const float* __restrict__ gamma, const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd, const void* __restrict__ dres,
                                                                 float* __restrict__ dx32, bf16_t* __restrict__ dx16,
                                                                 long long rows, int n, int ld) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv_n = 1.0f / (float)n;
    for (long long r = (long long)blockIdx.x * LNP_WAVES + wave; r < rows; r += (long long)gridDim.x * LNP_WAVES) {
        const long long base = r * ld;
        const float mu = mean[r], rs = rstd[r];
        float a = 0.f, b = 0.f;
        for (int j = lane; j < n; j += 64) {
            const float g = bf16_to_f32(dy[base + j]) * gamma[j];
            const float xh = (ld1<X_F32>(x, base + j) - mu) * rs;
            a += g;
            b = fmaf(g, xh, b);
        }
        const float c1 = wave_sum(a) * inv_n, c2 = wave_sum(b) * inv_n;
        for (int j = lane; j < ld; j += 64) {
            float v = 0.f;
            if (j < n) {
                const float g = bf16_to_f32(dy[base + j]) * gamma[j];
                const float xh = (ld1<X_F32>(x, base + j) - mu) * rs;
                v = rs * (g - c1 - xh * c2);
                if (dres) v += ld1<R_F32>(dres, base + j);
            }
            if (dx32) dx32[base + j] = v;
            if (dx16) dx16[base + j] = f32_to_bf16(v);
        }
    }
}

// slab s sums rows [s * per, (s + 1) * per) of dy * xhat and dy for the columns of its block: part[s][0 | 1][n]
template <bool X_F32>
__global__ __launch_bounds__(LNP_THREADS) void ln_pad_dgb_partial_kernel(const bf16_t* __restrict__ dy, const void* __restrict__ x,
                                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                         float* __restrict__ part, long long rows, long long per, int n, int ld) {
    const int j = blockIdx.x * LNP_THREADS + threadIdx.x;
    const int s = blockIdx.y;
    if (j >= n) return;
    const long long r0 = (long long)s * per;
    const long long r1 = r0 + per < rows ? r0 + per : rows;
    float dg = 0.f, db = 0.f;
    for (long long r = r0; r < r1; ++r) {
        const float d = bf16_to_f32(dy[r * ld + j]);
        dg = fmaf(d, (ld1<X_F32>(x, r * ld + j) - mean[r]) * rstd[r], dg);
        db += d;
    }
    part[((long long)s * 2 + 0) * n + j] = dg;
    part[((long long)s * 2 + 1) * n + j] = db;
}

int lnp_slabs(long long rows) {
    long long s = (rows + LNP_SLAB_ROWS - 1) / LNP_SLAB_ROWS;
    if (s > LNP_MAX_SLABS) s = LNP_MAX_SLABS;
    return s < 1 ? 1 : (int)s;
}

int lnp_shape(long long rows, int n, long long ld) {
    if (rows <= 0 || n <= 0 || n > LNP_MAX_N || ld < n || (ld & 7) || ld > (1 << 20)) return NRV_ERR_SHAPE;
    if (rows * ld > (1ll << 40)) return NRV_ERR_SHAPE;
    return 0;
}

}  // namespace

extern "C" int nrv_layernorm_pad_fwd(const void* x, int x_dtype, const float* gamma, const float* beta, void* y_bf16, float* mean,
                                     float* rstd, int64_t rows, int n, int64_t ld, float eps, void* stream) {
    if (lnp_shape(rows, n, ld)) return NRV_ERR_SHAPE;
    if (!x || !gamma || !beta || !y_bf16 || !mean || !rstd) return NRV_ERR_NULL;
    if (x_dtype != NRV_F32 && x_dtype != NRV_BF16) return NRV_ERR_DTYPE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int grid = grid_for(rows, LNP_WAVES, 8192);
    bf16_t* y = static_cast<bf16_t*>(y_bf16);
    if (x_dtype == NRV_F32) hipLaunchKernelGGL((ln_pad_fwd_kernel<true>), dim3(grid), dim3(LNP_THREADS), 0, s, x, gamma, beta, y, mean, rstd, (long long)rows, n, (int)ld, eps);
    else hipLaunchKernelGGL((ln_pad_fwd_kernel<false>), dim3(grid), dim3(LNP_THREADS), 0, s, x, gamma, beta, y, mean, rstd, (long long)rows, n, (int)ld, eps);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t nrv_layernorm_pad_bwd_workspace(int64_t rows, int n) {
    if (rows <= 0 || n <= 0) return 0;
    return (size_t)lnp_slabs(rows) * 2 * (size_t)n * sizeof(float);
}

extern "C" int nrv_layernorm_pad_bwd(const void* dy_bf16, const void* x, int x_dtype, const float* gamma, const float* mean,
                                     const float* rstd, const void* dres, int dres_dtype, float* dx_f32, void* dx_bf16,
                                     float* dgamma, float* dbeta, int accumulate, void* workspace, size_t workspace_bytes,
                                     int64_t rows, int n, int64_t ld, void* stream) {
    if (lnp_shape(rows, n, ld)) return NRV_ERR_SHAPE;
    if (!dy_bf16 || !x || !gamma || !mean || !rstd || !dgamma || !dbeta || !workspace || (!dx_f32 && !dx_bf16)) return NRV_ERR_NULL;
    if ((x_dtype != NRV_F32 && x_dtype != NRV_BF16) || (dres && dres_dtype != NRV_F32 && dres_dtype != NRV_BF16)) return NRV_ERR_DTYPE;
    if (workspace_bytes < nrv_layernorm_pad_bwd_workspace(rows, n)) return NRV_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bf16_t* dy = static_cast<const bf16_t*>(dy_bf16);
    bf16_t* dx16 = static_cast<bf16_t*>(dx_bf16);
    const int grid = grid_for(rows, LNP_WAVES, 8192);
    const bool xf = x_dtype == NRV_F32, rf = !dres || dres_dtype == NRV_F32;
    if (xf && rf) hipLaunchKernelGGL((ln_pad_bwd_kernel<true, true>), dim3(grid), dim3(LNP_THREADS), 0, s, dy, x, gamma, mean, rstd, dres, dx_f32, dx16, (long long)rows, n, (int)ld);
    else if (xf) hipLaunchKernelGGL((ln_pad_bwd_kernel<true, false>), dim3(grid), dim3(LNP_THREADS), 0, s, dy, x, gamma, mean, rstd, dres, dx_f32, dx16, (long long)rows, n, (int)ld);
    else if (rf) hipLaunchKernelGGL((ln_pad_bwd_kernel<false, true>), dim3(grid), dim3(LNP_THREADS), 0, s, dy, x, gamma, mean, rstd, dres, dx_f32, dx16, (long long)rows, n, (int)ld);
    else hipLaunchKernelGGL((ln_pad_bwd_kernel<false, false>), dim3(grid), dim3(LNP_THREADS), 0, s, dy, x, gamma, mean, rstd, dres, dx_f32, dx16, (long long)rows, n, (int)ld);
    NRV_CHECK_LAUNCH();
    const int slabs = lnp_slabs(rows);
    const long long per = (rows + slabs - 1) / slabs;
    float* part = static_cast<float*>(workspace);
    const dim3 pg((unsigned)((n + LNP_THREADS - 1) / LNP_THREADS), (unsigned)slabs);
    if (xf) hipLaunchKernelGGL((ln_pad_dgb_partial_kernel<true>), pg, dim3(LNP_THREADS), 0, s, dy, x, mean, rstd, part, (long long)rows, per, n, (int)ld);
    else hipLaunchKernelGGL((ln_pad_dgb_partial_kernel<false>), pg, dim3(LNP_THREADS), 0, s, dy, x, mean, rstd, part, (long long)rows, per, n, (int)ld);
    NRV_CHECK_LAUNCH();
    // part is [slabs][2 n], a row = dgamma | dbeta: the slabs added in index order
    hipLaunchKernelGGL(sum_rows_kernel<256>, dim3((unsigned)nrv_cdiv(2 * n, 256)), dim3(256), 0, s, part, slabs, 2 * n, dgamma, dbeta, n,
                       accumulate ? 1.0f : 0.0f);
    NRV_CHECK_LAUNCH();
    return 0;
}
