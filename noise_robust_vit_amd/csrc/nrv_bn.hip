// Batch normalisation over token rows (LeViT, levit.py:57-163): BatchNorm1d on [B*N, C] and BatchNorm2d on NHWC rows [B*H*W, C]
// are the same column statistics over T rows of the fp32 GEMM output y.
//
//   statistics: per (chunk of BN_CHUNK rows, column) a Welford (count, mean, M2) partial; the 4 row groups of a workgroup are
//               merged in a fixed order, then a second kernel merges the chunks of a column (Chan's formula, in double): one
//               wave per column, lane l takes chunks l, l + 64, ... in order, then a fixed shuffle tree.  It writes mean,
//               invstd = 1 / sqrt(M2 / T + eps), the combined (count, mean, M2) and the running update (momentum, unbiased
//               variance M2 / (T - 1)).  No sum / sumsq: columns whose mean is 1e3 x their spread stay exact.
//   apply     : z = gamma (y - mean) invstd + beta, optionally Hardswish, times a row-mode drop-path factor, plus an fp32
//               residual; stored as fp32 and / or bf16.  Eval mode reads the running mean / variance instead.
//   backward  : dz = upstream (x Hardswish'(z) where the activation sits, x the drop-path factor); per (chunk, column) partials of
//               sum dz and sum dz x^ merged per column like the statistics; dgamma = sum dz x^, dbeta = sum dz;
//               dy = gamma invstd (dz - mean(dz) - x^ mean(dz x^)) (training) or gamma invstd dz (eval), stored as bf16.
// No atomics: every sum has one fixed order, reruns are bit-identical.  Hardswish and its derivative are those of nrv_rows.hpp.
#include "nrv_rows.hpp"

#include <cmath>

namespace {

constexpr int BN_CHUNK = 512;     // rows per partial (fixed: the summation order depends on T and C only)
constexpr int BN_COLS = 64;       // columns per workgroup
constexpr int BN_GROUPS = 4;      // row groups per workgroup (256 threads)

__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const float* __restrict__ y, float* __restrict__ part,
                                                               long long T, int C) {
    __shared__ float sn[BN_GROUPS][BN_COLS], sm[BN_GROUPS][BN_COLS], sq[BN_GROUPS][BN_COLS];
    const int cl = threadIdx.x & (BN_COLS - 1), g = threadIdx.x / BN_COLS;
    const int col = blockIdx.x * BN_COLS + cl;
    const long long chunk = blockIdx.y;
    const long long r0 = chunk * BN_CHUNK;
    const long long r1 = r0 + BN_CHUNK < T ? r0 + BN_CHUNK : T;
    float n = 0.f, mean = 0.f, m2 = 0.f;
    if (col < C) {
        for (long long r = r0 + g; r < r1; r += BN_GROUPS) {
            const float x = y[r * C + col];
            n += 1.f;
            const float d = x - mean;
            mean += d / n;
            m2 = fmaf(d, x - mean, m2);
        }
    }
    sn[g][cl] = n; sm[g][cl] = mean; sq[g][cl] = m2;
    __syncthreads();
    if (g == 0 && col < C) {
        for (int k = 1; k < BN_GROUPS; ++k) {
            const float nb = sn[k][cl];
            if (nb == 0.f) continue;
            const float na = n, nn = na + nb, d = sm[k][cl] - mean;
            mean += d * (nb / nn);
            m2 += sq[k][cl] + d * d * (na * nb / nn);
            n = nn;
        }
        float* p = part + chunk * 3 * C;
        p[col] = n;
        p[C + col] = mean;
        p[2 * C + col] = m2;
    }
}

// Chan's merge of (nb, mb, qb) into (n, mean, m2)
__device__ __forceinline__ void chan_merge(double& n, double& mean, double& m2, double nb, double mb, double qb) {
    if (nb == 0.0) return;
    const double nn = n + nb, d = mb - mean;
    mean += d * (nb / nn);
    m2 += qb + d * d * (n * nb / nn);
    n = nn;
}

// one wave per column: lane l merges chunks l, l + 64, ... in order, then a fixed shuffle tree over the lanes
__global__ __launch_bounds__(256) void bn_stats_final_kernel(const float* __restrict__ part, int chunks, int C, float eps,
                                                             float momentum, float* __restrict__ mean_out,
                                                             float* __restrict__ invstd_out, float* __restrict__ stat_out,
                                                             float* __restrict__ run_mean, float* __restrict__ run_var) {
    const int lane = threadIdx.x & 63;
    const int col = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= C) return;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    for (int c = lane; c < chunks; c += 64) {
        const float* p = part + (long long)c * 3 * C;
        chan_merge(n, mean, m2, p[col], p[C + col], p[2 * C + col]);
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double nb = __shfl_down(n, off), mb = __shfl_down(mean, off), qb = __shfl_down(m2, off);
        if (lane < off) chan_merge(n, mean, m2, nb, mb, qb);
    }
    if (lane != 0) return;
    const double var = m2 / n;
    mean_out[col] = (float)mean;
    invstd_out[col] = (float)(1.0 / std::sqrt(var + (double)eps));
    stat_out[col] = (float)n;
    stat_out[C + col] = (float)mean;
    stat_out[2 * C + col] = (float)m2;
    if (run_mean) {
        const float unbiased = n > 1.0 ? (float)(m2 / (n - 1.0)) : (float)var;
        run_mean[col] = (1.f - momentum) * run_mean[col] + momentum * (float)mean;
        run_var[col] = (1.f - momentum) * run_var[col] + momentum * unbiased;
    }
}

struct BnApply {
    const float* y;
    const float* mean;
    const float* scale;        // invstd, or the running variance when from_var
    const float* gamma;
    const float* beta;
    const float* res;
    const float* keep;
    float* out_f32;
    bf16_t* out_bf16;
    float eps, survival;
    long long T, rows_per_sample;
    int C, from_var, act;
};

__device__ __forceinline__ float bn_invstd(const float* scale, int col, int from_var, float eps) {
    return from_var ? 1.0f / sqrtf(scale[col] + eps) : scale[col];
}

__global__ __launch_bounds__(256) void bn_apply_kernel(BnApply a) {
    const long long n4 = a.T * a.C / 4;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (long long)gridDim.x * blockDim.x) {
        const long long r = e * 4 / a.C;
        const int c0 = (int)(e * 4 - r * a.C);
        const f32x4_t yv = *reinterpret_cast<const f32x4_t*>(a.y + e * 4);
        const float f = a.keep ? a.keep[r / a.rows_per_sample] / a.survival : 1.f;
        f32x4_t z;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + k;
            float v = a.gamma[c] * ((yv[k] - a.mean[c]) * bn_invstd(a.scale, c, a.from_var, a.eps)) + a.beta[c];
            if (a.act) v = hardswish(v);
            if (a.keep) v *= f;
            z[k] = v;
        }
        if (a.res) {
            const f32x4_t rv = *reinterpret_cast<const f32x4_t*>(a.res + e * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) z[k] = rv[k] + z[k];
        }
        if (a.out_f32) *reinterpret_cast<f32x4_t*>(a.out_f32 + e * 4) = z;
        if (a.out_bf16) *reinterpret_cast<u32x2_t*>(a.out_bf16 + e * 4) = u32x2_t{pack_bf16x2(z[0], z[1]), pack_bf16x2(z[2], z[3])};
    }
}

struct BnBwd {
    const void* dz;
    const float* y;
    const float* mean;
    const float* scale;
    const float* gamma;
    const float* beta;
    const float* keep;
    float* part;               // [chunks][2][C]
    float* colm;               // [2][C]: mean(dz), mean(dz x^)
    float* dgamma;
    float* dbeta;
    bf16_t* dy;
    float eps, survival;
    long long T, rows_per_sample;
    int C, dz_f32, from_var, act, training, chunks;
};

// upstream gradient of the BN output z at (r, c), with x^ = (y - mean) invstd returned in xh
__device__ __forceinline__ float bn_dz(const BnBwd& a, long long r, int c, float& xh) {
    const float inv = bn_invstd(a.scale, c, a.from_var, a.eps);
    xh = (a.y[r * a.C + c] - a.mean[c]) * inv;
    float g = a.dz_f32 ? reinterpret_cast<const float*>(a.dz)[r * a.C + c]
                       : bf16_to_f32(reinterpret_cast<const bf16_t*>(a.dz)[r * a.C + c]);
    if (a.act) g *= hardswish_grad(a.gamma[c] * xh + a.beta[c]);
    if (a.keep) g *= a.keep[r / a.rows_per_sample] / a.survival;
    return g;
}

__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(BnBwd a) {
    __shared__ float s1[BN_GROUPS][BN_COLS], s2[BN_GROUPS][BN_COLS];
    const int cl = threadIdx.x & (BN_COLS - 1), g = threadIdx.x / BN_COLS;
    const int col = blockIdx.x * BN_COLS + cl;
    const long long chunk = blockIdx.y;
    const long long r0 = chunk * BN_CHUNK;
    const long long r1 = r0 + BN_CHUNK < a.T ? r0 + BN_CHUNK : a.T;
    float sd = 0.f, sdx = 0.f;
    if (col < a.C) {
        for (long long r = r0 + g; r < r1; r += BN_GROUPS) {
            float xh;
            const float d = bn_dz(a, r, col, xh);
            sd += d;
            sdx = fmaf(d, xh, sdx);
        }
    }
    s1[g][cl] = sd; s2[g][cl] = sdx;
    __syncthreads();
    if (g == 0 && col < a.C) {
        for (int k = 1; k < BN_GROUPS; ++k) { sd += s1[k][cl]; sdx += s2[k][cl]; }
        float* p = a.part + chunk * 2 * a.C;
        p[col] = sd;
        p[a.C + col] = sdx;
    }
}

__global__ __launch_bounds__(256) void bn_bwd_final_kernel(BnBwd a) {
    const int lane = threadIdx.x & 63;
    const int col = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= a.C) return;
    double sd = 0.0, sdx = 0.0;
    for (int c = lane; c < a.chunks; c += 64) {
        const float* p = a.part + (long long)c * 2 * a.C;
        sd += p[col];
        sdx += p[a.C + col];
    }
    for (int off = 32; off > 0; off >>= 1) {
        sd += __shfl_down(sd, off);
        sdx += __shfl_down(sdx, off);
    }
    if (lane != 0) return;
    a.dgamma[col] = (float)sdx;
    a.dbeta[col] = (float)sd;
    a.colm[col] = (float)(sd / (double)a.T);
    a.colm[a.C + col] = (float)(sdx / (double)a.T);
}

__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(BnBwd a) {
    const long long n = a.T * a.C;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const long long r = e / a.C;
        const int c = (int)(e - r * a.C);
        float xh;
        const float d = bn_dz(a, r, c, xh);
        const float k = a.gamma[c] * bn_invstd(a.scale, c, a.from_var, a.eps);
        const float v = a.training ? k * (d - a.colm[c] - xh * a.colm[a.C + c]) : k * d;
        a.dy[e] = f32_to_bf16(v);
    }
}

int bn_shape(long long T, int C) {
    if (T <= 0 || C <= 0 || (C & 3) || T > (1ll << 24) || T * C > (1ll << 40)) return NRV_ERR_SHAPE;
    return 0;
}

int bn_chunks(long long T) { return (int)nrv_cdiv(T, BN_CHUNK); }

}  // namespace

extern "C" size_t nrv_bn_workspace(int64_t T, int C) {
    if (bn_shape(T, C)) return 0;
    return ((size_t)bn_chunks(T) * 3 + 2) * (size_t)C * sizeof(float);
}

extern "C" int nrv_bn_stats(const float* y, int64_t T, int C, float eps, float momentum,
                            float* mean, float* invstd, float* stat, float* running_mean, float* running_var,
                            void* workspace, size_t workspace_bytes, void* stream) {
    if (bn_shape(T, C)) return NRV_ERR_SHAPE;
    if (!y || !mean || !invstd || !stat || !workspace) return NRV_ERR_NULL;
    if ((running_mean == nullptr) != (running_var == nullptr)) return NRV_ERR_NULL;
    if (!(eps >= 0.f) || !(momentum >= 0.f && momentum <= 1.f)) return NRV_ERR_SHAPE;
    if (workspace_bytes < nrv_bn_workspace(T, C)) return NRV_ERR_WORKSPACE;
    if (!nrv_aligned16(y) || (reinterpret_cast<uintptr_t>(workspace) & 3u)) return NRV_ERR_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int chunks = bn_chunks(T);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3((unsigned)nrv_cdiv(C, BN_COLS), (unsigned)chunks), dim3(256), 0, s, y, part, T, C);
    NRV_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3((unsigned)nrv_cdiv(C, 4)), dim3(256), 0, s, part, chunks, C, eps, momentum,
                       mean, invstd, stat, running_mean, running_var);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nrv_bn_apply(const float* y, const float* mean, const float* scale, int scale_is_var, float eps,
                            const float* gamma, const float* beta, int act,
                            const float* residual, const float* keep, float survival, int64_t rows_per_sample,
                            float* out_f32, void* out_bf16, int64_t T, int C, void* stream) {
    if (bn_shape(T, C)) return NRV_ERR_SHAPE;
    if (!y || !mean || !scale || !gamma || !beta) return NRV_ERR_NULL;
    if (!out_f32 && !out_bf16) return NRV_ERR_NULL;
    if (act != 0 && act != 1) return NRV_ERR_EPILOGUE;
    if (keep && (!(survival > 0.f) || rows_per_sample <= 0 || T % rows_per_sample)) return NRV_ERR_SHAPE;
    if (!nrv_aligned16(y) || (residual && !nrv_aligned16(residual)) || (out_f32 && !nrv_aligned16(out_f32)) ||
        (reinterpret_cast<uintptr_t>(out_bf16) & 7u))
        return NRV_ERR_ALIGN;
    BnApply a{y, mean, scale, gamma, beta, residual, keep, out_f32, static_cast<bf16_t*>(out_bf16), eps, survival, T,
              keep ? rows_per_sample : 1, C, scale_is_var ? 1 : 0, act};
    hipLaunchKernelGGL(bn_apply_kernel, dim3(grid_for(T * C / 4, 256, 8192)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nrv_bn_bwd(const void* dz, int dz_dtype, int act, const float* keep, float survival, int64_t rows_per_sample,
                          const float* y, const float* mean, const float* scale, int scale_is_var, float eps,
                          const float* gamma, const float* beta, int training,
                          float* dgamma, float* dbeta, void* dy_bf16,
                          void* workspace, size_t workspace_bytes, int64_t T, int C, void* stream) {
    if (bn_shape(T, C)) return NRV_ERR_SHAPE;
    if (!dz || !y || !mean || !scale || !gamma || !beta || !dgamma || !dbeta || !dy_bf16 || !workspace) return NRV_ERR_NULL;
    if (dz_dtype != NRV_F32 && dz_dtype != NRV_BF16) return NRV_ERR_DTYPE;
    if (act != 0 && act != 1) return NRV_ERR_EPILOGUE;
    if (keep && (!(survival > 0.f) || rows_per_sample <= 0 || T % rows_per_sample)) return NRV_ERR_SHAPE;
    if (workspace_bytes < nrv_bn_workspace(T, C)) return NRV_ERR_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(workspace) & 3u)) return NRV_ERR_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int chunks = bn_chunks(T);
    float* part = static_cast<float*>(workspace);
    BnBwd a{dz, y, mean, scale, gamma, beta, keep, part, part + (size_t)chunks * 2 * C, dgamma, dbeta,
            static_cast<bf16_t*>(dy_bf16), eps, survival, T, keep ? rows_per_sample : 1, C, dz_dtype == NRV_F32 ? 1 : 0,
            scale_is_var ? 1 : 0, act, training ? 1 : 0, chunks};
    hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3((unsigned)nrv_cdiv(C, BN_COLS), (unsigned)chunks), dim3(256), 0, s, a);
    NRV_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((unsigned)nrv_cdiv(C, 4)), dim3(256), 0, s, a);
    NRV_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_for(T * C, 256, 8192)), dim3(256), 0, s, a);
    NRV_CHECK_LAUNCH();
    return 0;
}
