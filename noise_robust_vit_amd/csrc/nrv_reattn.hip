// Re-attention on materialised matrices [B, H, Nq, Nk] (gfx950): DeepViT's head mixing followed by a LayerNorm over the heads
// at every (query, key) position (deepvit.py:47-53, 67-74).  S = scaled scores, W = reattn_weights ([h, g], fp32), gamma / beta =
// reattn_norm.1.{weight, bias} ([H], fp32):
//     P = softmax(S) (or Sinkhorn(S), nrv_sinkhorn_fwd)      M[b,g] = sum_h W[h,g] P[b,h]
//     mu = mean_g M    var = mean_g (M - mu)^2    x^[g] = (M[g] - mu) rsqrt(var + eps)    A[g] = x^[g] gamma[g] + beta[g]
// The variance is taken from the deviations (two passes over the H register values): across heads it is orders of magnitude
// below M^2, so E[x^2] - E[x]^2 would cancel.  mu and rstd are never stored: the backward recomputes them from P.
//
// Dtypes in memory: S, P, dA, dS, dP fp32; A fp32 or bf16.  Kept for the backward per layer: P in fp32 and A in bf16, 6 bytes per
// element (10 with the Sinkhorn path, which also keeps S).
//
//   nrv_reattn_softmax_fwd   one workgroup per query row (b, i) holds the row of ALL heads in LDS: per-head softmax with a wave per
//                            head, then every thread mixes and normalises its positions in registers.  S is read once, P and A
//                            are written once.
//   nrv_reattn_softmax_bwd   the same row ownership with two LDS images (dA -> dM -> dP in place; P).  A workgroup walks rows
//                            wg, wg + grid, ...; per position it recomputes M, mu, rstd, x^ and
//                                dbeta[g] += dA[g]     dgamma[g] += dA[g] x^[g]     dx^[g] = dA[g] gamma[g]
//                                dM[g] = rstd (dx^[g] - mean_g dx^ - x^[g] mean_g (dx^ x^))
//                            then dW[h,g] += P[h] . dM[g] (th_pairs), dP[h] = sum_g W[h,g] dM[g] (th_mix), dS = P (dP - <P, dP>).
//                            Parameter sums: fp32 inside a row, double across rows, one set of H H + 2 H doubles per workgroup in
//                            the workspace; a second kernel adds the sets in index order.
//   nrv_reattn_norm_fwd/bwd  mixing + LayerNorm alone on flat positions p = i * Nk + j (the robust path runs them around
//                            nrv_sinkhorn_fwd / bwd); the backward stages 512-position tiles in LDS.
//
// Accesses along j are 16-byte vectors when Nk % 4 == 0 (Nq * Nk % 4 == 0 for the flat kernels) and coalesced dwords otherwise.
// Per-head register arrays are indexed only through fully unrolled loops guarded by i < H.  Plain C++, vector stores only, no
// atomics: reruns are bit-identical.
#include "nrv_heads.hpp"

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// m[g] = sum_h W[h, g] x[h] for every g < H at V positions, all in registers
template <int V>
__device__ __forceinline__ void ra_mix(const float (&x)[TH_MAXH][V], const float* __restrict__ W, int H, float (&m)[TH_MAXH][V]) {
#pragma unroll
    for (int g = 0; g < TH_MAXH; ++g)
        if (g < H) {
#pragma unroll
            for (int v = 0; v < V; ++v) m[g][v] = 0.f;
#pragma unroll
            for (int h = 0; h < TH_MAXH; ++h)
                if (h < H) {
                    const float w = W[h * H + g];
#pragma unroll
                    for (int v = 0; v < V; ++v) m[g][v] = fmaf(w, x[h][v], m[g][v]);
                }
        }
}

// m[g] <- x^[g] = (m[g] - mu) rstd over the H heads (two-pass variance); returns rstd
template <int V>
__device__ __forceinline__ void ra_normalise(float (&m)[TH_MAXH][V], int H, float eps, float (&rstd)[V]) {
    const float inv_h = 1.0f / (float)H;
    float mu[V], var[V];
#pragma unroll
    for (int v = 0; v < V; ++v) mu[v] = 0.f, var[v] = 0.f;
#pragma unroll
    for (int g = 0; g < TH_MAXH; ++g)
        if (g < H) {
#pragma unroll
            for (int v = 0; v < V; ++v) mu[v] += m[g][v];
        }
#pragma unroll
    for (int v = 0; v < V; ++v) mu[v] *= inv_h;
#pragma unroll
    for (int g = 0; g < TH_MAXH; ++g)
        if (g < H) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
                m[g][v] -= mu[v];
                var[v] = fmaf(m[g][v], m[g][v], var[v]);
            }
        }
#pragma unroll
    for (int v = 0; v < V; ++v) rstd[v] = rsqrtf(fmaf(var[v], inv_h, eps));
#pragma unroll
    for (int g = 0; g < TH_MAXH; ++g)
        if (g < H) {
#pragma unroll
            for (int v = 0; v < V; ++v) m[g][v] *= rstd[v];
        }
}

// x[h] = P[h] at V positions  ->  x[g] = A[g]
template <int V>
__device__ __forceinline__ void ra_point_fwd(float (&x)[TH_MAXH][V], const float* __restrict__ W, const float* __restrict__ gamma,
                                             const float* __restrict__ beta, int H, float eps) {
    float m[TH_MAXH][V], rstd[V];
    ra_mix<V>(x, W, H, m);
    ra_normalise<V>(m, H, eps, rstd);
#pragma unroll
    for (int g = 0; g < TH_MAXH; ++g)
        if (g < H) {
            const float ga = gamma[g], be = beta[g];
#pragma unroll
            for (int v = 0; v < V; ++v) x[g][v] = fmaf(m[g][v], ga, be);
        }
}

// x[h] = P[h], d[g] = dA[g] at V positions  ->  d[g] = dM[g];  dg[g] += sum_v dA[g] x^[g],  db[g] += sum_v dA[g]
template <int V>
__device__ __forceinline__ void ra_point_bwd(const float (&x)[TH_MAXH][V], float (&d)[TH_MAXH][V], const float* __restrict__ W,
                                             const float* __restrict__ gamma, int H, float eps, float (&dg)[TH_MAXH],
                                             float (&db)[TH_MAXH]) {
    const float inv_h = 1.0f / (float)H;
    float m[TH_MAXH][V], rstd[V], s1[V], s2[V];
    ra_mix<V>(x, W, H, m);
    ra_normalise<V>(m, H, eps, rstd);
#pragma unroll
    for (int v = 0; v < V; ++v) s1[v] = 0.f, s2[v] = 0.f;
#pragma unroll
    for (int g = 0; g < TH_MAXH; ++g)
        if (g < H) {
            const float ga = gamma[g];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                db[g] += d[g][v];
                dg[g] = fmaf(d[g][v], m[g][v], dg[g]);
                d[g][v] *= ga;                                 // dx^
                s1[v] += d[g][v];
                s2[v] = fmaf(d[g][v], m[g][v], s2[v]);
            }
        }
#pragma unroll
    for (int v = 0; v < V; ++v) s1[v] *= inv_h, s2[v] *= inv_h;
#pragma unroll
    for (int g = 0; g < TH_MAXH; ++g)
        if (g < H) {
#pragma unroll
            for (int v = 0; v < V; ++v) d[g][v] = rstd[v] * ((d[g][v] - s1[v]) - m[g][v] * s2[v]);
        }
}

// every position of the LDS images sP (P) and sD (dA) with np positions: sD <- dM; the thread's dgamma / dbeta shares of this
// image (fp32) are added to its running double sums
template <int V>
__device__ __forceinline__ void ra_image_bwd(const float* sP, float* sD, int ld, const float* __restrict__ W,
                                             const float* __restrict__ gamma, int H, int np, float eps, double (&ag)[TH_MAXH],
                                             double (&ab)[TH_MAXH]) {
    float dg[TH_MAXH], db[TH_MAXH];
#pragma unroll
    for (int g = 0; g < TH_MAXH; ++g) dg[g] = 0.f, db[g] = 0.f;
    for (int p = threadIdx.x * V; p < np; p += TH_THREADS * V) {
        float x[TH_MAXH][V], d[TH_MAXH][V];
#pragma unroll
        for (int h = 0; h < TH_MAXH; ++h)
            if (h < H) {
                ldv<V>(sP + h * ld + p, x[h]);
                ldv<V>(sD + h * ld + p, d[h]);
            }
        ra_point_bwd<V>(x, d, W, gamma, H, eps, dg, db);
#pragma unroll
        for (int g = 0; g < TH_MAXH; ++g)
            if (g < H) stv<V>(sD + g * ld + p, d[g]);
    }
#pragma unroll
    for (int g = 0; g < TH_MAXH; ++g)
        if (g < H) {
            ag[g] += (double)dg[g];
            ab[g] += (double)db[g];
        }
}

// the workgroup's dgamma (out[0 .. H)) and dbeta (out[H .. 2H)) from its threads' sums: lanes by butterfly, then the four waves in
// order; red: TH_THREADS doubles of LDS
__device__ __forceinline__ void ra_vec_out(double* red, const double (&ag)[TH_MAXH], const double (&ab)[TH_MAXH], int H,
                                           double* __restrict__ out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
#pragma unroll
    for (int g = 0; g < TH_MAXH; ++g)
        if (g < H) {
            const double sg = wave_sum_f64(ag[g]), sb = wave_sum_f64(ab[g]);
            if (lane == 0) {
                red[wave * 2 * TH_MAXH + g] = sg;
                red[wave * 2 * TH_MAXH + TH_MAXH + g] = sb;
            }
        }
    __syncthreads();
    if ((int)threadIdx.x < 2 * H) {
        const int k = (int)threadIdx.x < H ? (int)threadIdx.x : TH_MAXH + (int)threadIdx.x - H;
        double s = 0.0;
        for (int w = 0; w < TH_THREADS / 64; ++w) s += red[w * 2 * TH_MAXH + k];
        out[threadIdx.x] = s;
    }
}

template <int V, class AT>
__global__ __launch_bounds__(TH_THREADS) void ra_softmax_fwd_kernel(const float* __restrict__ S, const float* __restrict__ W,
                                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                    float* __restrict__ P, AT* __restrict__ A, int H, int Nq, int Nk,
                                                                    float eps) {
    const int ld = th_ld(Nk);
    float* sP = th_smem;
    const long long row = blockIdx.x;                          // b * Nq + i
    const long long b = row / Nq, i = row - b * Nq;
    const long long hstride = (long long)Nq * Nk;
    const long long base = (b * H * Nq + i) * Nk;              // head 0 of this row
    th_load<V>(sP, ld, S + base, hstride, H, Nk);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int h = threadIdx.x >> 6; h < H; h += TH_THREADS / 64) {
        float* r = sP + h * ld;
        float m = -INFINITY;
        for (int j = lane; j < Nk; j += 64) m = fmaxf(m, r[j]);
        m = wave_max(m);
        float sum = 0.f;
        for (int j = lane; j < Nk; j += 64) {
            const float e = __builtin_amdgcn_exp2f((r[j] - m) * 1.4426950408889634f);
            r[j] = e;
            sum += e;
        }
        const float inv = 1.0f / wave_sum(sum);
        for (int j = lane; j < Nk; j += 64) r[j] *= inv;
    }
    __syncthreads();
    for (int p = threadIdx.x * V; p < Nk; p += TH_THREADS * V) {
        float x[TH_MAXH][V];
#pragma unroll
        for (int h = 0; h < TH_MAXH; ++h)
            if (h < H) {
                ldv<V>(sP + h * ld + p, x[h]);
                stv<V>(P + base + h * hstride + p, x[h]);
            }
        ra_point_fwd<V>(x, W, gamma, beta, H, eps);
#pragma unroll
        for (int g = 0; g < TH_MAXH; ++g)
            if (g < H) stv<V>(A + base + g * hstride + p, x[g]);
    }
}

template <int V>
__global__ __launch_bounds__(TH_THREADS) void ra_softmax_bwd_kernel(const float* __restrict__ dA, const float* __restrict__ P,
                                                                    const float* __restrict__ W, const float* __restrict__ gamma,
                                                                    float* __restrict__ dS, double* __restrict__ part, int H, int Nq,
                                                                    int Nk, long long rows, float eps) {
    const int ld = th_ld(Nk);
    double* red = reinterpret_cast<double*>(th_smem);          // TH_THREADS doubles for the final sums
    float* sD = th_smem + 2 * TH_THREADS;                      // dA, then dM, then dP
    float* sP = sD + H * ld;                                   // P
    const long long hstride = (long long)Nq * Nk;
    const int lane = threadIdx.x & 63;
    double accw = 0.0, ag[TH_MAXH], ab[TH_MAXH];
#pragma unroll
    for (int g = 0; g < TH_MAXH; ++g) ag[g] = 0.0, ab[g] = 0.0;
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const long long b = row / Nq, i = row - b * Nq;
        const long long base = (b * H * Nq + i) * Nk;
        __syncthreads();                                       // the previous row's images are done with
        th_load<V>(sD, ld, dA + base, hstride, H, Nk);
        th_load<V>(sP, ld, P + base, hstride, H, Nk);
        __syncthreads();
        ra_image_bwd<V>(sP, sD, ld, W, gamma, H, Nk, eps, ag, ab);                                     // sD = dM
        __syncthreads();
        accw += (double)th_pairs(sP, sD, ld, H, Nk);             // dW[h,g] += P[h] . dM[g]
        __syncthreads();
        th_mix<V, true>(sD, ld, W, H, Nk, [](int, int, const float (&)[V]) {},
                        [&](int h, int p, const float (&d)[V]) { stv<V>(sD + h * ld + p, d); });      // dP[h] = sum_g W[h,g] dM[g]
        __syncthreads();
        for (int h = threadIdx.x >> 6; h < H; h += TH_THREADS / 64) {
            const float* d = sD + h * ld;
            const float* pr = sP + h * ld;
            float dot = 0.f;
            for (int j = lane; j < Nk; j += 64) dot = fmaf(pr[j], d[j], dot);
            dot = wave_sum(dot);
            for (int j = lane * V; j < Nk; j += 64 * V) {                                              // dS = P (dP - <P, dP>)
                float pv[V], dv[V];
                ldv<V>(pr + j, pv);
                ldv<V>(d + j, dv);
#pragma unroll
                for (int v = 0; v < V; ++v) dv[v] = pv[v] * (dv[v] - dot);
                stv<V>(dS + base + h * hstride + j, dv);
            }
        }
    }
    double* out = part + (long long)blockIdx.x * (H * H + 2 * H);
    th_pairs_out(red, accw, H, out);
    ra_vec_out(red, ag, ab, H, out + H * H);
}

template <int V, class AT>
__global__ __launch_bounds__(TH_THREADS) void ra_norm_fwd_kernel(const float* __restrict__ P, const float* __restrict__ W,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 AT* __restrict__ A, int H, long long M, long long items, float eps) {
    // item = (b, group of V positions); heads are M apart
    const long long per = M / V;
    for (long long it = blockIdx.x * (long long)TH_THREADS + threadIdx.x; it < items; it += (long long)gridDim.x * TH_THREADS) {
        const long long b = it / per, p = (it - b * per) * V;
        const float* src = P + b * H * M + p;
        AT* dst = A + b * H * M + p;
        float x[TH_MAXH][V];
#pragma unroll
        for (int h = 0; h < TH_MAXH; ++h)
            if (h < H) ldv<V>(src + h * M, x[h]);
        ra_point_fwd<V>(x, W, gamma, beta, H, eps);
#pragma unroll
        for (int g = 0; g < TH_MAXH; ++g)
            if (g < H) stv<V>(dst + g * M, x[g]);
    }
}

template <int V>
__global__ __launch_bounds__(TH_THREADS) void ra_norm_bwd_kernel(const float* __restrict__ dA, const float* __restrict__ P,
                                                                 const float* __restrict__ W, const float* __restrict__ gamma,
                                                                 float* __restrict__ dP, double* __restrict__ part, int H, long long M,
                                                                 long long tiles_per_b, long long tiles, float eps) {
    const int ld = th_ld(TH_TILE);
    double* red = reinterpret_cast<double*>(th_smem);
    float* sD = th_smem + 2 * TH_THREADS;                      // dA, then dM
    float* sX = sD + H * ld;                                   // P
    double accw = 0.0, ag[TH_MAXH], ab[TH_MAXH];
#pragma unroll
    for (int g = 0; g < TH_MAXH; ++g) ag[g] = 0.0, ab[g] = 0.0;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long b = t / tiles_per_b, p0 = (t - b * tiles_per_b) * TH_TILE;
        const int np = (int)(M - p0 < TH_TILE ? M - p0 : TH_TILE);
        const long long base = b * H * M + p0;
        __syncthreads();
        th_load<V>(sD, ld, dA + base, M, H, np);
        th_load<V>(sX, ld, P + base, M, H, np);
        __syncthreads();
        ra_image_bwd<V>(sX, sD, ld, W, gamma, H, np, eps, ag, ab);                                     // sD = dM
        __syncthreads();
        accw += (double)th_pairs(sX, sD, ld, H, np);            // dW[h,g] += P[h] . dM[g]
        th_mix<V, true>(sD, ld, W, H, np, [](int, int, const float (&)[V]) {},
                        [&](int h, int p, const float (&d)[V]) { stv<V>(dP + base + h * M + p, d); });
    }
    double* out = part + (long long)blockIdx.x * (H * H + 2 * H);
    th_pairs_out(red, accw, H, out);
    ra_vec_out(red, ag, ab, H, out + H * H);
}

// out[k] = sum over the parts, in part order: k < H H is dW, then dgamma, then dbeta
__global__ void ra_reduce_kernel(const double* __restrict__ part, int nparts, int H, float* __restrict__ dW,
                                 float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int n = H * H + 2 * H;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    double s = 0.0;
#pragma unroll 8
    for (int q = 0; q < nparts; ++q) s += part[(long long)q * n + k];
    if (k < H * H) dW[k] = (float)s;
    else if (k < H * H + H) dgamma[k - H * H] = (float)s;
    else dbeta[k - H * H - H] = (float)s;
}

bool ra_shape_ok(int B, int H, int Nq, int Nk, float eps) { return th_shape_ok(B, H, Nq, Nk) && eps > 0.f; }

size_t ra_part_bytes(long long work, int H) { return (size_t)th_parts(work) * (H * H + 2 * H) * 8; }

}  // namespace

extern "C" int nrv_reattn_softmax_fwd(const float* S, const float* W, const float* gamma, const float* beta, float* P, void* A,
                                      int a_dtype, int B, int H, int Nq, int Nk, float eps, void* stream) {
    if (!S || !W || !gamma || !beta || !P || !A) return NRV_ERR_NULL;
    if (a_dtype != NRV_F32 && a_dtype != NRV_BF16) return NRV_ERR_DTYPE;
    if (!ra_shape_ok(B, H, Nq, Nk, eps)) return NRV_ERR_SHAPE;
    if (!nrv_aligned16(S) || !nrv_aligned16(P) || !nrv_aligned16(A)) return NRV_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t lds = (size_t)H * th_ld(Nk) * 4;
    const dim3 grid((unsigned)((long long)B * Nq)), block(TH_THREADS);
    const bool vec = Nk % 4 == 0;
#define RA_FWD(V, AT)                                                                                                   \
    do {                                                                                                                \
        static int attr = th_lds_attr(ra_softmax_fwd_kernel<V, AT>, TH_LDS_MAX);                                        \
        if (attr) return attr;                                                                                          \
        hipLaunchKernelGGL((ra_softmax_fwd_kernel<V, AT>), grid, block, lds, st, S, W, gamma, beta, P, static_cast<AT*>(A), H, Nq, Nk, eps); \
    } while (0)
    if (a_dtype == NRV_BF16) {
        if (vec) RA_FWD(4, bf16_t); else RA_FWD(1, bf16_t);
    } else {
        if (vec) RA_FWD(4, float); else RA_FWD(1, float);
    }
#undef RA_FWD
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t nrv_reattn_softmax_bwd_workspace(int B, int H, int Nq, int Nk) {
    if (!th_shape_ok(B, H, Nq, Nk)) return 0;
    return ra_part_bytes((long long)B * Nq, H);
}

extern "C" int nrv_reattn_softmax_bwd(const float* dA, const float* P, const float* W, const float* gamma, float* dS, float* dW,
                                      float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, int B, int H, int Nq,
                                      int Nk, float eps, void* stream) {
    if (!dA || !P || !W || !gamma || !dS || !dW || !dgamma || !dbeta || !workspace) return NRV_ERR_NULL;
    if (!ra_shape_ok(B, H, Nq, Nk, eps)) return NRV_ERR_SHAPE;
    if (!nrv_aligned16(dA) || !nrv_aligned16(P) || !nrv_aligned16(dS) || !nrv_aligned16(workspace)) return NRV_ERR_ALIGN;
    if (workspace_bytes < nrv_reattn_softmax_bwd_workspace(B, H, Nq, Nk)) return NRV_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long rows = (long long)B * Nq;
    const int parts = th_parts(rows);
    const size_t lds = ((size_t)2 * H * th_ld(Nk) + 2 * TH_THREADS) * 4;
    double* part = static_cast<double*>(workspace);
#define RA_BWD(V)                                                                                                       \
    do {                                                                                                                \
        static int attr = th_lds_attr(ra_softmax_bwd_kernel<V>, TH_LDS_MAX);                                            \
        if (attr) return attr;                                                                                          \
        hipLaunchKernelGGL((ra_softmax_bwd_kernel<V>), dim3(parts), dim3(TH_THREADS), lds, st, dA, P, W, gamma, dS, part, H, Nq, Nk, rows, eps); \
    } while (0)
    if (Nk % 4 == 0) RA_BWD(4); else RA_BWD(1);
#undef RA_BWD
    NRV_CHECK_LAUNCH();
    hipLaunchKernelGGL(ra_reduce_kernel, dim3((unsigned)nrv_cdiv(H * H + 2 * H, 64)), dim3(64), 0, st, part, parts, H, dW, dgamma, dbeta);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nrv_reattn_norm_fwd(const float* P, const float* W, const float* gamma, const float* beta, void* A, int a_dtype,
                                   int B, int H, int Nq, int Nk, float eps, void* stream) {
    if (!P || !W || !gamma || !beta || !A) return NRV_ERR_NULL;
    if (a_dtype != NRV_F32 && a_dtype != NRV_BF16) return NRV_ERR_DTYPE;
    if (!ra_shape_ok(B, H, Nq, Nk, eps)) return NRV_ERR_SHAPE;
    if (!nrv_aligned16(P) || !nrv_aligned16(A)) return NRV_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long M = (long long)Nq * Nk;
    const int V = M % 4 == 0 ? 4 : 1;
    const long long items = (long long)B * (M / V);
    const long long blocks = nrv_cdiv(items, TH_THREADS);
    const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536));
#define RA_NORM(V_, AT) hipLaunchKernelGGL((ra_norm_fwd_kernel<V_, AT>), grid, dim3(TH_THREADS), 0, st, P, W, gamma, beta, static_cast<AT*>(A), H, M, items, eps)
    if (a_dtype == NRV_BF16) {
        if (V == 4) RA_NORM(4, bf16_t); else RA_NORM(1, bf16_t);
    } else {
        if (V == 4) RA_NORM(4, float); else RA_NORM(1, float);
    }
#undef RA_NORM
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t nrv_reattn_norm_bwd_workspace(int B, int H, int Nq, int Nk) {
    if (!th_shape_ok(B, H, Nq, Nk)) return 0;
    return ra_part_bytes((long long)B * nrv_cdiv((long long)Nq * Nk, TH_TILE), H);
}

extern "C" int nrv_reattn_norm_bwd(const float* dA, const float* P, const float* W, const float* gamma, float* dP, float* dW,
                                   float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, int B, int H, int Nq,
                                   int Nk, float eps, void* stream) {
    if (!dA || !P || !W || !gamma || !dP || !dW || !dgamma || !dbeta || !workspace) return NRV_ERR_NULL;
    if (!ra_shape_ok(B, H, Nq, Nk, eps)) return NRV_ERR_SHAPE;
    if (!nrv_aligned16(dA) || !nrv_aligned16(P) || !nrv_aligned16(dP) || !nrv_aligned16(workspace)) return NRV_ERR_ALIGN;
    if (workspace_bytes < nrv_reattn_norm_bwd_workspace(B, H, Nq, Nk)) return NRV_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long M = (long long)Nq * Nk;
    const long long tiles_per_b = nrv_cdiv(M, TH_TILE), tiles = B * tiles_per_b;
    const int parts = th_parts(tiles);
    const size_t lds = ((size_t)2 * H * th_ld(TH_TILE) + 2 * TH_THREADS) * 4;
    double* part = static_cast<double*>(workspace);
#define RA_NORMB(V)                                                                                                     \
    do {                                                                                                                \
        static int attr = th_lds_attr(ra_norm_bwd_kernel<V>, TH_LDS_MAX);                                               \
        if (attr) return attr;                                                                                          \
        hipLaunchKernelGGL((ra_norm_bwd_kernel<V>), dim3(parts), dim3(TH_THREADS), lds, st, dA, P, W, gamma, dP, part, H, M, tiles_per_b, tiles, eps); \
    } while (0)
    if (M % 4 == 0) RA_NORMB(4); else RA_NORMB(1);
#undef RA_NORMB
    NRV_CHECK_LAUNCH();
    hipLaunchKernelGGL(ra_reduce_kernel, dim3((unsigned)nrv_cdiv(H * H + 2 * H, 64)), dim3(64), 0, st, part, parts, H, dW, dgamma, dbeta);
    NRV_CHECK_LAUNCH();
    return 0;
}
