// Talking-heads attention on materialised matrices [B, H, Nq, Nk] (gfx950): CaiT's head mixing before and after the
// normalisation (cait.py:107-118).  S = scaled scores, W1 = mix_heads_pre_attn, W2 = mix_heads_post_attn ([h, g], fp32):
//     T[b,g] = sum_h W1[h,g] S[b,h]      P = softmax(T) (or Sinkhorn(T), nrv_sinkhorn_fwd)      A[b,g] = sum_h W2[h,g] P[b,h]
//
// Dtypes in memory: S, P, dA, dS fp32; A fp32 or bf16 (the caller's choice -- nrv_bgemm rounds its operands to bf16 when it
// stages them, so a bf16 A costs the model nothing and halves that stream).  Kept for the backward per layer: S and P in
// fp32 and A in bf16, 10 bytes per element of [B, H, Nq, Nk].
//
//   nrv_th_softmax_fwd   one workgroup per query row (b, i) holds the row of ALL heads in LDS (H * Nk fp32, 66 KB at 16 x 1025):
//                        S is read once, T lives only in LDS, P and A are written once.
//   nrv_th_softmax_bwd   the same row ownership with two LDS images (dA -> dP -> dT in place; P, then S).  A workgroup walks
//                        rows wg, wg + grid, ... and keeps its share of dW1 / dW2 in registers: thread (h, g, split) sums
//                        x[h, j] y[g, j] over its j (fp32 per row, double across rows).  One set of 2 H H sums per workgroup goes to the workspace and a
//                        second kernel adds the sets in index order.
//   nrv_head_mix_fwd/bwd the mixing alone, on flat positions p = i * Nk + j (the robust path runs nrv_sinkhorn_fwd / bwd between
//                        two of them); the backward stages 512-position tiles in LDS for the same (h, g, split) sums.
//
// Accesses along j are 16-byte vectors when Nk % 4 == 0 (Nq * Nk % 4 == 0 for the flat kernels) and coalesced dwords otherwise:
// rows of 197 or 577 floats do not start on 16-byte boundaries.  The H x H matrices are read with wave-uniform indices (scalar
// loads).  Plain C++, vector stores only, no atomics: reruns are bit-identical.
#include "nrv_heads.hpp"

namespace {

template <int V, class AT>
__global__ __launch_bounds__(TH_THREADS) void th_softmax_fwd_kernel(const float* __restrict__ S, const float* __restrict__ W1,
                                                                    const float* __restrict__ W2, float* __restrict__ P,
                                                                    AT* __restrict__ A, int H, int Nq, int Nk) {
    const int ld = th_ld(Nk);
    float* sT = th_smem;
    const long long row = blockIdx.x;                          // b * Nq + i
    const long long b = row / Nq, i = row - b * Nq;
    const long long hstride = (long long)Nq * Nk;
    const long long base = (b * H * Nq + i) * Nk;              // head 0 of this row
    th_load<V>(sT, ld, S + base, hstride, H, Nk);
    __syncthreads();
    th_mix<V, false>(sT, ld, W1, H, Nk, [](int, int, const float (&)[V]) {},
                     [&](int g, int p, const float (&t)[V]) { stv<V>(sT + g * ld + p, t); });
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int g = threadIdx.x >> 6; g < H; g += TH_THREADS / 64) {
        float* r = sT + g * ld;
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
    th_mix<V, false>(sT, ld, W2, H, Nk, [&](int h, int p, const float (&x)[V]) { stv<V>(P + base + h * hstride + p, x); },
                     [&](int g, int p, const float (&a)[V]) { stv<V>(A + base + g * hstride + p, a); });
}

template <int V>
__global__ __launch_bounds__(TH_THREADS) void th_softmax_bwd_kernel(const float* __restrict__ dA, const float* __restrict__ P,
                                                                    const float* __restrict__ S, const float* __restrict__ W1,
                                                                    const float* __restrict__ W2, float* __restrict__ dS,
                                                                    double* __restrict__ part, int H, int Nq, int Nk, long long rows) {
    const int ld = th_ld(Nk);
    double* red = reinterpret_cast<double*>(th_smem);          // TH_THREADS doubles for the final sums
    float* sD = th_smem + 2 * TH_THREADS;                      // dA, then dP, then dT
    float* sP = sD + H * ld;                                   // P, then S
    const long long hstride = (long long)Nq * Nk;
    const int lane = threadIdx.x & 63;
    double acc1 = 0.0, acc2 = 0.0;
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const long long b = row / Nq, i = row - b * Nq;
        const long long base = (b * H * Nq + i) * Nk;
        __syncthreads();                                       // the previous row's images are done with
        th_load<V>(sD, ld, dA + base, hstride, H, Nk);
        th_load<V>(sP, ld, P + base, hstride, H, Nk);
        __syncthreads();
        acc2 += (double)th_pairs(sP, sD, ld, H, Nk);             // dW2[h,g] += P[h] . dA[g]
        __syncthreads();
        th_mix<V, true>(sD, ld, W2, H, Nk, [](int, int, const float (&)[V]) {},
                        [&](int h, int p, const float (&d)[V]) { stv<V>(sD + h * ld + p, d); });      // dP[h] = sum_g W2[h,g] dA[g]
        __syncthreads();
        for (int h = threadIdx.x >> 6; h < H; h += TH_THREADS / 64) {
            float* d = sD + h * ld;
            const float* pr = sP + h * ld;
            float dot = 0.f;
            for (int j = lane; j < Nk; j += 64) dot = fmaf(pr[j], d[j], dot);
            dot = wave_sum(dot);
            for (int j = lane; j < Nk; j += 64) d[j] = pr[j] * (d[j] - dot);                           // dT = P (dP - <P, dP>)
        }
        __syncthreads();
        th_load<V>(sP, ld, S + base, hstride, H, Nk);
        __syncthreads();
        acc1 += (double)th_pairs(sP, sD, ld, H, Nk);             // dW1[h,g] += S[h] . dT[g]
        th_mix<V, true>(sD, ld, W1, H, Nk, [](int, int, const float (&)[V]) {},
                        [&](int h, int p, const float (&d)[V]) { stv<V>(dS + base + h * hstride + p, d); });  // dS[h] = sum_g W1[h,g] dT[g]
    }
    double* out = part + (long long)blockIdx.x * 2 * H * H;
    th_pairs_out(red, acc1, H, out);
    th_pairs_out(red, acc2, H, out + H * H);
}

template <int V, class OT>
__global__ __launch_bounds__(TH_THREADS) void head_mix_fwd_kernel(const float* __restrict__ in, const float* __restrict__ W,
                                                                  OT* __restrict__ out, int H, long long M, long long items) {
    // item = (b, group of V positions); heads are M apart
    const long long per = M / V;
    for (long long it = blockIdx.x * (long long)TH_THREADS + threadIdx.x; it < items; it += (long long)gridDim.x * TH_THREADS) {
        const long long b = it / per, p = (it - b * per) * V;
        const float* src = in + b * H * M + p;
        OT* dst = out + b * H * M + p;
        float x[TH_MAXH][V];
#pragma unroll
        for (int h = 0; h < TH_MAXH; ++h)
            if (h < H) ldv<V>(src + h * M, x[h]);
        for (int g = 0; g < H; ++g) {
            float acc[V];
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = 0.f;
#pragma unroll
            for (int h = 0; h < TH_MAXH; ++h)
                if (h < H) {
                    const float w = W[h * H + g];
#pragma unroll
                    for (int v = 0; v < V; ++v) acc[v] = fmaf(w, x[h][v], acc[v]);
                }
            stv<V>(dst + g * M, acc);
        }
    }
}

template <int V>
__global__ __launch_bounds__(TH_THREADS) void head_mix_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ in,
                                                                  const float* __restrict__ W, float* __restrict__ din,
                                                                  double* __restrict__ part, int H, long long M, long long tiles_per_b,
                                                                  long long tiles) {
    const int ld = th_ld(TH_TILE);
    double* red = reinterpret_cast<double*>(th_smem);
    float* sD = th_smem + 2 * TH_THREADS;
    float* sX = sD + H * ld;
    double acc = 0.0;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long b = t / tiles_per_b, p0 = (t - b * tiles_per_b) * TH_TILE;
        const int np = (int)(M - p0 < TH_TILE ? M - p0 : TH_TILE);
        const long long base = b * H * M + p0;
        __syncthreads();
        th_load<V>(sD, ld, dout + base, M, H, np);
        th_load<V>(sX, ld, in + base, M, H, np);
        __syncthreads();
        acc += (double)th_pairs(sX, sD, ld, H, np);             // dW[h,g] += in[h] . dout[g]
        th_mix<V, true>(sD, ld, W, H, np, [](int, int, const float (&)[V]) {},
                        [&](int h, int p, const float (&d)[V]) { stv<V>(din + base + h * M + p, d); });
    }
    th_pairs_out(red, acc, H, part + (long long)blockIdx.x * H * H);
}

}  // namespace

extern "C" int nrv_th_softmax_fwd(const float* S, const float* W1, const float* W2, float* P, void* A, int a_dtype,
                                  int B, int H, int Nq, int Nk, void* stream) {
    if (!S || !W1 || !W2 || !P || !A) return NRV_ERR_NULL;
    if (a_dtype != NRV_F32 && a_dtype != NRV_BF16) return NRV_ERR_DTYPE;
    if (!th_shape_ok(B, H, Nq, Nk)) return NRV_ERR_SHAPE;
    if (!nrv_aligned16(S) || !nrv_aligned16(P) || !nrv_aligned16(A)) return NRV_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t lds = (size_t)H * th_ld(Nk) * 4;
    const dim3 grid((unsigned)((long long)B * Nq)), block(TH_THREADS);
    const bool vec = Nk % 4 == 0;
#define TH_FWD(V, AT)                                                                                                   \
    do {                                                                                                                \
        static int attr = th_lds_attr(th_softmax_fwd_kernel<V, AT>, TH_LDS_MAX);                                        \
        if (attr) return attr;                                                                                          \
        hipLaunchKernelGGL((th_softmax_fwd_kernel<V, AT>), grid, block, lds, st, S, W1, W2, P, static_cast<AT*>(A), H, Nq, Nk); \
    } while (0)
    if (a_dtype == NRV_BF16) {
        if (vec) TH_FWD(4, bf16_t); else TH_FWD(1, bf16_t);
    } else {
        if (vec) TH_FWD(4, float); else TH_FWD(1, float);
    }
#undef TH_FWD
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t nrv_th_softmax_bwd_workspace(int B, int H, int Nq, int Nk) {
    if (!th_shape_ok(B, H, Nq, Nk)) return 0;
    return (size_t)th_parts((long long)B * Nq) * 2 * H * H * 8;
}

extern "C" int nrv_th_softmax_bwd(const float* dA, const float* P, const float* S, const float* W1, const float* W2, float* dS,
                                  float* dW1, float* dW2, void* workspace, size_t workspace_bytes, int B, int H, int Nq, int Nk,
                                  void* stream) {
    if (!dA || !P || !S || !W1 || !W2 || !dS || !dW1 || !dW2 || !workspace) return NRV_ERR_NULL;
    if (!th_shape_ok(B, H, Nq, Nk)) return NRV_ERR_SHAPE;
    if (!nrv_aligned16(dA) || !nrv_aligned16(P) || !nrv_aligned16(S) || !nrv_aligned16(dS) || !nrv_aligned16(workspace)) return NRV_ERR_ALIGN;
    if (workspace_bytes < nrv_th_softmax_bwd_workspace(B, H, Nq, Nk)) return NRV_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long rows = (long long)B * Nq;
    const int parts = th_parts(rows);
    const size_t lds = ((size_t)2 * H * th_ld(Nk) + 2 * TH_THREADS) * 4;
    double* part = static_cast<double*>(workspace);
#define TH_BWD(V)                                                                                                       \
    do {                                                                                                                \
        static int attr = th_lds_attr(th_softmax_bwd_kernel<V>, TH_LDS_MAX);                                            \
        if (attr) return attr;                                                                                          \
        hipLaunchKernelGGL((th_softmax_bwd_kernel<V>), dim3(parts), dim3(TH_THREADS), lds, st, dA, P, S, W1, W2, dS, part, H, Nq, Nk, rows); \
    } while (0)
    if (Nk % 4 == 0) TH_BWD(4); else TH_BWD(1);
#undef TH_BWD
    NRV_CHECK_LAUNCH();
    const int n = 2 * H * H;
    hipLaunchKernelGGL(th_reduce_kernel, dim3((unsigned)nrv_cdiv(n, 64)), dim3(64), 0, st, part, parts, n, H * H, dW1, dW2);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nrv_head_mix_fwd(const float* in, const float* W, void* out, int out_dtype, int B, int H, int Nq, int Nk, void* stream) {
    if (!in || !W || !out) return NRV_ERR_NULL;
    if (out_dtype != NRV_F32 && out_dtype != NRV_BF16) return NRV_ERR_DTYPE;
    if (!th_shape_ok(B, H, Nq, Nk)) return NRV_ERR_SHAPE;
    if (!nrv_aligned16(in) || !nrv_aligned16(out)) return NRV_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long M = (long long)Nq * Nk;
    const int V = M % 4 == 0 ? 4 : 1;
    const long long items = (long long)B * (M / V);
    const long long blocks = nrv_cdiv(items, TH_THREADS);
    const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536));
#define TH_MIX(V_, OT) hipLaunchKernelGGL((head_mix_fwd_kernel<V_, OT>), grid, dim3(TH_THREADS), 0, st, in, W, static_cast<OT*>(out), H, M, items)
    if (out_dtype == NRV_BF16) {
        if (V == 4) TH_MIX(4, bf16_t); else TH_MIX(1, bf16_t);
    } else {
        if (V == 4) TH_MIX(4, float); else TH_MIX(1, float);
    }
#undef TH_MIX
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t nrv_head_mix_bwd_workspace(int B, int H, int Nq, int Nk) {
    if (!th_shape_ok(B, H, Nq, Nk)) return 0;
    const long long tiles = (long long)B * nrv_cdiv((long long)Nq * Nk, TH_TILE);
    return (size_t)th_parts(tiles) * H * H * 8;
}

extern "C" int nrv_head_mix_bwd(const float* dout, const float* in, const float* W, float* din, float* dW, void* workspace,
                                size_t workspace_bytes, int B, int H, int Nq, int Nk, void* stream) {
    if (!dout || !in || !W || !din || !dW || !workspace) return NRV_ERR_NULL;
    if (!th_shape_ok(B, H, Nq, Nk)) return NRV_ERR_SHAPE;
    if (!nrv_aligned16(dout) || !nrv_aligned16(in) || !nrv_aligned16(din) || !nrv_aligned16(workspace)) return NRV_ERR_ALIGN;
    if (workspace_bytes < nrv_head_mix_bwd_workspace(B, H, Nq, Nk)) return NRV_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long M = (long long)Nq * Nk;
    const long long tiles_per_b = nrv_cdiv(M, TH_TILE), tiles = B * tiles_per_b;
    const int parts = th_parts(tiles);
    const size_t lds = ((size_t)2 * H * th_ld(TH_TILE) + 2 * TH_THREADS) * 4;
    double* part = static_cast<double*>(workspace);
#define TH_MIXB(V)                                                                                                      \
    do {                                                                                                                \
        static int attr = th_lds_attr(head_mix_bwd_kernel<V>, TH_LDS_MAX);                                              \
        if (attr) return attr;                                                                                          \
        hipLaunchKernelGGL((head_mix_bwd_kernel<V>), dim3(parts), dim3(TH_THREADS), lds, st, dout, in, W, din, part, H, M, tiles_per_b, tiles); \
    } while (0)
    if (M % 4 == 0) TH_MIXB(4); else TH_MIXB(1);
#undef TH_MIXB
    NRV_CHECK_LAUNCH();
    hipLaunchKernelGGL(th_reduce_kernel, dim3((unsigned)nrv_cdiv(H * H, 64)), dim3(64), 0, st, part, parts, H * H, H * H, dW, dW);
    NRV_CHECK_LAUNCH();
    return 0;
}
