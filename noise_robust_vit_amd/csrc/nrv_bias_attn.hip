// LeViT attention with a learned, offset-indexed bias (levit.py:198-281 Attention, :298-403 AttentionSubsample, between the
// Linear_BN projections): S = scale q k^T + table[h, idx[i, j]], softmax or Sinkhorn (softmax, 3 x (row /, column /), row /),
// O = P V, and the Hardswish of the proj branch (levit.py:229-232) applied on the store -- one kernel per direction.
//
// Work split: one workgroup of 256 threads per (sample, head); thread i owns query row i (i < Nq), thread j owns key column j
// (j < Nk) in the column steps.  The score / probability matrix lives in LDS as fp32 [Nq][Nk + 1] (the odd row stride keeps row
// walks and column walks free of bank conflicts): P0 is never rounded to 16 bits, so the probabilities of keys whose scores sit
// tens of nats below a row's maximum -- routine with a learned bias -- keep their relative precision through the Sinkhorn
// rescalings and into the gradients of those keys.  Q / K / V rows are read from the projection outputs through a row stride and
// a per-head column offset (the interleaved [q | k | v] head groups of Attention, the separate q and [k | v] buffers of
// AttentionSubsample); every (sample, head) reads its K / V rows from L2 with all lanes of a wave on the same address.
//   forward : P0 = softmax(S) in LDS; Sinkhorn scalings a_t = 1 / (P0 b_{t-1}), b_t = 1 / (P0^T a_t) (t = 1..3, b_0 = 1), a_4;
//             O = diag(a4) P0 diag(b3) V.  Saved per (sample, head): lse [Nq], and for Sinkhorn a1..a4 [4][Nq], b1..b3 [3][Nk].
//   backward: dO = dA * Hardswish'(O); the LDS matrix holds dP = dO V^T and is walked back through the Sinkhorn steps (row steps
//             in-thread, column steps through a column sum); P0 is recomputed from the scores and lse where a step needs it.
//             dS = P0 (G - rowsum(G P0)); dQ in the row threads, dK = scale dS^T Q and dV = P^T dO in the column threads.
//             The table gradient folds dS through the inverse index (a CSR list of the (i, j) of every table entry, built by the
//             host once per geometry) into one partial per (head, entry, sample); reduce_partials_kernel (nrv_rows.hpp) sums the
//             partials of an entry over the samples in a fixed order.  No atomics: reruns are bit-identical.
// Nothing [B, H, Nq, Nk]-sized reaches HBM.  The row helpers (load_row / dot_row / axpy_row / store_row) and Hardswish are those of
// nrv_rows.hpp.
#include "nrv_rows.hpp"

#include <cmath>

namespace {

constexpr int BA_THREADS = 256;
constexpr int BA_NMAX = 256;                     // Nk (and so Nq) at most: one thread per key column
constexpr int BA_TMAX = 256;                     // table entries per head at most
constexpr int BA_LDS_BYTES = 160 * 1024;
constexpr int BA_FWD_EXTRA = 3 * BA_NMAX;        // floats beside the matrix: sa, sb, table column
constexpr int BA_BWD_EXTRA = 6 * BA_NMAX;        // column sum, b_0..b_3, table column

struct BiasParams {
    const bf16_t* q;
    const bf16_t* k;
    const bf16_t* v;
    long long ldq, ldk, ldv;     // row strides (elements); the gradients use the same layouts
    int hq, hk, hv;              // per-head column offsets
    const float* table;          // [H, T]
    const int* idx;              // [Nq, Nk]
    const int* inv_ptr;          // [T + 1]
    const int* inv_pos;          // [Nq * Nk]: flat i * Nk + j, grouped by entry
    bf16_t* o;                   // [B * Nq, H * DV]
    bf16_t* ao;                  // hardswish(o), same layout
    float* stats;                // [B * H, SZ]
    const bf16_t* da;            // bwd: gradient of hardswish(o)
    const bf16_t* os;            // bwd: the saved o
    bf16_t* dq;
    bf16_t* dk;
    bf16_t* dv;
    float* part;                 // [H, T, B]
    int B, H, Nq, Nk, T, SZ, lds_ld;
    float scale;
};

// 8 consecutive elements of a dO row = dA * Hardswish'(O) (the proj branch's activation, levit.py:229-232)
__device__ __forceinline__ void load_do8(const bf16_t* da, const bf16_t* o, float (&r)[8]) {
    const u32x4_t a = *reinterpret_cast<const u32x4_t*>(da);
    const u32x4_t ov = *reinterpret_cast<const u32x4_t*>(o);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        r[2 * e] = bf16lo_to_f32(a[e]) * hardswish_grad(bf16lo_to_f32(ov[e]));
        r[2 * e + 1] = bf16hi_to_f32(a[e]) * hardswish_grad(bf16hi_to_f32(ov[e]));
    }
}

template <int N>
__device__ __forceinline__ void load_do(const bf16_t* da, const bf16_t* o, float (&r)[N]) {
#pragma unroll
    for (int c = 0; c < N / 8; ++c) {
        float t[8];
        load_do8(da + c * 8, o + c * 8, t);
#pragma unroll
        for (int e = 0; e < 8; ++e) r[c * 8 + e] = t[e];
    }
}

// acc += w * dO row
template <int N>
__device__ __forceinline__ void axpy_do(float w, const bf16_t* da, const bf16_t* o, float (&acc)[N]) {
#pragma unroll
    for (int c = 0; c < N / 8; ++c) {
        float t[8];
        load_do8(da + c * 8, o + c * 8, t);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[c * 8 + e] = fmaf(w, t[e], acc[c * 8 + e]);
    }
}

template <int KD>
__device__ __forceinline__ void load_q_scaled(const BiasParams& p, int b, int h, int i, float (&q)[KD]) {
    load_row<KD>(p.q + ((long long)b * p.Nq + i) * p.ldq + (long long)h * p.hq, q);
#pragma unroll
    for (int d = 0; d < KD; ++d) q[d] *= p.scale;
}

// score of query i (q = scale q_i) against key j, whose row is krow
template <int KD>
__device__ __forceinline__ float score(const BiasParams& p, const float (&q)[KD], const bf16_t* krow, int i, int j, const float* stab) {
    return dot_row<KD>(q, krow) + stab[min((unsigned)p.idx[(long long)i * p.Nk + j], (unsigned)(p.T - 1))];
}

// ---------------------------------------------------------------------------------------------------------------------------
// forward: blockIdx.x = b * H + h
// ---------------------------------------------------------------------------------------------------------------------------
template <int KD, int DV, bool ROBUST>
__global__ __launch_bounds__(BA_THREADS) void battn_fwd_kernel(BiasParams p) {
    extern __shared__ float lds[];
    const int Nq = p.Nq, Nk = p.Nk, ld = p.lds_ld;
    float* sS = lds;
    float* sa = lds + Nq * ld;
    float* sb = sa + BA_NMAX;
    float* stab = sb + BA_NMAX;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.H, h = blockIdx.x - (blockIdx.x / p.H) * p.H;
    for (int t = tid; t < p.T; t += BA_THREADS) stab[t] = p.table[(long long)h * p.T + t];
    __syncthreads();
    const bool rowv = tid < Nq;
    const int i = rowv ? tid : 0;
    float* st = p.stats + ((long long)b * p.H + h) * p.SZ;
    const bf16_t* kb = p.k + (long long)b * Nk * p.ldk + (long long)h * p.hk;
    const bf16_t* vb = p.v + (long long)b * Nk * p.ldv + (long long)h * p.hv;
    float* srow = sS + i * ld;
    if (rowv) {
        float q[KD];
        load_q_scaled<KD>(p, b, h, i, q);
        float m = -INFINITY;
        for (int j = 0; j < Nk; ++j) {
            const float s = score<KD>(p, q, kb + j * p.ldk, i, j, stab);
            srow[j] = s;
            m = fmaxf(m, s);
        }
        float l = 0.f;
        for (int j = 0; j < Nk; ++j) {
            const float e = __expf(srow[j] - m);
            srow[j] = e;
            l += e;
        }
        const float rl = 1.0f / l;
        for (int j = 0; j < Nk; ++j) srow[j] *= rl;                  // P0 = softmax(S)
        st[i] = m + __logf(l);
    }
    float a = 1.f;
    if constexpr (ROBUST) {
        sb[tid] = 1.f;                                                // b_0
        __syncthreads();
        for (int t = 1; t <= 3; ++t) {
            if (rowv) {
                float r = 0.f;
                for (int j = 0; j < Nk; ++j) r += srow[j] * sb[j];
                a = 1.0f / r;
                st[t * Nq + i] = a;
                sa[i] = a;
            }
            __syncthreads();                                          // a_t visible; every row thread has read sb
            float bn = 0.f;
            if (tid < Nk) {
                float cs = 0.f;
                for (int k = 0; k < Nq; ++k) cs += sa[k] * sS[k * ld + tid];
                bn = 1.0f / cs;
                st[5 * Nq + (t - 1) * Nk + tid] = bn;
            }
            __syncthreads();                                          // every column thread has read sa
            sb[tid] = bn;
            __syncthreads();
        }
        if (rowv) {
            float r = 0.f;
            for (int j = 0; j < Nk; ++j) r += srow[j] * sb[j];
            a = 1.0f / r;                                             // a4
            st[4 * Nq + i] = a;
        }
    }
    if (rowv) {
        float o[DV];
#pragma unroll
        for (int d = 0; d < DV; ++d) o[d] = 0.f;
        for (int j = 0; j < Nk; ++j) {
            float w = srow[j];
            if constexpr (ROBUST) w *= sb[j];                         // P0 diag(b3); diag(a4) below
            axpy_row<DV>(w, vb + j * p.ldv, o);
        }
#pragma unroll
        for (int d = 0; d < DV; ++d) o[d] *= a;
        const long long orow = ((long long)b * Nq + i) * p.H * DV + (long long)h * DV;
        store_row<DV>(p.o + orow, o, 1.f);
        float ho[DV];
#pragma unroll
        for (int d = 0; d < DV; ++d) ho[d] = hardswish(o[d]);
        store_row<DV>(p.ao + orow, ho, 1.f);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward: blockIdx.x = b * H + h.  sD = dP, walked back to dS.
// ---------------------------------------------------------------------------------------------------------------------------
template <int KD, int DV, bool ROBUST>
__global__ __launch_bounds__(BA_THREADS) void battn_bwd_kernel(BiasParams p) {
    extern __shared__ float lds[];
    const int Nq = p.Nq, Nk = p.Nk, ld = p.lds_ld;
    float* sD = lds;
    float* shv = lds + Nq * ld;
    float* sbt = shv + BA_NMAX;          // [4][BA_NMAX]: b_0 (= 1) .. b_3 of every key
    float* stab = sbt + 4 * BA_NMAX;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.H, h = blockIdx.x - (blockIdx.x / p.H) * p.H;
    const float* st = p.stats + ((long long)b * p.H + h) * p.SZ;
    for (int t = tid; t < p.T; t += BA_THREADS) stab[t] = p.table[(long long)h * p.T + t];
    sbt[tid] = 1.f;
#pragma unroll
    for (int t = 1; t <= 3; ++t) sbt[t * BA_NMAX + tid] = (ROBUST && tid < Nk) ? st[5 * Nq + (t - 1) * Nk + tid] : 1.f;
    __syncthreads();
    const bool rowv = tid < Nq, colv = tid < Nk;
    const int i = rowv ? tid : 0;
    const int jc = colv ? tid : 0;
    const bf16_t* kb = p.k + (long long)b * Nk * p.ldk + (long long)h * p.hk;
    const bf16_t* vb = p.v + (long long)b * Nk * p.ldv + (long long)h * p.hv;
    const bf16_t* dab = p.da + (long long)b * Nq * p.H * DV + (long long)h * DV;
    const bf16_t* ob = p.os + (long long)b * Nq * p.H * DV + (long long)h * DV;
    float* drow = sD + i * ld;
    float q[KD];                          // row threads: scale q_i
    load_q_scaled<KD>(p, b, h, i, q);
    const float lse = st[i];
    float kj[KD];                         // column threads: k_j
    load_row<KD>(kb + (long long)jc * p.ldk, kj);

    // P0[i][j] of the row thread / P0[k][jc] of the column thread, recomputed from the scores and lse
    auto p0_row = [&](int j) { return __expf(score<KD>(p, q, kb + j * p.ldk, i, j, stab) - lse); };
    auto p0_col = [&](int k, float (&qk)[KD]) {
        load_q_scaled<KD>(p, b, h, k, qk);
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < KD; ++d) s = fmaf(qk[d], kj[d], s);
        return __expf(s + stab[min((unsigned)p.idx[(long long)k * Nk + jc], (unsigned)(p.T - 1))] - st[k]);
    };

    if (rowv) {
        float dov[DV];
        load_do<DV>(dab + (long long)i * p.H * DV, ob + (long long)i * p.H * DV, dov);
        for (int j = 0; j < Nk; ++j) drow[j] = dot_row<DV>(dov, vb + j * p.ldv);
    }
    if constexpr (ROBUST) {
        if (rowv) {
            // final row normalisation: output diag(a4) P0 diag(b3), input diag(a3) P0 diag(b3)
            const float a4 = st[4 * Nq + i], a3 = st[3 * Nq + i];
            float r = 0.f;
            for (int j = 0; j < Nk; ++j) r += drow[j] * p0_row(j) * sbt[3 * BA_NMAX + j];
            r *= a4;
            for (int j = 0; j < Nk; ++j) drow[j] = (drow[j] - r) * (a4 / a3);
        }
        for (int t = 3; t >= 1; --t) {
            // column step t: output diag(a_t) P0 diag(b_t), input diag(a_t) P0 diag(b_{t-1})
            __syncthreads();
            if (colv) {
                float hs = 0.f, qk[KD];
                for (int k = 0; k < Nq; ++k) hs += sD[k * ld + jc] * (st[t * Nq + k] * p0_col(k, qk));
                shv[jc] = hs * sbt[t * BA_NMAX + jc];
            }
            __syncthreads();
            if (rowv) {
                // row step t: output diag(a_t) P0 diag(b_{t-1}), input diag(a_{t-1}) P0 diag(b_{t-1})
                const float at = st[t * Nq + i], ap = t > 1 ? st[(t - 1) * Nq + i] : 1.f;
                float r = 0.f;
                for (int j = 0; j < Nk; ++j) {
                    const float g = (drow[j] - shv[j]) * (sbt[t * BA_NMAX + j] / sbt[(t - 1) * BA_NMAX + j]);
                    drow[j] = g;
                    r += g * p0_row(j) * sbt[(t - 1) * BA_NMAX + j];
                }
                r *= at;
                for (int j = 0; j < Nk; ++j) drow[j] = (drow[j] - r) * (at / ap);
            }
        }
    }
    // softmax backward dS = P0 (G - rowsum(G P0)); dQ = scale dS K
    if (rowv) {
        float r = 0.f;
        for (int j = 0; j < Nk; ++j) r += drow[j] * p0_row(j);
        float dq[KD];
#pragma unroll
        for (int d = 0; d < KD; ++d) dq[d] = 0.f;
        for (int j = 0; j < Nk; ++j) {
            const float ds = p0_row(j) * (drow[j] - r);
            drow[j] = ds;
            axpy_row<KD>(ds, kb + j * p.ldk, dq);
        }
        store_row<KD>(p.dq + ((long long)b * Nq + i) * p.ldq + (long long)h * p.hq, dq, p.scale);
    }
    __syncthreads();
    // dK_j = scale dS^T Q, dV_j = P^T dO (P = diag(a4) P0 diag(b3) for Sinkhorn)
    if (colv) {
        float dk[KD], dv[DV];
#pragma unroll
        for (int d = 0; d < KD; ++d) dk[d] = 0.f;
#pragma unroll
        for (int d = 0; d < DV; ++d) dv[d] = 0.f;
        const float b3 = sbt[3 * BA_NMAX + jc];
        for (int k = 0; k < Nq; ++k) {
            float qk[KD];
            float pk = p0_col(k, qk);
            if constexpr (ROBUST) pk *= st[4 * Nq + k] * b3;
            const float ds = sD[k * ld + jc];
#pragma unroll
            for (int d = 0; d < KD; ++d) dk[d] = fmaf(ds, qk[d], dk[d]);      // qk = scale q_k: dK = dS^T (scale Q)
            axpy_do<DV>(pk, dab + (long long)k * p.H * DV, ob + (long long)k * p.H * DV, dv);
        }
        store_row<KD>(p.dk + ((long long)b * Nk + jc) * p.ldk + (long long)h * p.hk, dk, 1.f);
        store_row<DV>(p.dv + ((long long)b * Nk + jc) * p.ldv + (long long)h * p.hv, dv, 1.f);
    }
    // table gradient of this (sample, head): entry t collects dS over its (i, j) list
    for (int t = tid; t < p.T; t += BA_THREADS) {
        float acc = 0.f;
        const int npos = Nq * Nk;
        const int e0 = min(max(p.inv_ptr[t], 0), npos), e1 = min(max(p.inv_ptr[t + 1], e0), npos);
        for (int e = e0; e < e1; ++e) {
            const int pos = (int)min((unsigned)p.inv_pos[e], (unsigned)(Nq * Nk - 1));
            const int qi = pos / Nk;
            acc += sD[qi * ld + (pos - qi * Nk)];
        }
        p.part[((long long)h * p.T + t) * p.B + b] = acc;
    }
}

size_t lds_bytes(int Nq, int Nk, bool bwd) {
    return ((size_t)Nq * (Nk + 1) + (bwd ? BA_BWD_EXTRA : BA_FWD_EXTRA)) * sizeof(float);
}

int setup(BiasParams& p, int B, int H, int Nq, int Nk, int kd, int dv, int T, int robust) {
    if (B <= 0 || H <= 0 || Nq <= 0 || Nk <= 0 || T <= 0) return NRV_ERR_SHAPE;
    if (Nq > Nk || Nk > BA_NMAX || T > BA_TMAX) return NRV_ERR_SHAPE;
    if (kd != 16 && kd != 32) return NRV_ERR_SHAPE;
    if (dv != 32 && dv != 64 && dv != 128) return NRV_ERR_SHAPE;
    if (robust != 0 && robust != 1) return NRV_ERR_SHAPE;
    if (lds_bytes(Nq, Nk, true) > (size_t)BA_LDS_BYTES) return NRV_ERR_SHAPE;
    if ((long long)B * H > 0x7fffffffll) return NRV_ERR_SHAPE;
    p.B = B; p.H = H; p.Nq = Nq; p.Nk = Nk; p.T = T;
    p.SZ = robust ? 5 * Nq + 3 * Nk : Nq;
    p.lds_ld = Nk + 1;
    p.scale = (float)(1.0 / std::sqrt((double)kd));
    return 0;
}

int check_operands(const void* q, int64_t ldq, int hq, const void* k, int64_t ldk, int hk, const void* v, int64_t ldv, int hv,
                   int H, int kd, int dv) {
    if (!q || !k || !v) return NRV_ERR_NULL;
    if ((ldq | ldk | ldv | hq | hk | hv) & 7) return NRV_ERR_ALIGN;
    if (hq < 0 || hk < 0 || hv < 0) return NRV_ERR_SHAPE;
    if ((int64_t)(H - 1) * hq + kd > ldq || (int64_t)(H - 1) * hk + kd > ldk || (int64_t)(H - 1) * hv + dv > ldv) return NRV_ERR_SHAPE;
    if (!nrv_aligned16(q) || !nrv_aligned16(k) || !nrv_aligned16(v)) return NRV_ERR_ALIGN;
    return 0;
}

template <int KD, int DV, bool R>
int launch_fwd(const BiasParams& p, hipStream_t s) {
    const size_t lds = lds_bytes(p.Nq, p.Nk, false);
    static int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(battn_fwd_kernel<KD, DV, R>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, BA_LDS_BYTES);
    if (attr) return attr;
    hipLaunchKernelGGL((battn_fwd_kernel<KD, DV, R>), dim3((unsigned)(p.B * p.H)), dim3(BA_THREADS), lds, s, p);
    NRV_CHECK_LAUNCH();
    return 0;
}

template <int KD, int DV, bool R>
int launch_bwd(const BiasParams& p, float* dtable, hipStream_t s) {
    const size_t lds = lds_bytes(p.Nq, p.Nk, true);
    static int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(battn_bwd_kernel<KD, DV, R>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, BA_LDS_BYTES);
    if (attr) return attr;
    hipLaunchKernelGGL((battn_bwd_kernel<KD, DV, R>), dim3((unsigned)(p.B * p.H)), dim3(BA_THREADS), lds, s, p);
    NRV_CHECK_LAUNCH();
    // dtable[h, t] = sum over the samples of part[h, t, b]
    hipLaunchKernelGGL((reduce_partials_kernel<256>), dim3((unsigned)(p.H * p.T)), dim3(256), 0, s, p.part, dtable, p.B, 1ll, 0ll);
    NRV_CHECK_LAUNCH();
    return 0;
}

template <bool BWD>
int dispatch(const BiasParams& p, int kd, int dv, int robust, float* dtable, hipStream_t s) {
#define NRV_BA_CASE(KD_, DV_)                                                                                           \
    if (kd == KD_ && dv == DV_) {                                                                                     \
        if (BWD) return robust ? launch_bwd<KD_, DV_, true>(p, dtable, s) : launch_bwd<KD_, DV_, false>(p, dtable, s); \
        return robust ? launch_fwd<KD_, DV_, true>(p, s) : launch_fwd<KD_, DV_, false>(p, s);                         \
    }
    NRV_BA_CASE(16, 32)
    NRV_BA_CASE(16, 64)
    NRV_BA_CASE(16, 128)
    NRV_BA_CASE(32, 32)
    NRV_BA_CASE(32, 64)
    NRV_BA_CASE(32, 128)
#undef NRV_BA_CASE
    return NRV_ERR_SHAPE;
}

}  // namespace

extern "C" size_t nrv_bias_attn_stats_size(int Nq, int Nk, int robust) {
    if (Nq <= 0 || Nk <= 0) return 0;
    return (size_t)(robust ? 5 * Nq + 3 * Nk : Nq);
}

extern "C" int nrv_bias_attn_fwd(const void* q, int64_t ldq, int hq, const void* k, int64_t ldk, int hk,
                                 const void* v, int64_t ldv, int hv, const float* table, const int32_t* idx,
                                 void* out_bf16, void* act_bf16, float* stats,
                                 int B, int heads, int Nq, int Nk, int kd, int dv, int n_offsets, int robust, void* stream) {
    BiasParams p{};
    int e = setup(p, B, heads, Nq, Nk, kd, dv, n_offsets, robust);
    if (e) return e;
    e = check_operands(q, ldq, hq, k, ldk, hk, v, ldv, hv, heads, kd, dv);
    if (e) return e;
    if (!table || !idx || !out_bf16 || !act_bf16 || !stats) return NRV_ERR_NULL;
    if (!nrv_aligned16(out_bf16) || !nrv_aligned16(act_bf16) || (reinterpret_cast<uintptr_t>(stats) & 3u) ||
        (reinterpret_cast<uintptr_t>(table) & 3u) || (reinterpret_cast<uintptr_t>(idx) & 3u))
        return NRV_ERR_ALIGN;
    p.q = static_cast<const bf16_t*>(q); p.k = static_cast<const bf16_t*>(k); p.v = static_cast<const bf16_t*>(v);
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.hq = hq; p.hk = hk; p.hv = hv;
    p.table = table;
    p.idx = idx;
    p.o = static_cast<bf16_t*>(out_bf16);
    p.ao = static_cast<bf16_t*>(act_bf16);
    p.stats = stats;
    return dispatch<false>(p, kd, dv, robust, nullptr, static_cast<hipStream_t>(stream));
}

extern "C" size_t nrv_bias_attn_bwd_workspace(int B, int heads, int n_offsets) {
    if (B <= 0 || heads <= 0 || n_offsets <= 0) return 0;
    return (size_t)B * heads * n_offsets * sizeof(float);
}

extern "C" int nrv_bias_attn_bwd(const void* q, int64_t ldq, int hq, const void* k, int64_t ldk, int hk,
                                 const void* v, int64_t ldv, int hv, const float* table, const int32_t* idx,
                                 const int32_t* inv_ptr, const int32_t* inv_pos,
                                 const void* out_bf16, const void* dact_bf16, const float* stats,
                                 void* dq, void* dk, void* dv_out, float* dtable, void* workspace, size_t workspace_bytes,
                                 int B, int heads, int Nq, int Nk, int kd, int dv, int n_offsets, int robust, void* stream) {
    BiasParams p{};
    int e = setup(p, B, heads, Nq, Nk, kd, dv, n_offsets, robust);
    if (e) return e;
    e = check_operands(q, ldq, hq, k, ldk, hk, v, ldv, hv, heads, kd, dv);
    if (e) return e;
    e = check_operands(dq, ldq, hq, dk, ldk, hk, dv_out, ldv, hv, heads, kd, dv);
    if (e) return e;
    if (!table || !idx || !inv_ptr || !inv_pos || !out_bf16 || !dact_bf16 || !stats || !dtable || !workspace) return NRV_ERR_NULL;
    if (workspace_bytes < nrv_bias_attn_bwd_workspace(B, heads, n_offsets)) return NRV_ERR_WORKSPACE;
    if (!nrv_aligned16(out_bf16) || !nrv_aligned16(dact_bf16) || (reinterpret_cast<uintptr_t>(stats) & 3u) ||
        (reinterpret_cast<uintptr_t>(table) & 3u) || (reinterpret_cast<uintptr_t>(idx) & 3u) ||
        (reinterpret_cast<uintptr_t>(inv_ptr) & 3u) || (reinterpret_cast<uintptr_t>(inv_pos) & 3u) ||
        (reinterpret_cast<uintptr_t>(dtable) & 3u) || (reinterpret_cast<uintptr_t>(workspace) & 3u))
        return NRV_ERR_ALIGN;
    p.q = static_cast<const bf16_t*>(q); p.k = static_cast<const bf16_t*>(k); p.v = static_cast<const bf16_t*>(v);
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.hq = hq; p.hk = hk; p.hv = hv;
    p.table = table;
    p.idx = idx;
    p.inv_ptr = inv_ptr;
    p.inv_pos = inv_pos;
    p.os = static_cast<const bf16_t*>(out_bf16);
    p.da = static_cast<const bf16_t*>(dact_bf16);
    p.stats = const_cast<float*>(stats);
    p.dq = static_cast<bf16_t*>(dq); p.dk = static_cast<bf16_t*>(dk); p.dv = static_cast<bf16_t*>(dv_out);
    p.part = static_cast<float*>(workspace);
    return dispatch<true>(p, kd, dv, robust, dtable, static_cast<hipStream_t>(stream));
}
