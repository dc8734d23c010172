// Streaming ("flash") softmax attention, one kernel family in two instantiations:
//   MEM = false: the fused multi-head self-attention for the shapes the single-pass kernels of nrv_attn.hip do not hold on
//                chip: any token count N (N > 256: ViT-B/16 at 384 px = 577 tokens after interpolate_embeddings,
//                vit.py:522-603; vit_h_14 = 257 tokens, vit.py:512-519) and head dims 32 / 64 / 80 / 96 / 128 (vit_h_14:
//                1280 / 16 = 80; SimpleViT(dim_head=...), simple_vit.py:101-114).  Keys / values are the N token rows.
//   MEM = true : the attention of the learnable-memory adapter (learnable_memory_vit.py:64-86): keys / values are the Nq token
//                rows followed by M memory rows (Nk = Nq + M), and an optional bit mask removes (query, key) pairs.
// nrv_attn_mem_fwd/bwd run MEM = false when M = 0 and there is no mask: no mask and an all-ones mask run the same arithmetic,
// so the results are bit-identical.
// Numerics contract of nrv_attn.hip: bf16 operands, fp32 MFMA accumulation, fp32 softmax in the exp2 domain, P fed to P.V in
// bf16 and normalised by the fp32 row sum, natural-log LSE.
//
// A workgroup of 4 waves owns 64 queries (forward, dQ) or 64 keys (dK / dV) of one (batch, head) and sweeps the other side
// in tiles of 64 rows staged in LDS; scores never leave the CU.
//   forward : online softmax -- running row max m and row sum l per query, O^T rescaled by exp2(m_old - m_new) per key tile
//   backward: P recomputed from q, k and the saved LSE; query-owner pass (dQ, delta = rowsum(dO * O)) + key-owner pass
//             (dK, dV), no atomics, deterministic
// MFMA orientation as in nrv_attn.hip (16x16x32 bf16): S^T = K Q^T, a lane owns one query column with its keys in
// registers; the bf16 P^T / dS^T accumulators ARE the B operands of O^T = V^T P^T / dQ^T = K^T dS^T (the k slots of a
// 32-key step are keys {4g .. 4g+3, 16+4g .. 16+4g+3} for lane group g in both operands); transposed A operands come from
// ds_read_b64_tr_b16.  The head dim is padded to DHP = 32 KS in LDS and registers (zero columns; dh = 80 -> 96).
//
// Tile image: [64 rows][DHP] bf16, rows of 2 DHP bytes, the 32-byte unit u of row r stored at unit u ^ ((r >> 1) & UM): one
// image serves the row reads (ds_read_b128) and the transposed reads of the same tile.
//
// What MEM = true adds:
//   key sources : key j < Nq is row b*Nq + j of qkv [B*Nq, 3*H*dh] (k / v columns); key j >= Nq is row b*mstride + j - Nq of
//                 mem_kv [*, 2*H*dh] (k columns h*dh.., v columns H*dh + h*dh..).  mstride = 0: one memory set for every
//                 sample; mstride = M: one set per sample.  A 64-key tile may hold rows of both sources.
//   mask        : bit (key & 31) of 32-bit word b*mask_bs + h*mask_hs + q*W + (key >> 5), W = ceil(Nk / 32); 1 = may attend.
//                 A masked score is -FLT_MAX (the reference's masked_fill value; here in the exp2 domain, where -FLT_MAX *
//                 log2e would overflow).  A row whose keys are all masked therefore keeps m = -FLT_MAX, exp2(0) = 1 for
//                 every key: uniform weights, as in the reference; its LSE is written as -FLT_MAX and the backward
//                 recognises it by that value (P = 1 / Nk there, not exp2(s - lse), whose operands would be ~1e38 apart).
//   backward    : masked pairs carry no score gradient (masked_fill's backward).  Token keys write dqkv (bf16), memory keys
//                 write fp32 per-sample rows of dmem [B*M, 2*H*dh]; shared memories are then summed over the batch in a
//                 fixed order (no atomics).
#include "nrv_attn_common.hpp"

#include <cfloat>

namespace {

using nrv_attn::LN2;
using nrv_attn::LOG2E;
using nrv_attn::pack_frag;
using nrv_attn::DROP_C0;
using nrv_attn::DROP_C1;
using nrv_attn::DROP_GOLD;
using nrv_attn::drop_head_key;
using nrv_attn::drop_keep;
using nrv_attn::drop_quad;
using nrv_attn::drop_row_key;
using nrv_attn::drop_word;

struct GenParams {
    const bf16_t* qkv;       // [B*Nq, 3*H*dh]
    const bf16_t* out;       // [B*Nq, H*dh]   (bwd)
    const bf16_t* dout;      // [B*Nq, H*dh]   (bwd)
    bf16_t* o;               // fwd output
    bf16_t* dqkv;            // bwd output, token rows
    float* lse;              // [B, H, Nq]
    float* delta;            // [B, H, Nq]
    int B, Nq, H, dh;
    float scale;
    int M, Nk, W;
    const bf16_t* mkv;       // MEM: [*, 2*H*dh] memory keys / values (M > 0)
    const unsigned* mask;    // MEM: bit mask or null
    float* dmem;             // MEM: bwd output, memory rows [B*M, 2*H*dh]
    long long mstride;       // MEM: memory rows per sample step, 0 or M
    long long mask_bs, mask_hs;
    // DROP instantiations (nrv_attn_drop_*): 64-bit seed in device memory, threshold T of the 16-bit decisions, 1 / (1 - T / 2^16)
    const unsigned long long* seed;
    unsigned drop_T;
    float drop_rs;
};

constexpr int GT = 64;          // rows of a streamed tile = rows owned by a workgroup (4 waves x 16)
constexpr int GEN_THREADS = 256;
constexpr float MASKED = -FLT_MAX;

template <int KS>
struct GenCfg {
    static constexpr int DHP = 32 * KS, RB = 2 * DHP, TILE = GT * RB, DT = DHP / 16;
    static constexpr int UNITS = RB / 32;                                  // 2, 4, 6, 8; wide heads: 10, 12
    static constexpr int UM = UNITS == 2 ? 1 : UNITS == 4 ? 3 : UNITS == 6 ? 1 : UNITS == 10 ? 1 : UNITS == 12 ? 3 : 7;   // XOR mask that stays inside a row
};

template <int KS>
__device__ __forceinline__ int tile_off(int r, int c /* 16-byte chunk */) {
    using C = GenCfg<KS>;
    return r * C::RB + ((((c >> 1) ^ ((r >> 1) & C::UM)) << 5) | ((c & 1) << 4));
}

// A tile in two halves: global -> registers (issued a tile ahead, in flight during the current tile's arithmetic), registers
// -> LDS.  A thread holds KS 16-byte chunks of a tile (64 rows x 4 KS chunks over 256 threads).
// Rows r0 .. r0 + 63 of a [N x dh] head slice with row stride ld; rows >= N and columns >= dh are zero.
template <int KS>
__device__ __forceinline__ void fetch_tile(u32x4_t (&v)[KS], const bf16_t* src, long long ld, int r0, int N, int dh, int tid) {
    using C = GenCfg<KS>;
    constexpr int CPR = C::DHP / 8;
    static_assert(GT * CPR / GEN_THREADS == KS, "chunks per thread");
#pragma unroll
    for (int i = 0; i < KS; ++i) {
        const int idx = i * GEN_THREADS + tid;
        const int r = idx / CPR, c = idx - r * CPR;
        v[i] = u32x4_t{0u, 0u, 0u, 0u};
        if (r0 + r < N && c * 8 < dh) v[i] = *reinterpret_cast<const u32x4_t*>(src + (long long)(r0 + r) * ld + c * 8);
    }
}
template <int KS>
__device__ __forceinline__ void put_tile(char* img, const u32x4_t (&v)[KS], int tid) {
    using C = GenCfg<KS>;
    constexpr int CPR = C::DHP / 8;
#pragma unroll
    for (int i = 0; i < KS; ++i) {
        const int idx = i * GEN_THREADS + tid;
        const int r = idx / CPR, c = idx - r * CPR;
        *reinterpret_cast<u32x4_t*>(img + tile_off<KS>(r, c)) = v[i];
    }
}

// MEM: k row of key j of (b, h) in either source (v = k + H*dh in both); null for j >= Nk
__device__ __forceinline__ const bf16_t* key_row(const GenParams& p, int b, int h, int j) {
    const long long hd = (long long)p.H * p.dh;
    if (j < p.Nq) return p.qkv + ((long long)b * p.Nq + j) * 3 * hd + hd + (long long)h * p.dh;
    if (j < p.Nk) return p.mkv + ((long long)b * p.mstride + (j - p.Nq)) * 2 * hd + (long long)h * p.dh;
    return nullptr;
}

// keys and values k0 .. k0 + 63 of (b, h) into registers (zero beyond Nk / dh); kbase = the k columns of (b, h) in qkv
template <int KS, bool MEM>
__device__ __forceinline__ void fetch_kv(u32x4_t (&kv)[KS], u32x4_t (&vv)[KS], const GenParams& p, const bf16_t* kbase, int b,
                                         int h, int k0, int tid) {
    const long long hd = (long long)p.H * p.dh;
    if constexpr (!MEM) {
        fetch_tile<KS>(kv, kbase, 3 * hd, k0, p.Nq, p.dh, tid);
        fetch_tile<KS>(vv, kbase + hd, 3 * hd, k0, p.Nq, p.dh, tid);
    } else {
        constexpr int CPR = GenCfg<KS>::DHP / 8;
#pragma unroll
        for (int i = 0; i < KS; ++i) {
            const int idx = i * GEN_THREADS + tid;
            const int r = idx / CPR, c = idx - r * CPR;
            kv[i] = vv[i] = u32x4_t{0u, 0u, 0u, 0u};
            const bf16_t* row = key_row(p, b, h, k0 + r);
            if (row && c * 8 < p.dh) {
                kv[i] = *reinterpret_cast<const u32x4_t*>(row + c * 8);
                vv[i] = *reinterpret_cast<const u32x4_t*>(row + hd + c * 8);
            }
        }
    }
}

// row fragment (A or B operand whose 16 rows are tile rows rb .. rb + 15): lane -> row rb + (lane & 15), k = 32 ks + 8 (lane >> 4) ..
template <int KS>
__device__ __forceinline__ bf16x8_t row_frag(const char* img, int rb, int ks, int lane) {
    return lds_read_b128(img + tile_off<KS>(rb + (lane & 15), 4 * ks + (lane >> 4)));
}
// transposed fragment (A operand): columns 16 dt .. 16 dt + 15 of tile rows rb + {4g .. 4g+3, 16+4g .. 16+4g+3}
template <int KS>
__device__ __forceinline__ bf16x8_t tr_frag(const char* img, int rb, int dt, int lane) {
    using C = GenCfg<KS>;
    const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
    const int r0 = rb + 4 * g + q, r1 = r0 + 16;
    const char* a0 = img + r0 * C::RB + ((dt ^ ((r0 >> 1) & C::UM)) << 5) + pp * 8;
    const char* a1 = img + r1 * C::RB + ((dt ^ ((r1 >> 1) & C::UM)) << 5) + pp * 8;
    return cat4(lds_read_tr16_b64(a0), lds_read_tr16_b64(a1));
}
// the lane's 8 features 32 ks + 8 g .. of one row (null row: zero)
__device__ __forceinline__ bf16x8_t frag_of(const bf16_t* row, int dh, int ks, int g) {
    const int d0 = 32 * ks + 8 * g;
    if (row && d0 < dh) return *reinterpret_cast<const bf16x8_t*>(row + d0);
    return bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
}
// the same for row `row` of a [N x dh] slice (zero beyond N / dh)
__device__ __forceinline__ bf16x8_t glob_frag(const bf16_t* src, long long ld, int row, int N, int dh, int ks, int g) {
    const int d0 = 32 * ks + 8 * g;
    if (row < N && d0 < dh) return *reinterpret_cast<const bf16x8_t*>(src + (long long)row * ld + d0);
    return bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
}
__device__ __forceinline__ float quad_max(float v) {        // over the 4 lanes that share a query / key column (lane ^ 16, ^ 32)
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float quad_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}
// MEM: the two mask words of query q for keys k0 .. k0 + 63 (k0 % 64 == 0); all ones without a mask or for padded queries
__device__ __forceinline__ void mask_words(const GenParams& p, int b, int h, int q, int k0, unsigned& w0, unsigned& w1) {
    w0 = w1 = ~0u;
    if (p.mask && q < p.Nq) {
        const unsigned* mr = p.mask + b * p.mask_bs + h * p.mask_hs + (long long)q * p.W;
        const int wi = k0 >> 5;
        w0 = mr[wi];
        w1 = wi + 1 < p.W ? mr[wi + 1] : 0u;
    }
}

// ---------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------
// DROP (MEM = false only): attention-weight dropout.  m and l are those of the undropped row; the dropped weights become zero in
// the bf16 P^T operand and 1 / (1 - p_eff) joins the final 1 / l.
template <int KS, bool MEM, bool DROP>
__global__ __launch_bounds__(GEN_THREADS) void attn_gen_fwd_kernel(const GenParams p) {
    static_assert(!(MEM && DROP), "no dropout with memory keys / score masks");
    using C = GenCfg<KS>;
    __shared__ __attribute__((aligned(16))) char smem[2 * C::TILE];
    char* kimg = smem;
    char* vimg = smem + C::TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, qc = lane & 15;
    const int N = p.Nq, Nk = MEM ? p.Nk : N, H = p.H, dh = p.dh;
    const int nqb = (N + GT - 1) / GT;
    const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
    const int b = bh / H, h = bh - b * H;
    const long long ldq = 3ll * H * dh;
    const bf16_t* qbase = p.qkv + (long long)b * N * ldq + h * dh;
    const bf16_t* kbase = qbase + (long long)H * dh;
    const int q = qb * GT + wave * 16 + qc;               // this lane's query
    const float sc = p.scale * LOG2E;

    bf16x8_t qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = glob_frag(qbase, ldq, q, N, dh, ks, g);
    float m = -INFINITY, l = 0.f;
    f32x4_t ot[C::DT];
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) ot[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    unsigned ag = 0u, a1 = 0u;                            // DROP: the row keys of this lane's query
    if constexpr (DROP) {
        const unsigned long long seed = *p.seed;
        ag = drop_row_key(drop_head_key(seed, (unsigned)bh, DROP_C0), (unsigned)q) + 2u * g * DROP_GOLD;
        a1 = drop_row_key(drop_head_key(seed, (unsigned)bh, DROP_C1), (unsigned)q);
    }
    u32x4_t kreg[KS], vreg[KS];                           // the next K / V tile, requested one tile ahead
    fetch_kv<KS, MEM>(kreg, vreg, p, kbase, b, h, 0, tid);
    for (int k0 = 0; k0 < Nk; k0 += GT) {
        unsigned mw0 = ~0u, mw1 = ~0u;
        if constexpr (MEM) mask_words(p, b, h, q, k0, mw0, mw1);
        __syncthreads();                                  // every wave is done with the previous tile
        put_tile<KS>(kimg, kreg, tid);
        put_tile<KS>(vimg, vreg, tid);
        __syncthreads();
        if (k0 + GT < Nk) fetch_kv<KS, MEM>(kreg, vreg, p, kbase, b, h, k0 + GT, tid);
        // S^T = K Q^T for the four 16-key sub-tiles; lane: keys k0 + 16 sub + 4 g + e of query q
        f32x4_t st[4];
        float tmax = -INFINITY;
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            f32x4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) a = mfma16(row_frag<KS>(kimg, sub * 16, ks, lane), qf[ks], a);
            const unsigned w = sub < 2 ? mw0 : mw1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = a[e] * sc;
                if constexpr (MEM)
                    if (!((w >> ((sub & 1) * 16 + 4 * g + e)) & 1u)) v = MASKED;
                a[e] = (k0 + sub * 16 + 4 * g + e < Nk) ? v : -INFINITY;
                tmax = fmaxf(tmax, a[e]);
            }
            st[sub] = a;
        }
        tmax = quad_max(tmax);
        const float mn = fmaxf(m, tmax);                  // finite: every tile holds a key < Nk (masked ones are -FLT_MAX)
        const float alpha = __builtin_amdgcn_exp2f(m - mn);   // m = -inf on the first tile: 0
        float ps = 0.f;
#pragma unroll
        for (int sub = 0; sub < 4; ++sub)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float pv = __builtin_amdgcn_exp2f(st[sub][e] - mn);
                st[sub][e] = pv;
                ps += pv;
            }
        l = l * alpha + quad_sum(ps);
        m = mn;
        if constexpr (DROP) {
#pragma unroll
            for (int sub = 0; sub < 4; ++sub) drop_quad(st[sub], ag, a1, (unsigned)(k0 >> 1) + sub * 8, p.drop_T, 1.0f);
        }
#pragma unroll
        for (int dt = 0; dt < C::DT; ++dt) ot[dt] *= alpha;
        // O^T += V^T P^T, two 32-key steps
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const bf16x8_t pf = pack_frag(st[2 * kk], st[2 * kk + 1]);
#pragma unroll
            for (int dt = 0; dt < C::DT; ++dt) ot[dt] = mfma16(tr_frag<KS>(vimg, kk * 32, dt, lane), pf, ot[dt]);
        }
    }
    if (q < N) {
        const float inv = DROP ? p.drop_rs / l : 1.0f / l;
        bf16_t* dst = p.o + ((long long)b * N + q) * ((long long)H * dh) + h * dh;
#pragma unroll
        for (int dt = 0; dt < C::DT; ++dt) {
            const int d0 = dt * 16 + 4 * g;
            if (d0 < dh) nrv_attn::store_bf16x4(dst + d0, ot[dt] * inv);
        }
        if (g == 0) p.lse[((long long)b * H + h) * N + q] = MEM && m == MASKED ? MASKED : (m + __builtin_amdgcn_logf(l)) * LN2;
    }
}

// ---------------------------------------------------------------------------------------------
// backward, query-owner pass: dQ = scale * dS K with dS = P o (dP - delta), dP = dO V^T; also writes delta = rowsum(dO o O)
// ---------------------------------------------------------------------------------------------
template <int KS, bool MEM, bool DROP>
__global__ __launch_bounds__(GEN_THREADS) void attn_gen_dq_kernel(const GenParams p) {
    static_assert(!(MEM && DROP), "no dropout with memory keys / score masks");
    using C = GenCfg<KS>;
    __shared__ __attribute__((aligned(16))) char smem[2 * C::TILE];
    char* kimg = smem;
    char* vimg = smem + C::TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, qc = lane & 15;
    const int N = p.Nq, Nk = MEM ? p.Nk : N, H = p.H, dh = p.dh;
    const int nqb = (N + GT - 1) / GT;
    const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
    const int b = bh / H, h = bh - b * H;
    const long long ldq = 3ll * H * dh, ldo = (long long)H * dh;
    const bf16_t* qbase = p.qkv + (long long)b * N * ldq + h * dh;
    const bf16_t* kbase = qbase + (long long)H * dh;
    const bf16_t* obase = p.out + (long long)b * N * ldo + h * dh;
    const bf16_t* dobase = p.dout + (long long)b * N * ldo + h * dh;
    const int q = qb * GT + wave * 16 + qc;
    const float sc = p.scale * LOG2E;

    bf16x8_t qf[KS], dof[KS];
    float dl = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        qf[ks] = glob_frag(qbase, ldq, q, N, dh, ks, g);
        dof[ks] = glob_frag(dobase, ldo, q, N, dh, ks, g);
        const bf16x8_t of = glob_frag(obase, ldo, q, N, dh, ks, g);
#pragma unroll
        for (int e = 0; e < 8; ++e) dl = fmaf(bf16_to_f32((unsigned short)dof[ks][e]), bf16_to_f32((unsigned short)of[e]), dl);
    }
    dl = quad_sum(dl);
    const long long sidx = ((long long)b * H + h) * N + (q < N ? q : 0);
    const float lsev = q < N ? p.lse[sidx] : 0.f;
    // every key masked (lse = -FLT_MAX): P = 1 / Nk, but no pair carries a score gradient, so the row adds nothing to dQ
    const float lse2 = q < N && !(MEM && lsev == MASKED) ? lsev * LOG2E : INFINITY;   // exp2(s - inf) = 0 for padded queries
    if (q < N && g == 0) p.delta[sidx] = dl;

    unsigned ag = 0u, a1 = 0u;                            // DROP: the row keys of this lane's query
    if constexpr (DROP) {
        const unsigned long long seed = *p.seed;
        ag = drop_row_key(drop_head_key(seed, (unsigned)bh, DROP_C0), (unsigned)q) + 2u * g * DROP_GOLD;
        a1 = drop_row_key(drop_head_key(seed, (unsigned)bh, DROP_C1), (unsigned)q);
    }
    f32x4_t dqt[C::DT];
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) dqt[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    u32x4_t kreg[KS], vreg[KS];                           // the next K / V tile, requested one tile ahead
    fetch_kv<KS, MEM>(kreg, vreg, p, kbase, b, h, 0, tid);
    for (int k0 = 0; k0 < Nk; k0 += GT) {
        unsigned mw0 = ~0u, mw1 = ~0u;
        if constexpr (MEM) mask_words(p, b, h, q, k0, mw0, mw1);
        __syncthreads();
        put_tile<KS>(kimg, kreg, tid);
        put_tile<KS>(vimg, vreg, tid);
        __syncthreads();
        if (k0 + GT < Nk) fetch_kv<KS, MEM>(kreg, vreg, p, kbase, b, h, k0 + GT, tid);
        f32x4_t ds[4];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            f32x4_t s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                s = mfma16(row_frag<KS>(kimg, sub * 16, ks, lane), qf[ks], s);
                dp = mfma16(row_frag<KS>(vimg, sub * 16, ks, lane), dof[ks], dp);
            }
            if constexpr (DROP) drop_quad(dp, ag, a1, (unsigned)(k0 >> 1) + sub * 8, p.drop_T, p.drop_rs);     // M o dP, before - delta
            const unsigned w = sub < 2 ? mw0 : mw1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool keep = !MEM || ((w >> ((sub & 1) * 16 + 4 * g + e)) & 1u);
                const bool valid = k0 + sub * 16 + 4 * g + e < Nk;
                const float pv = valid && keep ? __builtin_amdgcn_exp2f(fmaf(s[e], sc, -lse2)) : 0.f;
                ds[sub][e] = pv * (dp[e] - dl);               // masked pairs: no score gradient (and P = 0 or 1 / Nk)
            }
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const bf16x8_t df = pack_frag(ds[2 * kk], ds[2 * kk + 1]);
#pragma unroll
            for (int dt = 0; dt < C::DT; ++dt) dqt[dt] = mfma16(tr_frag<KS>(kimg, kk * 32, dt, lane), df, dqt[dt]);
        }
    }
    if (q < N) {
        bf16_t* dst = p.dqkv + ((long long)b * N + q) * ldq + h * dh;
#pragma unroll
        for (int dt = 0; dt < C::DT; ++dt) {
            const int d0 = dt * 16 + 4 * g;
            if (d0 < dh) nrv_attn::store_bf16x4(dst + d0, dqt[dt] * p.scale);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// backward, key-owner pass: dV = P^T dO, dK = scale * dS^T Q for 64 keys of one (batch, head).  Scores in [query][key]
// orientation: a lane owns one key column, its queries sit in registers and are the k slots of the dV^T / dK^T products.
// ---------------------------------------------------------------------------------------------
template <int KS, bool MEM, bool DROP>
__global__ __launch_bounds__(GEN_THREADS) void attn_gen_dkv_kernel(const GenParams p) {
    static_assert(!(MEM && DROP), "no dropout with memory keys / score masks");
    using C = GenCfg<KS>;
    // per-query words behind the two tiles: lse, delta; MEM adds the uniform P of a fully masked row and two mask words, DROP
    // the two row keys of the dropout decisions
    __shared__ __attribute__((aligned(16))) char smem[2 * C::TILE + (MEM ? 5 : DROP ? 4 : 2) * GT * 4];
    char* qimg = smem;
    char* doimg = smem + C::TILE;
    float* lse2s = reinterpret_cast<float*>(smem + 2 * C::TILE);
    float* dels = lse2s + GT;
    float* unis = dels + GT;                                         // MEM
    unsigned* a0s = reinterpret_cast<unsigned*>(dels + GT);          // DROP
    unsigned* a1s = a0s + GT;                                        // DROP
    unsigned* mws = reinterpret_cast<unsigned*>(unis + GT);          // MEM, [2][64]: the mask words of this block's keys per query
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, kc = lane & 15;
    const int N = p.Nq, Nk = MEM ? p.Nk : N, H = p.H, dh = p.dh;
    const int nkb = (Nk + GT - 1) / GT;
    const int bh = blockIdx.x / nkb, kb = blockIdx.x - bh * nkb;
    const int b = bh / H, h = bh - b * H;
    const long long ldq = 3ll * H * dh, ldo = (long long)H * dh;
    const bf16_t* qbase = p.qkv + (long long)b * N * ldq + h * dh;
    const bf16_t* kbase = qbase + (long long)H * dh;
    const bf16_t* dobase = p.dout + (long long)b * N * ldo + h * dh;
    const float* lse = p.lse + ((long long)b * H + h) * N;
    const float* delta = p.delta + ((long long)b * H + h) * N;
    const unsigned* mbase = p.mask ? p.mask + b * p.mask_bs + h * p.mask_hs : nullptr;
    const int kl = wave * 16 + kc;                        // this lane's key within the block
    const int key = kb * GT + kl;
    const int msel = kl >> 5, mbit = kl & 31;
    const float sc = p.scale * LOG2E;
    const float inv_nk = 1.0f / (float)Nk;

    bf16x8_t kf[KS], vf[KS];
    const bf16_t* krow = MEM ? key_row(p, b, h, key) : nullptr;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        if constexpr (MEM) {
            kf[ks] = frag_of(krow, dh, ks, g);
            vf[ks] = frag_of(krow ? krow + ldo : nullptr, dh, ks, g);
        } else {
            kf[ks] = glob_frag(kbase, ldq, key, N, dh, ks, g);
            vf[ks] = glob_frag(kbase + ldo, ldq, key, N, dh, ks, g);
        }
    }
    f32x4_t dkt[C::DT], dvt[C::DT];
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) dkt[dt] = dvt[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    u32x4_t qreg[KS], doreg[KS];                          // the next Q / dO tile and its statistics
    float lreg = INFINITY, dreg = 0.f, ureg = 0.f;
    unsigned mreg = ~0u;
    auto fetch_stats = [&](int q0) {
        if (tid < GT) {
            const int qq = q0 + tid;
            const float lv = qq < N ? lse[qq] : 0.f;
            const bool full = MEM && lv == MASKED;
            lreg = qq < N && !full ? lv * LOG2E : INFINITY;          // exp2(s - inf) = 0 for padded queries
            dreg = qq < N ? delta[qq] : 0.f;
            ureg = full ? inv_nk : 0.f;
        } else if (MEM && tid < 3 * GT) {
            const int i = tid - GT, qq = q0 + (i & 63), wi = kb * 2 + (i >> 6);
            mreg = (mbase && qq < N) ? (wi < p.W ? mbase[(long long)qq * p.W + wi] : 0u) : ~0u;
        }
    };
    // one tile ahead only where the registers are there: at head dims <= 64 the prefetch registers cost this kernel half its
    // occupancy (82 -> 128 VGPRs) and 17 % of its time (profiles/r04_streaming_attention_prefetch.txt).  Not with memory keys
    // or a mask: there it made the backward slower (B 32, Nq 257, M 10, H 16, dh 80: 0.169 -> 0.200 ms)
    constexpr bool AHEAD = KS >= 3 && !MEM;
    if (AHEAD) {
        fetch_tile<KS>(qreg, qbase, ldq, 0, N, dh, tid);
        fetch_tile<KS>(doreg, dobase, ldo, 0, N, dh, tid);
        fetch_stats(0);
    }
    for (int q0 = 0; q0 < N; q0 += GT) {
        __syncthreads();
        if (!AHEAD) {
            fetch_tile<KS>(qreg, qbase, ldq, q0, N, dh, tid);
            fetch_tile<KS>(doreg, dobase, ldo, q0, N, dh, tid);
            fetch_stats(q0);
        }
        if (tid < GT) {
            lse2s[tid] = lreg;
            dels[tid] = dreg;
            if constexpr (MEM) unis[tid] = ureg;
            if constexpr (DROP) {
                const unsigned long long seed = *p.seed;
                a0s[tid] = drop_row_key(drop_head_key(seed, (unsigned)bh, DROP_C0), (unsigned)(q0 + tid));
                a1s[tid] = drop_row_key(drop_head_key(seed, (unsigned)bh, DROP_C1), (unsigned)(q0 + tid));
            }
        } else if (MEM && tid < 3 * GT) {
            mws[tid - GT] = mreg;
        }
        put_tile<KS>(qimg, qreg, tid);
        put_tile<KS>(doimg, doreg, tid);
        __syncthreads();
        if (AHEAD && q0 + GT < N) {
            fetch_tile<KS>(qreg, qbase, ldq, q0 + GT, N, dh, tid);
            fetch_tile<KS>(doreg, dobase, ldo, q0 + GT, N, dh, tid);
            fetch_stats(q0 + GT);
        }
        f32x4_t pt[4], ds[4];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            // S[query 16 sub + 4 g + e][key] and dP = dO V^T in the same orientation
            f32x4_t s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                s = mfma16(row_frag<KS>(qimg, sub * 16, ks, lane), kf[ks], s);
                dp = mfma16(row_frag<KS>(doimg, sub * 16, ks, lane), vf[ks], dp);
            }
            const f32x4_t l4 = *reinterpret_cast<const f32x4_t*>(lse2s + sub * 16 + 4 * g);
            const f32x4_t d4 = *reinterpret_cast<const f32x4_t*>(dels + sub * 16 + 4 * g);
            f32x4_t u4 = {0.f, 0.f, 0.f, 0.f};
            u32x4_t w4 = {~0u, ~0u, ~0u, ~0u};
            if constexpr (MEM) {
                u4 = *reinterpret_cast<const f32x4_t*>(unis + sub * 16 + 4 * g);
                w4 = *reinterpret_cast<const u32x4_t*>(mws + msel * GT + sub * 16 + 4 * g);
            }
            u32x4_t r0 = {0u, 0u, 0u, 0u}, r1 = r0;
            if constexpr (DROP) {
                r0 = *reinterpret_cast<const u32x4_t*>(a0s + sub * 16 + 4 * g);
                r1 = *reinterpret_cast<const u32x4_t*>(a1s + sub * 16 + 4 * g);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool keep = !MEM || ((w4[e] >> mbit) & 1u);   // masked pairs: P = 0 (1 / Nk in a fully masked row), dS = 0
                const float pv = keep ? __builtin_amdgcn_exp2f(fmaf(s[e], sc, -l4[e])) : u4[e];
                if constexpr (DROP) {                               // P o keep feeds dV (1 / (1 - p_eff) at the store), M o dP feeds dS
                    const bool kept = drop_keep(drop_word(r0[e], r1[e], (unsigned)key >> 1), (unsigned)key, p.drop_T);
                    pt[sub][e] = kept ? pv : 0.f;
                    ds[sub][e] = pv * ((kept ? dp[e] * p.drop_rs : 0.f) - d4[e]);
                } else {
                    pt[sub][e] = pv;
                    ds[sub][e] = keep ? pv * (dp[e] - d4[e]) : 0.f;
                }
            }
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const bf16x8_t pf = pack_frag(pt[2 * kk], pt[2 * kk + 1]);
            const bf16x8_t df = pack_frag(ds[2 * kk], ds[2 * kk + 1]);
#pragma unroll
            for (int dt = 0; dt < C::DT; ++dt) {
                dvt[dt] = mfma16(tr_frag<KS>(doimg, kk * 32, dt, lane), pf, dvt[dt]);
                dkt[dt] = mfma16(tr_frag<KS>(qimg, kk * 32, dt, lane), df, dkt[dt]);
            }
        }
    }
    if (key < N) {
        bf16_t* dk = p.dqkv + ((long long)b * N + key) * ldq + ldo + h * dh;
        bf16_t* dv = dk + ldo;
#pragma unroll
        for (int dt = 0; dt < C::DT; ++dt) {
            const int d0 = dt * 16 + 4 * g;
            if (d0 < dh) {
                nrv_attn::store_bf16x4(dk + d0, dkt[dt] * p.scale);
                nrv_attn::store_bf16x4(dv + d0, DROP ? dvt[dt] * p.drop_rs : dvt[dt]);
            }
        }
    } else if constexpr (MEM) {
        if (key < Nk) {
            float* dk = p.dmem + ((long long)b * p.M + (key - N)) * 2 * ldo + h * dh;
            float* dv = dk + ldo;
#pragma unroll
            for (int dt = 0; dt < C::DT; ++dt) {
                const int d0 = dt * 16 + 4 * g;
                if (d0 < dh) {
                    *reinterpret_cast<f32x4_t*>(dk + d0) = dkt[dt] * p.scale;
                    *reinterpret_cast<f32x4_t*>(dv + d0) = dvt[dt];
                }
            }
        }
    }
}

// introspection (recorder.py:24-31): P[b,h,q,k] = exp(scale q.k - lse[b,h,q]) in fp32, any N / dh; a plain VALU kernel
__global__ __launch_bounds__(256) void attn_gen_probs_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ lse,
                                                             float* __restrict__ probs, int B, int N, int H, int dh, float scale) {
    __shared__ float qs[16][129];
    const int bh = blockIdx.x, q0 = blockIdx.y * 16;
    const int b = bh / H, h = bh - b * H;
    const long long ldq = 3ll * H * dh;
    const bf16_t* base = qkv + (long long)b * N * ldq + h * dh;
    for (int i = threadIdx.x; i < 16 * dh; i += 256) {
        const int r = i / dh, d = i - r * dh;
        qs[r][d] = (q0 + r < N) ? bf16_to_f32(base[(long long)(q0 + r) * ldq + d]) : 0.f;
    }
    __syncthreads();
    const int qi = threadIdx.x & 15;
    const int q = q0 + qi;
    const float l = q < N ? lse[((long long)b * H + h) * N + q] : 0.f;
    for (int key = threadIdx.x >> 4; key < N; key += 16) {
        const bf16_t* kp = base + (long long)H * dh + (long long)key * ldq;
        float acc = 0.f;
        for (int c = 0; c < dh / 8; ++c) {
            const bf16x8_t kv = *reinterpret_cast<const bf16x8_t*>(kp + c * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf(qs[qi][c * 8 + e], bf16_to_f32((unsigned short)kv[e]), acc);
        }
        if (q < N) probs[(((long long)b * H + h) * N + q) * N + key] = __expf(acc * scale - l);
    }
}

// shared memories: the per-sample rows summed over the batch in a fixed order (no atomics), in two passes of this kernel.
// Group y of `count` consecutive blocks of n4 float4 (blocks stride4 apart) is summed in block order into
// dst + y * count * stride4: pass 1 sums groups of MEM_SUM_GROUP samples in place (into each group's first sample), pass 2 the
// group sums into the output.  A thread reads its element of every block before it writes, so the in-place pass is safe.
constexpr int MEM_SUM_GROUP = 16;
__global__ __launch_bounds__(256) void mem_batch_sum_kernel(const float* src, float* dst, long long n4, long long stride4,
                                                            int count, int total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int first = blockIdx.y * count, n = min(count, total - first);
    const f32x4_t* s = reinterpret_cast<const f32x4_t*>(src) + (long long)first * stride4 + i;
    f32x4_t acc = s[0];
    for (int j = 1; j < n; ++j) acc += s[(long long)j * stride4];
    reinterpret_cast<f32x4_t*>(dst)[(long long)first * stride4 + i] = acc;
}

// bool / uint8 [rows, cols] (non-zero = 1) -> 32-bit words [rows, ceil(cols / 32)], bit c & 31 of word c >> 5
__global__ __launch_bounds__(256) void mask_pack_kernel(const unsigned char* __restrict__ m, unsigned* __restrict__ bits,
                                                        long long rows, int cols, int W) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * W) return;
    const long long r = i / W;
    const int c0 = (int)(i - r * W) * 32;
    const unsigned char* src = m + r * cols;
    unsigned w = 0u;
    for (int c = 0; c < 32 && c0 + c < cols; ++c) w |= (src[c0 + c] != 0 ? 1u : 0u) << c;
    bits[i] = w;
}

int ks_of(int dh) {
    switch (dh) {
        case 32: return 1;
        case 64: return 2;
        case 80: case 96: return 3;
        case 128: return 4;
        default: return 0;
    }
}

// forward: one workgroup per 64 queries; backward: the dQ pass over query blocks, then the dK / dV pass over key blocks
template <int KS, bool MEM, bool DROP = false>
int launch(const GenParams& p, bool bwd, hipStream_t s) {
    const long long gq = (long long)p.B * p.H * ((p.Nq + GT - 1) / GT);
    if (!bwd) {
        hipLaunchKernelGGL((attn_gen_fwd_kernel<KS, MEM, DROP>), dim3((unsigned)gq), dim3(GEN_THREADS), 0, s, p);
        NRV_CHECK_LAUNCH();
        return 0;
    }
    const long long gk = (long long)p.B * p.H * ((p.Nk + GT - 1) / GT);
    hipLaunchKernelGGL((attn_gen_dq_kernel<KS, MEM, DROP>), dim3((unsigned)gq), dim3(GEN_THREADS), 0, s, p);
    NRV_CHECK_LAUNCH();
    hipLaunchKernelGGL((attn_gen_dkv_kernel<KS, MEM, DROP>), dim3((unsigned)gk), dim3(GEN_THREADS), 0, s, p);
    NRV_CHECK_LAUNCH();
    return 0;
}
template <bool MEM, bool DROP = false>
int launch_dh(const GenParams& p, bool bwd, hipStream_t s) {
    switch (ks_of(p.dh)) {
        case 1: return launch<1, MEM, DROP>(p, bwd, s);
        case 2: return launch<2, MEM, DROP>(p, bwd, s);
        case 3: return launch<3, MEM, DROP>(p, bwd, s);
        case 4: return launch<4, MEM, DROP>(p, bwd, s);
        default: return NRV_ERR_SHAPE;
    }
}

bool aligned4(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3u) == 0; }

// shape / stride checks shared by the memory forward and backward (before any pointer is touched)
int check_args(int B, int Nq, int M, int H, int dh, long long mstride, long long mask_bs, long long mask_hs) {
    if (B <= 0 || Nq <= 0 || H <= 0 || M < 0 || ks_of(dh) == 0) return NRV_ERR_SHAPE;
    if (M > 0 && mstride != 0 && mstride != M) return NRV_ERR_SHAPE;
    if (mask_bs < 0 || mask_hs < 0) return NRV_ERR_SHAPE;
    const long long Nk = (long long)Nq + M;
    if (Nk > 0x7fffffffll - GT) return NRV_ERR_SHAPE;
    if ((long long)B * H * ((Nk + GT - 1) / GT) > 0x7fffffffll) return NRV_ERR_SHAPE;
    return 0;
}

GenParams make_params(const void* qkv, const void* mem_kv, long long mstride, int M, const unsigned* mask, long long mask_bs,
                      long long mask_hs, int B, int Nq, int H, int dh, float scale) {
    GenParams p{};
    p.qkv = static_cast<const bf16_t*>(qkv);
    p.mkv = static_cast<const bf16_t*>(mem_kv);
    p.mask = mask;
    p.mstride = mstride;
    p.mask_bs = mask_bs; p.mask_hs = mask_hs;
    p.B = B; p.Nq = Nq; p.M = M; p.Nk = Nq + M; p.H = H; p.dh = dh; p.W = (Nq + M + 31) / 32;
    p.scale = scale;
    return p;
}

}  // namespace

// Called by the C ABI entries of nrv_attn.hip for the shapes its single-pass kernels do not take (host-side dispatch on
// N and dh: one code path per shape class).  Arguments are already null- and alignment-checked there.
NRV_INTERNAL int nrv_attn_gen_supported(int B, int N, int H, int dh) {
    if (B <= 0 || N <= 0 || H <= 0 || ks_of(dh) == 0) return 0;
    if ((long long)B * H * ((N + GT - 1) / GT) > 0x7fffffffll) return 0;
    if ((long long)N * 3 * H * dh > 0x7fffffffll) return 0;
    return 1;
}

NRV_INTERNAL int nrv_attn_gen_fwd(const void* qkv, void* out, float* lse, int B, int N, int H, int dh, float scale, hipStream_t s) {
    GenParams p = make_params(qkv, nullptr, 0, 0, nullptr, 0, 0, B, N, H, dh, scale);
    p.o = static_cast<bf16_t*>(out);
    p.lse = lse;
    return launch_dh<false>(p, false, s);
}

NRV_INTERNAL int nrv_attn_gen_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* delta_ws,
                     int B, int N, int H, int dh, float scale, hipStream_t s) {
    GenParams p = make_params(qkv, nullptr, 0, 0, nullptr, 0, 0, B, N, H, dh, scale);
    p.out = static_cast<const bf16_t*>(out);
    p.dout = static_cast<const bf16_t*>(dout);
    p.dqkv = static_cast<bf16_t*>(dqkv);
    p.lse = const_cast<float*>(lse);
    p.delta = delta_ws;
    return launch_dh<false>(p, true, s);
}

// attention-weight dropout (nrv_attn_drop_fwd / _bwd of nrv_attn.hip, T > 0): the DROP instantiations
NRV_INTERNAL int nrv_attn_gen_drop_fwd(const void* qkv, void* out, float* lse, const unsigned long long* seed, unsigned T, float rs,
                     int B, int N, int H, int dh, float scale, hipStream_t s) {
    GenParams p = make_params(qkv, nullptr, 0, 0, nullptr, 0, 0, B, N, H, dh, scale);
    p.o = static_cast<bf16_t*>(out);
    p.lse = lse;
    p.seed = seed; p.drop_T = T; p.drop_rs = rs;
    return launch_dh<false, true>(p, false, s);
}

NRV_INTERNAL int nrv_attn_gen_drop_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* delta_ws,
                     const unsigned long long* seed, unsigned T, float rs, int B, int N, int H, int dh, float scale, hipStream_t s) {
    GenParams p = make_params(qkv, nullptr, 0, 0, nullptr, 0, 0, B, N, H, dh, scale);
    p.out = static_cast<const bf16_t*>(out);
    p.dout = static_cast<const bf16_t*>(dout);
    p.dqkv = static_cast<bf16_t*>(dqkv);
    p.lse = const_cast<float*>(lse);
    p.delta = delta_ws;
    p.seed = seed; p.drop_T = T; p.drop_rs = rs;
    return launch_dh<false, true>(p, true, s);
}

NRV_INTERNAL int nrv_attn_gen_probs(const void* qkv, const float* lse, float* probs, int B, int N, int H, int dh, float scale, hipStream_t s) {
    hipLaunchKernelGGL(attn_gen_probs_kernel, dim3((unsigned)(B * H), (unsigned)((N + 15) / 16)), dim3(256), 0, s,
                       static_cast<const bf16_t*>(qkv), lse, probs, B, N, H, dh, scale);
    NRV_CHECK_LAUNCH();
    return 0;
}

// Memory keys and a score mask (lucid_vit.Adapter).  Without either the plain instantiation runs: bit-identical, see the top.
extern "C" int nrv_attn_mem_fwd(const void* qkv_bf16, const void* mem_kv_bf16, int64_t mem_bstride, int M,
                                const uint32_t* mask, int64_t mask_bstride, int64_t mask_hstride,
                                void* out_bf16, float* lse, int B, int Nq, int H, int dh, float scale, void* stream) {
    if (!qkv_bf16 || !out_bf16 || !lse || (M > 0 && !mem_kv_bf16)) return NRV_ERR_NULL;
    if (int rc = check_args(B, Nq, M, H, dh, mem_bstride, mask_bstride, mask_hstride)) return rc;
    if (!nrv_aligned16(qkv_bf16) || !nrv_aligned16(out_bf16) || (M > 0 && !nrv_aligned16(mem_kv_bf16)) || !aligned4(lse) ||
        (mask && !aligned4(mask)))
        return NRV_ERR_ALIGN;
    GenParams p = make_params(qkv_bf16, mem_kv_bf16, mem_bstride, M, mask, mask_bstride, mask_hstride, B, Nq, H, dh, scale);
    p.o = static_cast<bf16_t*>(out_bf16);
    p.lse = lse;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return M == 0 && !mask ? launch_dh<false>(p, false, s) : launch_dh<true>(p, false, s);
}

extern "C" int nrv_attn_mem_bwd(const void* qkv_bf16, const void* out_bf16, const void* dout_bf16, const float* lse,
                                const void* mem_kv_bf16, int64_t mem_bstride, int M,
                                const uint32_t* mask, int64_t mask_bstride, int64_t mask_hstride,
                                void* dqkv_bf16, float* dmem_f32, float* dmem_sum_f32, float* delta_ws,
                                int B, int Nq, int H, int dh, float scale, void* stream) {
    if (!qkv_bf16 || !out_bf16 || !dout_bf16 || !lse || !dqkv_bf16 || !delta_ws || (M > 0 && (!mem_kv_bf16 || !dmem_f32)))
        return NRV_ERR_NULL;
    if (int rc = check_args(B, Nq, M, H, dh, mem_bstride, mask_bstride, mask_hstride)) return rc;
    if (dmem_sum_f32 && (M == 0 || mem_bstride != 0)) return NRV_ERR_SHAPE;       // the batch sum is for shared memories
    if (!nrv_aligned16(qkv_bf16) || !nrv_aligned16(out_bf16) || !nrv_aligned16(dout_bf16) || !nrv_aligned16(dqkv_bf16) ||
        (M > 0 && (!nrv_aligned16(mem_kv_bf16) || !nrv_aligned16(dmem_f32))) || (dmem_sum_f32 && !nrv_aligned16(dmem_sum_f32)) ||
        !aligned4(lse) || !aligned4(delta_ws) || (mask && !aligned4(mask)))
        return NRV_ERR_ALIGN;
    GenParams p = make_params(qkv_bf16, mem_kv_bf16, mem_bstride, M, mask, mask_bstride, mask_hstride, B, Nq, H, dh, scale);
    p.out = static_cast<const bf16_t*>(out_bf16);
    p.dout = static_cast<const bf16_t*>(dout_bf16);
    p.dqkv = static_cast<bf16_t*>(dqkv_bf16);
    p.dmem = dmem_f32;
    p.lse = const_cast<float*>(lse);
    p.delta = delta_ws;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = M == 0 && !mask ? launch_dh<false>(p, true, s) : launch_dh<true>(p, true, s);
    if (rc || !dmem_sum_f32) return rc;
    const long long n4 = (long long)M * 2 * H * dh / 4;
    const unsigned gx = (unsigned)((n4 + 255) / 256);
    const int groups = (B + MEM_SUM_GROUP - 1) / MEM_SUM_GROUP;
    hipLaunchKernelGGL(mem_batch_sum_kernel, dim3(gx, (unsigned)groups), dim3(256), 0, s, dmem_f32, dmem_f32, n4, n4, MEM_SUM_GROUP, B);
    NRV_CHECK_LAUNCH();
    hipLaunchKernelGGL(mem_batch_sum_kernel, dim3(gx, 1u), dim3(256), 0, s, dmem_f32, dmem_sum_f32, n4, n4 * MEM_SUM_GROUP, groups, groups);
    NRV_CHECK_LAUNCH();
    return 0;
}

// Wide single-head-style attention (T2T-ViT's stage transformers, t2t.py:76-83: heads = 1, dim_head = 147 stored as 152): the
// MEM = false instantiation at KS = 5 / 6, i.e. 128 < dh <= 192 with dh % 8 == 0.  The limit is the 64 KB of static LDS: the
// key-owner pass holds two [64][32 KS] bf16 tiles and 512 bytes of statistics, 49 664 bytes at KS = 6 and over 64 KB at KS = 8.
static int wide_ks(int dh) { return (dh & 7) || dh <= 128 || dh > 192 ? 0 : dh <= 160 ? 5 : 6; }
static int wide_args(int B, int N, int H, int dh) {
    if (B <= 0 || N <= 0 || H <= 0 || wide_ks(dh) == 0) return NRV_ERR_SHAPE;
    if ((long long)N > 0x7fffffffll - GT || (long long)B * H * ((N + GT - 1) / GT) > 0x7fffffffll) return NRV_ERR_SHAPE;
    if ((long long)N * 3 * H * dh > 0x7fffffffll) return NRV_ERR_SHAPE;
    return 0;
}

extern "C" int nrv_attn_wide_fwd(const void* qkv_bf16, void* out_bf16, float* lse, int B, int N, int H, int dh, float scale,
                                 void* stream) {
    if (int rc = wide_args(B, N, H, dh)) return rc;
    if (!qkv_bf16 || !out_bf16 || !lse) return NRV_ERR_NULL;
    if (!nrv_aligned16(qkv_bf16) || !nrv_aligned16(out_bf16) || !aligned4(lse)) return NRV_ERR_ALIGN;
    GenParams p = make_params(qkv_bf16, nullptr, 0, 0, nullptr, 0, 0, B, N, H, dh, scale);
    p.o = static_cast<bf16_t*>(out_bf16);
    p.lse = lse;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return wide_ks(dh) == 5 ? launch<5, false>(p, false, s) : launch<6, false>(p, false, s);
}

extern "C" int nrv_attn_wide_bwd(const void* qkv_bf16, const void* out_bf16, const void* dout_bf16, const float* lse,
                                 void* dqkv_bf16, float* delta_ws, int B, int N, int H, int dh, float scale, void* stream) {
    if (int rc = wide_args(B, N, H, dh)) return rc;
    if (!qkv_bf16 || !out_bf16 || !dout_bf16 || !lse || !dqkv_bf16 || !delta_ws) return NRV_ERR_NULL;
    if (!nrv_aligned16(qkv_bf16) || !nrv_aligned16(out_bf16) || !nrv_aligned16(dout_bf16) || !nrv_aligned16(dqkv_bf16) ||
        !aligned4(lse) || !aligned4(delta_ws))
        return NRV_ERR_ALIGN;
    GenParams p = make_params(qkv_bf16, nullptr, 0, 0, nullptr, 0, 0, B, N, H, dh, scale);
    p.out = static_cast<const bf16_t*>(out_bf16);
    p.dout = static_cast<const bf16_t*>(dout_bf16);
    p.dqkv = static_cast<bf16_t*>(dqkv_bf16);
    p.lse = const_cast<float*>(lse);
    p.delta = delta_ws;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return wide_ks(dh) == 5 ? launch<5, false>(p, true, s) : launch<6, false>(p, true, s);
}

extern "C" int nrv_mask_pack_bits(const void* mask_u8, uint32_t* bits, int64_t rows, int cols, void* stream) {
    if (!mask_u8 || !bits) return NRV_ERR_NULL;
    if (rows <= 0 || cols <= 0) return NRV_ERR_SHAPE;
    const int W = (cols + 31) / 32;
    if (rows * W / 256 >= 0x7fffffffll) return NRV_ERR_SHAPE;
    if (!aligned4(bits)) return NRV_ERR_ALIGN;
    const long long n = rows * W;
    hipLaunchKernelGGL(mask_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const unsigned char*>(mask_u8), bits, (long long)rows, cols, W);
    NRV_CHECK_LAUNCH();
    return 0;
}
