// Streaming softmax attention with extra key / value rows and a boolean score mask: the attention of the learnable-memory
// adapter (learnable_memory_vit.py:64-86).  Queries are the Nq token rows; keys / values are those Nq rows followed by M
// memory rows (Nk = Nq + M), and an optional bit mask removes (query, key) pairs from the softmax.
//
// Same numerics contract and MFMA orientation as nrv_attn_gen.hip (bf16 operands, fp32 MFMA accumulation, fp32 softmax in the
// exp2 domain, P fed to P.V in bf16, natural-log LSE), same tile image and same 64-row tiles.  What differs:
//   key sources : key j < Nq is row b*Nq + j of qkv [B*Nq, 3*H*dh] (k / v columns); key j >= Nq is row b*mstride + j - Nq of
//                 mem_kv [*, 2*H*dh] (k columns h*dh.., v columns H*dh + h*dh..).  mstride = 0: one memory set for every
//                 sample; mstride = M: one set per sample.  A 64-key tile may hold rows of both sources.
//   mask        : bit (key & 31) of 32-bit word b*mask_bs + h*mask_hs + q*W + (key >> 5), W = ceil(Nk / 32); 1 = may attend.
//                 A masked score is -FLT_MAX (the reference's masked_fill value; here in the exp2 domain, where -FLT_MAX *
//                 log2e would overflow).  A row whose keys are all masked therefore keeps m = -FLT_MAX, exp2(0) = 1 for
//                 every key: uniform weights, as in the reference; its LSE is written as -FLT_MAX and the backward
//                 recognises it by that value (P = 1 / Nk there, not exp2(s - lse), whose operands would be ~1e38 apart).
//                 No mask and an all-ones mask run the same arithmetic: the results are bit-identical.
//   backward    : query-owner pass (dQ, delta) and key-owner pass (dK, dV) as in nrv_attn_gen.hip; masked pairs carry no
//                 score gradient (masked_fill's backward).  Token keys write dqkv (bf16), memory keys write fp32 per-sample
//                 rows of dmem [B*M, 2*H*dh]; shared memories are then summed over the batch in a fixed order (no atomics).
#include "nrv_attn_common.hpp"

#include <cfloat>

namespace {

using nrv_attn::LN2;
using nrv_attn::LOG2E;
using nrv_attn::pack_frag;

struct MemParams {
    const bf16_t* qkv;       // [B*Nq, 3*H*dh]
    const bf16_t* mkv;       // [*, 2*H*dh] memory keys / values (M > 0)
    const unsigned* mask;    // bit mask or null
    const bf16_t* out;       // [B*Nq, H*dh]   (bwd)
    const bf16_t* dout;      // [B*Nq, H*dh]   (bwd)
    bf16_t* o;               // fwd output
    bf16_t* dqkv;            // bwd output, token rows
    float* dmem;             // bwd output, memory rows [B*M, 2*H*dh]
    float* lse;              // [B, H, Nq]
    float* delta;            // [B, H, Nq]
    long long mstride;       // memory rows per sample step: 0 or M
    long long mask_bs, mask_hs;
    int B, Nq, M, Nk, H, dh, W;
    float scale;
};

constexpr int GT = 64;
constexpr int MEM_THREADS = 256;
constexpr float MASKED = -FLT_MAX;

template <int KS>
struct Cfg {
    static constexpr int DHP = 32 * KS, RB = 2 * DHP, TILE = GT * RB, DT = DHP / 16;
    static constexpr int UNITS = RB / 32;
    static constexpr int UM = UNITS == 2 ? 1 : UNITS == 4 ? 3 : UNITS == 6 ? 1 : 7;
};

template <int KS>
__device__ __forceinline__ int tile_off(int r, int c) {
    using C = Cfg<KS>;
    return r * C::RB + ((((c >> 1) ^ ((r >> 1) & C::UM)) << 5) | ((c & 1) << 4));
}

// k row of key j of (b, h) in either source (v = k + H*dh in both); null for j >= Nk
__device__ __forceinline__ const bf16_t* key_row(const MemParams& p, int b, int h, int j) {
    const long long hd = (long long)p.H * p.dh;
    if (j < p.Nq) return p.qkv + ((long long)b * p.Nq + j) * 3 * hd + hd + (long long)h * p.dh;
    if (j < p.Nk) return p.mkv + ((long long)b * p.mstride + (j - p.Nq)) * 2 * hd + (long long)h * p.dh;
    return nullptr;
}

// rows k0 .. k0 + 63 of the keys and values into registers (zero beyond Nk / dh)
template <int KS>
__device__ __forceinline__ void fetch_kv(u32x4_t (&kv)[KS], u32x4_t (&vv)[KS], const MemParams& p, int b, int h, int k0, int tid) {
    constexpr int CPR = Cfg<KS>::DHP / 8;
    const long long hd = (long long)p.H * p.dh;
#pragma unroll
    for (int i = 0; i < KS; ++i) {
        const int idx = i * MEM_THREADS + tid;
        const int r = idx / CPR, c = idx - r * CPR;
        kv[i] = vv[i] = u32x4_t{0u, 0u, 0u, 0u};
        const bf16_t* row = key_row(p, b, h, k0 + r);
        if (row && c * 8 < p.dh) {
            kv[i] = *reinterpret_cast<const u32x4_t*>(row + c * 8);
            vv[i] = *reinterpret_cast<const u32x4_t*>(row + hd + c * 8);
        }
    }
}
// rows r0 .. r0 + 63 of a [N x dh] slice with row stride ld
template <int KS>
__device__ __forceinline__ void fetch_rows(u32x4_t (&v)[KS], const bf16_t* src, long long ld, int r0, int N, int dh, int tid) {
    constexpr int CPR = Cfg<KS>::DHP / 8;
#pragma unroll
    for (int i = 0; i < KS; ++i) {
        const int idx = i * MEM_THREADS + tid;
        const int r = idx / CPR, c = idx - r * CPR;
        v[i] = u32x4_t{0u, 0u, 0u, 0u};
        if (r0 + r < N && c * 8 < dh) v[i] = *reinterpret_cast<const u32x4_t*>(src + (long long)(r0 + r) * ld + c * 8);
    }
}
template <int KS>
__device__ __forceinline__ void put_tile(char* img, const u32x4_t (&v)[KS], int tid) {
    constexpr int CPR = Cfg<KS>::DHP / 8;
#pragma unroll
    for (int i = 0; i < KS; ++i) {
        const int idx = i * MEM_THREADS + tid;
        const int r = idx / CPR, c = idx - r * CPR;
        *reinterpret_cast<u32x4_t*>(img + tile_off<KS>(r, c)) = v[i];
    }
}
template <int KS>
__device__ __forceinline__ bf16x8_t row_frag(const char* img, int rb, int ks, int lane) {
    return lds_read_b128(img + tile_off<KS>(rb + (lane & 15), 4 * ks + (lane >> 4)));
}
template <int KS>
__device__ __forceinline__ bf16x8_t tr_frag(const char* img, int rb, int dt, int lane) {
    using C = Cfg<KS>;
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
__device__ __forceinline__ float quad_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float quad_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}
// the two mask words of query q for keys k0 .. k0 + 63 (k0 % 64 == 0); all ones without a mask or for padded queries
__device__ __forceinline__ void mask_words(const MemParams& p, int b, int h, int q, int k0, unsigned& w0, unsigned& w1) {
    w0 = w1 = ~0u;
    if (p.mask && q < p.Nq) {
        const unsigned* mr = p.mask + b * p.mask_bs + h * p.mask_hs + (long long)q * p.W;
        const int wi = k0 >> 5;
        w0 = mr[wi];
        w1 = wi + 1 < p.W ? mr[wi + 1] : 0u;
    }
}

// ---------------------------------------------------------------------------------------------
// forward: online softmax over the Nk keys, 64 queries of one (batch, head) per workgroup
// ---------------------------------------------------------------------------------------------
template <int KS>
__global__ __launch_bounds__(MEM_THREADS) void attn_mem_fwd_kernel(const MemParams p) {
    using C = Cfg<KS>;
    __shared__ __attribute__((aligned(16))) char smem[2 * C::TILE];
    char* kimg = smem;
    char* vimg = smem + C::TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, qc = lane & 15;
    const int Nq = p.Nq, Nk = p.Nk, H = p.H, dh = p.dh;
    const int nqb = (Nq + GT - 1) / GT;
    const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
    const int b = bh / H, h = bh - b * H;
    const long long ldq = 3ll * H * dh;
    const bf16_t* qbase = p.qkv + (long long)b * Nq * ldq + h * dh;
    const int q = qb * GT + wave * 16 + qc;
    const float sc = p.scale * LOG2E;

    bf16x8_t qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = frag_of(q < Nq ? qbase + (long long)q * ldq : nullptr, dh, ks, g);
    float m = -INFINITY, l = 0.f;
    f32x4_t ot[C::DT];
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) ot[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    u32x4_t kreg[KS], vreg[KS];
    fetch_kv<KS>(kreg, vreg, p, b, h, 0, tid);
    for (int k0 = 0; k0 < Nk; k0 += GT) {
        unsigned mw0, mw1;
        mask_words(p, b, h, q, k0, mw0, mw1);
        __syncthreads();
        put_tile<KS>(kimg, kreg, tid);
        put_tile<KS>(vimg, vreg, tid);
        __syncthreads();
        if (k0 + GT < Nk) fetch_kv<KS>(kreg, vreg, p, b, h, k0 + GT, tid);
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
                if (!((w >> ((sub & 1) * 16 + 4 * g + e)) & 1u)) v = MASKED;
                a[e] = (k0 + sub * 16 + 4 * g + e < Nk) ? v : -INFINITY;
                tmax = fmaxf(tmax, a[e]);
            }
            st[sub] = a;
        }
        tmax = quad_max(tmax);
        const float mn = fmaxf(m, tmax);                  // finite: every tile holds a key < Nk (masked ones are -FLT_MAX)
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
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
#pragma unroll
        for (int dt = 0; dt < C::DT; ++dt) ot[dt] *= alpha;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const bf16x8_t pf = pack_frag(st[2 * kk], st[2 * kk + 1]);
#pragma unroll
            for (int dt = 0; dt < C::DT; ++dt) ot[dt] = mfma16(tr_frag<KS>(vimg, kk * 32, dt, lane), pf, ot[dt]);
        }
    }
    if (q < Nq) {
        const float inv = 1.0f / l;
        bf16_t* dst = p.o + ((long long)b * Nq + q) * ((long long)H * dh) + h * dh;
#pragma unroll
        for (int dt = 0; dt < C::DT; ++dt) {
            const int d0 = dt * 16 + 4 * g;
            if (d0 < dh) nrv_attn::store_bf16x4(dst + d0, ot[dt] * inv);
        }
        if (g == 0) p.lse[((long long)b * H + h) * Nq + q] = m == MASKED ? MASKED : (m + __builtin_amdgcn_logf(l)) * LN2;
    }
}

// ---------------------------------------------------------------------------------------------
// backward, query-owner pass: dQ = scale * dS K, delta = rowsum(dO o O)
// ---------------------------------------------------------------------------------------------
template <int KS>
__global__ __launch_bounds__(MEM_THREADS) void attn_mem_dq_kernel(const MemParams p) {
    using C = Cfg<KS>;
    __shared__ __attribute__((aligned(16))) char smem[2 * C::TILE];
    char* kimg = smem;
    char* vimg = smem + C::TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, qc = lane & 15;
    const int Nq = p.Nq, Nk = p.Nk, H = p.H, dh = p.dh;
    const int nqb = (Nq + GT - 1) / GT;
    const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
    const int b = bh / H, h = bh - b * H;
    const long long ldq = 3ll * H * dh, ldo = (long long)H * dh;
    const int q = qb * GT + wave * 16 + qc;
    const bool qv = q < Nq;
    const bf16_t* qrow = qv ? p.qkv + ((long long)b * Nq + q) * ldq + h * dh : nullptr;
    const bf16_t* orow = qv ? p.out + ((long long)b * Nq + q) * ldo + h * dh : nullptr;
    const bf16_t* dorow = qv ? p.dout + ((long long)b * Nq + q) * ldo + h * dh : nullptr;
    const float sc = p.scale * LOG2E;

    bf16x8_t qf[KS], dof[KS];
    float dl = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        qf[ks] = frag_of(qrow, dh, ks, g);
        dof[ks] = frag_of(dorow, dh, ks, g);
        const bf16x8_t of = frag_of(orow, dh, ks, g);
#pragma unroll
        for (int e = 0; e < 8; ++e) dl = fmaf(bf16_to_f32((unsigned short)dof[ks][e]), bf16_to_f32((unsigned short)of[e]), dl);
    }
    dl = quad_sum(dl);
    const long long sidx = ((long long)b * H + h) * Nq + (qv ? q : 0);
    const float lsev = qv ? p.lse[sidx] : 0.f;
    // every key masked (lse = -FLT_MAX): P = 1 / Nk, but no pair carries a score gradient, so the row adds nothing to dQ
    const float lse2 = qv && lsev != MASKED ? lsev * LOG2E : INFINITY;      // exp2(s - inf) = 0 for padded queries
    if (qv && g == 0) p.delta[sidx] = dl;

    f32x4_t dqt[C::DT];
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) dqt[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    u32x4_t kreg[KS], vreg[KS];
    fetch_kv<KS>(kreg, vreg, p, b, h, 0, tid);
    for (int k0 = 0; k0 < Nk; k0 += GT) {
        unsigned mw0, mw1;
        mask_words(p, b, h, q, k0, mw0, mw1);
        __syncthreads();
        put_tile<KS>(kimg, kreg, tid);
        put_tile<KS>(vimg, vreg, tid);
        __syncthreads();
        if (k0 + GT < Nk) fetch_kv<KS>(kreg, vreg, p, b, h, k0 + GT, tid);
        f32x4_t ds[4];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            f32x4_t s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                s = mfma16(row_frag<KS>(kimg, sub * 16, ks, lane), qf[ks], s);
                dp = mfma16(row_frag<KS>(vimg, sub * 16, ks, lane), dof[ks], dp);
            }
            const unsigned w = sub < 2 ? mw0 : mw1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool keep = (w >> ((sub & 1) * 16 + 4 * g + e)) & 1u;
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
    if (qv) {
        bf16_t* dst = p.dqkv + ((long long)b * Nq + q) * ldq + h * dh;
#pragma unroll
        for (int dt = 0; dt < C::DT; ++dt) {
            const int d0 = dt * 16 + 4 * g;
            if (d0 < dh) nrv_attn::store_bf16x4(dst + d0, dqt[dt] * p.scale);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// backward, key-owner pass: dV = P^T dO, dK = scale * dS^T Q for 64 keys (token or memory rows) of one (batch, head)
// ---------------------------------------------------------------------------------------------
template <int KS>
__global__ __launch_bounds__(MEM_THREADS) void attn_mem_dkv_kernel(const MemParams p) {
    using C = Cfg<KS>;
    __shared__ __attribute__((aligned(16))) char smem[2 * C::TILE + 5 * GT * 4];
    char* qimg = smem;
    char* doimg = smem + C::TILE;
    float* lse2s = reinterpret_cast<float*>(smem + 2 * C::TILE);
    float* dels = lse2s + GT;
    float* unis = dels + GT;
    unsigned* mws = reinterpret_cast<unsigned*>(unis + GT);          // [2][64]: the mask words of this block's keys per query
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, kc = lane & 15;
    const int Nq = p.Nq, Nk = p.Nk, H = p.H, dh = p.dh;
    const int nkb = (Nk + GT - 1) / GT;
    const int bh = blockIdx.x / nkb, kb = blockIdx.x - bh * nkb;
    const int b = bh / H, h = bh - b * H;
    const long long ldq = 3ll * H * dh, ldo = (long long)H * dh;
    const bf16_t* qbase = p.qkv + (long long)b * Nq * ldq + h * dh;
    const bf16_t* dobase = p.dout + (long long)b * Nq * ldo + h * dh;
    const float* lse = p.lse + ((long long)b * H + h) * Nq;
    const float* delta = p.delta + ((long long)b * H + h) * Nq;
    const unsigned* mbase = p.mask ? p.mask + b * p.mask_bs + h * p.mask_hs : nullptr;
    const int kl = wave * 16 + kc;                        // this lane's key within the block
    const int key = kb * GT + kl;
    const int msel = kl >> 5, mbit = kl & 31;
    const float sc = p.scale * LOG2E;
    const float inv_nk = 1.0f / (float)Nk;

    const bf16_t* krow = key_row(p, b, h, key);
    bf16x8_t kf[KS], vf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        kf[ks] = frag_of(krow, dh, ks, g);
        vf[ks] = frag_of(krow ? krow + ldo : nullptr, dh, ks, g);
    }
    f32x4_t dkt[C::DT], dvt[C::DT];
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) dkt[dt] = dvt[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    u32x4_t qreg[KS], doreg[KS];
    for (int q0 = 0; q0 < Nq; q0 += GT) {
        __syncthreads();
        fetch_rows<KS>(qreg, qbase, ldq, q0, Nq, dh, tid);
        fetch_rows<KS>(doreg, dobase, ldo, q0, Nq, dh, tid);
        if (tid < GT) {
            const int qq = q0 + tid;
            const float lv = qq < Nq ? lse[qq] : 0.f;
            const bool full = lv == MASKED;
            lse2s[tid] = qq < Nq && !full ? lv * LOG2E : INFINITY;
            dels[tid] = qq < Nq ? delta[qq] : 0.f;
            unis[tid] = full ? inv_nk : 0.f;
        } else if (tid < 3 * GT) {
            const int i = tid - GT, qq = q0 + (i & 63), wi = kb * 2 + (i >> 6);
            mws[i] = (mbase && qq < Nq) ? (wi < p.W ? mbase[(long long)qq * p.W + wi] : 0u) : ~0u;
        }
        put_tile<KS>(qimg, qreg, tid);
        put_tile<KS>(doimg, doreg, tid);
        __syncthreads();
        f32x4_t pt[4], ds[4];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            f32x4_t s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                s = mfma16(row_frag<KS>(qimg, sub * 16, ks, lane), kf[ks], s);
                dp = mfma16(row_frag<KS>(doimg, sub * 16, ks, lane), vf[ks], dp);
            }
            const f32x4_t l4 = *reinterpret_cast<const f32x4_t*>(lse2s + sub * 16 + 4 * g);
            const f32x4_t d4 = *reinterpret_cast<const f32x4_t*>(dels + sub * 16 + 4 * g);
            const f32x4_t u4 = *reinterpret_cast<const f32x4_t*>(unis + sub * 16 + 4 * g);
            const u32x4_t w4 = *reinterpret_cast<const u32x4_t*>(mws + msel * GT + sub * 16 + 4 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool keep = (w4[e] >> mbit) & 1u;
                const float pv = keep ? __builtin_amdgcn_exp2f(fmaf(s[e], sc, -l4[e])) : u4[e];
                pt[sub][e] = pv;
                ds[sub][e] = keep ? pv * (dp[e] - d4[e]) : 0.f;
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
    if (key < Nq) {
        bf16_t* dk = p.dqkv + ((long long)b * Nq + key) * ldq + ldo + h * dh;
        bf16_t* dv = dk + ldo;
#pragma unroll
        for (int dt = 0; dt < C::DT; ++dt) {
            const int d0 = dt * 16 + 4 * g;
            if (d0 < dh) {
                nrv_attn::store_bf16x4(dk + d0, dkt[dt] * p.scale);
                nrv_attn::store_bf16x4(dv + d0, dvt[dt]);
            }
        }
    } else if (key < Nk) {
        float* dk = p.dmem + ((long long)b * p.M + (key - Nq)) * 2 * ldo + h * dh;
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

template <int KS>
int launch_fwd(const MemParams& p, hipStream_t s) {
    const long long grid = (long long)p.B * p.H * ((p.Nq + GT - 1) / GT);
    hipLaunchKernelGGL(attn_mem_fwd_kernel<KS>, dim3((unsigned)grid), dim3(MEM_THREADS), 0, s, p);
    NRV_CHECK_LAUNCH();
    return 0;
}
template <int KS>
int launch_bwd(const MemParams& p, hipStream_t s) {
    const long long gq = (long long)p.B * p.H * ((p.Nq + GT - 1) / GT);
    const long long gk = (long long)p.B * p.H * ((p.Nk + GT - 1) / GT);
    hipLaunchKernelGGL(attn_mem_dq_kernel<KS>, dim3((unsigned)gq), dim3(MEM_THREADS), 0, s, p);
    NRV_CHECK_LAUNCH();
    hipLaunchKernelGGL(attn_mem_dkv_kernel<KS>, dim3((unsigned)gk), dim3(MEM_THREADS), 0, s, p);
    NRV_CHECK_LAUNCH();
    return 0;
}

bool aligned4(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3u) == 0; }

// shape / stride checks shared by the forward and the backward (before any pointer is touched)
int check_args(int B, int Nq, int M, int H, int dh, long long mstride, long long mask_bs, long long mask_hs) {
    if (B <= 0 || Nq <= 0 || H <= 0 || M < 0 || ks_of(dh) == 0) return NRV_ERR_SHAPE;
    if (M > 0 && mstride != 0 && mstride != M) return NRV_ERR_SHAPE;
    if (mask_bs < 0 || mask_hs < 0) return NRV_ERR_SHAPE;
    const long long Nk = (long long)Nq + M;
    if (Nk > 0x7fffffffll - GT) return NRV_ERR_SHAPE;
    if ((long long)B * H * ((Nk + GT - 1) / GT) > 0x7fffffffll) return NRV_ERR_SHAPE;
    return 0;
}

void fill(MemParams& p, const void* qkv, const void* mem_kv, long long mstride, int M, const unsigned* mask, long long mask_bs,
          long long mask_hs, int B, int Nq, int H, int dh, float scale) {
    p.qkv = static_cast<const bf16_t*>(qkv);
    p.mkv = static_cast<const bf16_t*>(mem_kv);
    p.mask = mask;
    p.mstride = mstride;
    p.mask_bs = mask_bs; p.mask_hs = mask_hs;
    p.B = B; p.Nq = Nq; p.M = M; p.Nk = Nq + M; p.H = H; p.dh = dh; p.W = (Nq + M + 31) / 32;
    p.scale = scale;
}

}  // namespace

extern "C" int nrv_attn_mem_fwd(const void* qkv_bf16, const void* mem_kv_bf16, int64_t mem_bstride, int M,
                                const uint32_t* mask, int64_t mask_bstride, int64_t mask_hstride,
                                void* out_bf16, float* lse, int B, int Nq, int H, int dh, float scale, void* stream) {
    if (!qkv_bf16 || !out_bf16 || !lse || (M > 0 && !mem_kv_bf16)) return NRV_ERR_NULL;
    if (int rc = check_args(B, Nq, M, H, dh, mem_bstride, mask_bstride, mask_hstride)) return rc;
    if (!nrv_aligned16(qkv_bf16) || !nrv_aligned16(out_bf16) || (M > 0 && !nrv_aligned16(mem_kv_bf16)) || !aligned4(lse) ||
        (mask && !aligned4(mask)))
        return NRV_ERR_ALIGN;
    MemParams p{};
    fill(p, qkv_bf16, mem_kv_bf16, mem_bstride, M, mask, mask_bstride, mask_hstride, B, Nq, H, dh, scale);
    p.o = static_cast<bf16_t*>(out_bf16);
    p.lse = lse;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (ks_of(dh)) {
        case 1: return launch_fwd<1>(p, s);
        case 2: return launch_fwd<2>(p, s);
        case 3: return launch_fwd<3>(p, s);
        default: return launch_fwd<4>(p, s);
    }
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
    MemParams p{};
    fill(p, qkv_bf16, mem_kv_bf16, mem_bstride, M, mask, mask_bstride, mask_hstride, B, Nq, H, dh, scale);
    p.out = static_cast<const bf16_t*>(out_bf16);
    p.dout = static_cast<const bf16_t*>(dout_bf16);
    p.dqkv = static_cast<bf16_t*>(dqkv_bf16);
    p.dmem = dmem_f32;
    p.lse = const_cast<float*>(lse);
    p.delta = delta_ws;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc;
    switch (ks_of(dh)) {
        case 1: rc = launch_bwd<1>(p, s); break;
        case 2: rc = launch_bwd<2>(p, s); break;
        case 3: rc = launch_bwd<3>(p, s); break;
        default: rc = launch_bwd<4>(p, s); break;
    }
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
