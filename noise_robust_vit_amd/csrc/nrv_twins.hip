// Twins-SVT kernels (gfx950): sub-sampled global attention (every query of a map against at most 128 pooled keys of its sample,
// twins_svt.py:123-154) and the position-encoding generator PEG (x + depthwise conv(x) + bias on the fp32 stream,
// twins_svt.py:81-87).
//
// subattn.  One workgroup of four waves owns the fixed chunk of SA_CHUNK query rows `chunk` of one (sample, head).  It stages the
// head's K and V once as LDS row images [32 * NKS keys][dh + 8] (rows >= Nk are zeros, never read from memory), NKS =
// ceil(Nk / 32).  Scores are formed TRANSPOSED, S^T = K Q^T, with mfma_f32_16x16x32_bf16: a lane then holds the keys 16 kb + 4 g + r
// (g = lane >> 4, r = register) of ONE query (lane & 15), so the row statistics are sums over its registers and two lane
// exchanges (xor 16, 32), and the accumulator registers of two key blocks, packed to bf16, are the B operand of the products
// that sum over keys (O^T = V^T P^T, dQ^T = K^T dS^T) with no lane movement: the k order of such a fragment is
// key = 32 s + 16 (j >> 2) + 4 g + (j & 3), which is the order ds_read_b64_tr_b16 delivers from the row images.
//   forward : a wave walks the 16-row query tiles wave, wave + 4, ... of the chunk.  e = exp(scale s - m) is rounded to bf16 once
//             for P V; l sums the unrounded e; out = bf16(acc / l), lse = m + log l.
//   backward: the workgroup walks the chunk in steps of 64 rows.  Q and dO of the step are staged as row images; wave w takes
//             rows 16 w .. 16 w + 15: P^T = exp(scale s - lse), dP^T = V dO^T, dS^T = P^T (dP^T - sum_keys P^T dP^T) -- every key
//             of a row is on chip, so no saved delta (and no `out`) is needed -- dQ from the registers, and P, dS (bf16, the one
//             rounding both of their products see) go to LDS as [row][key] images.  After a barrier wave w owns the key blocks
//             w, w + 4: dK += dS^T Q and dV += P^T dO over the 64 rows with transposed reads of the four images, in fp32
//             registers across all steps.  A key block has one owner: no sum across waves, no atomics.  One fp32 partial
//             [2][32 NKS][dh] per chunk; subattn_red_kernel adds the chunks in index order and stores bf16 dk / dv.
//             SA_CHUNK is a constant: the order of every sum, and with it the bits, is the same on every machine.
//   LDS (dh 64, Nk 128): forward 2 * 128 * 72 * 2 = 36 864 B static; backward 36 864 + 2 * 64 * 72 * 2 + 2 * 64 * 136 * 2 =
//             90 112 B dynamic (one workgroup per CU).  Registers at <dh 64, Nk 128>: forward 73 VGPRs + 16 AGPRs, backward
//             177 VGPRs + 80 AGPRs (one wave per SIMD, which the LDS budget allows anyway); no scratch in either.
//
// PEG.  Memory-bound fp32: one thread = (token, 4 channels), the taps through the caches (a 3 x 3 halo re-reads every input 9
// times from L1 / L2, as nrv_pool_dwconv_* does).  dw / dbias: per-sample partials added in index order by tap_wred_kernel
// (nrv_rows.hpp), which the Pool layer's and the 3x3 depthwise convolution's backward share.  Grids are exact.
#include "nrv_attn_common.hpp"
#include "nrv_rows.hpp"

#include <cmath>

namespace {

using nrv_attn::pack_frag;
using nrv_attn::store_bf16x4;

constexpr int SA_CHUNK = 512;    // query rows per workgroup (fixed: the summation order depends on nothing else)
constexpr int SA_STEP = 64;      // rows per backward step: 4 waves x one 16-row tile
constexpr int SA_MAXNK = 128;

struct SubParams {
    const bf16_t* q;
    const bf16_t* k;
    const bf16_t* v;
    const bf16_t* dout;    // [B*Nq, H*dh]          (bwd)
    bf16_t* out;           // [B*Nq, H*dh]          (fwd)
    bf16_t* dq;            // laid out like q       (bwd)
    float* lse;            // [B, H, Nq]
    float* part;           // [B*H, chunks, 2, nkp, dh]   (bwd)
    long long ldq, ldk, ldv;
    int Nq, Nk, H, chunks, nkp;
    float scale;
};

// rows of a [rows_img][DH] slice (row stride ld) -> an LDS row image with LD elements per row; rows >= rows_valid are zeros
template <int DH, int LD>
__device__ __forceinline__ void stage_rows(bf16_t* img, const bf16_t* __restrict__ src, long long ld, int rows_img, int rows_valid) {
    constexpr int CH = DH / 8;
    for (int idx = threadIdx.x; idx < rows_img * CH; idx += 256) {
        const int r = idx / CH, c = idx - r * CH;
        u32x4_t v = {0u, 0u, 0u, 0u};
        if (r < rows_valid) v = *reinterpret_cast<const u32x4_t*>(src + (long long)r * ld + c * 8);
        *reinterpret_cast<u32x4_t*>(img + r * LD + c * 8) = v;
    }
}

// fragment with the image's row on the lane: element j = img[r0 + (lane & 15)][32 ks + 8 (lane >> 4) + j]
template <int LD>
__device__ __forceinline__ bf16x8_t row_frag(const bf16_t* img, int r0, int ks, int lane) {
    return lds_read_b128(img + (r0 + (lane & 15)) * LD + 32 * ks + 8 * (lane >> 4));
}

// fragment with the image's column on the lane: element j = img[rb + 16 (j >> 2) + 4 (lane >> 4) + (j & 3)][16 dt + (lane & 15)]
template <int LD>
__device__ __forceinline__ bf16x8_t tr_frag(const bf16_t* img, int rb, int dt, int lane) {
    const int g = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
    const bf16_t* a0 = img + (rb + 4 * g + qq) * LD + 16 * dt + 4 * pp;
    return cat4(lds_read_tr16_b64(a0), lds_read_tr16_b64(a0 + 16 * LD));
}

// scale * s as one fp32 rounding in BOTH kernels: the empty asm keeps the compiler from fusing the product into the
// subtraction of the row maximum / of lse that follows (an FMA there leaves P = 1 + an ulp for a single key instead of 1)
__device__ __forceinline__ float scaled_score(float acc, float scale) {
    float v = acc * scale;
    asm("" : "+v"(v));
    return v;
}

template <int DH, int NKS>
__global__ __launch_bounds__(256) void subattn_fwd_kernel(SubParams p) {
    constexpr int LD = DH + 8, NKB = 2 * NKS, KS = DH / 32, DT = DH / 16;
    __shared__ __attribute__((aligned(16))) bf16_t sk[NKS * 32 * LD];
    __shared__ __attribute__((aligned(16))) bf16_t sv[NKS * 32 * LD];
    const int chunk = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c15 = lane & 15;
    const int Nk = p.Nk;
    stage_rows<DH, LD>(sk, p.k + (long long)b * Nk * p.ldk + h * DH, p.ldk, NKS * 32, Nk);
    stage_rows<DH, LD>(sv, p.v + (long long)b * Nk * p.ldv + h * DH, p.ldv, NKS * 32, Nk);
    __syncthreads();
    const int q_begin = chunk * SA_CHUNK;
    const int q_end = p.Nq - q_begin < SA_CHUNK ? p.Nq : q_begin + SA_CHUNK;
    for (int q0 = q_begin + 16 * wave; q0 < q_end; q0 += 64) {
        const int q = q0 + c15;
        const bool ok = q < q_end;
        const bf16_t* qp = p.q + ((long long)b * p.Nq + q) * p.ldq + h * DH + 8 * g;
        bf16x8_t qf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = ok ? *reinterpret_cast<const bf16x8_t*>(qp + 32 * ks) : bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
        f32x4_t s[NKB];
        float m = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
            if (16 * kb < Nk) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) acc = mfma16(row_frag<LD>(sk, 16 * kb, ks, lane), qf[ks], acc);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = 16 * kb + 4 * g + r < Nk ? scaled_score(acc[r], p.scale) : -INFINITY;
                s[kb][r] = v;
                m = fmaxf(m, v);
            }
        }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float l = 0.f;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __expf(s[kb][r] - m);
                s[kb][r] = e;
                l += e;
            }
        }
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        f32x4_t o[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s2 = 0; s2 < NKS; ++s2) {
            if (32 * s2 < Nk) {
                const bf16x8_t pf = pack_frag(s[2 * s2], s[2 * s2 + 1]);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) o[dt] = mfma16(tr_frag<LD>(sv, 32 * s2, dt, lane), pf, o[dt]);
            }
        }
        if (ok) {
            const float rl = 1.0f / l;
            bf16_t* op = p.out + (((long long)b * p.Nq + q) * p.H + h) * DH + 4 * g;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) store_bf16x4(op + 16 * dt, o[dt] * rl);
            if (g == 0) p.lse[((long long)b * p.H + h) * p.Nq + q] = m + __logf(l);
        }
    }
}

extern __shared__ __attribute__((aligned(16))) char sa_smem[];

template <int DH, int NKS>
constexpr size_t subattn_bwd_lds() {
    return (size_t)2 * (2 * NKS * 32 * (DH + 8) + 2 * SA_STEP * (DH + 8) + 2 * SA_STEP * (NKS * 32 + 8));      // K, V; Q, dO; dS, P
}

template <int DH, int NKS>
__global__ __launch_bounds__(256) void subattn_bwd_kernel(SubParams p) {
    constexpr int LD = DH + 8, LX = NKS * 32 + 8, NKB = 2 * NKS, KS = DH / 32, DT = DH / 16, KBW = (NKB + 3) / 4;
    bf16_t* sk = reinterpret_cast<bf16_t*>(sa_smem);
    bf16_t* sv = sk + NKS * 32 * LD;
    bf16_t* sq = sv + NKS * 32 * LD;
    bf16_t* sdo = sq + SA_STEP * LD;
    bf16_t* xs = sdo + SA_STEP * LD;          // dS of the step, [row][key]
    bf16_t* xp = xs + SA_STEP * LX;           // P of the step
    const int chunk = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c15 = lane & 15;
    const int Nk = p.Nk;
    stage_rows<DH, LD>(sk, p.k + (long long)b * Nk * p.ldk + h * DH, p.ldk, NKS * 32, Nk);
    stage_rows<DH, LD>(sv, p.v + (long long)b * Nk * p.ldv + h * DH, p.ldv, NKS * 32, Nk);
    const int q_begin = chunk * SA_CHUNK;
    const int q_end = p.Nq - q_begin < SA_CHUNK ? p.Nq : q_begin + SA_CHUNK;
    f32x4_t dka[KBW][DT], dva[KBW][DT];
#pragma unroll
    for (int i = 0; i < KBW; ++i)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            dka[i][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            dva[i][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
    for (int s0 = q_begin; s0 < q_end; s0 += SA_STEP) {
        __syncthreads();                       // the previous step's key owners are done with the four step images
        const int rows = q_end - s0 < SA_STEP ? q_end - s0 : SA_STEP;
        stage_rows<DH, LD>(sq, p.q + ((long long)b * p.Nq + s0) * p.ldq + h * DH, p.ldq, SA_STEP, rows);
        stage_rows<DH, LD>(sdo, p.dout + (((long long)b * p.Nq + s0) * p.H + h) * DH, (long long)p.H * DH, SA_STEP, rows);
        __syncthreads();
        {
            // row phase: this wave's 16 rows against every key
            const int q = s0 + 16 * wave + c15;
            const bool ok = q < q_end;
            const float lse = ok ? p.lse[((long long)b * p.H + h) * p.Nq + q] : INFINITY;      // rows past the end: P = 0
            bf16x8_t qf[KS], dof[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                qf[ks] = row_frag<LD>(sq, 16 * wave, ks, lane);
                dof[ks] = row_frag<LD>(sdo, 16 * wave, ks, lane);
            }
            f32x4_t pr[NKB], ds[NKB];
            float delta = 0.f;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                f32x4_t as = {0.f, 0.f, 0.f, 0.f}, ad = {0.f, 0.f, 0.f, 0.f};
                if (16 * kb < Nk) {
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        as = mfma16(row_frag<LD>(sk, 16 * kb, ks, lane), qf[ks], as);
                        ad = mfma16(row_frag<LD>(sv, 16 * kb, ks, lane), dof[ks], ad);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // the forward's own rounding of scale * s (scaled_score): a single key gives P = 1 and dS = 0 exactly
                    const float pv = 16 * kb + 4 * g + r < Nk ? __expf(scaled_score(as[r], p.scale) - lse) : 0.f;
                    pr[kb][r] = pv;
                    ds[kb][r] = ad[r];
                    delta = fmaf(pv, ad[r], delta);
                }
            }
            delta += __shfl_xor(delta, 16, 64);
            delta += __shfl_xor(delta, 32, 64);
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) ds[kb][r] = pr[kb][r] * (ds[kb][r] - delta);
            f32x4_t dq[DT];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) dq[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s2 = 0; s2 < NKS; ++s2) {
                if (32 * s2 < Nk) {
                    const bf16x8_t df = pack_frag(ds[2 * s2], ds[2 * s2 + 1]);
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) dq[dt] = mfma16(tr_frag<LD>(sk, 32 * s2, dt, lane), df, dq[dt]);
                }
            }
            if (ok) {
                bf16_t* dp = p.dq + ((long long)b * p.Nq + q) * p.ldq + h * DH + 4 * g;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) store_bf16x4(dp + 16 * dt, dq[dt] * p.scale);
            }
            const int row = 16 * wave + c15;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                store_bf16x4(xs + row * LX + 16 * kb + 4 * g, ds[kb]);
                store_bf16x4(xp + row * LX + 16 * kb + 4 * g, pr[kb]);
            }
        }
        __syncthreads();
        // key phase: this wave's key blocks against the 64 rows of the step
#pragma unroll
        for (int i = 0; i < KBW; ++i) {
            const int kb = wave + 4 * i;
            if (kb < NKB && 16 * kb < Nk) {
#pragma unroll
                for (int h2 = 0; h2 < SA_STEP / 32; ++h2) {
                    const bf16x8_t fs = tr_frag<LX>(xs, 32 * h2, kb, lane), fp = tr_frag<LX>(xp, 32 * h2, kb, lane);
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) {
                        dka[i][dt] = mfma16(fs, tr_frag<LD>(sq, 32 * h2, dt, lane), dka[i][dt]);
                        dva[i][dt] = mfma16(fp, tr_frag<LD>(sdo, 32 * h2, dt, lane), dva[i][dt]);
                    }
                }
            }
        }
    }
    float* part = p.part + (((long long)b * p.H + h) * p.chunks + chunk) * 2ll * p.nkp * DH;
#pragma unroll
    for (int i = 0; i < KBW; ++i) {
        const int kb = wave + 4 * i;
        if (kb < NKB && 16 * kb < Nk) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = 16 * kb + 4 * g + r;
                    part[key * DH + 16 * dt + c15] = dka[i][dt][r] * p.scale;
                    part[(p.nkp + key) * DH + 16 * dt + c15] = dva[i][dt][r];
                }
        }
    }
}

// dk / dv = the chunks' partials added in index order, one bf16 rounding.  One thread = 8 features of one key of dk or dv.
__global__ __launch_bounds__(256) void subattn_red_kernel(const float* __restrict__ part, bf16_t* __restrict__ dk, bf16_t* __restrict__ dv,
                                                          long long ldk, long long ldv, long long items, int H, int Nk, int nkp, int chunks,
                                                          int dh) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int c8 = dh >> 3;
    const int c = (int)(i % c8) * 8;
    long long r = i / c8;
    const int key = (int)(r % Nk);
    r /= Nk;
    const int which = (int)(r & 1);
    const long long bh = r >> 1;
    const float* src = part + ((bh * chunks * 2 + which) * nkp + key) * dh + c;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < chunks; ++ch) {
        const f32x4_t a = *reinterpret_cast<const f32x4_t*>(src), bq = *reinterpret_cast<const f32x4_t*>(src + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { acc[e] += a[e]; acc[4 + e] += bq[e]; }
        src += 2ll * nkp * dh;
    }
    const long long b = bh / H;
    const int h = (int)(bh - b * H);
    bf16_t* dst = which ? dv + (b * Nk + key) * ldv : dk + (b * Nk + key) * ldk;
    store_row(dst + h * dh + c, acc);
}

int sub_chunks(int Nq) { return (int)nrv_cdiv(Nq, SA_CHUNK); }
int sub_nkp(int Nk) { return (int)nrv_cdiv(Nk, 32) * 32; }

bool sub_shape_ok(int B, int H, int Nq, int Nk, int dh, long long ldq, long long ldk, long long ldv) {
    if (!(B >= 1 && B <= 65535 && H >= 1 && H <= 65535 && Nq >= 1 && Nk >= 1 && Nk <= SA_MAXNK && (dh == 32 || dh == 64))) return false;
    const long long w = (long long)H * dh;
    if (ldq < w || ldk < w || ldv < w || ldq % 8 || ldk % 8 || ldv % 8) return false;
    return (long long)B * Nq <= (1ll << 40) / ldq && (long long)B * Nk <= (1ll << 40) / (ldk > ldv ? ldk : ldv);
}

size_t sub_workspace(int B, int H, int Nq, int Nk, int dh) {
    return (size_t)B * H * sub_chunks(Nq) * 2 * sub_nkp(Nk) * dh * sizeof(float);
}

template <int DH, int NKS>
int sub_fwd_launch(const SubParams& p, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL((subattn_fwd_kernel<DH, NKS>), grid, dim3(256), 0, st, p);
    NRV_CHECK_LAUNCH();
    return 0;
}

template <int DH, int NKS>
int sub_bwd_launch(const SubParams& p, dim3 grid, hipStream_t st) {
    constexpr size_t lds = subattn_bwd_lds<DH, NKS>();
    static int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(subattn_bwd_kernel<DH, NKS>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (attr) return attr;
    hipLaunchKernelGGL((subattn_bwd_kernel<DH, NKS>), grid, dim3(256), lds, st, p);
    NRV_CHECK_LAUNCH();
    return 0;
}

#define SUB_DISPATCH(FN, p, grid, st, dh, nks)                                            \
    do {                                                                                  \
        if (dh == 32) {                                                                   \
            if (nks == 1) return FN<32, 1>(p, grid, st);                                  \
            if (nks == 2) return FN<32, 2>(p, grid, st);                                  \
            if (nks == 3) return FN<32, 3>(p, grid, st);                                  \
            return FN<32, 4>(p, grid, st);                                                \
        }                                                                                 \
        if (nks == 1) return FN<64, 1>(p, grid, st);                                      \
        if (nks == 2) return FN<64, 2>(p, grid, st);                                      \
        if (nks == 3) return FN<64, 3>(p, grid, st);                                      \
        return FN<64, 4>(p, grid, st);                                                    \
    } while (0)

int sub_fwd_dispatch(const SubParams& p, dim3 grid, hipStream_t st, int dh, int nks) { SUB_DISPATCH(sub_fwd_launch, p, grid, st, dh, nks); }
int sub_bwd_dispatch(const SubParams& p, dim3 grid, hipStream_t st, int dh, int nks) { SUB_DISPATCH(sub_bwd_launch, p, grid, st, dh, nks); }

// ---------------------------------------------------------------------------------------------
// PEG: out = x + bias[c] + sum_t w[c, t] x(p + off_t) on fp32 rows [B*H*W, C]
// ---------------------------------------------------------------------------------------------
// one thread = (token, 4 channels).  FLIP = false: dst = src + bias + conv(src), t = ky * KS + kx ascending.
// FLIP = true (the input gradient): dst = src + the gather of src through the flipped taps, no bias.
template <int KS, bool FLIP>
__global__ __launch_bounds__(256) void peg_conv_kernel(const float* __restrict__ src, const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ dst, long long items, int H, int W, int C) {
    constexpr int R = KS / 2, KK = KS * KS;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int c4 = C >> 2;
    const long long tok = i / c4;
    const int c = (int)(i - tok * c4) * 4;
    const long long b = tok / ((long long)H * W);
    const int rem = (int)(tok - b * H * W);
    const int y = rem / W, x = rem - y * W;
    const float* sb = src + b * H * W * C + c;
    const float* wc = w + (long long)c * KK;
    f32x4_t acc = *reinterpret_cast<const f32x4_t*>(src + tok * C + c);
    if (!FLIP) {
        const f32x4_t bv = *reinterpret_cast<const f32x4_t*>(bias + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += bv[j];
    }
#pragma unroll
    for (int ky = 0; ky < KS; ++ky) {
        const int iy = y + ky - R;
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
            const int ix = x + kx - R;
            if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
            const f32x4_t xv = *reinterpret_cast<const f32x4_t*>(sb + ((long long)iy * W + ix) * C);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(wc[j * KK + (FLIP ? KK - 1 - (ky * KS + kx) : ky * KS + kx)], xv[j], acc[j]);
        }
    }
    *reinterpret_cast<f32x4_t*>(dst + tok * C + c) = acc;
}

// per-sample partials: part[(b * (KK + 1) + t) * C + c] = sum over the tokens in row-major order of dy(b, p, c) x(b, p + off_t, c)
// for t < KK, of dy(b, p, c) for t = KK (the bias).  One thread = one partial; c is the fastest index.
__global__ __launch_bounds__(256) void peg_dw_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ part,
                                                     long long items, int H, int W, int C, int ks) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int KK = ks * ks, R = ks / 2;
    const int c = (int)(i % C);
    const long long r = i / C;
    const int t = (int)(r % (KK + 1));
    const long long b = r / (KK + 1);
    const int ky = t / ks, kx = t - ky * ks;
    const float* xb = x + b * H * W * C + c;
    const float* db = dy + b * H * W * C + c;
    float acc = 0.f;
    for (int y = 0; y < H; ++y) {
        const int iy = y + ky - R;
        if (t < KK && (iy < 0 || iy >= H)) continue;
        for (int xx = 0; xx < W; ++xx) {
            const float gq = db[((long long)y * W + xx) * C];
            if (t == KK) { acc += gq; continue; }
            const int ix = xx + kx - R;
            if (ix < 0 || ix >= W) continue;
            acc = fmaf(gq, xb[((long long)iy * W + ix) * C], acc);
        }
    }
    part[i] = acc;
}

bool peg_shape_ok(int B, int H, int W, int C, int ks) {
    if (!(B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W <= (1ll << 24) && C > 0 && C % 8 == 0 && C <= (1 << 20) &&
          (ks == 3 || ks == 5 || ks == 7)))
        return false;
    const long long rows = (long long)B * H * W;
    return rows * C <= (1ll << 40) && nrv_cdiv(rows * (C / 4), 256) <= NRV_MAX_BLOCKS && nrv_cdiv((long long)B * 50 * C, 256) <= NRV_MAX_BLOCKS;
}

template <bool FLIP>
void peg_conv_launch(const float* src, const float* w, const float* bias, float* dst, int B, int H, int W, int C, int ks, hipStream_t st) {
    const long long items = (long long)B * H * W * (C / 4);
    const dim3 grid((unsigned)nrv_cdiv(items, 256));
    NRV_DISPATCH_KS(ks, hipLaunchKernelGGL((peg_conv_kernel<KS, FLIP>), grid, dim3(256), 0, st, src, w, bias, dst, items, H, W, C));
}

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" int nrv_subattn_plan(int Nq, int Nk, int dh, nrv_subattn_plan_t* plan) {
    if (!plan) return NRV_ERR_NULL;
    if (!sub_shape_ok(1, 1, Nq, Nk, dh, dh, dh, dh)) return NRV_ERR_SHAPE;
    plan->chunk = SA_CHUNK;
    plan->chunks = sub_chunks(Nq);
    plan->nk_pad = sub_nkp(Nk);
    return 0;
}

extern "C" int nrv_subattn_fwd(const void* q_bf16, int64_t ldq, const void* k_bf16, int64_t ldk, const void* v_bf16, int64_t ldv,
                               void* out_bf16, float* lse, int B, int H, int Nq, int Nk, int dh, float scale, void* stream) {
    if (!sub_shape_ok(B, H, Nq, Nk, dh, ldq, ldk, ldv)) return NRV_ERR_SHAPE;
    if (!q_bf16 || !k_bf16 || !v_bf16 || !out_bf16 || !lse) return NRV_ERR_NULL;
    if (!nrv_aligned16(q_bf16) || !nrv_aligned16(k_bf16) || !nrv_aligned16(v_bf16) || !nrv_aligned16(out_bf16) ||
        (reinterpret_cast<uintptr_t>(lse) & 3u))
        return NRV_ERR_ALIGN;
    SubParams p{};
    p.q = static_cast<const bf16_t*>(q_bf16); p.k = static_cast<const bf16_t*>(k_bf16); p.v = static_cast<const bf16_t*>(v_bf16);
    p.out = static_cast<bf16_t*>(out_bf16); p.lse = lse;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv;
    p.Nq = Nq; p.Nk = Nk; p.H = H; p.chunks = sub_chunks(Nq); p.nkp = sub_nkp(Nk); p.scale = scale;
    return sub_fwd_dispatch(p, dim3((unsigned)p.chunks, (unsigned)H, (unsigned)B), static_cast<hipStream_t>(stream), dh, p.nkp / 32);
}

extern "C" size_t nrv_subattn_bwd_workspace(int B, int H, int Nq, int Nk, int dh) {
    if (!sub_shape_ok(B, H, Nq, Nk, dh, (long long)H * dh, (long long)H * dh, (long long)H * dh)) return 0;
    return sub_workspace(B, H, Nq, Nk, dh);
}

extern "C" int nrv_subattn_bwd(const void* q_bf16, int64_t ldq, const void* k_bf16, int64_t ldk, const void* v_bf16, int64_t ldv,
                               const void* dout_bf16, const float* lse, void* dq_bf16, void* dk_bf16, void* dv_bf16, void* workspace,
                               size_t workspace_bytes, int B, int H, int Nq, int Nk, int dh, float scale, void* stream) {
    if (!sub_shape_ok(B, H, Nq, Nk, dh, ldq, ldk, ldv)) return NRV_ERR_SHAPE;
    if (!q_bf16 || !k_bf16 || !v_bf16 || !dout_bf16 || !lse || !dq_bf16 || !dk_bf16 || !dv_bf16 || !workspace) return NRV_ERR_NULL;
    if (workspace_bytes < sub_workspace(B, H, Nq, Nk, dh)) return NRV_ERR_WORKSPACE;
    if (!nrv_aligned16(q_bf16) || !nrv_aligned16(k_bf16) || !nrv_aligned16(v_bf16) || !nrv_aligned16(dout_bf16) || !nrv_aligned16(dq_bf16) ||
        !nrv_aligned16(dk_bf16) || !nrv_aligned16(dv_bf16) || !nrv_aligned16(workspace) || (reinterpret_cast<uintptr_t>(lse) & 3u))
        return NRV_ERR_ALIGN;
    SubParams p{};
    p.q = static_cast<const bf16_t*>(q_bf16); p.k = static_cast<const bf16_t*>(k_bf16); p.v = static_cast<const bf16_t*>(v_bf16);
    p.dout = static_cast<const bf16_t*>(dout_bf16); p.dq = static_cast<bf16_t*>(dq_bf16); p.lse = const_cast<float*>(lse);
    p.part = static_cast<float*>(workspace);
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv;
    p.Nq = Nq; p.Nk = Nk; p.H = H; p.chunks = sub_chunks(Nq); p.nkp = sub_nkp(Nk); p.scale = scale;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int e = sub_bwd_dispatch(p, dim3((unsigned)p.chunks, (unsigned)H, (unsigned)B), st, dh, p.nkp / 32);
    if (e) return e;
    const long long items = (long long)B * H * 2 * Nk * (dh / 8);
    hipLaunchKernelGGL(subattn_red_kernel, dim3((unsigned)nrv_cdiv(items, 256)), dim3(256), 0, st, p.part, static_cast<bf16_t*>(dk_bf16),
                       static_cast<bf16_t*>(dv_bf16), (long long)ldk, (long long)ldv, items, H, Nk, p.nkp, p.chunks, dh);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nrv_peg_fwd(const float* x_f32, const float* w, const float* bias, float* out_f32, int B, int H, int W, int C, int ks,
                           void* stream) {
    if (!peg_shape_ok(B, H, W, C, ks)) return NRV_ERR_SHAPE;
    if (!x_f32 || !w || !bias || !out_f32) return NRV_ERR_NULL;
    if (!nrv_aligned16(x_f32) || !nrv_aligned16(bias) || !nrv_aligned16(out_f32) || (reinterpret_cast<uintptr_t>(w) & 3u)) return NRV_ERR_ALIGN;
    peg_conv_launch<false>(x_f32, w, bias, out_f32, B, H, W, C, ks, static_cast<hipStream_t>(stream));
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t nrv_peg_bwd_workspace(int B, int H, int W, int C, int ks) {
    if (!peg_shape_ok(B, H, W, C, ks)) return 0;
    return (size_t)B * (ks * ks + 1) * C * sizeof(float);
}

extern "C" int nrv_peg_bwd(const float* x_f32, const float* w, const float* dy_f32, float* dx_f32, float* dw, float* dbias, void* workspace,
                           size_t workspace_bytes, int B, int H, int W, int C, int ks, void* stream) {
    if (!peg_shape_ok(B, H, W, C, ks)) return NRV_ERR_SHAPE;
    if (!x_f32 || !w || !dy_f32 || !dx_f32 || !dw || !dbias || !workspace) return NRV_ERR_NULL;
    if (workspace_bytes < nrv_peg_bwd_workspace(B, H, W, C, ks)) return NRV_ERR_WORKSPACE;
    if (!nrv_aligned16(x_f32) || !nrv_aligned16(dy_f32) || !nrv_aligned16(dx_f32) || !nrv_aligned16(workspace) ||
        (reinterpret_cast<uintptr_t>(w) & 3u) || (reinterpret_cast<uintptr_t>(dw) & 3u) || (reinterpret_cast<uintptr_t>(dbias) & 3u))
        return NRV_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* part = static_cast<float*>(workspace);
    peg_conv_launch<true>(dy_f32, w, nullptr, dx_f32, B, H, W, C, ks, st);
    NRV_CHECK_LAUNCH();
    const int KK = ks * ks;
    const long long parts = (long long)B * (KK + 1) * C;
    hipLaunchKernelGGL(peg_dw_kernel, dim3((unsigned)nrv_cdiv(parts, 256)), dim3(256), 0, st, x_f32, dy_f32, part, parts, H, W, C, ks);
    NRV_CHECK_LAUNCH();
    // dw [C, KK] and dbias [C] = the per-sample partials summed over the samples in index order
    hipLaunchKernelGGL(tap_wred_kernel<256>, dim3((unsigned)nrv_cdiv((long long)(KK + 1) * C, 256)), dim3(256), 0, st, part, dw, dbias, B, C, KK);
    NRV_CHECK_LAUNCH();
    return 0;
}
