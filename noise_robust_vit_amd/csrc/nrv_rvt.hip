// RvT kernels (gfx950): the 2-D axial rotary embedding on the q and k blocks of the packed qkv, a plain depthwise ks x ks
// convolution on token-major rows with class rows in front of every sample's plane, and the GEGLU gate.  All three are
// memory-bound: every lane moves 16 bytes (8 bf16) per access, the arithmetic is fp32 in registers with one bf16 rounding on
// the store.  Every reduction runs in a fixed order (no atomics): reruns are bit-identical.  Grids are exact (one work item per
// thread, no capped grid-stride loop).  The bf16 <-> fp32 row accesses are those of nrv_rows.hpp, the GELU pieces those of
// nrv_common.hpp.
#include "nrv_rows.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
// rotary: one thread = 8 features (four pairs) of the q or the k block of one (patch row, head).  A pair (2m, 2m+1) is one
// 32-bit word; pairs at or behind dr keep their bits.  sgn = +1 forward, -1 backward (the transposed rotation).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rotary_kernel(bf16_t* __restrict__ qkv, const float* __restrict__ sn, const float* __restrict__ cs,
                                                     long long items, int N, int lead, int H, int dh, int dr, float sgn) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int nch = (dr + 7) >> 3, half = dr >> 1, Np = N - lead;
    const int ch = (int)(i % nch);
    long long r = i / nch;
    const int hb = (int)(r % (2 * H));                  // q heads 0 .. H-1, then k heads: the first 2*H*dh columns of a row
    r /= 2 * H;
    const int t = (int)(r % Np);
    const long long b = r / Np;
    bf16_t* p = qkv + ((b * N + lead + t) * 3ll * H + hb) * dh + ch * 8;
    u32x4_t v = *reinterpret_cast<const u32x4_t*>(p);
    const float* st = sn + (long long)t * half + ch * 4;
    const float* ct = cs + (long long)t * half + ch * 4;
    float s[4], c[4];
    if ((half & 3) == 0) {                               // table rows are 16-byte multiples: one load each
        const f32x4_t sv = *reinterpret_cast<const f32x4_t*>(st), cv = *reinterpret_cast<const f32x4_t*>(ct);
#pragma unroll
        for (int e = 0; e < 4; ++e) { s[e] = sv[e]; c[e] = cv[e]; }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = ch * 4 + e < half;
            s[e] = in ? st[e] : 0.f;
            c[e] = in ? ct[e] : 1.f;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (ch * 4 + e < half) {
            const float x0 = bf16lo_to_f32(v[e]), x1 = bf16hi_to_f32(v[e]), se = s[e] * sgn;
            v[e] = pack_bf16x2(fmaf(x0, c[e], -(x1 * se)), fmaf(x1, c[e], x0 * se));
        }
    }
    *reinterpret_cast<u32x4_t*>(p) = v;
}

// ---------------------------------------------------------------------------------------------
// depthwise ks x ks, stride 1, zero padding ks / 2, on rows [B*(lead + H*W), C].  One workgroup per (spatial tile of 14 x 14
// tokens, slab of 64 channels, sample): the tile with its halo and the slab's taps are staged in LDS (zeros outside the
// plane; class rows are never read), then 8 lanes x 8 channels cover a token and 32 tokens are in flight.
//   KS 7: 20*20*64*2 + 49*64*4 = 63 744 bytes of static LDS.
// ---------------------------------------------------------------------------------------------
constexpr int DWC_TILE = 14, DWC_CB = 64;

template <int KS>
__device__ __forceinline__ void dwc_stage(bf16_t* tile, const bf16_t* __restrict__ src, long long row0, int ty0, int tx0, int H, int W,
                                          int C, int c0, bool cok, int lc, int tg) {
    constexpr int R = KS / 2, TW = DWC_TILE + 2 * R;
    for (int i = tg; i < TW * TW; i += 32) {
        const int ly = i / TW, lx = i - ly * TW;
        const int y = ty0 + ly - R, x = tx0 + lx - R;
        u32x4_t v = {0u, 0u, 0u, 0u};
        if (cok && y >= 0 && y < H && x >= 0 && x < W) v = *reinterpret_cast<const u32x4_t*>(src + (row0 + (long long)y * W + x) * C + c0);
        *reinterpret_cast<u32x4_t*>(tile + i * DWC_CB + lc * 8) = v;
    }
}

// dst(p) = sum_t w[t] src(p + off_t), t = ky * KS + kx ascending; FLIP: the taps reversed (the input gradient), and the class
// rows of dst written as zeros
template <int KS, bool FLIP>
__global__ __launch_bounds__(256) void dwc_conv_kernel(const bf16_t* __restrict__ src, const float* __restrict__ w, bf16_t* __restrict__ dst,
                                                       int H, int W, int lead, int C, int tiles_x) {
    constexpr int R = KS / 2, KK = KS * KS, TW = DWC_TILE + 2 * R;
    __shared__ __attribute__((aligned(16))) bf16_t tile[TW * TW * DWC_CB];
    __shared__ __attribute__((aligned(16))) float wl[KK * DWC_CB];
    const int b = blockIdx.z, slab = blockIdx.y;
    const int ty0 = ((int)blockIdx.x / tiles_x) * DWC_TILE, tx0 = ((int)blockIdx.x % tiles_x) * DWC_TILE;
    const int lc = threadIdx.x & 7, tg = threadIdx.x >> 3;
    const int c0 = slab * DWC_CB + lc * 8;
    const bool cok = c0 < C;
    const long long row0 = (long long)b * (lead + H * W) + lead;
    for (int i = threadIdx.x; i < KK * DWC_CB; i += 256) {
        const int t = i / DWC_CB, cc = slab * DWC_CB + (i - t * DWC_CB);
        wl[i] = cc < C ? w[(long long)cc * KK + (FLIP ? KK - 1 - t : t)] : 0.f;
    }
    dwc_stage<KS>(tile, src, row0, ty0, tx0, H, W, C, c0, cok, lc, tg);
    __syncthreads();
    if (!cok) return;
    for (int p = tg; p < DWC_TILE * DWC_TILE; p += 32) {
        const int ly = p / DWC_TILE, lx = p - ly * DWC_TILE;
        const int y = ty0 + ly, x = tx0 + lx;
        if (y >= H || x >= W) continue;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < KS; ++ky) {
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) {
                float xv[8];
                load_row(tile + ((ly + ky) * TW + lx + kx) * DWC_CB + lc * 8, xv);
                const float* wp = wl + (ky * KS + kx) * DWC_CB + lc * 8;
                const f32x4_t w0 = *reinterpret_cast<const f32x4_t*>(wp), w1 = *reinterpret_cast<const f32x4_t*>(wp + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[j] = fmaf(w0[j], xv[j], acc[j]);
                    acc[4 + j] = fmaf(w1[j], xv[4 + j], acc[4 + j]);
                }
            }
        }
        store_row(dst + (row0 + (long long)y * W + x) * C + c0, acc);
    }
    if (FLIP && blockIdx.x == 0) {
        for (int l = tg; l < lead; l += 32)
            *reinterpret_cast<u32x4_t*>(dst + ((long long)b * (lead + H * W) + l) * C + c0) = u32x4_t{0u, 0u, 0u, 0u};
    }
}

// per-sample partials of the tap gradient: part[(b*C + c) * KK + t] = sum_p dout(b, p, c) a(b, p + off_t, c), p in row-major
// order.  One workgroup per (slab of 64 channels, sample) walks the plane's tiles; 8 lanes x 8 channels, and each of the 32
// lane groups owns the taps t = group, group + 32: no reduction across threads.
template <int KS>
__global__ __launch_bounds__(256) void dwc_dw_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ dout, float* __restrict__ part,
                                                     int H, int W, int lead, int C) {
    constexpr int R = KS / 2, KK = KS * KS, TW = DWC_TILE + 2 * R, NT = (KK + 31) / 32;
    __shared__ __attribute__((aligned(16))) bf16_t tile[TW * TW * DWC_CB];
    const int b = blockIdx.y, slab = blockIdx.x;
    const int lc = threadIdx.x & 7, tg = threadIdx.x >> 3;
    const int c0 = slab * DWC_CB + lc * 8;
    const bool cok = c0 < C;
    const long long row0 = (long long)b * (lead + H * W) + lead;
    float acc[NT][8];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[n][j] = 0.f;
    for (int ty0 = 0; ty0 < H; ty0 += DWC_TILE) {
        for (int tx0 = 0; tx0 < W; tx0 += DWC_TILE) {
            __syncthreads();
            dwc_stage<KS>(tile, a, row0, ty0, tx0, H, W, C, c0, cok, lc, tg);
            __syncthreads();
            const int th = H - ty0 < DWC_TILE ? H - ty0 : DWC_TILE, tw = W - tx0 < DWC_TILE ? W - tx0 : DWC_TILE;
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int t = tg + 32 * n;
                if (!cok || t >= KK) continue;
                const int ky = t / KS, kx = t - ky * KS;
                for (int ly = 0; ly < th; ++ly) {
                    for (int lx = 0; lx < tw; ++lx) {
                        float g[8], xv[8];
                        load_row(dout + (row0 + (long long)(ty0 + ly) * W + tx0 + lx) * C + c0, g);
                        load_row(tile + ((ly + ky) * TW + lx + kx) * DWC_CB + lc * 8, xv);
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[n][j] = fmaf(g[j], xv[j], acc[n][j]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int t = tg + 32 * n;
        if (!cok || t >= KK) continue;
#pragma unroll
        for (int j = 0; j < 8; ++j) part[((long long)b * C + c0 + j) * KK + t] = acc[n][j];
    }
}

// ---------------------------------------------------------------------------------------------
// GEGLU (rvt.py:80-83): u = [x | g] per row, h = x gelu(g).  One thread = 8 columns of a row.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void geglu_fwd_kernel(const bf16_t* __restrict__ u, long long ld_u, bf16_t* __restrict__ h, long long items,
                                                        int hidden) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int h8 = hidden >> 3;
    const long long r = i / h8;
    const int c = (int)(i - r * h8) * 8;
    float x[8], g[8], o[8];
    load_row(u + r * ld_u + c, x);
    load_row(u + r * ld_u + hidden + c, g);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = x[j] * gelu_fwd(g[j]);
    store_row(h + r * hidden + c, o);
}

// du[:, :hidden] = dh gelu(g), du[:, hidden:] = dh x gelu'(g), both recomputed from u
__global__ __launch_bounds__(256) void geglu_bwd_kernel(const bf16_t* __restrict__ u, long long ld_u, const bf16_t* __restrict__ dh,
                                                        bf16_t* __restrict__ du, long long items, int hidden) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int h8 = hidden >> 3;
    const long long r = i / h8;
    const int c = (int)(i - r * h8) * 8;
    float x[8], g[8], d[8], dx[8], dg[8];
    load_row(u + r * ld_u + c, x);
    load_row(u + r * ld_u + hidden + c, g);
    load_row(dh + r * hidden + c, d);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float ge, gd;
        gelu_both(g[j], ge, gd);
        dx[j] = d[j] * ge;
        dg[j] = d[j] * x[j] * gd;
    }
    store_row(du + r * 2ll * hidden + c, dx);
    store_row(du + r * 2ll * hidden + hidden + c, dg);
}

bool rotary_shape_ok(int B, int N, int lead, int H, int dh, int dr) {
    return B > 0 && N > 0 && (lead == 0 || lead == 1) && N > lead && H > 0 && dh > 0 && dh % 8 == 0 && dr >= 2 && dr % 2 == 0 && dr <= dh &&
           (long long)B * N * 3 * H * dh <= (1ll << 40);
}

int rotary_launch(void* qkv, const float* sn, const float* cs, int B, int N, int lead, int H, int dh, int dr, float sgn, void* stream) {
    if (!rotary_shape_ok(B, N, lead, H, dh, dr)) return NRV_ERR_SHAPE;
    if (!qkv || !sn || !cs) return NRV_ERR_NULL;
    if (!nrv_aligned16(qkv) || !nrv_aligned16(sn) || !nrv_aligned16(cs)) return NRV_ERR_ALIGN;
    const long long items = (long long)B * (N - lead) * 2 * H * ((dr + 7) / 8);
    const long long blocks = nrv_cdiv(items, 256);
    if (blocks > NRV_MAX_BLOCKS) return NRV_ERR_SHAPE;
    hipLaunchKernelGGL(rotary_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<bf16_t*>(qkv), sn, cs,
                       items, N, lead, H, dh, dr, sgn);
    NRV_CHECK_LAUNCH();
    return 0;
}

bool dwc_shape_ok(int B, int H, int W, int lead, int C, int ks) {
    return B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W <= (1ll << 24) && (lead == 0 || lead == 1) && C > 0 && C % 8 == 0 &&
           C <= 65535 * DWC_CB && (ks == 3 || ks == 5 || ks == 7);
}

template <int KS, bool FLIP>
void dwc_conv_launch(const void* src, const float* w, void* dst, int B, int H, int W, int lead, int C, hipStream_t st) {
    const int tx = (int)nrv_cdiv(W, DWC_TILE), ty = (int)nrv_cdiv(H, DWC_TILE);
    hipLaunchKernelGGL((dwc_conv_kernel<KS, FLIP>), dim3((unsigned)(tx * ty), (unsigned)nrv_cdiv(C, DWC_CB), B), dim3(256), 0, st,
                       static_cast<const bf16_t*>(src), w, static_cast<bf16_t*>(dst), H, W, lead, C, tx);
}

template <int KS>
void dwc_dw_launch(const void* a, const void* dout, float* part, int B, int H, int W, int lead, int C, hipStream_t st) {
    hipLaunchKernelGGL((dwc_dw_kernel<KS>), dim3((unsigned)nrv_cdiv(C, DWC_CB), B), dim3(256), 0, st, static_cast<const bf16_t*>(a),
                       static_cast<const bf16_t*>(dout), part, H, W, lead, C);
}

bool geglu_shape_ok(long long ld_u, long long rows, int hidden) {
    return rows > 0 && hidden > 0 && hidden % 8 == 0 && ld_u >= 2ll * hidden && ld_u % 8 == 0 && rows <= (1ll << 40) / hidden &&
           nrv_cdiv(rows * (hidden / 8), 256) <= NRV_MAX_BLOCKS;
}

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" int nrv_rotary_fwd(void* qkv_bf16, const float* sin_t, const float* cos_t, int B, int N, int lead, int H, int dh, int dr,
                              void* stream) {
    return rotary_launch(qkv_bf16, sin_t, cos_t, B, N, lead, H, dh, dr, 1.0f, stream);
}

extern "C" int nrv_rotary_bwd(void* dqkv_bf16, const float* sin_t, const float* cos_t, int B, int N, int lead, int H, int dh, int dr,
                              void* stream) {
    return rotary_launch(dqkv_bf16, sin_t, cos_t, B, N, lead, H, dh, dr, -1.0f, stream);
}

extern "C" int nrv_dwconv_fwd(const void* a, const float* w, void* out_bf16, int B, int H, int W, int lead, int C, int ks, void* stream) {
    if (!dwc_shape_ok(B, H, W, lead, C, ks)) return NRV_ERR_SHAPE;
    if (!a || !w || !out_bf16) return NRV_ERR_NULL;
    if (!nrv_aligned16(a) || !nrv_aligned16(out_bf16)) return NRV_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    NRV_DISPATCH_KS(ks, (dwc_conv_launch<KS, false>(a, w, out_bf16, B, H, W, lead, C, st)));
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t nrv_dwconv_bwd_workspace(int B, int H, int W, int C, int ks) {
    if (!dwc_shape_ok(B, H, W, 0, C, ks)) return 0;
    return (size_t)B * C * ks * ks * 4;
}

extern "C" int nrv_dwconv_bwd(const void* a, const float* w, const void* dout, void* da_bf16, float* dw, void* workspace,
                              size_t workspace_bytes, int B, int H, int W, int lead, int C, int ks, void* stream) {
    if (!dwc_shape_ok(B, H, W, lead, C, ks)) return NRV_ERR_SHAPE;
    if (!a || !w || !dout || !da_bf16 || !dw || !workspace) return NRV_ERR_NULL;
    if (workspace_bytes < nrv_dwconv_bwd_workspace(B, H, W, C, ks)) return NRV_ERR_WORKSPACE;
    if (!nrv_aligned16(a) || !nrv_aligned16(dout) || !nrv_aligned16(da_bf16) || !nrv_aligned16(workspace)) return NRV_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* part = static_cast<float*>(workspace);
    NRV_DISPATCH_KS(ks, (dwc_conv_launch<KS, true>(dout, w, da_bf16, B, H, W, lead, C, st)));
    NRV_CHECK_LAUNCH();
    NRV_DISPATCH_KS(ks, (dwc_dw_launch<KS>(a, dout, part, B, H, W, lead, C, st)));
    NRV_CHECK_LAUNCH();
    // dw [C, KK] = the per-sample partials [B][C * KK] summed over the samples in index order (C KK <= 65535 * 64 * 49: an int)
    const int n = C * ks * ks;
    hipLaunchKernelGGL(sum_rows_kernel<256>, dim3((unsigned)nrv_cdiv(n, 256)), dim3(256), 0, st, part, B, n, dw, dw, n, 0.f);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nrv_geglu_fwd(const void* u_bf16, int64_t ld_u, void* h_bf16, int64_t rows, int hidden, void* stream) {
    if (!geglu_shape_ok(ld_u, rows, hidden)) return NRV_ERR_SHAPE;
    if (!u_bf16 || !h_bf16) return NRV_ERR_NULL;
    if (!nrv_aligned16(u_bf16) || !nrv_aligned16(h_bf16)) return NRV_ERR_ALIGN;
    const long long items = rows * (hidden / 8);
    hipLaunchKernelGGL(geglu_fwd_kernel, dim3((unsigned)nrv_cdiv(items, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const bf16_t*>(u_bf16), (long long)ld_u, static_cast<bf16_t*>(h_bf16), items, hidden);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nrv_geglu_bwd(const void* u_bf16, int64_t ld_u, const void* dh_bf16, void* du_bf16, int64_t rows, int hidden,
                             void* stream) {
    if (!geglu_shape_ok(ld_u, rows, hidden)) return NRV_ERR_SHAPE;
    if (!u_bf16 || !dh_bf16 || !du_bf16) return NRV_ERR_NULL;
    if (!nrv_aligned16(u_bf16) || !nrv_aligned16(dh_bf16) || !nrv_aligned16(du_bf16)) return NRV_ERR_ALIGN;
    const long long items = rows * (hidden / 8);
    hipLaunchKernelGGL(geglu_bwd_kernel, dim3((unsigned)nrv_cdiv(items, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const bf16_t*>(u_bf16), (long long)ld_u, static_cast<const bf16_t*>(dh_bf16), static_cast<bf16_t*>(du_bf16),
                       items, hidden);
    NRV_CHECK_LAUNCH();
    return 0;
}
