// Shifted-window multi-head attention of the Swin Transformer (swin.py:112-267 between the two Linears): cyclic shift, window
// partition, scores + learned relative-position bias + the -100 shift mask, softmax or Sinkhorn (swin.py:239-246), P.V, reverse
// partition and reverse shift -- one kernel per direction, all of the rearrangement done as index arithmetic.
//
// Work split: one wave (64 lanes) per (window, head); lane i owns slot i of the window (N = Wh*Ww <= 64 slots, lanes >= N idle).
// Slot (i, j) of window (wy, wx) is the token ((wy*Wh + i + sh) mod pH, (wx*Ww + j + sw) mod pW) of the padded grid, read from and
// written back to that token's row of the projection's [tokens, 3C] output: no permuted copy of anything is made.
//   forward : K, V of the window -> LDS (bf16); lane i keeps its score row S[i][0..63] in fp32 registers, then P0 = softmax(S),
//             and for Sinkhorn the scaling vectors a_t = 1 / (P0 b_{t-1}), b_t = 1 / (P0^T a_t) (t = 1..3, b_0 = 1), a_4; the
//             final matrix is diag(a4) P0 diag(b3).  Column sums read an fp32 copy of P0 in LDS (never fp16: the -100 mask makes
//             columns whose entries are e^-100 smaller than the row's maximum routine, and Sinkhorn rescales exactly those).
//             Saved: lse per (token, head), and for Sinkhorn a1 b1 a2 b2 a3 b3 a4 (a_t of the token as a query, b_t as a key).
//   backward: lane i recomputes its P0 row from lse, dP = dO V^T, and walks the Sinkhorn steps back (row steps in-lane, column
//             steps through an LDS column sum); dS = P0 (G - rowsum(G P0)); dQ_i in-lane; then P and dS go to LDS and lane j
//             forms dK_j = scale dS^T Q and dV_j = P^T dO.  The relative-position-table gradient is dS folded through the index:
//             each workgroup sums it over a fixed chunk of WA_CHUNK windows of one head in registers and writes one partial per
//             table entry; reduce_partials_kernel (nrv_rows.hpp) adds the partials of each entry in a fixed order.  No atomics:
//             bit-reproducible.
// Nothing [windows, H, N, N]-sized reaches HBM.  The row helpers (load_row / dot_row / axpy_row / store_row, on global and LDS rows)
// are those of nrv_rows.hpp.
#include "nrv_rows.hpp"

#include <cmath>

namespace {

constexpr int WA_N = 64;         // slots per window, at most
constexpr int WA_CHUNK = 8;      // windows per table-gradient partial (fixed: the summation order depends on nothing else)
constexpr int WA_TMAX = 225;     // (2*8 - 1)^2 table rows at most

struct WinParams {
    const bf16_t* qkv;     // [B*pH*pW, 3C]
    const float* table;    // [T, H]
    const bf16_t* dout;    // [B*pH*pW, C]      (bwd)
    bf16_t* o;             // [B*pH*pW, C]      (fwd)
    bf16_t* dqkv;          // [B*pH*pW, 3C]     (bwd)
    float* stats;          // [B*pH*pW, H, S], S = 1 (softmax) or 8 (Sinkhorn)
    float* part;           // [H, T, chunks]    (bwd)
    int pH, pW, C, H, Wh, Ww, sh, sw, nWx, nWin1, N, T, chunks;   // nWin1 = windows per sample
    long long nwin;        // B * nWin1
    float scale;
};

// swizzled fp32 [64][64] LDS matrix: row writes (one row per lane) and column reads (one column per lane) are both conflict-free
__device__ __forceinline__ int sw_idx(int i, int j) { return i * 64 + ((j + i) & 63); }

__device__ __forceinline__ long long slot_row(const WinParams& p, long long win, int i) {
    const long long b = win / p.nWin1;
    const int w = (int)(win - b * p.nWin1);
    const int wy = w / p.nWx, wx = w - (w / p.nWx) * p.nWx;
    const int yi = i / p.Ww, xi = i - yi * p.Ww;
    int y = wy * p.Wh + yi + p.sh, x = wx * p.Ww + xi + p.sw;
    if (y >= p.pH) y -= p.pH;
    if (x >= p.pW) x -= p.pW;
    return (b * p.pH + y) * p.pW + x;
}

// shift-region id of a position of the ROLLED grid along one axis (swin.py:203-236: slices (0, -ws), (-ws, -s), (-s, None) filled in
// that order; with s == 0 the last slice is the whole axis and overwrites the others, so every position gets id 2)
__device__ __forceinline__ int region_1d(int pos, int extent, int ws, int s) {
    if (s == 0) return 2;
    return pos < extent - ws ? 0 : (pos < extent - s ? 1 : 2);
}

__device__ __forceinline__ int slot_region(const WinParams& p, long long win, int i) {
    const int w = (int)(win % p.nWin1);
    const int wy = w / p.nWx, wx = w - (w / p.nWx) * p.nWx;
    const int yi = i / p.Ww, xi = i - yi * p.Ww;
    return region_1d(wy * p.Wh + yi, p.pH, p.Wh, p.sh) * 3 + region_1d(wx * p.Ww + xi, p.pW, p.Ww, p.sw);
}

template <int DH>
__device__ __forceinline__ void copy_row_lds(const bf16_t* src, bool ok, bf16_t* dst) {
#pragma unroll
    for (int c = 0; c < DH / 8; ++c)
        *reinterpret_cast<u32x4_t*>(dst + c * 8) = ok ? *reinterpret_cast<const u32x4_t*>(src + c * 8) : u32x4_t{0u, 0u, 0u, 0u};
}

// score of lane i's query against key j (j < N): (scale q_i) . k_j + table[rel(i, j)] (+ -100 across shift regions).
// q holds scale * q_i; stab = the head's table column in LDS.
struct ScoreCtx {
    int base, tw, ri;
    bool masked;
};

__device__ __forceinline__ ScoreCtx score_ctx(const WinParams& p, long long win, int i) {
    ScoreCtx c;
    const int yi = i / p.Ww, xi = i - yi * p.Ww;
    c.tw = 2 * p.Ww - 1;
    c.base = (yi + p.Wh - 1) * c.tw + xi + p.Ww - 1;
    c.masked = p.sh + p.sw > 0;
    c.ri = c.masked ? slot_region(p, win, i) : 0;
    return c;
}

template <int DH>
__device__ __forceinline__ float score(const WinParams& p, long long win, const ScoreCtx& c, int j, const float (&q)[DH],
                                       const bf16_t* sk, const float* stab) {
    const int yj = j / p.Ww, xj = j - yj * p.Ww;
    float v = dot_row<DH>(q, sk + j * DH) + stab[c.base - (yj * c.tw + xj)];
    if (c.masked && slot_region(p, win, j) != c.ri) v += -100.0f;
    return v;
}

__device__ __forceinline__ void stage_table(const WinParams& p, int h, float* stab) {
    for (int t = threadIdx.x; t < p.T; t += WA_N) stab[t] = p.table[(long long)t * p.H + h];
}

// ---------------------------------------------------------------------------------------------------------------------------
// forward: one wave per (window, head), blockIdx.x = window * H + head.  Lane i's score / probability row is row i of the
// swizzled fp32 matrix sS (LDS): runtime loops over the keys, no large register arrays.
// ---------------------------------------------------------------------------------------------------------------------------
template <int DH, bool ROBUST>
__global__ __launch_bounds__(64) void wattn_fwd_kernel(WinParams p) {
    __shared__ __attribute__((aligned(16))) bf16_t sk[WA_N * DH];
    __shared__ __attribute__((aligned(16))) bf16_t sv[WA_N * DH];
    __shared__ float sS[WA_N * WA_N];
    __shared__ float stab[WA_TMAX];
    __shared__ float sa[WA_N], sb[WA_N];
    const int lane = threadIdx.x;
    const long long win = blockIdx.x / p.H;
    const int h = (int)(blockIdx.x - win * p.H);
    const int N = p.N;
    const bool valid = lane < N;
    const int i = valid ? lane : 0;
    const long long row = slot_row(p, win, i);
    const long long ld = 3ll * p.C;
    const bf16_t* src = p.qkv + row * ld + h * DH;
    copy_row_lds<DH>(src + p.C, valid, sk + lane * DH);
    copy_row_lds<DH>(src + 2 * p.C, valid, sv + lane * DH);
    stage_table(p, h, stab);
    float q[DH];
    load_row<DH>(src, q);
#pragma unroll
    for (int d = 0; d < DH; ++d) q[d] *= p.scale;
    __syncthreads();

    const ScoreCtx c = score_ctx(p, win, i);
    float m = -INFINITY;
    for (int j = 0; j < N; ++j) {
        const float v = score<DH>(p, win, c, j, q, sk, stab);
        sS[sw_idx(lane, j)] = v;
        m = fmaxf(m, v);
    }
    float l = 0.f;
    for (int j = 0; j < N; ++j) {
        const float e = __expf(sS[sw_idx(lane, j)] - m);
        sS[sw_idx(lane, j)] = e;
        l += e;
    }
    const float rl = 1.0f / l;
    for (int j = 0; j < N; ++j) sS[sw_idx(lane, j)] = valid ? sS[sw_idx(lane, j)] * rl : 0.f;     // P0 = softmax(S)
    float* st = p.stats + (row * p.H + h) * (ROBUST ? 8 : 1);
    if (valid) st[0] = m + __logf(l);

    float a = 1.f;
    if constexpr (ROBUST) {
        sb[lane] = 1.f;                                            // b_0
        __syncthreads();
        for (int t = 1; t <= 3; ++t) {
            float r = 0.f;
            for (int j = 0; j < N; ++j) r += sS[sw_idx(lane, j)] * sb[j];
            a = valid ? 1.0f / r : 0.f;
            if (valid) st[2 * t - 1] = a;
            sa[lane] = a;
            __syncthreads();                                       // rows of P0 and a_t visible; every lane has read sb
            float cs = 0.f;
            for (int k = 0; k < N; ++k) cs += sa[k] * sS[sw_idx(k, lane)];
            const float b = valid ? 1.0f / cs : 0.f;
            if (valid) st[2 * t] = b;
            __syncthreads();                                       // every lane has read sa
            sb[lane] = b;
            __syncthreads();
        }
        float r = 0.f;
        for (int j = 0; j < N; ++j) r += sS[sw_idx(lane, j)] * sb[j];
        a = 1.0f / r;                                              // a4
        if (valid) st[7] = a;
    }

    float o[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) o[d] = 0.f;
    for (int j = 0; j < N; ++j) {
        float w = sS[sw_idx(lane, j)];
        if constexpr (ROBUST) w *= sb[j];                          // P0 diag(b3); diag(a4) on the store
        axpy_row<DH>(w, sv + j * DH, o);
    }
    if (valid) store_row<DH>(p.o + row * p.C + h * DH, o, a);
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward: one wave per (chunk of WA_CHUNK windows, head); grid (chunks, H).  sS = P0 (then the final P), sD = dP (then dS),
// both swizzled fp32 [64][64]; sX = K, V during the row phase, then Q, dO for the column phase.
// ---------------------------------------------------------------------------------------------------------------------------
template <int DH, bool ROBUST>
__global__ __launch_bounds__(64) void wattn_bwd_kernel(WinParams p) {
    __shared__ __attribute__((aligned(16))) bf16_t sX[2 * WA_N * DH];
    __shared__ float sS[WA_N * WA_N], sD[WA_N * WA_N];
    __shared__ float stab[WA_TMAX];
    __shared__ float sat[5][WA_N];       // a_0 (= 1) .. a_4 of every query slot
    __shared__ float sbt[4][WA_N];       // b_0 (= 1) .. b_3 of every key slot
    __shared__ float shv[WA_N];
    bf16_t* sk = sX;
    bf16_t* sv = sX + WA_N * DH;
    const int lane = threadIdx.x;
    const int h = blockIdx.y;
    const int chunk = blockIdx.x;
    const int N = p.N;
    const bool valid = lane < N;
    const int i = valid ? lane : 0;
    const long long ld = 3ll * p.C;
    const int tw = 2 * p.Ww - 1;
    stage_table(p, h, stab);
    float tacc[4] = {0.f, 0.f, 0.f, 0.f};

    const long long w0 = (long long)chunk * WA_CHUNK;
    const long long w1 = w0 + WA_CHUNK < p.nwin ? w0 + WA_CHUNK : p.nwin;
    for (long long win = w0; win < w1; ++win) {
        const long long row = slot_row(p, win, i);
        const bf16_t* src = p.qkv + row * ld + h * DH;
        const bf16_t* dsrc = p.dout + row * p.C + h * DH;
        copy_row_lds<DH>(src + p.C, valid, sk + lane * DH);
        copy_row_lds<DH>(src + 2 * p.C, valid, sv + lane * DH);
        const float* st = p.stats + (row * p.H + h) * (ROBUST ? 8 : 1);
        if constexpr (ROBUST) {
            sat[0][lane] = 1.f;
            sbt[0][lane] = 1.f;
#pragma unroll
            for (int t = 1; t <= 4; ++t) sat[t][lane] = valid ? st[2 * t - 1] : 0.f;
#pragma unroll
            for (int t = 1; t <= 3; ++t) sbt[t][lane] = valid ? st[2 * t] : 0.f;
        }
        const float lse = st[0];
        __syncthreads();

        // row phase: lane i owns row i of sS / sD
        {
            float q[DH];
            load_row<DH>(src, q);
#pragma unroll
            for (int d = 0; d < DH; ++d) q[d] *= p.scale;
            const ScoreCtx c = score_ctx(p, win, i);
            for (int j = 0; j < N; ++j) sS[sw_idx(lane, j)] = valid ? __expf(score<DH>(p, win, c, j, q, sk, stab) - lse) : 0.f;
        }
        {
            float dov[DH];
            load_row<DH>(dsrc, dov);
            for (int j = 0; j < N; ++j) sD[sw_idx(lane, j)] = valid ? dot_row<DH>(dov, sv + j * DH) : 0.f;
        }
        if constexpr (ROBUST) {
            const float a4 = sat[4][i], a3 = sat[3][i];
            // final row normalisation: output diag(a4) P0 diag(b3), input diag(a3) P0 diag(b3)
            float r = 0.f;
            for (int j = 0; j < N; ++j) r += sD[sw_idx(lane, j)] * sS[sw_idx(lane, j)] * sbt[3][j];
            r *= a4;
            for (int j = 0; j < N; ++j) sD[sw_idx(lane, j)] = valid ? (sD[sw_idx(lane, j)] - r) * (a4 / a3) : 0.f;
            for (int t = 3; t >= 1; --t) {
                // column step t: output diag(a_t) P0 diag(b_t), input diag(a_t) P0 diag(b_{t-1})
                __syncthreads();
                float hs = 0.f;
                for (int k = 0; k < N; ++k) hs += sD[sw_idx(k, lane)] * (sat[t][k] * sS[sw_idx(k, lane)]);
                shv[lane] = valid ? hs * sbt[t][lane] : 0.f;
                __syncthreads();
                const float at = sat[t][i], ap = sat[t - 1][i];
                r = 0.f;
                for (int j = 0; j < N; ++j) {
                    const float gj = (sD[sw_idx(lane, j)] - shv[j]) * (sbt[t][j] / sbt[t - 1][j]);
                    sD[sw_idx(lane, j)] = gj;
                    r += gj * sS[sw_idx(lane, j)] * sbt[t - 1][j];
                }
                // row step t: output diag(a_t) P0 diag(b_{t-1}), input diag(a_{t-1}) P0 diag(b_{t-1})
                r *= at;
                for (int j = 0; j < N; ++j) sD[sw_idx(lane, j)] = valid ? (sD[sw_idx(lane, j)] - r) * (at / ap) : 0.f;
            }
        }
        // softmax backward dS = P0 (G - rowsum(G P0)); then sS takes the final P (Sinkhorn: diag(a4) P0 diag(b3))
        float dq[DH];
#pragma unroll
        for (int d = 0; d < DH; ++d) dq[d] = 0.f;
        {
            float r = 0.f;
            for (int j = 0; j < N; ++j) r += sD[sw_idx(lane, j)] * sS[sw_idx(lane, j)];
            const float a4 = ROBUST ? sat[4][i] : 1.f;
            for (int j = 0; j < N; ++j) {
                const float p0 = sS[sw_idx(lane, j)];
                const float ds = p0 * (sD[sw_idx(lane, j)] - r);
                sD[sw_idx(lane, j)] = ds;
                if constexpr (ROBUST) sS[sw_idx(lane, j)] = a4 * p0 * sbt[3][j];
                axpy_row<DH>(ds, sk + j * DH, dq);
            }
        }
        if (valid) store_row<DH>(p.dqkv + row * ld + h * DH, dq, p.scale);
        __syncthreads();                           // K / V are dead: sX takes Q and dO
        copy_row_lds<DH>(src, valid, sX + lane * DH);
        copy_row_lds<DH>(dsrc, valid, sX + (WA_N + lane) * DH);
        __syncthreads();
        {
            float dk[DH], dv[DH];
#pragma unroll
            for (int d = 0; d < DH; ++d) { dk[d] = 0.f; dv[d] = 0.f; }
            for (int k = 0; k < N; ++k) {
                axpy_row<DH>(sD[sw_idx(k, lane)], sX + k * DH, dk);
                axpy_row<DH>(sS[sw_idx(k, lane)], sX + (WA_N + k) * DH, dv);
            }
            if (valid) {
                store_row<DH>(p.dqkv + row * ld + p.C + h * DH, dk, p.scale);
                store_row<DH>(p.dqkv + row * ld + 2 * p.C + h * DH, dv, 1.f);
            }
        }
        // table gradient: entry t = (dy, dx) collects dS[i][j] over the pairs with coord_i - coord_j = (dy, dx)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = lane + u * WA_N;
            if (t < p.T) {
                const int dy = t / tw - (p.Wh - 1), dx = t - (t / tw) * tw - (p.Ww - 1);
                const int y0 = dy > 0 ? dy : 0, y1 = dy < 0 ? p.Wh + dy : p.Wh;
                const int x0 = dx > 0 ? dx : 0, x1 = dx < 0 ? p.Ww + dx : p.Ww;
                float acc = 0.f;
                for (int yi = y0; yi < y1; ++yi)
                    for (int xi = x0; xi < x1; ++xi)
                        acc += sD[sw_idx(yi * p.Ww + xi, (yi - dy) * p.Ww + xi - dx)];
                tacc[u] += acc;
            }
        }
        __syncthreads();                           // the next window overwrites every LDS region
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int t = lane + u * WA_N;
        if (t < p.T) p.part[((long long)h * p.T + t) * p.chunks + chunk] = tacc[u];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// stochastic depth, row mode (torchvision StochasticDepth(p, "row"), swin.py:519,532-533): a per-sample factor keep[b] / survival
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sd_add_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                     const float* __restrict__ keep, float* __restrict__ out, float survival,
                                                     long long n4, long long per_sample4) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (long long)gridDim.x * blockDim.x) {
        const float f = keep[e / per_sample4] / survival;
        const f32x4_t xv = *reinterpret_cast<const f32x4_t*>(x + e * 4);
        const f32x4_t yv = *reinterpret_cast<const f32x4_t*>(y + e * 4);
        f32x4_t o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = xv[k] + yv[k] * f;
        *reinterpret_cast<f32x4_t*>(out + e * 4) = o;
    }
}

__global__ __launch_bounds__(256) void sd_scale_kernel(const float* __restrict__ dy, const float* __restrict__ keep,
                                                       bf16_t* __restrict__ out, float survival, long long n4, long long per_sample4) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (long long)gridDim.x * blockDim.x) {
        const float f = keep[e / per_sample4] / survival;
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(dy + e * 4);
        *reinterpret_cast<u32x2_t*>(out + e * 4) = u32x2_t{pack_bf16x2(v[0] * f, v[1] * f), pack_bf16x2(v[2] * f, v[3] * f)};
    }
}

// shared argument rules of the three window entry points; fills p (pointers excepted)
int setup(WinParams& p, int B, int pH, int pW, int C, int heads, int Wh, int Ww, int sh, int sw) {
    if (B <= 0 || heads <= 0 || C <= 0 || Wh <= 0 || Ww <= 0 || pH <= 0 || pW <= 0) return NRV_ERR_SHAPE;
    if (C % heads) return NRV_ERR_SHAPE;
    const int dh = C / heads;
    if (dh != 32 && dh != 64) return NRV_ERR_SHAPE;
    if (Wh * Ww > WA_N || (2 * Wh - 1) * (2 * Ww - 1) > WA_TMAX) return NRV_ERR_SHAPE;
    if (pH % Wh || pW % Ww) return NRV_ERR_SHAPE;
    if (sh < 0 || sw < 0 || sh >= Wh || sw >= Ww) return NRV_ERR_SHAPE;
    const long long nwin = (long long)B * (pH / Wh) * (pW / Ww);
    if (nwin * heads > 0x7fffffffll || (long long)B * pH * pW * 3 * C > (1ll << 40)) return NRV_ERR_SHAPE;
    p.pH = pH; p.pW = pW; p.C = C; p.H = heads; p.Wh = Wh; p.Ww = Ww; p.sh = sh; p.sw = sw;
    p.nWx = pW / Ww; p.nWin1 = (pH / Wh) * (pW / Ww); p.N = Wh * Ww; p.T = (2 * Wh - 1) * (2 * Ww - 1);
    p.nwin = nwin;
    p.chunks = (int)((nwin + WA_CHUNK - 1) / WA_CHUNK);
    p.scale = (float)(1.0 / std::sqrt((double)dh));
    return 0;
}

template <int DH, bool R>
int launch_fwd(const WinParams& p, hipStream_t s) {
    hipLaunchKernelGGL((wattn_fwd_kernel<DH, R>), dim3((unsigned)(p.nwin * p.H)), dim3(WA_N), 0, s, p);
    NRV_CHECK_LAUNCH();
    return 0;
}

template <int DH, bool R>
int launch_bwd(const WinParams& p, float* dtable, hipStream_t s) {
    hipLaunchKernelGGL((wattn_bwd_kernel<DH, R>), dim3((unsigned)p.chunks, (unsigned)p.H), dim3(WA_N), 0, s, p);
    NRV_CHECK_LAUNCH();
    // dtable[t, h] = sum over the chunks of part[h, t, chunk]
    hipLaunchKernelGGL((reduce_partials_kernel<256>), dim3((unsigned)p.T, (unsigned)p.H), dim3(256), 0, s, p.part, dtable, p.chunks,
                       (long long)p.H, 1ll);
    NRV_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int nrv_window_attn_fwd(const void* qkv_bf16, const float* table, void* out_bf16, float* stats,
                                   int B, int pH, int pW, int C, int heads, int Wh, int Ww, int sh, int sw, int robust,
                                   void* stream) {
    WinParams p{};
    const int e = setup(p, B, pH, pW, C, heads, Wh, Ww, sh, sw);
    if (e) return e;
    if (!qkv_bf16 || !table || !out_bf16 || !stats) return NRV_ERR_NULL;
    if (!nrv_aligned16(qkv_bf16) || !nrv_aligned16(out_bf16) || (reinterpret_cast<uintptr_t>(stats) & 3u) ||
        (reinterpret_cast<uintptr_t>(table) & 3u))
        return NRV_ERR_ALIGN;
    p.qkv = static_cast<const bf16_t*>(qkv_bf16);
    p.table = table;
    p.o = static_cast<bf16_t*>(out_bf16);
    p.stats = stats;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int dh = C / heads;
    if (dh == 32) return robust ? launch_fwd<32, true>(p, s) : launch_fwd<32, false>(p, s);
    return robust ? launch_fwd<64, true>(p, s) : launch_fwd<64, false>(p, s);
}

extern "C" size_t nrv_window_attn_bwd_workspace(int B, int pH, int pW, int C, int heads, int Wh, int Ww) {
    WinParams p{};
    if (setup(p, B, pH, pW, C, heads, Wh, Ww, 0, 0)) return 0;
    return (size_t)p.chunks * p.H * p.T * sizeof(float);
}

extern "C" int nrv_window_attn_bwd(const void* qkv_bf16, const float* table, const void* dout_bf16, const float* stats,
                                   void* dqkv_bf16, float* dtable, void* workspace, size_t workspace_bytes,
                                   int B, int pH, int pW, int C, int heads, int Wh, int Ww, int sh, int sw, int robust,
                                   void* stream) {
    WinParams p{};
    const int e = setup(p, B, pH, pW, C, heads, Wh, Ww, sh, sw);
    if (e) return e;
    if (!qkv_bf16 || !table || !dout_bf16 || !stats || !dqkv_bf16 || !dtable || !workspace) return NRV_ERR_NULL;
    if (workspace_bytes < (size_t)p.chunks * p.H * p.T * sizeof(float)) return NRV_ERR_WORKSPACE;
    if (!nrv_aligned16(qkv_bf16) || !nrv_aligned16(dout_bf16) || !nrv_aligned16(dqkv_bf16) ||
        (reinterpret_cast<uintptr_t>(stats) & 3u) || (reinterpret_cast<uintptr_t>(table) & 3u) ||
        (reinterpret_cast<uintptr_t>(dtable) & 3u) || (reinterpret_cast<uintptr_t>(workspace) & 3u))
        return NRV_ERR_ALIGN;
    p.qkv = static_cast<const bf16_t*>(qkv_bf16);
    p.table = table;
    p.dout = static_cast<const bf16_t*>(dout_bf16);
    p.stats = const_cast<float*>(stats);
    p.dqkv = static_cast<bf16_t*>(dqkv_bf16);
    p.part = static_cast<float*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int dh = C / heads;
    if (dh == 32) return robust ? launch_bwd<32, true>(p, dtable, s) : launch_bwd<32, false>(p, dtable, s);
    return robust ? launch_bwd<64, true>(p, dtable, s) : launch_bwd<64, false>(p, dtable, s);
}

extern "C" int nrv_sd_add_f32(const float* x, const float* y, const float* keep, float* out, float survival,
                              int64_t rows, int64_t rows_per_sample, int dim, void* stream) {
    if (!x || !y || !keep || !out) return NRV_ERR_NULL;
    if (rows <= 0 || rows_per_sample <= 0 || rows % rows_per_sample || dim <= 0 || (dim & 3) || !(survival > 0.f))
        return NRV_ERR_SHAPE;
    if (!nrv_aligned16(x) || !nrv_aligned16(y) || !nrv_aligned16(out) || (reinterpret_cast<uintptr_t>(keep) & 3u)) return NRV_ERR_ALIGN;
    const long long n4 = rows * (long long)dim / 4, ps4 = rows_per_sample * (long long)dim / 4;
    hipLaunchKernelGGL(sd_add_kernel, dim3(grid_for(n4, 256, 4096)), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, keep, out, survival, n4, ps4);
    NRV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nrv_sd_scale_bf16(const float* dy, const float* keep, void* out_bf16, float survival,
                                 int64_t rows, int64_t rows_per_sample, int dim, void* stream) {
    if (!dy || !keep || !out_bf16) return NRV_ERR_NULL;
    if (rows <= 0 || rows_per_sample <= 0 || rows % rows_per_sample || dim <= 0 || (dim & 3) || !(survival > 0.f))
        return NRV_ERR_SHAPE;
    if (!nrv_aligned16(dy) || (reinterpret_cast<uintptr_t>(out_bf16) & 7u) || (reinterpret_cast<uintptr_t>(keep) & 3u)) return NRV_ERR_ALIGN;
    const long long n4 = rows * (long long)dim / 4, ps4 = rows_per_sample * (long long)dim / 4;
    hipLaunchKernelGGL(sd_scale_kernel, dim3(grid_for(n4, 256, 4096)), dim3(256), 0, static_cast<hipStream_t>(stream), dy, keep,
                       static_cast<bf16_t*>(out_bf16), survival, n4, ps4);
    NRV_CHECK_LAUNCH();
    return 0;
}
