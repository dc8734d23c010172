"""References for the kernels that own all heads of a materialised [B, H, Nq, Nk] matrix: talking heads
(csrc/nrv_talking_heads.hip) and re-attention (csrc/nrv_reattn.hip), both on the helpers of csrc/nrv_heads.hpp.

For each of the eight entry points: the fp64 reference of every output with a per-element bound, an fp32 emulation of the kernel's
arithmetic (tests/test_heads_ref_host.py shows that the bounds hold for it and that wrong kernels break them), and the seeded
inputs and case lists the GPU test (tests/test_heads_edges_gpu.py) and the host test share.

    talking heads   T[g] = sum_h W1[h,g] S[h]     P = softmax(T)     A[g] = sum_h W2[h,g] P[h]
                    dP[h] = sum_g W2[h,g] dA[g]   dT = P (dP - <P, dP>)   dS[h] = sum_g W1[h,g] dT[g]
                    dW2[h,g] = sum P[h] dA[g]     dW1[h,g] = sum S[h] dT[g]
    re-attention    P = softmax(S)     M[g] = sum_h W[h,g] P[h]     d = M - mean_g M     rstd = (mean_g d^2 + eps)^-1/2
                    x^ = d rstd        A = x^ gamma + beta
                    dbeta = sum dA     dgamma = sum dA x^     dx^ = dA gamma
                    dM = rstd ((dx^ - mean_g dx^) - x^ mean_g (dx^ x^))     dW[h,g] = sum P[h] dM[g]
                    dP[h] = sum_g W[h,g] dM[g]     dS = P (dP - <P, dP>)
    head_mix / reattn_norm are the mixing (and the norm) alone on flat positions, with the gradients of the same formulas.

As in tests/test_talking_heads_gpu.py and tests/test_reattn_gpu.py the backward references and the A of both families read the
KERNEL'S OWN P (an exact input of theirs); P is checked against the fp64 softmax separately.

The bounds are derived from the kernels' rounding points, not tuned.  u = 2^-23 (U32, twice the fp32 unit roundoff: the slack of
the gamma_n bound), b = 2^-8 (BF16).  |W| x and |W|^T x stand for the mixing with the absolute matrix; e_x is the bound of x.
  mix        an fma chain over the H heads from 0:  e = (H + 1) u (|W| |x|) + |W| e_x          (either orientation)
  T          e_T = (H + 1) u (|W1| |S|)
  P          relative error rel = 2 max_j e_T + (max_j |T - max T| + 5) 2^-22 + 2^-21 + (Nk + 8) u: the error of T passed through
             numerator and denominator, the exp2 argument's subtraction and scaling, the exponential's two ulps, the Nk-term row
             sum with its reciprocal and product (re-attention: e_T = 0, T = S);  e_P = rel P
  A (th)     (H + 1) u (|W2| P);  stored as bf16: e + b (|A| + e)   (bf16 keeps 8 significant bits: half an ulp is up to 2^-8 |A|)
  dP         e_dP = (H + 1) u (|W2|^T |dA|)
  dT, dS(ra) P (dP - <P, dP>), D = sum_j P |dP|:
             e = P (e_dP + sum_j P e_dP + (Nk + 2) u D + u (|dP| + D)) + u |ref|     -- P D is the cancellation term
  dS (th)    (H + 1) u (|W1|^T |dT|) + |W1|^T e_dT
  H x H sums a thread's four fp32 chains of at most 257 terms per image and their three adds, then double across splits, images,
  and [H]    parts and one cast: 260 u sum |x| |y| + sum |x| e_y, PER (h, g) ENTRY and per g (dbeta: 260 u sum |dA|)
  LayerNorm  e_M = (H + 1) u (|W| P);  mu: e_mu = mean_g e_M + (H + 1) u mean_g |M|;  d = M - mu: E = max_g e_M + e_mu + u max_g |d|.
             x^_g = d_g r(d) has the derivative  r dd_g - x^_g r (sum_k x^_k dd_k / H), and mean_k |x^_k| <= 1, so an error of E in
             every d_k moves x^_g by at most (1 + |x^_g|) rstd E -- the 2 rstd of a value with |x^| <= 1; eps > 0 floors the
             variance, so rstd <= eps^-1/2 and the bound stays finite where all heads agree.  The H-term variance chain, rsqrtf
             and the product add (H + 6) u |x^|:   e_x = (1 + |x^|) rstd E + (H + 6) u |x^|,   rstd: relative rstd E + (H + 6) u
  A (ra)     |gamma| e_x + u |A|;  bf16 as above
  dM         dx = dA gamma (e_dx = u |dx|), s1 = mean_g dx, s2 = mean_g dx x^:
             e_s1 = (H + 1) u mean |dx| + mean e_dx,   e_s2 = (H + 2) u mean |dx x^| + mean (|dx| e_x + e_dx |x^|),
             e_in = e_dx + e_s1 + e_x |s2| + |x^| e_s2 + 2 u (|dx| + |s1| + |x^ s2|),   e_dM = rstd e_in + |dM| (rstd E + (H + 7) u)
  dP (ra)    (H + 1) u (|W|^T |dM|) + |W|^T e_dM
fp32 has no numbers below 2^-126 (TINY) that a kernel is bound to keep (the fast exponential flushes them), so every P inside
a bound is P + TINY and every bound has TINY added.

The emulations keep the kernels' fp32 order where it changes a sum: the fma chains over the heads; the softmax row sum and the
dot <P, dP> per lane (keys lane, lane + 64, ...) and then the xor butterfly 32, 16, ..., 1; th_pairs' thread (h, g, split) with
its four chains over the 4-position groups split, split + nsplit, ... and (a0 + a1) + (a2 + a3); dgamma / dbeta per thread over
its positions (V = 4 or 1 consecutive, then a stride of 256 V) inside one image.  What the kernels add in double (splits, images,
workgroups) is added in double here, in any order.  exp2 and rsqrt are the correctly rounded ones.
"""
from __future__ import annotations

import torch

from rvt_ref import BF16, U32, _fma32, _gen, bf16, ratio  # noqa: F401

TINY = 2.0 ** -126
EPS = 1e-5                        # DeepViT's LayerNorm over the heads
TH_MAXH, TH_MAXNK, TH_THREADS, TH_TILE, TH_PARTS = 16, 1025, 256, 512, 1024
KINDS = ("random", "peaked", "flat", "identity")
NSUM = 260                        # terms of a parameter sum's fp32 part and what follows it (module docstring)

# (B, H, Nq, Nk) of the fused row kernels: Nk = 1 .. 5; the th_ld bump on the scalar (57, 1017) and the vector path (60, 1020);
# the 64-lane edge; the 256-thread th_mix edge, scalar and vector (1020 / 1024); H = 3, 11, 12, 15 leave th_pairs threads idle,
# H = 5, 6, 7 take a ragged second wave-per-head pass; every H has a scalar and a vector Nk; 16 x 1025 is the LDS maximum
FUSED_CASES = (
    (1, 1, 1, 1), (2, 2, 3, 1), (2, 3, 2, 2), (1, 16, 1, 2), (1, 5, 3, 3), (1, 15, 2, 3), (2, 7, 1, 4), (2, 12, 3, 4), (1, 1, 3, 4),
    (2, 11, 2, 5), (2, 16, 2, 5),
    (2, 3, 1, 57), (1, 12, 2, 57), (2, 5, 2, 60), (1, 16, 1, 60),
    (1, 2, 3, 63), (2, 7, 1, 64), (2, 15, 1, 64), (1, 11, 2, 65), (1, 1, 2, 65),
    (2, 3, 2, 255), (1, 11, 1, 255), (1, 3, 1, 256), (2, 2, 1, 256), (1, 12, 1, 256), (1, 5, 2, 257), (1, 7, 3, 257),
    (1, 5, 1, 1017), (2, 2, 2, 1017), (1, 7, 2, 1020), (1, 15, 1, 1020), (1, 3, 2, 1021), (1, 16, 1, 1021),
    (2, 1, 1, 1024), (1, 11, 1, 1024), (1, 16, 2, 1024), (1, 2, 3, 1025), (1, 12, 1, 1025), (1, 15, 1, 1025), (2, 16, 1, 1025),
)
BUMP_CASES = {"bump scalar": (57, 1017), "bump vector": (60, 1020)}       # Nk at which th_ld adds its bank-conflict bump
FUSED_ALL_KINDS = ((2, 3, 2, 2), (2, 7, 1, 4), (2, 11, 2, 5), (2, 3, 1, 57))     # the GPU test runs all four kinds here
ROW_WALK_CASES = ((3, 3, 345, 5), (7, 5, 293, 4))                          # 1035 and 2051 rows > TH_PARTS workgroups
# (B, H, Nq, Nk) of the flat kernels: M = Nq Nk = 1 .. 5 (a tile of one to five positions), the 512-position tile edge, two tiles
# and their edges, 1028 (vector, a 4-position last tile); every H of {1, 3, 8, 11, 16} has a scalar and a vector M
FLAT_CASES = (
    (2, 1, 1, 1), (2, 16, 1, 1), (2, 3, 1, 2), (2, 8, 3, 1), (2, 11, 2, 2), (2, 1, 2, 2), (2, 16, 1, 5), (2, 3, 5, 1),
    (2, 3, 7, 73), (2, 8, 7, 73), (2, 8, 2, 256), (2, 16, 2, 256), (2, 11, 27, 19), (2, 1, 27, 19), (2, 16, 3, 341),
    (2, 3, 4, 256), (2, 11, 4, 256), (2, 8, 1, 1025), (2, 1, 5, 205), (2, 11, 4, 257), (2, 16, 4, 257),
)
FLAT_M = (1, 2, 3, 4, 5, 511, 512, 513, 1023, 1024, 1025, 1028)
FLAT_ALL_KINDS = ((2, 3, 1, 2), (2, 11, 2, 2), (2, 16, 1, 5))
TILE_WALK_CASES = ((41, 4, 26, 500), (41, 3, 25, 501))                     # 1066 and 1025 tiles > TH_PARTS workgroups
GRID_CAP_CASES = ((2, 1, 8193, 1025), (2, 1, 32770, 1024))                 # scalar and vector: more than 65 536 x 256 items


def th_ld(np_: int) -> int:
    """csrc/nrv_heads.hpp th_ld, restated"""
    l = ((np_ + 3) & ~3) + 4
    return l if l & 63 else l + 4


def vec(n: int) -> int:
    """the kernels' V: 16-byte accesses when the row (fused) or the sample (flat) is a multiple of four positions"""
    return 4 if n % 4 == 0 else 1


# ----------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------
def inputs(B, H, Nq, Nk, kind="random"):
    """Seeded fp32 inputs of both families: S, dA [B, H, Nq, Nk]; W1, W2 (talking heads), W (re-attention) [H, H]; gamma, beta [H].
    random    S ~ 1.5 N(0,1), W ~ N(0,1) / sqrt(H), gamma ~ 1 + 0.5 N, beta ~ 0.5 N
    peaked    one key of every row stands 30 nats above the largest of the others in every head: the tail of softmax(S) is about
              1e-13, a normal fp32 number.  The re-attention W is the averaging matrix with a relative spread of 0.006 sqrt(H), so at
              the peak all heads of M agree to about 0.3 %: the regime the kernel's header names, a variance orders of magnitude
              below M^2 and close to eps
    flat      S constant along the keys: P = 1 / Nk (exactly when Nk is a power of two), dT is the pure cancellation term
    identity  W = I, gamma = 1, beta = 0"""
    assert kind in KINDS
    g = _gen("heads", B, H, Nq, Nk, kind)
    S = 1.5 * torch.randn(B, H, Nq, Nk, generator=g)
    dA = torch.randn(B, H, Nq, Nk, generator=g)
    W1, W2, W = (torch.randn(H, H, generator=g) / H ** 0.5 for _ in range(3))
    gamma = 1.0 + 0.5 * torch.randn(H, generator=g)
    beta = 0.5 * torch.randn(H, generator=g)
    if kind == "peaked":
        key = torch.randint(0, Nk, (B, 1, Nq, 1), generator=g).expand(B, H, Nq, 1)
        S = S.scatter(-1, key, S.amax(-1, keepdim=True) + 30.0)
        W = (1.0 + 0.006 * H ** 0.5 * torch.randn(H, H, generator=g)) / H
    elif kind == "flat":
        S = S[..., :1].expand(B, H, Nq, Nk).contiguous()
    elif kind == "identity":
        W1, W2, W = torch.eye(H), torch.eye(H), torch.eye(H)
        gamma, beta = torch.ones(H), torch.zeros(H)
    return {"S": S.contiguous(), "dA": dA, "W1": W1.contiguous(), "W2": W2.contiguous(), "W": W.contiguous(), "gamma": gamma, "beta": beta}


# ----------------------------------------------------------------------------------------------
# fp64 references and bounds
# ----------------------------------------------------------------------------------------------
def _mix(x, W):
    """out[g] = sum_h W[h, g] x[h]"""
    return torch.einsum("bhij,hg->bgij", x, W)


def _mix_t(d, W):
    """out[h] = sum_g W[h, g] d[g]"""
    return torch.einsum("bgij,hg->bhij", d, W)


def _pairs(x, y):
    return torch.einsum("bhij,bgij->hg", x, y)


def _hv(v):
    return v.view(1, -1, 1, 1)


def _d(*ts):
    return tuple(t.detach().double().cpu() for t in ts)


def _stored(ref, e, bf):
    """the bound of a value the kernel stores as fp32 or as bf16 (one rounding of the fp32 value)"""
    return e + (BF16 * (ref.abs() + e) if bf else 0.0) + TINY


def softmax_ref(T, eT):
    """(P, bound) of the row softmax of T [.., Nk] whose own error is at most eT"""
    Nk = T.shape[-1]
    P = torch.softmax(T, dim=-1)
    gap = (T - T.amax(-1, keepdim=True)).abs().amax(-1, keepdim=True)
    rel = 2 * eT.amax(-1, keepdim=True) + (gap + 5) * 2.0 ** -22 + 2.0 ** -21 + (Nk + 8) * U32
    return P, rel * (P + TINY) + TINY


def _softmax_bwd_ref(P, dP, e_dP):
    """(P (dP - <P, dP>), its bound) for an exact P"""
    Nk = P.shape[-1]
    Pm = P + TINY
    ref = P * (dP - (P * dP).sum(-1, keepdim=True))
    D = (Pm * dP.abs()).sum(-1, keepdim=True)
    e = Pm * (e_dP + (Pm * e_dP).sum(-1, keepdim=True) + (Nk + 2) * U32 * D + U32 * (dP.abs() + D)) + U32 * ref.abs()
    return ref, e


def th_fwd_ref(S, W1, W2, P_kernel=None, bf=False):
    """P and its bound from S; A and its bound from the kernel's P (the fp64 P where none is given)"""
    S, W1, W2 = _d(S, W1, W2)
    H = S.shape[1]
    T = _mix(S, W1)
    P, Pb = softmax_ref(T, (H + 1) * U32 * _mix(S.abs(), W1.abs()))
    Pk = P if P_kernel is None else _d(P_kernel)[0]
    A = _mix(Pk, W2)
    return {"P": P, "P_bound": Pb, "A": A, "A_bound": _stored(A, (H + 1) * U32 * _mix(Pk.abs() + TINY, W2.abs()), bf)}


def th_bwd_ref(dA, P, S, W1, W2):
    dA, P, S, W1, W2 = _d(dA, P, S, W1, W2)
    H = S.shape[1]
    dP = _mix_t(dA, W2)
    dT, e_dT = _softmax_bwd_ref(P, dP, (H + 1) * U32 * _mix_t(dA.abs(), W2.abs()))
    dS = _mix_t(dT, W1)
    return {"dS": dS, "dS_bound": (H + 1) * U32 * _mix_t(dT.abs(), W1.abs()) + _mix_t(e_dT, W1.abs()) + TINY,
            "dW1": _pairs(S, dT), "dW1_bound": NSUM * U32 * _pairs(S.abs(), dT.abs()) + _pairs(S.abs(), e_dT) + TINY,
            "dW2": _pairs(P, dA), "dW2_bound": NSUM * U32 * _pairs(P.abs() + TINY, dA.abs()) + TINY}


def mix_fwd_ref(x, W, bf=False):
    x, W = _d(x, W)
    out = _mix(x, W)
    return {"out": out, "out_bound": _stored(out, (x.shape[1] + 1) * U32 * _mix(x.abs(), W.abs()), bf)}


def mix_bwd_ref(dout, x, W):
    dout, x, W = _d(dout, x, W)
    return {"din": _mix_t(dout, W), "din_bound": (x.shape[1] + 1) * U32 * _mix_t(dout.abs(), W.abs()) + TINY,
            "dW": _pairs(x, dout), "dW_bound": NSUM * U32 * _pairs(x.abs(), dout.abs()) + TINY}


def _norm_parts(P, W, eps):
    """x^, rstd, their bounds (e_x; E, the error of a deviation) and M from an exact P (module docstring, LayerNorm)"""
    H = P.shape[1]
    M = _mix(P, W)
    e_M = (H + 1) * U32 * _mix(P.abs() + TINY, W.abs())
    d = M - M.mean(1, keepdim=True)
    rstd = torch.rsqrt((d * d).mean(1, keepdim=True) + eps)
    xh = d * rstd
    E = e_M.amax(1, keepdim=True) + e_M.mean(1, keepdim=True) + (H + 1) * U32 * M.abs().mean(1, keepdim=True) + U32 * d.abs().amax(1, keepdim=True)
    e_x = (1 + xh.abs()) * rstd * E + (H + 6) * U32 * xh.abs()
    return xh, rstd, e_x, E


def ra_softmax_ref(S):
    S = _d(S)[0]
    P, Pb = softmax_ref(S, torch.zeros_like(S))
    return {"P": P, "P_bound": Pb}


def ra_norm_fwd_ref(P, W, gamma, beta, eps=EPS, bf=False):
    """A and its bound from the P the kernel read (re-attention's fused forward: the P it wrote)"""
    P, W, gamma, beta = _d(P, W, gamma, beta)
    xh, _, e_x, _ = _norm_parts(P, W, eps)
    A = xh * _hv(gamma) + _hv(beta)
    return {"A": A, "A_bound": _stored(A, _hv(gamma).abs() * e_x + U32 * A.abs(), bf)}


def ra_bwd_ref(dA, P, W, gamma, eps=EPS, softmax=True):
    """dW, dgamma, dbeta and dS (the fused backward, softmax=True) or dP (the flat one), with bounds"""
    dA, P, W, gamma = _d(dA, P, W, gamma)
    H = P.shape[1]
    xh, rstd, e_x, E = _norm_parts(P, W, eps)
    dx = dA * _hv(gamma)
    e_dx = U32 * dx.abs()
    s1, s2 = dx.mean(1, keepdim=True), (dx * xh).mean(1, keepdim=True)
    e_s1 = (H + 1) * U32 * dx.abs().mean(1, keepdim=True) + e_dx.mean(1, keepdim=True)
    e_s2 = (H + 2) * U32 * (dx * xh).abs().mean(1, keepdim=True) + (dx.abs() * e_x + e_dx * xh.abs()).mean(1, keepdim=True)
    dM = rstd * ((dx - s1) - xh * s2)
    e_in = e_dx + e_s1 + e_x * s2.abs() + xh.abs() * e_s2 + 2 * U32 * (dx.abs() + s1.abs() + (xh * s2).abs())
    e_dM = rstd * e_in + dM.abs() * (rstd * E + (H + 7) * U32)
    dP = _mix_t(dM, W)
    e_dP = (H + 1) * U32 * _mix_t(dM.abs(), W.abs()) + _mix_t(e_dM, W.abs())
    Pm = P.abs() + TINY
    r = {"dW": _pairs(P, dM), "dW_bound": NSUM * U32 * _pairs(Pm, dM.abs()) + _pairs(Pm, e_dM) + TINY,
         "dgamma": (dA * xh).sum((0, 2, 3)), "dgamma_bound": NSUM * U32 * (dA * xh).abs().sum((0, 2, 3)) + (dA.abs() * e_x).sum((0, 2, 3)) + TINY,
         "dbeta": dA.sum((0, 2, 3)), "dbeta_bound": NSUM * U32 * dA.abs().sum((0, 2, 3)) + TINY}
    if softmax:
        dS, e_dS = _softmax_bwd_ref(P, dP, e_dP)
        r["dS"], r["dS_bound"] = dS, e_dS + TINY
    else:
        r["dP"], r["dP_bound"] = dP, e_dP + TINY
    return r


# ----------------------------------------------------------------------------------------------
# emulation of the kernels' fp32 arithmetic.  Images are [R, H, n]: R rows of a fused kernel or R tiles of a flat one
# ----------------------------------------------------------------------------------------------
_LOG2E = torch.tensor(1.4426950408889634, dtype=torch.float32)


def _rows(t):
    """[B, H, Nq, Nk] -> [B*Nq, H, Nk]"""
    B, H, Nq, Nk = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * Nq, H, Nk)


def _unrows(t, B):
    R, H, Nk = t.shape
    return t.reshape(B, R // B, H, Nk).permute(0, 2, 1, 3).contiguous()


def _tiles(t):
    """[B, H, Nq, Nk] -> [B*tiles, H, TH_TILE], the last tile of a sample padded with zeros"""
    B, H = t.shape[:2]
    M = t.shape[2] * t.shape[3]
    nt = -(-M // TH_TILE)
    f = torch.zeros(B, H, nt * TH_TILE, dtype=t.dtype)
    f[:, :, :M] = t.reshape(B, H, M)
    return f.reshape(B, H, nt, TH_TILE).permute(0, 2, 1, 3).reshape(B * nt, H, TH_TILE)


def _untiles(t, B, Nq, Nk):
    R, H, _ = t.shape
    return t.reshape(B, R // B, H, TH_TILE).permute(0, 2, 1, 3).reshape(B, H, -1)[:, :, :Nq * Nk].reshape(B, H, Nq, Nk).contiguous()


def mix_emul(x, W, transpose=False):
    """th_mix / head_mix / ra_mix on [R, H, n]: acc = 0, then fma(w, x[i], acc) for i = 0 .. H-1.  transpose=False: out[g] =
    sum_h W[h, g] x[h]; True: out[h] = sum_g W[h, g] x[g]"""
    H = x.shape[1]
    Wm = W.t() if transpose else W                                        # Wm[i, o]
    acc = torch.zeros_like(x)
    for i in range(H):
        acc = _fma32(Wm[i].reshape(1, H, 1), x[:, i:i + 1], acc)
    return acc


def _lanes(t, fill):
    """[.., n] -> [.., steps, 64]: key j = step * 64 + lane"""
    n = t.shape[-1]
    steps = -(-n // 64)
    out = torch.full(t.shape[:-1] + (steps * 64,), fill, dtype=t.dtype)
    out[..., :n] = t
    return out.reshape(t.shape[:-1] + (steps, 64))


def _butterfly(v):
    """wave_sum: v += shfl_xor(v, o) for o = 32 .. 1 on [.., 64]; every lane ends with the same bits, lane 0 is returned"""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., :1]


def softmax_emul(T, drop_last=False):
    """The wave-per-head softmax of [.., Nk] fp32.  drop_last (a wrong kernel): the last key is left out of the row sum"""
    Nk = T.shape[-1]
    m = T.amax(-1, keepdim=True)
    e = torch.exp2(((T - m) * _LOG2E).double()).float()
    el = _lanes(e, 0.0)
    if drop_last:
        el.reshape(el.shape[:-2] + (-1,))[..., Nk - 1] = 0.0
    s = torch.zeros(el.shape[:-2] + (64,))
    for k in range(el.shape[-2]):
        s = s + el[..., k, :]
    inv = 1.0 / _butterfly(s)
    return e * inv


def softmax_bwd_emul(P, dP):
    """d = P (dP - dot), dot = the lanes' fma chains over keys lane, lane + 64, .. and the butterfly"""
    pl, dl = _lanes(P, 0.0), _lanes(dP, 0.0)
    dot = torch.zeros(pl.shape[:-2] + (64,))
    for k in range(pl.shape[-2]):
        dot = _fma32(pl[..., k, :], dl[..., k, :], dot)
    return P * (dP - _butterfly(dot))


def _pad4(t, garbage=0.0):
    """an LDS image's positions n .. round-up-to-4: zero (th_load); garbage != 0 is a wrong kernel"""
    n = t.shape[-1]
    out = torch.full(t.shape[:-1] + ((n + 3) & ~3,), garbage, dtype=t.dtype)
    out[..., :n] = t
    return out


def pairs_emul(x, y, idle_twice=False):
    """th_pairs + th_pairs_out + the reduce kernel on images x, y [R, H, n4] (n4 % 4 == 0): fp64 [H, H].  Thread (split, h, g)
    runs four fma chains over the 4-position groups split, split + nsplit, ..; the image's sum is (a0 + a1) + (a2 + a3) in fp32;
    everything after that is double.  idle_twice (a wrong kernel): the threads past nsplit * H * H are not idle but walk as split
    `nsplit` would, so pairs 0 .. 255 - nsplit H H count the groups nsplit, 2 nsplit, .. twice"""
    R, H, n4 = x.shape
    pairs = H * H
    nsplit = TH_THREADS // pairs
    q = n4 // 4
    steps = -(-q // nsplit)
    xs, ys = (torch.zeros(R, H, steps * nsplit * 4) for _ in range(2))
    xs[..., :n4], ys[..., :n4] = x, y
    xs, ys = xs.reshape(R, H, 1, steps, nsplit, 4), ys.reshape(R, 1, H, steps, nsplit, 4)
    acc = torch.zeros(R, H, H, nsplit, 4)
    for t in range(steps):
        acc = _fma32(xs[:, :, :, t], ys[:, :, :, t], acc)
    img = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])        # fp32, [R, H, H, nsplit]
    out = img.double().sum((0, 3))
    if idle_twice:
        extra = torch.zeros(R, H, H, 4)
        for t in range(1, steps):                                          # groups nsplit, 2 nsplit, ..: split 0's steps 1 ..
            extra = _fma32(xs[:, :, :, t, 0], ys[:, :, :, t, 0], extra)
        e = ((extra[..., 0] + extra[..., 1]) + (extra[..., 2] + extra[..., 3])).double().sum(0).reshape(-1)
        e[TH_THREADS - nsplit * pairs:] = 0.0
        out = out + e.reshape(H, H)
    return out


def th_fwd_emul(S, W1, W2, drop_last=False):
    """(P fp32, A fp32): nrv_th_softmax_fwd; bf16(A) is the bf16 launch's A"""
    B = S.shape[0]
    P = softmax_emul(mix_emul(_rows(S), W1), drop_last)
    return _unrows(P, B), _unrows(mix_emul(P, W2), B)


def th_bwd_emul(dA, P, S, W1, W2, untransposed=False, pad_garbage=0.0, idle_twice=False):
    """(dS fp32, dW1, dW2 fp32): nrv_th_softmax_bwd.  Wrong kernels: untransposed (both gradient mixes read W[g, h]), pad_garbage
    (the pad positions of the scalar path's images hold that value when th_pairs sums S . dT), idle_twice (pairs_emul, on dW2)"""
    B = S.shape[0]
    d, p, s = _rows(dA), _rows(P), _rows(S)
    dW2 = pairs_emul(_pad4(p), _pad4(d), idle_twice)
    dT = softmax_bwd_emul(p, mix_emul(d, W2, transpose=not untransposed))
    dW1 = pairs_emul(_pad4(s, pad_garbage), _pad4(dT, pad_garbage))
    return _unrows(mix_emul(dT, W1, transpose=not untransposed), B), dW1.float(), dW2.float()


def mix_fwd_emul(x, W):
    B = x.shape[0]
    return _unrows(mix_emul(_rows(x), W), B)


def mix_bwd_emul(dout, x, W, untransposed=False):
    """(din, dW fp32): nrv_head_mix_bwd on 512-position tiles"""
    B, _, Nq, Nk = x.shape
    d, xt = _tiles(dout), _tiles(x)
    return _untiles(mix_emul(d, W, transpose=not untransposed), B, Nq, Nk), pairs_emul(xt, d).float()


def _normalise_emul(m, eps, one_pass=False):
    """ra_normalise on [R, H, n]: (x^, rstd).  one_pass (a wrong kernel): var = E[m^2] - E[m]^2"""
    H = m.shape[1]
    inv_h = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(H), dtype=torch.float32)
    mu = torch.zeros_like(m[:, :1])
    for g in range(H):
        mu = mu + m[:, g:g + 1]
    mu = mu * inv_h
    d = m - mu
    var = torch.zeros_like(mu)
    if one_pass:
        for g in range(H):
            var = _fma32(m[:, g:g + 1], m[:, g:g + 1], var)
        rstd = torch.rsqrt((_fma32(var, inv_h, -(mu * mu)) + torch.tensor(eps, dtype=torch.float32)).double()).float()
    else:
        for g in range(H):
            var = _fma32(d[:, g:g + 1], d[:, g:g + 1], var)
        rstd = torch.rsqrt(_fma32(var, inv_h, torch.tensor(eps, dtype=torch.float32)).double()).float()
    return d * rstd, rstd


def norm_point_emul(p, W, gamma, beta, eps=EPS, one_pass=False):
    """ra_point_fwd on [R, H, n]: A fp32"""
    xh, _ = _normalise_emul(mix_emul(p, W), eps, one_pass)
    return _fma32(xh, gamma.reshape(1, -1, 1), beta.reshape(1, -1, 1))


def _threads(t, V):
    """[R, H, n] -> [R, H, steps, 256, V]: thread t's positions are t V .. t V + V - 1, then a stride of 256 V"""
    R, H, n = t.shape
    w = TH_THREADS * V
    steps = -(-n // w)
    out = torch.zeros(R, H, steps * w)
    out[..., :n] = t
    return out.reshape(R, H, steps, TH_THREADS, V)


def image_bwd_emul(p, d, W, gamma, eps, V, skip_last_wave=False):
    """ra_image_bwd + ra_vec_out + the reduce kernel on images [R, H, n]: (dM fp32 [R, H, n], dgamma fp64 [H], dbeta fp64 [H]).
    skip_last_wave (a wrong kernel): threads 192 .. 255 are left out of dgamma"""
    H = p.shape[1]
    inv_h = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(H), dtype=torch.float32)
    xh, rstd = _normalise_emul(mix_emul(p, W), eps)
    xt, dt = _threads(xh, V), _threads(d, V)
    dg, db = torch.zeros(p.shape[0], H, TH_THREADS), torch.zeros(p.shape[0], H, TH_THREADS)
    for k in range(xt.shape[2]):
        for v in range(V):
            db = db + dt[:, :, k, :, v]
            dg = _fma32(dt[:, :, k, :, v], xt[:, :, k, :, v], dg)
    if skip_last_wave:
        dg = dg[..., :192]
    dx = d * gamma.reshape(1, -1, 1)
    s1, s2 = torch.zeros_like(dx[:, :1]), torch.zeros_like(dx[:, :1])
    for g in range(H):
        s1 = s1 + dx[:, g:g + 1]
        s2 = _fma32(dx[:, g:g + 1], xh[:, g:g + 1], s2)
    s1, s2 = s1 * inv_h, s2 * inv_h
    dM = rstd * ((dx - s1) - xh * s2)
    return dM, dg.double().sum((0, 2)), db.double().sum((0, 2))


def ra_fwd_emul(S, W, gamma, beta, eps=EPS, drop_last=False, one_pass=False):
    """(P fp32, A fp32): nrv_reattn_softmax_fwd"""
    B = S.shape[0]
    P = softmax_emul(_rows(S), drop_last)
    return _unrows(P, B), _unrows(norm_point_emul(P, W, gamma, beta, eps, one_pass), B)


def ra_norm_fwd_emul(P, W, gamma, beta, eps=EPS, one_pass=False):
    return _unrows(norm_point_emul(_rows(P), W, gamma, beta, eps, one_pass), P.shape[0])


def ra_bwd_emul(dA, P, W, gamma, eps=EPS, untransposed=False, skip_last_wave=False):
    """(dS, dW, dgamma, dbeta) fp32: nrv_reattn_softmax_bwd"""
    B, _, _, Nk = P.shape
    p, d = _rows(P), _rows(dA)
    dM, dg, db = image_bwd_emul(p, d, W, gamma, eps, vec(Nk), skip_last_wave)
    dW = pairs_emul(_pad4(p), _pad4(dM))
    dS = softmax_bwd_emul(p, mix_emul(dM, W, transpose=not untransposed))
    return _unrows(dS, B), dW.float(), dg.float(), db.float()


def ra_norm_bwd_emul(dA, P, W, gamma, eps=EPS, untransposed=False, skip_last_wave=False):
    """(dP, dW, dgamma, dbeta) fp32: nrv_reattn_norm_bwd on 512-position tiles"""
    B, _, Nq, Nk = P.shape
    p, d = _tiles(P), _tiles(dA)
    dM, dg, db = image_bwd_emul(p, d, W, gamma, eps, vec(Nq * Nk), skip_last_wave)
    dP = _untiles(mix_emul(dM, W, transpose=not untransposed), B, Nq, Nk)
    return dP, pairs_emul(p, dM).float(), dg.float(), db.float()
