"""fp64 restatements of the PatchConvNet kernels (include/nrv.h, ABI 17), their per-element error bounds, and the seeded inputs
of tests/test_pcn_edges_gpu.py (test infrastructure, plain torch, no kernels).

Every restatement takes the kernels' own operands (bf16 or fp32), upcasts them to float64 and returns float64.  The backward
restatements are written out by hand; tests/test_pcn_ref_host.py holds them against torch.autograd of the forward ones.

Bounds.  EPS = 2^-24 (half an fp32 ulp, relative), BF = 2^-8 (one bf16 ulp, relative).
  * An fp32 sum of n terms in any order is within acc(n, sum|terms|) = (n + 8) EPS sum|terms| of the exact sum; the 8 covers the
    few roundings that form one term (a scale, a product).
  * Where the summed terms are themselves computed values, their own error e_term is carried along: |factor| e_term is added per
    term.  The chains below (e_u -> e_dd -> e_da, e_ds -> e_dz -> e_dp -> e_dmean) do nothing else.
  * The kernels' GELU is erf by Abramowitz-Stegun 7.1.26 (|erf error| <= 1.5e-7, so 0.75e-7 on Phi) with one v_rcp and one v_exp
    (1 ulp each, on factors that are at most 1): PHI_ABS = 5e-7 bounds the absolute error of Phi(u) and of gelu'(u) =
    Phi + u phi at an exact u.  |gelu'| <= 1.13 and |gelu''| <= 0.8 carry an error of u into gelu(u) and gelu'(u).
  * Values through __expf / __logf (the SE gate, lse, P) keep the project's 1e-5 relative (EXP_REL); class-attention gradient
    rows keep its 2e-2 (ROW_REL), per key row against the largest reference row of the same (sample, head).
"""
from __future__ import annotations

import math
from typing import Optional

import torch

D = torch.float64
EPS = 2.0 ** -24
BF = 2.0 ** -8
PHI_ABS = 5e-7
EXP_REL = 1e-5
ROW_REL = 2e-2


def up(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(D)


def acc(n: int, sum_abs):
    return (n + 8) * EPS * sum_abs


def bf16_tol(ref: torch.Tensor, A=0.0) -> torch.Tensor:
    return BF * ref.abs() + A


def excess(got: torch.Tensor, ref: torch.Tensor, tol) -> float:
    """Worst |got - ref| / tol over all elements (0 / 0 counts as 0, x / 0 as inf): <= 1 means every element is inside its bound."""
    err = (up(got).cpu() - ref.cpu()).abs()
    tol = torch.as_tensor(tol, dtype=D).cpu().expand_as(err)
    r = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def gelu(u: torch.Tensor) -> torch.Tensor:
    return u * 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))


def dgelu(u: torch.Tensor) -> torch.Tensor:
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


# ---- depthwise 3x3 --------------------------------------------------------------------------------------------------------------
def _shift(x: torch.Tensor, dy: int, dx: int) -> torch.Tensor:
    """[B, H, W, C] -> the same shape with out(y, x) = in(y + dy, x + dx), zero outside the map."""
    B, H, W, C = x.shape
    p = x.new_zeros(B, H + 2, W + 2, C)
    p[:, 1:H + 1, 1:W + 1] = x
    return p[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def dwconv_fwd(a, w, bias, B: int, H: int, W: int) -> dict:
    """d = gelu(pre), pre(y, x) = bias + sum_t w[t] a(y + t / 3 - 1, x + t % 3 - 1); sq = sum over the map of d.  Rows [B*H*W, C]."""
    C = a.shape[1]
    x, w9, b = up(a).reshape(B, H, W, C), up(w).reshape(C, 9), up(bias)
    taps = [_shift(x, t // 3 - 1, t % 3 - 1) for t in range(9)]
    pre = b + sum(w9[:, t] * taps[t] for t in range(9))
    abs_pre = b.abs() + sum((w9[:, t] * taps[t]).abs() for t in range(9))
    d = gelu(pre)
    e_u = acc(9, abs_pre)
    d_A = 1.13 * e_u + pre.abs() * PHI_ABS + 2 * EPS * d.abs()
    return {"pre": pre.reshape(-1, C), "d": d.reshape(-1, C), "d_A": d_A.reshape(-1, C), "sq": d.sum((1, 2)),
            "sq_tol": acc(H * W, d.abs().sum((1, 2))) + d_A.sum((1, 2)), "_taps": taps, "_e_u": e_u, "_pre": pre}


def dwconv_bwd(a, w, bias, dg, s, dmean, B: int, H: int, W: int) -> dict:
    """dd = (dg s[b] + dmean[b] / (H W)) gelu'(pre); dw[c, t] = sum dd tap_t, db = sum dd; da(p) = sum_t w[t] dd(p - off_t), WITHOUT
    the stream factor (the caller multiplies it in).  e_da is the fp32 error bound of that un-multiplied da."""
    C = a.shape[1]
    f = dwconv_fwd(a, w, bias, B, H, W)
    w9, taps, pre = up(w).reshape(C, 9), f["_taps"], f["_pre"]
    g, sc, dm = up(dg).reshape(B, H, W, C), up(s)[:, None, None, :], up(dmean)[:, None, None, :] / (H * W)
    v0, v0abs = g * sc + dm, (g * sc).abs() + dm.abs()
    gp = dgelu(pre)
    dd = v0 * gp
    e_dd = v0abs * (PHI_ABS + 0.8 * f["_e_u"]) + 4 * EPS * v0abs * gp.abs()
    n = B * H * W
    dw = torch.stack([(dd * taps[t]).sum((0, 1, 2)) for t in range(9)], 1)
    dw_tol = torch.stack([acc(n, (dd * taps[t]).abs().sum((0, 1, 2))) + (e_dd * taps[t].abs()).sum((0, 1, 2)) for t in range(9)], 1)
    db, db_tol = dd.sum((0, 1, 2)), acc(n, dd.abs().sum((0, 1, 2))) + e_dd.sum((0, 1, 2))
    back = [(-(t // 3 - 1), -(t % 3 - 1)) for t in range(9)]
    da = sum(w9[:, t] * _shift(dd, *back[t]) for t in range(9))
    e_da = sum(w9[:, t].abs() * _shift(e_dd, *back[t]) for t in range(9)) + acc(9, sum((w9[:, t] * _shift(dd, *back[t])).abs() for t in range(9)))
    return {"dd": dd.reshape(-1, C), "da": da.reshape(-1, C), "e_da": e_da.reshape(-1, C), "dw": dw, "dw_tol": dw_tol, "db": db,
            "db_tol": db_tol}


# ---- the 8-bit gelu' stream (include/nrv.h, NRV_EPI_BIAS_GELU_Q8) ---------------------------------------------------------------
def q8_offsets(M: int, N: int, ld: int) -> torch.Tensor:
    m, n = torch.arange(M)[:, None], torch.arange(N)[None, :]
    return (m >> 1) * 2 * ld + (n >> 6) * 128 + (m & 1) * 64 + (n & 63)


def q8_pack(g: torch.Tensor, ld: Optional[int] = None, fill: int = 0) -> torch.Tensor:
    """uint8 [rows_even * ld]: q = round(202 g) + 26 of g [M, N] (N % 64 == 0), byte (m, n) at (m >> 1) 2 ld + (n >> 6) 128 +
    (m & 1) 64 + (n & 63); rows rounded up to even; bytes no element maps to hold `fill`."""
    M, N = g.shape
    ld = N if ld is None else ld
    assert N % 64 == 0 and ld % 16 == 0 and ld >= N
    q = (torch.round(202.0 * up(g).cpu()) + 26.0).clamp(0, 255).to(torch.uint8)
    buf = torch.full(((M + 1) // 2 * 2 * ld,), fill, dtype=torch.uint8)
    buf[q8_offsets(M, N, ld).reshape(-1)] = q.reshape(-1)
    return buf


def q8_unpack(buf: torch.Tensor, M: int, N: int, ld: Optional[int] = None) -> torch.Tensor:
    ld = N if ld is None else ld
    return (buf.detach().cpu().reshape(-1)[q8_offsets(M, N, ld)].to(D) - 26.0) / 202.0


# ---- squeeze-and-excitation -----------------------------------------------------------------------------------------------------
def se_fwd(sq, HW: int, wr, br, we, be) -> dict:
    rd = wr.shape[0]
    sq, br, be = up(sq), up(br), up(be)
    C = sq.shape[1]
    wr, we = up(wr).reshape(rd, C), up(we).reshape(C, rd)
    mean = sq / HW
    pre = mean @ wr.t() + br
    hid = pre.clamp_min(0.0)
    z = hid @ we.t() + be
    return {"mean": mean, "pre": pre, "hid": hid, "z": z, "s": torch.sigmoid(z)}


def se_bwd(dg, d, sq, HW: int, s, hid, wr, we) -> dict:
    """ds = sum_hw dg d; dz = ds s (1 - s); dp = [hid > 0] W_e^T dz; dmean = W_r^T dp; dW_e = sum_b dz hid^T, db_e = sum_b dz,
    dW_r = sum_b dp mean^T, db_r = sum_b dp.  `*_tol`: the fp32 bound of each, the error of ds carried down the chain."""
    s, hid, sq = up(s), up(hid), up(sq)
    B, C = s.shape
    rd = hid.shape[1]
    wr, we = up(wr).reshape(rd, C), up(we).reshape(C, rd)
    prod = (up(dg) * up(d)).reshape(B, HW, C)
    ds, e_ds = prod.sum(1), acc(HW, prod.abs().sum(1))
    sp = s * (1.0 - s)
    dz = ds * sp
    e_dz = e_ds * sp + 3 * EPS * dz.abs()
    gate = (hid > 0).to(D)
    dp = (dz @ we) * gate
    e_dp = (e_dz @ we.abs() + acc(C, dz.abs() @ we.abs())) * gate
    dmean = dp @ wr
    mean = sq / HW
    return {"ds": ds, "dz": dz, "dp": dp, "dmean": dmean, "dmean_tol": e_dp @ wr.abs() + acc(rd, dp.abs() @ wr.abs()),
            "dwe": dz.t() @ hid, "dwe_tol": e_dz.t() @ hid.abs() + acc(B, dz.abs().t() @ hid.abs()),
            "dbe": dz.sum(0), "dbe_tol": e_dz.sum(0) + acc(B, dz.abs().sum(0)),
            "dwr": dp.t() @ mean, "dwr_tol": e_dp.t() @ mean.abs() + acc(B, dp.abs().t() @ mean.abs()),
            "dbr": dp.sum(0), "dbr_tol": e_dp.sum(0) + acc(B, dp.abs().sum(0))}


# ---- LayerScale residual --------------------------------------------------------------------------------------------------------
def _ls_f(rows: int, keep, survival: float, rps: int) -> torch.Tensor:
    if keep is None:
        return torch.ones(rows, 1, dtype=D)
    surv = float(torch.tensor(survival, dtype=torch.float32))          # the ABI takes survival as a float
    return (up(keep) / surv).repeat_interleave(rps)[:, None]


def ls_add(x, y, gamma, keep=None, survival: float = 1.0, rps: int = 1) -> dict:
    f = _ls_f(x.shape[0], keep, survival, rps).to(x.device)
    t = f * up(gamma) * up(y)
    return {"out": up(x) + t, "tol": 4 * EPS * (up(x).abs() + t.abs())}       # 1 / survival, keep f, f gamma, the fma: four roundings


def ls_bwd(dy, y, gamma, keep=None, survival: float = 1.0, rps: int = 1) -> dict:
    f = _ls_f(dy.shape[0], keep, survival, rps).to(dy.device)
    v = up(dy) * f
    return {"dz": v * up(gamma), "dgamma": (v * up(y)).sum(0), "dgamma_tol": acc(dy.shape[0], (v * up(y)).abs().sum(0))}


# ---- class attention ------------------------------------------------------------------------------------------------------------
def ca_rows(c, p, B: int, Np: int, H: int, dh: int) -> torch.Tensor:
    """Class rows c [B, >= H dh] and patch rows p [B Np, >= H dh] (any strides; None when Np == 0) -> per-key rows [B, H, 1 + Np, dh]."""
    C = H * dh
    k = up(c)[:B, :C].reshape(B, 1, H, dh)
    if Np > 0:
        k = torch.cat((k, up(p)[:B * Np, :C].reshape(B, Np, H, dh)), 1)
    return k.transpose(1, 2)


def cls_attn_fwd(q, kc, kp, vc, vp, B: int, H: int, Np: int, dh: int, scale: float) -> dict:
    Q = up(q)[:B, :H * dh].reshape(B, H, dh)
    K, V = ca_rows(kc, kp, B, Np, H, dh), ca_rows(vc, vp, B, Np, H, dh)
    S = torch.einsum("bhd,bhjd->bhj", Q, K) * scale
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    Nk = Np + 1
    s_abs = scale * torch.einsum("bhd,bhjd->bhj", Q.abs(), K.abs()).max(-1).values
    o_abs = torch.einsum("bhj,bhjd->bhd", P, V.abs())
    return {"o": torch.einsum("bhj,bhjd->bhd", P, V).reshape(B, H * dh), "o_A": ((Nk + 8) * EPS + EXP_REL) * o_abs.reshape(B, H * dh),
            "lse": lse, "lse_tol": EXP_REL * lse.abs() + acc(dh, s_abs), "P": P, "_Q": Q, "_K": K, "_V": V}


def cls_attn_bwd(q, kc, kp, vc, vp, dout, B: int, H: int, Np: int, dh: int, scale: float) -> dict:
    """dq [B, H, dh]; dk, dv per key [B, H, 1 + Np, dh] (key 0 = the class row): dP_j = dout . v_j, dS = P (dP - sum_j P_j dP_j),
    dk_j = scale dS_j q, dv_j = P_j dout, dq = scale sum_j dS_j k_j."""
    f = cls_attn_fwd(q, kc, kp, vc, vp, B, H, Np, dh, scale)
    Q, K, V, P = f["_Q"], f["_K"], f["_V"], f["P"]
    do = up(dout)[:B, :H * dh].reshape(B, H, dh)
    dP = torch.einsum("bhd,bhjd->bhj", do, V)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    return {"dq": scale * torch.einsum("bhj,bhjd->bhd", dS, K), "dk": scale * dS[..., None] * Q[:, :, None, :],
            "dv": P[..., None] * do[:, :, None, :], "P": P, "dP": dP, "dS": dS, "lse": f["lse"]}


def row_err(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """|got - ref| of each [..., rows, dh] row over the largest reference row norm of its (sample, head): [..., rows]."""
    got, ref = up(got).cpu(), ref.cpu()
    big = ref.norm(dim=-1).max(dim=-1, keepdim=True).values
    num = (got - ref).norm(dim=-1)
    return torch.where(big > 0, num / big.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num)))


# ---- seeded inputs: the cases of tests/test_pcn_edges_gpu.py, on the CPU ---------------------------------------------------------
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed: int, scale: float = 1.0, dtype=torch.float32) -> torch.Tensor:
    return (torch.randn(*shape, generator=_gen(seed)) * scale).to(dtype)


# (B, H, W, C): H != W, C not a multiple of the 64-channel block, one-row and one-column maps, fewer tokens than row groups
DW_CASES = ((2, 3, 5, 8), (3, 5, 3, 72), (2, 1, 7, 64), (2, 7, 1, 64), (1, 1, 1, 8), (2, 6, 9, 128), (1, 3, 5, 64))
DW_Q8_ONLY = ((3, 3, 3, 64),)          # 9 rows per sample: the sample boundaries fall inside a row pair of the byte stream


def dw_inputs(B: int, H: int, W: int, C: int, seed: int = 0) -> dict:
    n = B * H * W
    base = _randn((C,), seed + 1, 0.05) + 0.04 * torch.sign(_randn((C,), seed + 2))
    w = base[:, None] * torch.arange(1, 10, dtype=torch.float32)[None, :]          # distinct per tap: no mirrored tap can cancel
    g = torch.rand(n, C, generator=_gen(seed + 8), dtype=D) * 1.258 - 0.129         # the range of gelu_erf'
    return {"a": _randn((n, C), seed + 3, dtype=torch.bfloat16), "w": w.contiguous(), "bias": _randn((C,), seed + 4, 0.1),
            "dg": _randn((n, C), seed + 5, dtype=torch.bfloat16), "s": torch.sigmoid(_randn((B, C), seed + 6)),
            "dmean": _randn((B, C), seed + 7), "g": g, "g16": g.to(torch.bfloat16), "g8": q8_pack(g) if C % 64 == 0 else None}


# (B, C, rd, HW): C not a multiple of 64 or 256, C > 256, rd not a multiple of the 4 waves, rd < 4, the documented limits
SE_CASES = ((1, 8, 2, 1), (3, 72, 18, 15), (2, 264, 66, 4), (5, 320, 1, 7), (2, 320, 3, 7), (2, 4096, 1024, 2))
SE_MIN_PRE = 1e-3


def se_inputs(B: int, C: int, rd: int, HW: int, seed: int = 0) -> dict:
    """b_r is chosen so that no hidden pre-activation is near 0: unit j either has one sign for every sample (odd j positive, even j
    negative) or, on even j where two samples' pre-activations lie 0.1 apart, changes sign between them."""
    d = _randn((B * HW, C), seed + 1, dtype=torch.bfloat16)
    sq = d.float().reshape(B, HW, C).sum(1)
    wr = _randn((rd, C), seed + 2, 0.3 * math.sqrt(HW / C))
    we, be = _randn((C, rd), seed + 3, 1.0 / math.sqrt(rd)), _randn((C,), seed + 4, 0.1)
    lin = (up(sq) / HW) @ up(wr).t()                                                # [B, rd]
    u = torch.rand(rd, generator=_gen(seed + 5), dtype=D)
    srt = lin.sort(0).values
    lo, hi = srt[0], srt[-1]
    sign = torch.where(torch.arange(rd) % 2 == 1, 1.0, -1.0).to(D)
    br = sign * (0.3 + 0.5 * (hi - lo) + 0.5 * u) - 0.5 * (hi + lo)
    if B >= 2:
        gaps = srt[1:] - srt[:-1]
        gmax, gi = gaps.max(0)
        mid = 0.5 * (srt.gather(0, gi[None])[0] + srt.gather(0, gi[None] + 1)[0])
        br = torch.where((torch.arange(rd) % 2 == 0) & (gmax >= 0.1), -mid, br)
    br = br.float()
    ref = se_fwd(sq, HW, wr, br, we, be)
    return {"d": d, "dg": _randn((B * HW, C), seed + 6, dtype=torch.bfloat16), "sq": sq, "wr": wr, "br": br, "we": we, "be": be,
            "s32": ref["s"].float(), "hid32": ref["hid"].float(), "ref": ref}


# (rows, C, rows_per_sample): fewer rows than one 128-row partial, exactly one, a sample boundary inside a partial, C % 64 != 0
LS_CASES = ((1, 4, 1), (127, 36, 127), (128, 64, 32), (129, 68, 43), (300, 100, 75), (257, 260, 257))


def ls_inputs(rows: int, C: int, rps: int, seed: int = 0) -> dict:
    ns = rows // rps
    # one 0 and one 1 at least; sample 0 is kept and sample 1 dropped.  A one-sample case runs once with each.
    keeps = [torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0][:ns])] if ns > 1 else [torch.zeros(1), torch.ones(1)]
    return {"x": _randn((rows, C), seed + 1), "y": _randn((rows, C), seed + 2), "gamma": _randn((C,), seed + 3, 0.1),
            "dy": _randn((rows, C), seed + 4), "keeps": keeps}


# (dh, Np, heads, B): one and two keys, dh / 8 lanes that do not divide 256 (40, 72, 520), the second 512-element pass (520, 1024),
# Nk at the 256-thread stride (256, 257) and at the 4096 limit
CA_CASES = ((8, 1, 1, 2), (8, 2, 3, 2), (40, 3, 3, 2), (72, 5, 2, 3), (520, 9, 1, 2), (64, 255, 2, 1), (64, 256, 1, 1), (64, 4095, 1, 2),
            (1024, 3, 1, 1))
CA_STRIDED = ((40, 3, 3, 2), (64, 255, 2, 1))
CA_NP0 = ((8, 1, 2), (72, 2, 3), (520, 1, 1))          # (dh, heads, B) with Np = 0


def ca_inputs(dh: int, Np: int, H: int, B: int, seed: int = 0) -> dict:
    C = H * dh
    bf = torch.bfloat16
    return {"q": _randn((B, C), seed + 1, dtype=bf), "kc": _randn((B, C), seed + 2, dtype=bf), "vc": _randn((B, C), seed + 3, dtype=bf),
            "kp": _randn((B * Np, C), seed + 4, dtype=bf) if Np else None, "vp": _randn((B * Np, C), seed + 5, dtype=bf) if Np else None,
            "dout": _randn((B, C), seed + 6, dtype=bf), "scale": dh ** -0.5}


PEAKED = {"dh": 64, "Np": 196, "H": 2, "B": 2, "nats": 20.0}


def ca_peaked_inputs(peak_key: int, seed: int = 0) -> dict:
    """Every head's query is the first unit vector; key `peak_key` (0 = the class key) scores 20 nats above the others' ~N(0, 0.1^2 / dh)."""
    dh, Np, H, B = PEAKED["dh"], PEAKED["Np"], PEAKED["H"], PEAKED["B"]
    C = H * dh
    q = torch.zeros(B, C)
    q[:, ::dh] = 1.0
    kc, kp = _randn((B, C), seed + 2, 0.1), _randn((B * Np, C), seed + 4, 0.1)
    peak = PEAKED["nats"] * dh ** 0.5
    if peak_key == 0:
        kc[:, ::dh] = peak
    else:
        kp.reshape(B, Np, C)[:, peak_key - 1, ::dh] = peak
    bf = torch.bfloat16
    return {"q": q.to(bf), "kc": kc.to(bf), "kp": kp.to(bf), "vc": _randn((B, C), seed + 3, dtype=bf), "vp": _randn((B * Np, C), seed + 5, dtype=bf),
            "dout": _randn((B, C), seed + 6, dtype=bf), "scale": dh ** -0.5}


# Peaked backward: with one key 20 nats up, 1 - P_peak ~ 196 e^-20 = 4e-7 while the saved fp32 lse (~ 20) is only known to an
# ulp, 2e-6.  dS = P (dP - D) therefore cancels to the size of lse's rounding: dk and dq, ~ 1e-7 of an ordinary gradient, carry an
# absolute error of that order whatever the summation order, and miss ROW_REL.  The host test measures the fp32 emulation's
# worst row (lse at its rounded value and one ulp to either side: the forward is held to 1e-5, far more than an ulp) at 15.7
# (patch key) and 13.5 (class key) times the largest reference row; the GPU test allows twice PEAKED_EMU.  dv does not cancel and
# keeps ROW_REL.  What still binds dk and dq there is the absolute bound of check_ca_peaked_abs.
PEAKED_EMU = 16.0


def check_ca_peaked_abs(ref: dict, dq, dk, q, K) -> dict:
    """The error of P, EXP_REL relative, reaches dS_j through D = sum P dP as P_j EXP_REL max|dP| at most (twice: P_j itself): every
    element of dk within 4 EXP_REL scale max|q| max|dP| and of dq within 4 EXP_REL scale max|k| max|dP|, plus one bf16 ulp."""
    B, H, Nk, dh = ref["dk"].shape
    scale = float(ref["dk"].abs().max() / (ref["dS"].abs().max() * up(q).abs().max()))
    m = 4 * EXP_REL * scale * float(ref["dP"].abs().max())
    return {"dk_abs": excess(dk, ref["dk"], bf16_tol(ref["dk"], m * float(up(q).abs().max()))),
            "dq_abs": excess(up(dq).reshape(B, H, dh), ref["dq"], bf16_tol(ref["dq"], m * float(up(K).abs().max())))}

# ---- the checks, shared by the host emulation and the GPU tests: worst |error| / bound per output (<= 1 passes) ------------------
def check_dw_fwd(ref: dict, d, sq) -> dict:
    return {"d": excess(d, ref["d"], bf16_tol(ref["d"], ref["d_A"])), "sq": excess(sq, ref["sq"], ref["sq_tol"])}


def check_dw_bwd(ref: dict, g: Optional[torch.Tensor], da, dw, db) -> dict:
    """g: the fp64 factor the stream holds (the bf16 values, or q8_unpack of the bytes), None without a stream.  The decode of a byte
    is one fma on |q| / 202 + 26 / 202 <= 1.4: 2 EPS 1.4 |da| on top of the product's own rounding."""
    g = torch.ones_like(ref["da"]) if g is None else g
    want = ref["da"] * g
    A = g.abs() * ref["e_da"] + 2 * EPS * want.abs() + 2.8 * EPS * ref["da"].abs()
    return {"da": excess(da, want, bf16_tol(want, A)), "dw": excess(up(dw).reshape(-1, 9), ref["dw"], ref["dw_tol"]),
            "db": excess(db, ref["db"], ref["db_tol"])}


def check_se_fwd(ref: dict, s, hid) -> dict:
    return {"s": excess(s, ref["s"], EXP_REL * ref["s"]), "hid": excess(hid, ref["hid"], EXP_REL * ref["hid"])}


def check_se_bwd(ref: dict, dmean, dwr, dbr, dwe, dbe) -> dict:
    got = {"dmean": dmean, "dwr": dwr, "dbr": dbr, "dwe": dwe, "dbe": dbe}
    return {k: excess(up(v).reshape(ref[k].shape), ref[k], ref[k + "_tol"]) for k, v in got.items()}


def check_ca_fwd(ref: dict, o, lse) -> dict:
    return {"o": excess(o, ref["o"], bf16_tol(ref["o"], ref["o_A"])), "lse": excess(up(lse).reshape(ref["lse"].shape), ref["lse"], ref["lse_tol"])}


def check_ca_bwd(ref: dict, dq, dk, dv) -> dict:
    """dq [B, H dh], dk / dv per key [B, H, Nk, dh].  Rows against ROW_REL; dv = P_j dout is one product of a value through __expf:
    per element one bf16 ulp plus EXP_REL."""
    B, H, Nk, dh = ref["dk"].shape
    return {"dq": float(row_err(up(dq).reshape(B, H, 1, dh), ref["dq"][:, :, None]).max()) / ROW_REL,
            "dk": float(row_err(dk, ref["dk"]).max()) / ROW_REL, "dv": float(row_err(dv, ref["dv"]).max()) / ROW_REL,
            "dv_elem": excess(dv, ref["dv"], bf16_tol(ref["dv"], (EXP_REL + 2 * EPS) * ref["dv"].abs()))}


# ---- the outputs that are one fp32 product: the same product in torch fp32, rounded to bf16, bit for bit ------------------------
def se_apply_bits(d, s, HW: int) -> torch.Tensor:
    return (d.float() * s.float().repeat_interleave(HW, 0)).to(torch.bfloat16)


def dgelu_bits(dx, g16) -> torch.Tensor:
    return (dx.float() * g16.float()).to(torch.bfloat16)


def ls_dz_bits(dy, gamma, keep=None, survival: float = 1.0, rps: int = 1) -> torch.Tensor:
    """bf16((dy f) gamma), f = keep (1 / survival), each step one IEEE fp32 operation as in the kernel."""
    v = dy.float()
    if keep is not None:
        inv = torch.ones((), dtype=torch.float32, device=dy.device) / torch.tensor(survival, dtype=torch.float32, device=dy.device)
        v = v * (keep.float() * inv).repeat_interleave(rps)[:, None]
    return (v * gamma.float()).to(torch.bfloat16)
