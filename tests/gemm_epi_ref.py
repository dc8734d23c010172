"""Exact-accumulator operands, fp64 definitions, an fp32 restatement and counted bounds for the NT / TN GEMM epilogues
(csrc/nrv_gemm.hip: epilogue_lin, epilogue_remap, the split-K reduction; csrc/nrv_common.hpp: gelu_both4, gelu_both, pack_bf16x2).
Host and device (torch, any device); tests/test_gemm_epi_ref_host.py proves the bounds on the restatement and shows that each
of MISTAKES fails on its named case; tests/test_gemm_epi_edges_gpu.py judges the kernels with the same `judge_nt` / `tn_ref`.

The exact-accumulator argument.  A product of two bf16 numbers has 16 significant bits and is exact in fp32 (so it is inside the
MFMA).  With small-integer operands every partial sum of a dot product is an integer; while it stays below 2^24 it is exact in
fp32 in ANY summation order, the MFMA-internal one, the order of the K-steps and of split-K slabs included.  The accumulator a
workgroup hands to its epilogue is then a known integer, and every linear epilogue is ONE IEEE fp32 operation per step on exact
inputs, followed by one round-to-nearest-even to bf16 -- all of it reproducible bit for bit:
    NONE            c = acc
    BIAS            c = fl(acc + bias)
    BIAS_RESIDUAL   c = fl(fl(acc + bias) + aux)            (aux fp32, or bf16 widened exactly)
    DGELU           c = fl(acc aux)                          (aux bf16: integer x bf16 has at most 16 bits, exact)
    DGELU_Q8        c = fl(acc fma(q, 1/202, -26/202))       (the fma rounds once, the product once)
    TN              C = beta C0 + sum_t dY[t, m] X[t, n],  dbias = dbias_beta dbias0 + sum_t dY[t, m]      (integers)
The order was read from the code: epilogue_lin does `x = val; x += bias4; [gelu]; x += a | x *= a; pack_bf16x2`, epilogue_remap
does `x = val + bias4; [gelu]; x += aux | x *= aux; pack_bf16x2` -- the same order, (acc + bias) first, then the operand.
pack_bf16x2 is the compiler's fp32 -> bf16 cast (v_cvt_pk_bf16_f32): round to nearest, ties to even, once.

Only the GELU epilogues need a bound, and with u = acc + bias exact (operands below) the bound speaks about the GELU function
alone.  U = 2^-24 is the unit round-off of fp32: one rounding costs at most U |x|; v_rcp_f32 and v_exp_f32 are good to one ulp,
2 U relative.  Hats are the fp64 values.  gelu_both (gelu_parts) and gelu_both4 fold their constants differently; every count
below is the larger of the two, and where hipcc may or may not contract a multiply-add the uncontracted count.
    t      = rcp(1 + p |u| / sqrt 2)    |u| c: constant and product (2), scaled by p x / d <= 1, the constant p (1), the fma (1),
                                        the reciprocal (2):   rel_t = U (3 + 3 p x / d)
                                        (gelu_both4 folds p / sqrt 2 into one constant: 3 roundings in it, the same count)
    e      = exp2(-u^2 log2(e) / 2)     gelu_both4: w = fl(u k) (2), w^2 (1 + 2 x 2 = 5 on the argument); gelu_parts: fl(fl(u u) k) (3)
                                        d exp2(a) = ln 2 exp2(a) da and |a| ln 2 = u^2 / 2:   rel_e = U (5 u^2 / 2 + 2)
    P(t)   = t (a1 + t (a2 + ... t a5)) running error of the Horner chain, per stage s' = fl(s t + a):
                                        err' = err t + U (|s| t + |s'| + |a|)   (product, sum, the rounded constant), from U |a5|;
                                        the last product: errP = err t + U |P|;  the error of t enters through t P'(t) rel_t
    h      = e P / 2 = erfc(|u|/sqrt 2)/2   dh = e / 2 (errP + |t P'(t)| rel_t) + h (rel_e + U) + 1.5e-7 / 2
                                        (the product with e, the Abramowitz-Stegun 7.1.26 error of erf halved; 0.5 is exact)
    Phi    = 1 - h | h  (gelu_parts),  1/2 + copysign(fma(e, q, -1/2), u)  (gelu_both4: the fma's result is <= 1/2)
                                        dPhi = dh + U / 2 + U Phi
    phi    = fl(e c)                    dphi = phi (rel_e + 2 U)
    g      = fl(u Phi)                  delta_g  = |u| dPhi + U |g|
    g'     = fma(u, phi, Phi)           delta_dg = |u| dphi + dPhi + U |g'| + U |u phi|
For u <= -4 the bound of g is absolute (|u| (0.75e-7 + U / 2)) although g itself is 1e-4 and smaller: gelu_both4 computes Phi
there as 1/2 - (1/2 - h) and loses h's relative accuracy; that is the kernel's arithmetic, and the 1.5e-7 of the erf formula is
absolute anyway.  All terms are first order in U; nothing is tuned.  The checks (judge_nt):
    fp32 out        |h - gelu64(u)| <= delta_g(u)
    bf16 out        rne(ref - delta_g(u)) <= h <= rne(ref + delta_g(u)), rne = nearest-even to bf16 of the fp32 neighbour inside:
    gelu' bf16      the same with delta_dg(u).  Rounding is monotone, so this is exactly the set of bf16 numbers a kernel whose
                    fp32 value lies within delta of the reference can store -- the tightest check there is, with no rounding
                    allowance to choose.  The figure printed for these two is |h - ref| / (2^-9 |ref| (1 + 2^-8) + delta), the
                    form this check was first proposed in: bf16 keeps 8 significant bits, so nearest-even itself reaches
                    2^-8 |ref| (1.0039 rounds to 1 or 1.0078) and the figure goes up to 2 for a correct kernel (1.97 .. 1.98
                    on the restatement); it is reported, not asserted.
    gelu' byte      |q - (202 gelu'64(u) + 26)| <= 0.5 + 202 delta_dg(u) + 256 U      (the fma's rounding: |y| < 256)
                    0.5 admits either direction on an exact tie of the byte conversion
    DGELU_Q8        bit for bit, as above.

Operands (all deterministic, torch.Generator on the CPU, seeded from the record's name):
    dense_exact     A in {-1, 0, 1} with P(nonzero) = 1/2, B integers in [-2, 2], bias integers in [-16, 16], aux integers in
                    [-32, 32] (fp32 and bf16 form), a random bf16 aux for DGELU, random bytes for DGELU_Q8.
                    Condition (host test, every record): max |acc| <= 128 and max |acc + bias + aux| <= 256: every result an
                    integer that bf16 holds exactly.
    fractional_aux  dense_exact with an fp32 aux of multiples of 2^-12: (acc + bias) + aux is exact in fp32 and not a bf16
                    number.  The last min(16, width) columns of every column tile are the tie band: the sum is +-2^b (1 + (2 j + 1)
                    / 256), exactly half way between two bf16 neighbours; j is even in the first half of every 8-column chunk of the band
                    (the even neighbour is the one nearer zero: nearest-even and truncation agree, round-half-up differs) and odd
                    in the second half (nearest-even and round-half-up agree, truncation differs).  The ragged column tile's last
                    8-column chunk lies in the band.
    gelu_ladder     one-hot A (row m has its 1 at m % K), B[n, k] from LADDER, so acc[m, n] = B[n, m % K] exactly; with
                    bias = 0, or bias multiples of 2^-10 in [-0.5, 0.5): u = acc + bias is exact in fp32 and known.
    gelu_dense      A +-1 with P = 1/8, B +-1 with P = 1/4, the fractional bias: every u depends on the whole K loop.
                    Condition (host test, every record): at least 90 % of the elements at |u| <= 6.5.
    tn_dense        dY in {-1, 0, 1}, X integers in [-2, 2], integer start values of C and dbias.
"""
from __future__ import annotations

import math
import zlib

import torch

F32, BF16 = torch.float32, torch.bfloat16
U = 2.0 ** -24

# epilogue ids of include/nrv.h (the tests assert them against noise_robust_vit_amd._lib)
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESIDUAL, EPI_DGELU, EPI_BIAS_GELU_Q8, EPI_DGELU_Q8 = range(7)
Q8_SCALE, Q8_ZERO = 202.0, 26.0

AS_P = 0.3275911
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)      # a1 .. a5
AS_ERR = 1.5e-7


def _gen(*key) -> torch.Generator:
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(repr(key).encode()))


def _ints(shape, lo, hi, *key) -> torch.Tensor:
    """uniform integers in [lo, hi] as fp32"""
    return torch.randint(lo, hi + 1, shape, generator=_gen(*key)).to(F32)


def _signs(shape, one_in, *key) -> torch.Tensor:
    """+1 and -1 with probability 1 / one_in each, zero otherwise"""
    r = torch.randint(0, one_in, shape, generator=_gen(*key))
    return (r == 0).to(F32) - (r == 1).to(F32)


def ratio(err, bound) -> float:
    """max |err| / bound (0 / 0 counts as 0; a NaN counts as inf)"""
    if bool(err.isnan().any()):
        return float("inf")
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


# ----------------------------------------------------------------------------------------------
# fp64 definitions
# ----------------------------------------------------------------------------------------------
def Phi64(u):
    return 0.5 * torch.special.erfc(-u.double() / math.sqrt(2.0))          # erfc: relative accuracy in the negative tail


def phi64(u):
    u = u.double()
    return torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def gelu64(u):
    return u.double() * Phi64(u)


def dgelu64(u):
    return Phi64(u) + u.double() * phi64(u)


def remap_row(m, group, stride, offset):
    """out_group / a_group: row m of the product lives at row (m // group) stride + m % group + offset"""
    if group <= 0:
        return m
    return m // group * stride + m % group + offset


def q8_offset(m, n, ld):
    """byte (m, n) of the 8-bit gelu' stream (include/nrv.h): row pairs, 64-column blocks, the two rows of a block adjacent"""
    return (m >> 1) * 2 * ld + (n >> 6) * 128 + (m & 1) * 64 + (n & 63)


def q8_store(q, ld):
    """[M, N] bytes -> the flat storage of (M rounded up to even) x ld bytes, 255 where nothing is stored"""
    M, N = q.shape
    ME = (M + 1) // 2 * 2
    flat = torch.full((ME * ld,), 255, dtype=torch.uint8, device=q.device)
    m = torch.arange(M, device=q.device)[:, None]
    n = torch.arange(N, device=q.device)[None, :]
    flat[q8_offset(m, n, ld).reshape(-1)] = q.reshape(-1)
    return flat


def q8_load(flat, M, N, ld):
    m = torch.arange(M, device=flat.device)[:, None]
    n = torch.arange(N, device=flat.device)[None, :]
    return flat[q8_offset(m, n, ld).reshape(-1)].reshape(M, N)


def nt_ref64(acc, epi, bias=None, aux=None):
    """fp64 definition of every NT epilogue: (C, gelu' | None).  `aux`: the operand in the rows of C (after any broadcast or
    remap), bytes for DGELU_Q8."""
    acc = acc.double()
    if epi == EPI_NONE:
        return acc, None
    if epi == EPI_BIAS:
        return acc + bias.double(), None
    if epi in (EPI_BIAS_GELU, EPI_BIAS_GELU_Q8):
        u = acc + bias.double()
        return gelu64(u), dgelu64(u)
    if epi == EPI_BIAS_RESIDUAL:
        return acc + (0.0 if bias is None else bias.double()) + aux.double(), None
    if epi == EPI_DGELU:
        return acc * aux.double(), None
    if epi == EPI_DGELU_Q8:
        return acc * (aux.double() - Q8_ZERO) / Q8_SCALE, None
    raise ValueError(epi)


def q8_ref64(u):
    """the real number the byte stands for"""
    return Q8_SCALE * dgelu64(u) + Q8_ZERO


def tn_ref(dY, X, c0=None, db0=None, beta=0.0, dbias_beta=0.0, a_group=0, T=None):
    """fp64: (beta C0 + dY[rows]^T X, dbias_beta dbias0 + colsum(dY[rows])); rows = the a_group remap of the tokens 0 .. T-1"""
    T = X.shape[0] if T is None else T
    rows = tn_rows(T, a_group, X.device)
    a = dY[rows].double()
    c = a.t() @ X[:T].double()
    db = a.sum(0)
    if beta:
        c = c + beta * c0.double()
    if dbias_beta:
        db = db + dbias_beta * db0.double()
    return c, db


def tn_rows(T, a_group, device="cpu"):
    """the row of dY token t reads: the class-token remap (stride a_group + 1, offset 1) of tests/gemm_paths.py, or t itself"""
    t = torch.arange(T, device=device)
    return remap_row(t, a_group, a_group + 1, 1)


# ----------------------------------------------------------------------------------------------
# counted bounds of the GELU epilogues (module docstring)
# ----------------------------------------------------------------------------------------------
def gelu_bounds(u):
    """(gelu64, gelu'64, delta_g, delta_dg) per element of the exact u"""
    u = u.double()
    au = u.abs()
    x = au / math.sqrt(2.0)
    d = 1.0 + AS_P * x
    t = 1.0 / d
    e = torch.exp(-0.5 * u * u)
    a1, a2, a3, a4, a5 = AS_A
    s = torch.full_like(u, a5)
    err = torch.full_like(u, U * abs(a5))
    for a in (a4, a3, a2, a1):
        s2 = s * t + a
        err = err * t + U * (s.abs() * t + s2.abs() + abs(a))
        s = s2
    P = s * t
    errP = err * t + U * P.abs()
    tdP = t * (a1 + t * (2 * a2 + t * (3 * a3 + t * (4 * a4 + t * 5 * a5))))
    rel_t = U * (3.0 + 3.0 * AS_P * x / d)
    rel_e = U * (2.5 * u * u + 2.0)
    h = 0.5 * torch.special.erfc(x)
    dh = 0.5 * e * (errP + tdP.abs() * rel_t) + h * (rel_e + U) + 0.5 * AS_ERR
    Phi, phi = Phi64(u), phi64(u)
    dPhi = dh + 0.5 * U + U * Phi
    dphi = phi * (rel_e + 2.0 * U)
    g, dg = u * Phi, Phi + u * phi
    delta_g = au * dPhi + U * g.abs()
    delta_dg = au * dphi + dPhi + U * dg.abs() + U * (u * phi).abs()
    return g, dg, delta_g, delta_dg


def bf16_bound(ref, delta):
    """the reported figure's denominator (module docstring); not asserted"""
    return 2.0 ** -9 * ref.abs() * (1.0 + 2.0 ** -8) + delta


def _f32_inside(x, up):
    """the fp32 neighbour of the fp64 x at or above it (up) / at or below it"""
    y = x.to(F32)
    inf = torch.full_like(y, float("inf") if up else float("-inf"))
    wrong = (y.double() < x) if up else (y.double() > x)
    return torch.where(wrong, torch.nextafter(y, inf), y)


def bf16_outside(got, ref, delta):
    """bool: the bf16 number `got` is not the nearest-even rounding of any fp32 number within delta of ref"""
    lo = _f32_inside(ref - delta, True).to(BF16).double()
    hi = _f32_inside(ref + delta, False).to(BF16).double()
    g = got.double()
    return ~((g >= lo) & (g <= hi))


def q8_bound(delta_dg):
    return 0.5 + Q8_SCALE * delta_dg + 256.0 * U


# ----------------------------------------------------------------------------------------------
# the fp32 restatement, one function per device helper
# ----------------------------------------------------------------------------------------------
def _f(x):
    return float(torch.tensor(x, dtype=F32))


def _fma(a, b, c):
    """fmaf: products of fp32 numbers are exact in double; one rounding to fp32 (the double sum is exact or far from a tie)"""
    a = a.double() if torch.is_tensor(a) else float(a)
    b = b.double() if torch.is_tensor(b) else float(b)
    c = c.double() if torch.is_tensor(c) else float(c)
    return (a * b + c).to(F32)


def _mul(a, b):
    return _fma(a, b, 0.0)


def _rcp(x):
    return (1.0 / x.double()).to(F32)                      # the correctly rounded one; v_rcp_f32 is within one ulp of it


def _exp2(x):
    return torch.exp2(x.double()).to(F32)


MISTAKES = ("tanh_gelu", "bias_after_gelu", "dgelu_without_u_phi", "dgelu_from_acc_without_bias", "bf16_truncate",
            "bf16_round_half_up", "residual_rounded_to_bf16", "bias_rounded_to_bf16", "dgelu_q8_rounded_twice", "q8_zero_25.5",
            "q8_scale_200", "q8_decode_200", "k_dropped_off_diagonal")
TN_MISTAKES = ("beta_per_slab", "dbias_beta_ignored", "token_tail_dropped")


def pack_bf16x2(x, mistake=None):
    """pack_bf16x2: fp32 -> bf16, round to nearest, ties to even (torch's cast is the same rounding)"""
    x = x.to(F32)
    if mistake in ("bf16_truncate", "bf16_round_half_up"):
        bits = x.contiguous().view(torch.int32)
        if mistake == "bf16_round_half_up":
            bits = bits + 0x8000                           # half an ulp of the magnitude, then cut
        return (bits & -65536).view(F32).to(BF16)
    return x.to(BF16)


def gelu_both(u, mistake=None):
    """gelu_parts + gelu_both (the scalar form: epilogue_remap's, nrv_rvt.hip's): (g, g') in fp32"""
    u = u.to(F32)
    x = _mul(u.abs(), _f(0.70710678118654752))
    t = _rcp(_fma(x, _f(AS_P), 1.0))
    e = _exp2(_mul(_mul(u, u), _f(-0.72134752044448170)))
    a1, a2, a3, a4, a5 = (_f(a) for a in AS_A)
    p = _fma(t, a5, a4)
    p = _fma(p, t, a3)
    p = _fma(p, t, a2)
    p = _fma(p, t, a1)
    half = _mul(_mul(_mul(p, t), e), 0.5)
    Phi = torch.where(u >= 0, (1.0 - half.double()).to(F32), half)
    phi = _mul(e, _f(0.39894228040143268))
    return _finish(u, Phi, phi, mistake, True)


def gelu_both4(u, mistake=None, contract=True):
    """gelu_both4 (the packed form of epilogue_lin): 0.5 folded into the polynomial, p / sqrt 2 into one constant, the sign select
    into a copysign.  `contract`: hipcc fuses each `a * b + c` of the vector code into an fma (its default), or rounds twice."""
    u = u.to(F32)
    mad = _fma if contract else (lambda a, b, c: (_mul(a, b).double() + (c.double() if torch.is_tensor(c) else c)).to(F32))
    w = _mul(u, _f(0.84932180028801904))
    w2 = _mul(w, w)
    c = _f(_f(AS_P) * _f(0.70710678118654752))
    t = _rcp(_fma(u.abs(), c, 1.0))
    e = _exp2(-w2)
    a1, a2, a3, a4, a5 = (0.5 * _f(a) for a in AS_A)
    q = mad(t, a5, a4)
    q = mad(q, t, a3)
    q = mad(q, t, a2)
    q = mad(q, t, a1)
    q = _mul(q, t)
    z = mad(e, q, -0.5)
    Phi = (0.5 + torch.copysign(z, u).double()).to(F32)
    phi = _mul(e, _f(0.39894228040143268))
    return _finish(u, Phi, phi, mistake, contract)


def _finish(u, Phi, phi, mistake, contract):
    if mistake == "tanh_gelu":
        ud = u.double()
        k = math.sqrt(2.0 / math.pi)
        th = torch.tanh(k * (ud + 0.044715 * ud ** 3))
        g = 0.5 * ud * (1.0 + th)
        dg = 0.5 * (1.0 + th) + 0.5 * ud * (1.0 - th * th) * k * (1.0 + 3 * 0.044715 * ud * ud)
        return g.to(F32), dg.to(F32)
    g = _mul(u, Phi)
    if mistake == "dgelu_without_u_phi":
        return g, Phi
    dg = _fma(u, phi, Phi) if contract else (_mul(u, phi).double() + Phi.double()).to(F32)
    return g, dg


def q8_pack4(dg, mistake=None):
    """q8_pack4: fma(g', 202, 26), then v_cvt_pk_u8_f32: nearest (ties to even here), saturating"""
    scale = 200.0 if mistake == "q8_scale_200" else Q8_SCALE
    zero = 25.5 if mistake == "q8_zero_25.5" else Q8_ZERO
    y = _fma(dg, scale, zero)
    return torch.round(y).clamp(0, 255).to(torch.uint8)


def q8_unpack4(q, mistake=None):
    """q8_unpack4: fma(q, 1/202, -26/202), both constants rounded to fp32 first"""
    scale = 200.0 if mistake == "q8_decode_200" else Q8_SCALE
    return _fma(q.to(F32), _f(1.0 / scale), _f(-Q8_ZERO / scale))


def epilogue(acc, epi, out_dtype, bias=None, aux=None, mistake=None, scalar_gelu=False):
    """epilogue_lin / epilogue_remap on the fp32 accumulator: (C of out_dtype, gelu' stream | None: bf16, or bytes for the _Q8 id).
    `aux` in the rows of C.  Order: (acc + bias), the GELU, then + aux or * aux, then pack_bf16x2 (module docstring).
    `scalar_gelu`: epilogue_remap's per-element gelu_both instead of epilogue_lin's gelu_both4 (the library refuses that launch)."""
    x = acc.to(F32)
    stream = None
    b = bias
    if b is not None and mistake == "bias_rounded_to_bf16":
        b = b.to(BF16).to(F32)
    if epi in (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_Q8, EPI_BIAS_RESIDUAL) and b is not None:
        u = x + b
    else:
        u = x
    if epi in (EPI_BIAS_GELU, EPI_BIAS_GELU_Q8):
        both = gelu_both if scalar_gelu else gelu_both4
        g, dg = both(u, mistake)
        if mistake == "bias_after_gelu":
            g = both(x, mistake)[0] + b
        if mistake == "dgelu_from_acc_without_bias":
            dg = both(x, mistake)[1]
        u = g
        stream = q8_pack4(dg, mistake) if epi == EPI_BIAS_GELU_Q8 else pack_bf16x2(dg, mistake)
    if epi == EPI_BIAS_RESIDUAL:
        a = aux.to(F32)
        if mistake == "residual_rounded_to_bf16":
            a = a.to(BF16).to(F32)
        u = u + a
    elif epi == EPI_DGELU:
        u = u * aux.to(F32)
    elif epi == EPI_DGELU_Q8:
        a = q8_unpack4(aux, mistake)
        if mistake == "dgelu_q8_rounded_twice":
            a = a.to(BF16).to(F32)
        u = u * a
    return (u if out_dtype == F32 else pack_bf16x2(u, mistake)), stream


def accumulate(A, B, mistake=None, k_drop=5):
    """the exact accumulator in fp32 (integers below 2^24: any order).  `k_dropped_off_diagonal`: column k_drop of the K loop is
    skipped for every row m with m % K != k_drop -- the rows whose one-hot operand of the placement test holds a zero there."""
    a = A.to(F32)
    if mistake == "k_dropped_off_diagonal":
        Kd = a.shape[1]
        a = a.clone()
        m = torch.arange(a.shape[0], device=a.device)
        a[m % Kd != k_drop, k_drop] = 0.0
    return a @ B.to(F32).t()


def tn_restated(dY, X, c0, db0, beta, dbias_beta, splits=1, kt_q=None, kt_r=0, a_group=0, T=None, mistake=None):
    """the TN kernels and their reduction in fp32: split s sums its K-tiles of 64 tokens into a slab (the first kt_r splits one
    tile more), the reduction adds the slabs to beta C0 once.  (C, dbias) in fp32."""
    T = X.shape[0] if T is None else T
    rows = tn_rows(T, a_group, X.device)
    a = dY[rows].to(F32)
    M = a.shape[1]
    if mistake == "token_tail_dropped":
        a = a.clone()
        a[M:] = 0.0
    x = X[:T].to(F32)
    kt = -(-T // 64)
    kt_q = kt // splits if kt_q is None else kt_q
    assert kt_q * splits + kt_r == kt
    c = torch.zeros(M, x.shape[1], dtype=F32, device=x.device)
    db = torch.zeros(M, dtype=F32, device=x.device)
    if mistake != "beta_per_slab" and beta:
        c = c + beta * c0.to(F32)
    if dbias_beta and mistake != "dbias_beta_ignored":
        db = db + dbias_beta * db0.to(F32)
    t0 = 0
    for s in range(splits):
        t1 = min(T, t0 + 64 * (kt_q + (1 if s < kt_r else 0)))
        slab = a[t0:t1].t() @ x[t0:t1]
        if mistake == "beta_per_slab" and beta:
            slab = slab + beta * c0.to(F32)
        c = c + slab
        db = db + a[t0:t1].sum(0)
        t0 = t1
    return c, db


# ----------------------------------------------------------------------------------------------
# operands
# ----------------------------------------------------------------------------------------------
def _ladder():
    vals = [0.0]
    for s in (1.0, -1.0):
        vals += [s * 2.0 ** -20, s * 2.0 ** -7]
        for b in range(-6, 3):                               # the binades [2^-6, 2^-5) ... [4, 8)
            vals += [s * 2.0 ** b * (1.0 + m / 128.0) for m in (0, 17, 34, 51, 68, 85, 102, 127)]
        vals += [s * 6.0, s * 8.0, s * 10.0]
    t = torch.tensor(vals, dtype=F32)
    assert torch.equal(t.to(BF16).to(F32), t) and len(set(vals)) == len(vals)
    return t


LADDER = _ladder()            # 155 bf16 values


def fractional_bias(N, *key):
    """multiples of 2^-10 in [-0.5, 0.5)"""
    return _ints((N,), -512, 511, "fbias", *key) * 2.0 ** -10


def one_hot_A(M, Kd):
    A = torch.zeros(M, Kd, dtype=BF16)
    A[torch.arange(M), torch.arange(M) % Kd] = 1.0
    return A


def dense_exact(rec):
    """dict: A, B (bf16), bias (fp32), aux32 / aux16 (the integer residual), auxg (bf16, random: the DGELU operand), auxq
    (bytes: the DGELU_Q8 operand), acc (fp32, exact)"""
    M, N, Kd = rec.M, rec.N, rec.K
    r = torch.randint(0, 4, (M, Kd), generator=_gen("A", rec.name))
    A = ((r == 2).to(F32) - (r == 3).to(F32)).to(BF16)
    B = _ints((N, Kd), -2, 2, "B", rec.name).to(BF16)
    aux = _ints((M, N), -32, 32, "aux", rec.name)
    auxg = (torch.randn(M, N, generator=_gen("auxg", rec.name)) * 0.5).to(BF16)
    auxq = torch.randint(0, 255, (M, N), generator=_gen("auxq", rec.name)).to(torch.uint8)
    return dict(A=A, B=B, bias=_ints((N,), -16, 16, "bias", rec.name), aux32=aux, aux16=aux.to(BF16), auxg=auxg, auxq=auxq,
                acc=accumulate(A, B))


def tie_band(rec):
    """(band, odd): bool [N]; the last min(16, width) columns of every column tile, and the second half of each 8-column chunk
    (one lane's 16-byte store of bf16) of the band"""
    band = torch.zeros(rec.N, dtype=torch.bool)
    odd = torch.zeros(rec.N, dtype=torch.bool)
    for n0 in range(0, rec.N, rec.tile_n):
        n1 = min(rec.N, n0 + rec.tile_n)
        w = min(16, n1 - n0)
        band[n1 - w:n1] = True
    odd = band & (torch.arange(rec.N) % 8 >= 4)
    return band, odd


def fractional_aux(rec, ops=None):
    """dense_exact's dict with aux32 replaced (module docstring) and band / odd (bool [N]) added"""
    ops = dict(dense_exact(rec) if ops is None else ops)
    M, N = rec.M, rec.N
    s = ops["acc"] + ops["bias"]
    aux = _ints((M, N), -32 * 4096, 32 * 4096, "faux", rec.name) * 2.0 ** -12
    band, odd = tie_band(rec)
    g = _gen("ties", rec.name)
    j = torch.randint(0, 64, (M, N), generator=g) * 2 + odd.to(torch.int64)[None, :]
    b = torch.randint(-1, 3, (M, N), generator=g).to(F32)
    sign = torch.randint(0, 2, (M, N), generator=g).to(F32) * 2 - 1
    tie = sign * torch.exp2(b) * (1.0 + (2 * j + 1).to(F32) / 256.0)
    aux[:, band] = (tie - s)[:, band]
    ops.update(aux32=aux, band=band, odd=odd)
    del ops["aux16"]
    return ops


def gelu_ladder(rec, with_bias):
    M, N, Kd = rec.M, rec.N, rec.K
    A = one_hot_A(M, Kd)
    idx = (37 * torch.arange(N)[:, None] + 11 * torch.arange(Kd)[None, :]) % len(LADDER)
    B = LADDER[idx].to(BF16)
    bias = fractional_bias(N, rec.name) if with_bias else torch.zeros(N)
    return dict(A=A, B=B, bias=bias, acc=B.to(F32)[:, torch.arange(M) % Kd].t().contiguous())


def gelu_dense(rec):
    M, N, Kd = rec.M, rec.N, rec.K
    A = _signs((M, Kd), 16, "gA", rec.name).to(BF16)           # +-1 with P = 1/8 together
    B = _signs((N, Kd), 8, "gB", rec.name).to(BF16)            # +-1 with P = 1/4 together
    return dict(A=A, B=B, bias=fractional_bias(N, rec.name), acc=accumulate(A, B))


def tn_dense(M, N, T, a_group, *key):
    """dict: dY [rows dY needs, M] and X [T, N] (bf16), c0 [M, N] and db0 [M] (fp32 integers).  The rows a remap skips hold
    values too: they must not be read."""
    arows = T if a_group == 0 else T // a_group * (a_group + 1)
    r = torch.randint(0, 4, (arows, M), generator=_gen("dY", *key))
    dY = ((r == 2).to(F32) - (r == 3).to(F32)).to(BF16)
    return dict(dY=dY, X=_ints((T, N), -2, 2, "X", *key).to(BF16), c0=_ints((M, N), -64, 64, "c0", *key),
                db0=_ints((M,), -64, 64, "db0", *key))


# ----------------------------------------------------------------------------------------------
# the judge the host test (on the restatement and its mistakes) and the GPU test (on the kernels) share
# ----------------------------------------------------------------------------------------------
def judge_nt(ops, epi, out_dtype, aux, out, stream):
    """{check name: (bad: bool [M, N], worst error / bound | None)} of one launch's C and gelu' stream (bf16 or byte ROWS [M, N]).
    Linear epilogues: bit for bit against `epilogue`; with `band` in ops the ties are judged by name.  GELU: the counted bounds
    (bf16: the interval of the module docstring; the figure beside it is the reported one)."""
    acc, bias = ops["acc"], ops["bias"]
    res = {}
    if epi in (EPI_BIAS_GELU, EPI_BIAS_GELU_Q8):
        u = acc.double() + bias.double()
        g, dg, delta_g, delta_dg = gelu_bounds(u)
        err = (out.double() - g).abs()
        if out_dtype == F32:
            res["out"] = (~(err <= delta_g), ratio(err, delta_g))
        else:
            res["out"] = (bf16_outside(out, g, delta_g), ratio(err, bf16_bound(g, delta_g)))
        if stream is not None and epi == EPI_BIAS_GELU:
            res["stream"] = (bf16_outside(stream, dg, delta_dg), ratio((stream.double() - dg).abs(), bf16_bound(dg, delta_dg)))
        elif stream is not None:
            err, bound = (stream.double() - (Q8_SCALE * dg + Q8_ZERO)).abs(), q8_bound(delta_dg)
            res["stream"] = (~(err <= bound), ratio(err, bound))
        return res
    want, _ = epilogue(acc, epi, out_dtype, bias, aux)
    bad = (out != want) | out.isnan()
    if "band" in ops:
        band, odd = ops["band"].to(bad.device), ops["odd"].to(bad.device)
        res["off_band"] = (bad & ~band[None, :], None)
        res["ties_even_below"] = (bad & (band & ~odd)[None, :], None)
        res["ties_even_above"] = (bad & (band & odd)[None, :], None)
    else:
        res["out"] = (bad, None)
    return res


def failed(res):
    return sorted(k for k, (bad, _) in res.items() if bool(bad.any()))
