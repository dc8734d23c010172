"""LayerNorm, padded LayerNorm, batch norm and bf16 column sums at their lane, chunk, slab and dtype edges: case tables, input
builders, fp64 references, fp32 emulations of the kernels' summation order and a restatement of the dispatch rules (test infrastructure,
no kernels).  Used by tests/test_norm_ref_host.py (CPU) and tests/test_norm_edges_gpu.py.

The kernels: csrc/nrv_norm.hip (nrv_layernorm_fwd / _bwd, nrv_colsum_bf16), csrc/nrv_t2t.hip (nrv_layernorm_pad_*) and csrc/nrv_bn.hip.

Every comparison is per row (y, dx - dres, mean, rstd) or per column (dgamma, dbeta, the BN statistics, BN z and dy, the column sums)
against an fp64 evaluation of the definition on the inputs AS STORED (a bf16 input is its bf16 value).  The rows of a case are of nine
kinds and the columns of five (LN_ROW_KINDS, BN_COL_KINDS), so that a row or column the kernel gets wrong cannot hide behind the others.

Bounds.  u = 2^-24 (fp32 unit round-off), ub = 2^-8 (a bf16 store, as the issue sets it).  None of them is taken from a kernel's result.
  LayerNorm row, n_sum = additions on the longest path of a row sum (per lane, then the shuffle tree):
    mean    (n_sum + 2) u |x|max                          a sum of dim terms of at most |x|max, times 1 / dim
    x^      E = 2 (n_sum + 8) u K,  K = (|x|max + |mean|) rstd     x - mu inherits mu's error n_sum u |x|max and its own rounding
            u (|x| + |mu|); times rstd.  K >= |x^|max, so the relative error of rstd ((n_sum + 8) u, below) is inside the factor 2
    rstd    rstd [(n_sum + 8) u + (n_sum u K)^2]          the centred sum of squares is first-order blind to a shift of mu (sum d = 0):
            what remains is the rounding of the n_sum additions, the squares, the division and the root, and the shift squared
    y       |gamma|max E + 4 u |y|max + ub |y_j|      (the store term is the element's own, so every element is held to it)
    dx-dres rstd G (2 + X) [2 (n_sum + 8) u + E + (n_sum u K)^2] + store,   G = |dy gamma|max, X = max(1, |x^|max):
            dx = rstd (g - mean(g) - x^ mean(g x^)); each of the three terms is at most G X, mean(g x^) inherits G E from x^ and n_sum u G X
            from its sum, x^ itself E; store = ub |dx_j| for the bf16 output, 2 u |dx|max for the fp32 one (the addition of dres), and 0
            when G = 0: then the bracket is exactly 0 and 0 + dres is exact, so a zero-dy row must return dres bit for bit (fp32)
    dgamma  per column  sum_r |dy| (E_r + 4 u |x^|) + n_col u sum_r |dy x^| + 2 u (|preset| + |dgamma|);  dbeta the same without x^
            (n_col: additions on the longest path through the row slots, the workgroup sum and the partial-row reduction)
  Batch norm column, n_w = Welford steps of a row group + group merges + 8 (the chunk merge is fp64):
    mean    n_w u |y|max
    M2      2 n_w u (M2 + sqrt(T M2) (|y|max + |mean|))    each step's d (x - mean') carries the running mean's error n_w u |mean|
            times |d| + |d'|; summed, at most n_w u |mean| 2 sqrt(T M2) (Cauchy-Schwarz); plus the rounding of the sum itself
    invstd  invstd^3 bound(M2) / (2 T) + 4 u invstd       d invstd / d var = -invstd^3 / 2
    running momentum bound(value) + 4 u (|old| + |value|)
    x^      E = invstd bound(mean) + |y - mean|max bound(invstd) + 4 u K   (eval mode: 6 u K, the statistics are inputs)
    z       1.5 f |gamma| E + 6 u |z|max + ub |z_j| (bf16)       Hardswish is 1.5-Lipschitz; f = 1 / survival where keep is given
    dbeta   n_w u sum|dz'| + sum|dz f| H       dz' = dz hs'(z) f;  H = |gamma| E / 3 + 4 u: hs' has slope 1 / 3 between the kinks, and
            z / 3 + 1 / 2 is rounded absolutely (at most 2 u (|z| / 3 + 1 / 2) <= 4 u), not relative to a result that cancels near z = -3/2
    dgamma  n_w u sum|dz' x^| + sum|dz'| E + sum|dz f x^| H
    dy      |gamma invstd| (D H + bound(dbeta) / T + E |m2| + X bound(dgamma) / T + 6 u (D + |m1| + X |m2|))
            + bound(invstd) / invstd |dy|max + ub |dy_j|,  D = |dz'|max-ish (1.5 f |dz|max), m1 = mean(dz'), m2 = mean(dz' x^)
    Hardswish' jumps at +-3: elements whose fp64 z lies within 2^-9 of +-3 are left out of the dy comparison only (BN_KINK), at most 1 %
    of a case's elements and at most max(1, 2 %) of any column's rows (asserted on the CPU for every case).
  Column sum: n_c u sum|x| + 2 u (|beta out| + |result|), n_c = additions per lane + the 4-way sum + the partial reduction.
The fp32 emulations below follow the kernels' own order and stay within HALF of every bound on every case (test_norm_ref_host.py prints
and records the worst ratio per family), which leaves a factor of two for another order of the same sums.
"""
from __future__ import annotations

import os
import re
import zlib
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24
UB = 2.0 ** -8
F = np.float32

# ---------------------------------------------------------------------------------------------------------------------------------
# dispatch rules of csrc/nrv_norm.hip, restated (read_dispatch reads the same numbers back out of the source)
# ---------------------------------------------------------------------------------------------------------------------------------
LN_THREADS = 256
LN_WAVES = LN_THREADS // 64
LN_SPLIT = 512                                   # dim <= LN_SPLIT: half a wave per row
LN_STEPS = (1, 2, 3, 4, 5, 6, 8, 16)
LN_BWD_BLOCKS = 1024
COLSUM_ROWCHUNKS = 128
RR_LANES = 64
LNP_SLAB_ROWS, LNP_MAX_SLABS = 128, 128
BN_CHUNK, BN_GROUPS = 512, 4
BN_KINK = 2.0 ** -9


def ln_lpr(dim: int) -> int:
    return 32 if dim <= LN_SPLIT else 64


def ln_maxj(dim: int) -> int:
    lpr = ln_lpr(dim)
    chunks = (dim // 4 + lpr - 1) // lpr
    return next((s for s in LN_STEPS if chunks <= s), 16)


def ln_inst(dim: int):
    """(MAXJ, LPR) of the instantiation that runs `dim` (launch_ln_*: the half-wave form clamps MAXJ to 4)"""
    lpr = ln_lpr(dim)
    return (min(ln_maxj(dim), 4) if lpr == 32 else ln_maxj(dim)), lpr


def ln_reachable():
    """every (MAXJ, LPR) a legal dim (a multiple of 8 up to 4096) reaches"""
    return sorted({ln_inst(d) for d in range(8, 4097, 8)})


def read_dispatch(csrc: str) -> dict:
    """LN_THREADS, the half-wave split and the dispatched chunk counts as csrc/nrv_norm.hip states them"""
    with open(os.path.join(csrc, "nrv_norm.hip")) as f:
        text = f.read()
    threads = int(re.search(r"constexpr int LN_THREADS = (\d+);", text).group(1))
    split = int(re.search(r"int ln_lpr\(int dim\) \{ return dim <= (\d+) \? 32 : 64; \}", text).group(1))
    steps = tuple(int(v) for v in re.search(r"static const int steps\[8\] = \{([0-9, ]+)\};", text).group(1).split(","))
    cases = tuple(int(v) for v in re.findall(r"case (\d+): \{ constexpr int J = \1; CALL; \} break;", text))
    default = int(re.search(r"default: \{ constexpr int J = (\d+); CALL; \} break;", text).group(1))
    return {"threads": threads, "split": split, "steps": steps, "switch": cases + (default,)}


def lnp_slabs(rows: int) -> int:
    return max(1, min(LNP_MAX_SLABS, (rows + LNP_SLAB_ROWS - 1) // LNP_SLAB_ROWS))


def colsum_split(T: int):
    rpc = max(4, -(-T // COLSUM_ROWCHUNKS))
    return rpc, -(-T // rpc)


# ---------------------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------------------
# out: which dx the backward writes ("f32" | "bf16" | "both");  dres: 0 none, 1 fp32, 2 bf16;  acc: accumulate onto preset dgamma / dbeta
LnCase = namedtuple("LnCase", "dim rows xbf dres eps out acc")
PadCase = namedtuple("PadCase", "n ld rows xbf dres eps out acc")
# per: rows per sample of `keep` (0: no keep);  mom: momentum of the running update;  out / res: what bn_apply writes and adds
BnCase = namedtuple("BnCase", "T C dzbf act per training mom out res")
CsCase = namedtuple("CsCase", "T N ld beta")

# 264 and 1032 are not in the issue's list: without them MAXJ = 3 of the half-wave form and MAXJ = 5 of the 64-lane form never run
LN_DIMS_64 = (520, 776, 1032, 1288, 1536, 1544, 1800, 2048, 2056, 4088, 4096)
LN_DIMS_32 = (8, 64, 136, 264, 392, 504, 512)
LN_ROWS = 9
OUTS = ("f32", "bf16", "both")
LN_ROW_KINDS = ("plain", "mean 1e3 x spread", "constant", "spread 1e-4", "spread 1e3", "one element 1e4", "dy zero", "dy in one column", "plain")


def _ln_cases():
    out = []
    for di, dim in enumerate(LN_DIMS_32 + LN_DIMS_64):
        for xbf in (0, 1):
            for dres in (0, 1, 2):
                k = di + xbf
                out.append(LnCase(dim, LN_ROWS, xbf, dres, (1e-5, 1e-6)[(k + dres) % 2], OUTS[(k + 2 * dres) % 3], (di + dres + xbf) % 2))
    for dim in (136, 1800):
        out += [LnCase(dim, 1, 0, 1, 1e-6, "both", 0), LnCase(dim, 2, 1, 2, 1e-5, "bf16", 1)]
    return tuple(out)


LN_CASES = _ln_cases()
LN_GUARDED = LnCase(1800, 9, 0, 2, 1e-6, "both", 1)

PAD_SHAPES = ((1, 8), (9, 16), (64, 64), (65, 72), (147, 152), (147, 168), (1323, 1328), (4096, 4096))
PAD_ROWS = (1, 9, 127, 129)


def _pad_cases():
    out = []
    for si, (n, ld) in enumerate(PAD_SHAPES):
        for ri, rows in enumerate(PAD_ROWS):
            k = si * 4 + ri                                     # x dtype, dres and accumulate: each of the 12 combinations at least twice
            out.append(PadCase(n, ld, rows, k % 2, (k // 2) % 3, (1e-5, 1e-6)[(si + ri) % 2], OUTS[(si + 2 * ri) % 3], (k // 6 + si) % 2))
    return tuple(out)


PAD_CASES = _pad_cases()
BN_TS = (1, 2, 3, 5, 512, 513, 1000)
BN_CS = (4, 20, 64, 68, 132)
BN_PER = {1: 1, 2: 1, 3: 3, 5: 1, 512: 128, 513: 171, 1000: 250, 32769: 10923}
BN_COL_KINDS = ("plain", "mean 1e3 x spread", "constant", "one outlier row", "spread 1e-4")
BN_EPS = 1e-5
BN_SURVIVAL = 0.7


def _bn_cases():
    out = []
    for ti, T in enumerate(BN_TS):
        for ci, C in enumerate(BN_CS):
            k = ti * 5 + ci
            out.append(BnCase(T, C, k % 2, (k // 2) % 2, BN_PER[T] if (ti + 2 * ci) % 3 != 1 else 0, 0 if (ti + ci) % 4 == 3 else 1,
                              (0.1, 0.0, 1.0)[(ti + ci) % 3], OUTS[(2 * ti + ci) % 3], (ti + ci) % 2))
    out.append(BnCase(32769, 4, 1, 1, BN_PER[32769], 1, 0.1, "bf16", 0))
    return tuple(out)


BN_CASES = _bn_cases()
CS_SHAPES = ((1, 8, 8), (2, 64, 72), (5, 520, 520), (5, 520, 1032), (129, 1536, 1536), (513, 1016, 1024), (4097, 8, 16))
CS_CASES = tuple(CsCase(T, N, ld, beta) for (T, N, ld) in CS_SHAPES for beta in (0.0, 1.0, -0.5))
CS_COL_KINDS = ("plain", "all equal", "alternating +-large", "one nonzero row")

# "Reseed a case that does not meet it and list it": cases whose first draw broke the Hardswish-kink cap -> the draw that meets it
RESEEDED = {}


def case_id(c) -> str:
    return type(c).__name__[:-4].lower() + "-" + "-".join(f"{v:g}" if isinstance(v, float) else str(v) for v in c)


def _rng(c, salt=0):
    return np.random.default_rng(zlib.crc32(repr((tuple(c), RESEEDED.get(c, 0), salt)).encode()))


def bf16r(a):
    """round to bf16 (nearest even), returned as fp32"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F)).to(torch.bfloat16).to(torch.float32).numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs.  Everything is a float32 numpy array; what the kernel reads as bf16 holds bf16 values
# ---------------------------------------------------------------------------------------------------------------------------------
def _ln_rows(rng, rows, n, xbf):
    x = rng.standard_normal((rows, n))
    dy = rng.standard_normal((rows, n))
    for r in range(rows):
        kind = r % 9
        if kind == 1:
            x[r] += 1e2 if xbf else 1e3
        elif kind == 2:
            x[r] = 1.7
        elif kind == 3:
            x[r] *= 1e-4
        elif kind == 4:
            x[r] *= 1e3
        elif kind == 5:
            x[r, n // 3] = 1e4
        elif kind == 6:
            dy[r] = 0.0
        elif kind == 7:
            keep = dy[r, min(1, n - 1)]
            dy[r] = 0.0
            dy[r, min(1, n - 1)] = keep + 1.0
    return (bf16r(x) if xbf else x.astype(F)), bf16r(dy)


def _ln_params(rng, n):
    gamma = 1.0 + 0.5 * rng.standard_normal(n)
    gamma[0] = 0.0
    gamma[n - 1] = -1.3
    return gamma.astype(F), (0.5 * rng.standard_normal(n)).astype(F)


def ln_inputs(c) -> dict:
    """LnCase or PadCase -> x, dy, dres [rows, ld] (pad columns NaN), gamma, beta, dgamma0, dbeta0 [n]"""
    pad = isinstance(c, PadCase)
    n, ld = (c.n, c.ld) if pad else (c.dim, c.dim)
    rng = _rng(c)
    x, dy = _ln_rows(rng, c.rows, n, c.xbf)
    gamma, beta = _ln_params(rng, n)
    dres = rng.standard_normal((c.rows, n))
    dres = None if c.dres == 0 else (dres.astype(F) if c.dres == 1 else bf16r(dres))

    def wide(a):
        if a is None or ld == n:
            return a
        w = np.full((c.rows, ld), np.nan, dtype=F)
        w[:, :n] = a
        return w
    return {"x": wide(x), "dy": wide(dy), "dres": wide(dres), "gamma": gamma, "beta": beta, "n": n, "ld": ld,
            "dgamma0": rng.standard_normal(n).astype(F), "dbeta0": rng.standard_normal(n).astype(F)}


def bn_inputs(c: BnCase) -> dict:
    rng = _rng(c)
    T, C = c.T, c.C
    y = rng.standard_normal((T, C))
    for col in range(C):
        kind = col % 5
        if kind == 1:
            y[:, col] += 1e3
        elif kind == 2:
            y[:, col] = 0.6
        elif kind == 3 and T > 1:
            y[T // 2, col] = 1e4
        elif kind == 4:
            y[:, col] *= 1e-4
    gamma = 1.0 + 0.5 * rng.standard_normal(C)
    gamma[0], gamma[C - 1] = 0.0, -1.3
    beta = rng.standard_normal(C)
    dz = rng.standard_normal((T, C))
    keep = None
    if c.per:
        keep = (rng.random(T // c.per) < BN_SURVIVAL).astype(F)
        if keep.size > 1:
            keep[0], keep[-1] = 1.0, 0.0
    return {"y": y.astype(F), "gamma": gamma.astype(F), "beta": beta.astype(F), "dz": bf16r(dz) if c.dzbf else dz.astype(F), "keep": keep,
            "res": rng.standard_normal((T, C)).astype(F) if c.res else None,
            "run_mean": (0.1 * rng.standard_normal(C)).astype(F), "run_var": (0.5 + rng.random(C)).astype(F)}


def cs_inputs(c: CsCase) -> dict:
    """X is a [T, N] view of `back` [T + 8, ld], whose pad columns and tail rows hold NaN"""
    rng = _rng(CsCase(c.T, c.N, c.ld, 0.0))                    # the three betas of a shape share its data
    X = rng.standard_normal((c.T, c.N))
    for col in range(c.N):
        kind = col % 4
        if kind == 1:
            X[:, col] = 0.3
        elif kind == 2:
            X[:, col] = 256.0 * (1 - 2 * (np.arange(c.T) % 2)) + 0.01 * X[:, col]
        elif kind == 3:
            X[:, col] = 0.0
            X[c.T // 2, col] = 1.5
    back = np.full((c.T + 8, c.ld), np.nan, dtype=F)
    back[:c.T, :c.N] = bf16r(X)
    return {"back": back, "X": back[:c.T, :c.N], "out0": rng.standard_normal(c.N).astype(F)}


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 references: the definitions, written out
# ---------------------------------------------------------------------------------------------------------------------------------
def ln_ref(c, i) -> dict:
    n = i["n"]
    x, dy = i["x"][:, :n].astype(np.float64), i["dy"][:, :n].astype(np.float64)
    g, b = i["gamma"].astype(np.float64), i["beta"].astype(np.float64)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / np.sqrt(var + c.eps)
    xh = (x - mean[:, None]) * rstd[:, None]
    gg = dy * g
    c1, c2 = (gg * xh).mean(1), gg.mean(1)
    core = (gg - c2[:, None] - xh * c1[:, None]) * rstd[:, None]
    dres = 0.0 if i["dres"] is None else i["dres"][:, :n].astype(np.float64)
    dgamma, dbeta = (dy * xh).sum(0), dy.sum(0)
    if c.acc:
        dgamma, dbeta = dgamma + i["dgamma0"], dbeta + i["dbeta0"]
    return {"mean": mean, "rstd": rstd, "xh": xh, "y": xh * g + b, "core": core, "dx": core + dres, "dres": dres,
            "dgamma": dgamma, "dbeta": dbeta}


def hardswish(z):
    return z * np.clip(z + 3.0, 0.0, 6.0) / 6.0


def hardswish_grad(z):
    return np.where(z < -3.0, 0.0, np.where(z <= 3.0, z / 3.0 + 0.5, 1.0))


def _keep_rows(keep, per, T, dtype):
    return np.ones(T, dtype) if keep is None else (keep.astype(dtype)[np.arange(T) // per] / dtype(BN_SURVIVAL))


def bn_ref(c: BnCase, i) -> dict:
    """Training: batch statistics with the biased variance, the running variance updated with M2 / (T - 1) -- and at T = 1, where torch
    refuses training-mode batch norm, the definition written out: var = 0, the running variance updated with the biased value (0), as the
    kernel's comment says.  Eval: the running statistics normalise and are not updated."""
    T, C = c.T, c.C
    y = i["y"].astype(np.float64)
    g, b = i["gamma"].astype(np.float64), i["beta"].astype(np.float64)
    r = {}
    if c.training:
        mean = y.mean(0)
        m2 = ((y - mean) ** 2).sum(0)
        var = m2 / T
        invstd = 1.0 / np.sqrt(var + BN_EPS)
        unb = m2 / (T - 1) if T > 1 else var
        r.update(m2=m2, run_mean=(1 - c.mom) * i["run_mean"].astype(np.float64) + c.mom * mean,
                 run_var=(1 - c.mom) * i["run_var"].astype(np.float64) + c.mom * unb, unb=unb)
    else:
        mean = i["run_mean"].astype(np.float64)
        invstd = 1.0 / np.sqrt(i["run_var"].astype(np.float64) + BN_EPS)
    xh = (y - mean) * invstd
    zpre = g * xh + b
    f = _keep_rows(i["keep"], c.per, T, np.float64)[:, None]
    z = (hardswish(zpre) if c.act else zpre) * f
    if i["res"] is not None:
        z = z + i["res"]
    dzp = i["dz"].astype(np.float64) * (hardswish_grad(zpre) if c.act else 1.0) * f
    dgamma, dbeta = (dzp * xh).sum(0), dzp.sum(0)
    k = g * invstd
    dy = k * (dzp - dbeta / T - xh * dgamma / T) if c.training else k * dzp
    kink = (np.abs(np.abs(zpre) - 3.0) < BN_KINK) if c.act else np.zeros((T, C), bool)
    r.update(mean=mean, invstd=invstd, xh=xh, zpre=zpre, z=z, dzp=dzp, f=f, dgamma=dgamma, dbeta=dbeta, dy=dy, kink=kink)
    return r


def kink_cap_ok(c: BnCase, kink) -> bool:
    return kink.sum() <= 0.01 * kink.size and bool((kink.sum(0) <= max(1, int(0.02 * c.T))).all())


def cs_ref(c: CsCase, i):
    return c.beta * i["out0"].astype(np.float64) + i["X"].astype(np.float64).sum(0)


# ---------------------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def ln_path(c):
    """(n_sum, n_col): additions on the longest path of a row sum and of a dgamma column"""
    if isinstance(c, PadCase):
        slabs = lnp_slabs(c.rows)
        return -(-c.n // 64) + 6, -(-c.rows // slabs) + slabs
    J, lpr = ln_inst(c.dim)
    slots = LN_WAVES * 64 // lpr
    grid = min(LN_BWD_BLOCKS, -(-c.rows // slots))
    return 4 * J + {32: 5, 64: 6}[lpr], -(-c.rows // (grid * slots)) + slots + -(-grid // RR_LANES) + RR_LANES


def ln_bounds(c, i, ref) -> dict:
    n = i["n"]
    n_sum, n_col = ln_path(c)
    x, dy = np.abs(i["x"][:, :n].astype(np.float64)), np.abs(i["dy"][:, :n].astype(np.float64))
    g = np.abs(i["gamma"].astype(np.float64))
    xmax = x.max(1)
    K = (xmax + np.abs(ref["mean"])) * ref["rstd"]
    E = 2 * (n_sum + 8) * U * K
    rel_rs = (n_sum + 8) * U + (n_sum * U * K) ** 2
    ymax = np.abs(ref["y"]).max(1)
    G = (dy * g).max(1)
    X = np.maximum(1.0, np.abs(ref["xh"]).max(1))
    core = ref["rstd"] * G * (2 + X) * (2 * (n_sum + 8) * U + E + (n_sum * U * K) ** 2)
    dxmax = np.abs(ref["dx"]).max(1)
    axh = np.abs(ref["xh"])
    pre = 2 * U * ((np.abs(i["dgamma0"]) if c.acc else 0.0) + np.abs(ref["dgamma"]))
    preb = 2 * U * ((np.abs(i["dbeta0"]) if c.acc else 0.0) + np.abs(ref["dbeta"]))
    return {"mean": (n_sum + 2) * U * xmax, "rstd": ref["rstd"] * rel_rs, "y": (g.max() * E + 4 * U * ymax)[:, None] + UB * np.abs(ref["y"]),
            "dx32": core + np.where(G > 0, 2 * U * dxmax, 0.0), "dx16": core[:, None] + UB * np.abs(ref["dx"]),
            "dgamma": (dy * (E[:, None] + 4 * U * axh)).sum(0) + n_col * U * (dy * axh).sum(0) + pre,
            "dbeta": n_col * U * dy.sum(0) + preb}


def bn_bounds(c: BnCase, i, ref) -> dict:
    T = c.T
    ay = np.abs(i["y"].astype(np.float64))
    g = np.abs(i["gamma"].astype(np.float64))
    ymax, amean, inv = ay.max(0), np.abs(ref["mean"]), ref["invstd"]
    n_w = min(-(-T // BN_GROUPS), BN_CHUNK // BN_GROUPS) + BN_GROUPS + 8
    K = (ymax + amean) * inv
    b = {}
    if c.training:
        m2 = ref["m2"]
        b["mean"] = n_w * U * ymax
        b["m2"] = 2 * n_w * U * (m2 + np.sqrt(T * m2) * (ymax + amean))
        b["invstd"] = inv ** 3 * b["m2"] / (2 * T) + 4 * U * inv
        b["run_mean"] = c.mom * b["mean"] + 4 * U * (np.abs(i["run_mean"]) + amean)
        b["run_var"] = c.mom * b["m2"] / max(T - 1, 1) + 4 * U * (np.abs(i["run_var"]) + ref["unb"])
        E = inv * b["mean"] + np.abs(i["y"] - ref["mean"]).max(0) * b["invstd"] + 4 * U * K
        rel_inv = b["invstd"] / inv
    else:
        E = 6 * U * K
        rel_inv = 4 * U
    f = ref["f"]
    zmax = np.abs(ref["z"]).max(0)
    zb = 1.5 * f.max() * g * E + 6 * U * zmax
    b["z32"], b["z16"] = zb, zb + UB * np.abs(ref["z"])
    adz, axh = np.abs(i["dz"].astype(np.float64)) * f, np.abs(ref["xh"])
    adzp = np.abs(ref["dzp"])
    act = 1.0 if c.act else 0.0
    b["dbeta"] = n_w * U * adzp.sum(0) + act * adz.sum(0) * (g * E / 3 + 4 * U) + 2 * U * np.abs(ref["dbeta"])
    b["dgamma"] = n_w * U * (adzp * axh).sum(0) + adzp.sum(0) * E + act * (adz * axh).sum(0) * (g * E / 3 + 4 * U) + 2 * U * np.abs(ref["dgamma"])
    D = 1.5 * adz.max(0)
    X = np.maximum(1.0, axh.max(0))
    dymax = np.abs(ref["dy"]).max(0)
    if c.training:
        m1, m2_ = np.abs(ref["dbeta"]) / T, np.abs(ref["dgamma"]) / T
        inner = act * D * (g * E / 3 + 4 * U) + b["dbeta"] / T + E * m2_ + X * b["dgamma"] / T + 6 * U * (D + m1 + X * m2_)
    else:
        inner = act * D * (g * E / 3 + 4 * U) + 6 * U * D
    b["dy"] = g * inv * inner + rel_inv * dymax + UB * np.abs(ref["dy"])
    return b


def cs_bound(c: CsCase, i, ref):
    rpc, chunks = colsum_split(c.T)
    n_c = -(-rpc // 4) + 2 + -(-chunks // RR_LANES) + RR_LANES
    return n_c * U * np.abs(i["X"].astype(np.float64)).sum(0) + 2 * U * (np.abs(c.beta * i["out0"]) + np.abs(ref))


def ratio(got, ref, bound, axis=None, skip=None) -> float:
    """worst |got - ref| / bound.  A bound per row (axis 1) or per column (axis 0) is held against the row's or column's largest error, a
    bound per element (a row or column term plus the element's own store term) against each element.  A zero bound demands equality; NaN
    is over."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    if skip is not None:
        err = np.where(skip, 0.0, err)
    bound = np.asarray(bound, np.float64)
    if axis is not None and err.ndim == 2 and bound.ndim < 2:
        err = err.max(axis)
    elif axis == 1 and bound.ndim == 1:
        bound = bound[:, None]
    bound = np.broadcast_to(bound, err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def ln_check(c, i, got) -> dict:
    """got: y, mean, rstd, dx32 and / or dx16 [rows, ld], dgamma, dbeta -> {output: worst error / bound}.  The pad columns of y and dx
    must be exactly zero."""
    n = i["n"]
    ref = ln_ref(c, i)
    bnd = ln_bounds(c, i, ref)
    out = {"mean": ratio(got["mean"], ref["mean"], bnd["mean"]), "rstd": ratio(got["rstd"], ref["rstd"], bnd["rstd"]),
           "y": ratio(got["y"][:, :n], ref["y"], bnd["y"], 1), "dgamma": ratio(got["dgamma"], ref["dgamma"], bnd["dgamma"]),
           "dbeta": ratio(got["dbeta"], ref["dbeta"], bnd["dbeta"])}
    pads = [got["y"][:, n:]]
    for k in ("dx32", "dx16"):
        if got.get(k) is not None:
            out[k] = ratio(np.asarray(got[k][:, :n], np.float64) - ref["dres"], ref["core"], bnd[k], 1)
            pads.append(got[k][:, n:])
    for p in pads:
        if p.size and not (np.asarray(p) == 0).all():
            out["pad"] = np.inf
    return out


def bn_check(c: BnCase, i, got) -> dict:
    ref = bn_ref(c, i)
    bnd = bn_bounds(c, i, ref)
    out = {}
    if c.training:
        for k in ("mean", "invstd", "m2", "run_mean", "run_var"):
            out[k] = ratio(got[k], ref[k], bnd[k])
        out["count"] = 0.0 if (np.asarray(got["count"]) == c.T).all() else np.inf
    else:
        out["run_mean"] = 0.0 if np.array_equal(got["run_mean"], i["run_mean"]) and np.array_equal(got["run_var"], i["run_var"]) else np.inf
    for k in ("z32", "z16"):
        if got.get(k) is not None:
            out[k] = ratio(got[k], ref["z"], bnd[k], 0)
    out["dgamma"] = ratio(got["dgamma"], ref["dgamma"], bnd["dgamma"])
    out["dbeta"] = ratio(got["dbeta"], ref["dbeta"], bnd["dbeta"])
    out["dy"] = ratio(got["dy"], ref["dy"], bnd["dy"], 0, skip=ref["kink"])
    return out


def cs_check(c: CsCase, i, got) -> dict:
    ref = cs_ref(c, i)
    return {"out": ratio(got, ref, cs_bound(c, i, ref))}


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 emulations in the kernels' own order.  `wrong` names one of the mistakes test_norm_ref_host.py lists
# ---------------------------------------------------------------------------------------------------------------------------------
def _tree(s):
    """the xor shuffle tree over the last axis (every lane ends with the same sum)"""
    L = s.shape[-1]
    o = L // 2
    lanes = np.arange(L)
    while o > 0:
        s = s + s[..., lanes ^ o]
        o //= 2
    return s[..., 0]


def _sum4(v):
    return (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3]) if v.shape[-1] == 4 else v[..., 0]


def _lane_sum(v, valid, drop_partial=False):
    """v [rows, J, L, E]: per lane over j in order, then the tree.  Chunks past the row hold zeros."""
    s = np.zeros(v.shape[:1] + v.shape[2:3], F)
    for j in range(v.shape[1]):
        if drop_partial and valid[j].any() and not valid[j].all():
            continue
        s = s + _sum4(v[:, j])
    return _tree(s)


def reduce_rows(partial, dst, beta, per_partial=False):
    """reduce_rows_kernel: lane rl sums partial rows rl, rl + 64, ... in order; lane 0 adds the 64 lanes in order"""
    P, ncols = partial.shape
    lanes = np.zeros((RR_LANES, ncols), F)
    for p in range(P):
        lanes[p % RR_LANES] = lanes[p % RR_LANES] + partial[p]
        if per_partial and beta != 0:
            lanes[p % RR_LANES] = lanes[p % RR_LANES] + F(beta) * dst
    t = np.zeros(ncols, F)
    for k in range(RR_LANES):
        t = t + lanes[k]
    return (F(beta) * dst + t) if (beta != 0 and not per_partial) else t


def ln_emul(c, i, wrong=None, store=True) -> dict:
    """nrv_layernorm_fwd / _bwd (LnCase) or nrv_layernorm_pad_* (PadCase); the backward reads the forward's fp32 mean and rstd.
    `store` = False keeps the fp32 values a bf16 store would round."""
    pad = isinstance(c, PadCase)
    n, ld, rows = i["n"], i["ld"], c.rows
    lim = ld if (pad and wrong == "sums to ld") else n
    if pad:                                  # lane l of the row's wave takes columns l, l + 64, ...
        J, L = -(-lim // 64), 64
        idx = (np.arange(J)[:, None] * 64 + np.arange(64)[None, :])[:, :, None]
    else:                                    # lane l of the row's lane group takes the 4-element chunks l, l + LPR, ...
        J, L = ln_inst(n)
        idx = (np.arange(L)[None, :, None] + L * np.arange(J)[:, None, None]) * 4 + np.arange(4)[None, None, :]
    valid = idx < lim                        # idx, valid [J, L, 1 | 4]: the column an element of the register image holds
    vj = valid.reshape(J, -1)
    span = max(int(idx.max()) + 1, ld)

    def lay(a):
        """[rows, ld] or [n] -> the register image, zero where the kernel loads nothing"""
        src = np.zeros(a.shape[:-1] + (span,), F)
        src[..., :a.shape[-1]] = a
        return np.where(valid, src[..., idx], F(0))
    x, dy = i["x"].astype(F), i["dy"].astype(F)
    g, b = i["gamma"], i["beta"]
    gl, bl = lay(g), lay(b)
    inv = F(1.0) / F(n)
    with np.errstate(invalid="ignore", over="ignore"):
        v = lay(x)
        drop = wrong == "partial chunk dropped" and not pad and L == 64
        mu = _lane_sum(v, vj, drop) * inv
        if wrong == "pair shares the mean" and not pad and L == 32:
            mu = mu.copy()
            mu[1::2] = mu[0::2][:rows // 2]
        mub = mu[:, None, None, None]
        if wrong == "E[x^2] - mean^2":
            var = _lane_sum(v * v, vj) * inv - mu * mu
        else:
            d = np.where(valid[None], v - mub, F(0))
            var = _lane_sum(d * d, vj, drop) * inv
        rs = (F(1.0) / np.sqrt(var + F(c.eps))).astype(F)
        rsb = rs[:, None, None, None]
        xh = np.where(valid[None], (v - mub) * rsb, F(0))
        y = xh * gl[None] + bl[None]
        # backward
        dl = lay(dy)
        gg = dl * (F(1) if wrong == "c1 c2 from dy" else gl[None])
        c1 = _lane_sum(gg * xh, vj) * inv
        c2 = _lane_sum(gg, vj) * inv
        gg = dl * gl[None]
        core = (gg - c2[:, None, None, None] - xh * c1[:, None, None, None]) * rsb
        dx = core
        if i["dres"] is not None:
            dx = core + lay(i["dres"].astype(F))
        pg, pb = dl * xh, dl

    def flat(a):
        out = np.zeros((rows, ld), F)
        m = valid & (idx < ld)
        out[:, idx[m]] = a[:, m]
        if pad and wrong != "sums to ld":
            out[:, n:] = 0
        return out
    st = bf16r if store else (lambda a: a)
    res = {"mean": mu, "rstd": rs, "y": st(flat(y))}
    dxf = flat(dx)
    if pad and wrong == "pads carry dres" and i["dres"] is not None:
        dxf[:, n:] = i["dres"][:, n:]
    if c.out in ("f32", "both"):
        res["dx32"] = dxf
    if c.out in ("bf16", "both"):
        res["dx16"] = st(flat(core) if (wrong == "bf16 drops dres" and c.out == "bf16") else dxf)
    pg, pb = flat(pg)[:, :n], flat(pb)[:, :n]
    # column sums
    if pad:
        slabs = lnp_slabs(rows)
        per = rows // slabs if wrong == "slab rounded down" else -(-rows // slabs)
        dg, db = np.zeros(n, F), np.zeros(n, F)
        for s in range(slabs):
            sg, sb = np.zeros(n, F), np.zeros(n, F)
            for r in range(s * per, min(rows, (s + 1) * per)):
                sg, sb = sg + pg[r], sb + pb[r]
            dg, db = dg + sg, db + sb
        if c.acc:
            dg, db = i["dgamma0"] + dg, i["dbeta0"] + db
    else:
        slots = LN_WAVES * 64 // L
        grid = -(-rows // slots)
        assert grid <= LN_BWD_BLOCKS
        part = np.zeros((grid, 2 * n), F)
        for blk in range(grid):
            r0, r1 = blk * slots, min(rows, (blk + 1) * slots)
            if wrong == "last workgroup lost" and r1 - r0 < slots:
                continue
            sg, sb = pg[r0].copy(), pb[r0].copy()
            for r in range(r0 + 1, r1):
                sg, sb = sg + pg[r], sb + pb[r]
            part[blk, :n], part[blk, n:] = sg, sb
        t = reduce_rows(part, np.concatenate([i["dgamma0"], i["dbeta0"]]), 1.0 if c.acc else 0.0)
        dg, db = t[:n], t[n:]
    res["dgamma"], res["dbeta"] = dg, db
    return res


def _chan(n, mean, m2, nb, mb, qb, skip=True):
    """Chan's merge of (nb, mb, qb) into (n, mean, m2), elementwise"""
    with np.errstate(divide="ignore", invalid="ignore"):
        nn = n + nb
        d = mb - mean
        mean2 = mean + d * (nb / nn)
        m22 = m2 + qb + d * d * (n * nb / nn)
    if skip:
        z = nb == 0
        return np.where(z, n, nn), np.where(z, mean, mean2), np.where(z, m2, m22)
    return nn, mean2, m22


def _groups(a, T, fill=0.0):
    """[T, C] -> [chunks, steps, BN_GROUPS, C] (row r0 + g + 4 s of a chunk) and its validity"""
    chunks = -(-T // BN_CHUNK)
    p = np.full((chunks * BN_CHUNK,) + a.shape[1:], fill, a.dtype)
    p[:T] = a
    ok = (np.arange(chunks * BN_CHUNK) < T).reshape(chunks, BN_CHUNK // BN_GROUPS, BN_GROUPS, 1)
    return p.reshape((chunks, BN_CHUNK // BN_GROUPS, BN_GROUPS) + a.shape[1:]), ok


def _lanes64(vals):
    """[chunks, ...] float64 -> sum in bn_bwd_final_kernel's order: lane l takes chunks l, l + 64, ..., then the shfl_down tree"""
    lanes = np.zeros((64,) + vals.shape[1:])
    for ch in range(vals.shape[0]):
        lanes[ch % 64] = lanes[ch % 64] + vals[ch]
    off = 32
    while off > 0:
        lanes[:off] = lanes[:off] + lanes[off:2 * off]
        off //= 2
    return lanes[0]


def bn_stats_emul(c: BnCase, i, wrong=None) -> dict:
    T, C = c.T, c.C
    y = i["y"]
    if wrong == "sum and sum of squares":
        mean = (y.sum(0, dtype=F) / F(T)).astype(F)
        var = ((y * y).sum(0, dtype=F) / F(T) - mean * mean).astype(F)
        n, mean, m2 = np.full(C, float(T)), mean.astype(np.float64), var.astype(np.float64) * T
    else:
        skip_p, skip_f = wrong != "no skip in the group merge", wrong != "no skip in the chunk merge"
        yg, ok = _groups(y, T)
        chunks = yg.shape[0]
        n, mean, m2 = (np.zeros((chunks, BN_GROUPS, C), F) for _ in range(3))
        for s in range(yg.shape[1]):
            x, v = yg[:, s], ok[:, s]
            n1 = n + F(1)
            d = x - mean
            mean1 = mean + d / n1
            m21 = d * (x - mean1) + m2
            n, mean, m2 = np.where(v, n1, n), np.where(v, mean1, mean), np.where(v, m21, m2)
        N, M, Q = n[:, 0], mean[:, 0], m2[:, 0]
        for k in range(1, BN_GROUPS):
            N, M, Q = _chan(N, M, Q, n[:, k], mean[:, k], m2[:, k], skip_p)
        N, M, Q = N.astype(F), M.astype(F), Q.astype(F)
        ln_, lm, lq = (np.zeros((64, C)) for _ in range(3))
        for ch in range(chunks):
            l = ch % 64
            ln_[l], lm[l], lq[l] = _chan(ln_[l], lm[l], lq[l], N[ch].astype(np.float64), M[ch].astype(np.float64), Q[ch].astype(np.float64), skip_f)
        off = 32
        while off > 0:
            ln_[:off], lm[:off], lq[:off] = _chan(ln_[:off], lm[:off], lq[:off], ln_[off:2 * off], lm[off:2 * off], lq[off:2 * off], skip_f)
            off //= 2
        n, mean, m2 = ln_[0], lm[0], lq[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        var = m2 / n
        unb = np.where(n > 1.0, m2 / (n - 1.0), var) if wrong != "biased running variance" else var
        mom = F(c.mom)
        r = {"mean": mean.astype(F), "invstd": (1.0 / np.sqrt(var + np.float64(F(BN_EPS)))).astype(F), "count": n.astype(F), "m2": m2.astype(F),
             "run_mean": (F(1) - mom) * i["run_mean"] + mom * mean.astype(F), "run_var": (F(1) - mom) * i["run_var"] + mom * unb.astype(F)}
    return r


def bn_emul(c: BnCase, i, wrong=None, store=True) -> dict:
    """nrv_bn_stats -> nrv_bn_apply -> nrv_bn_bwd as the model runs them (training), or apply / bwd on the running statistics (eval)"""
    T, C = c.T, c.C
    y, g, b = i["y"], i["gamma"], i["beta"]
    if c.training:
        r = bn_stats_emul(c, i, wrong)
        mean, inv = r["mean"], r["invstd"]
    else:
        r = {"run_mean": i["run_mean"].copy(), "run_var": i["run_var"].copy()}
        mean, inv = i["run_mean"], (F(1) / np.sqrt(i["run_var"] + F(BN_EPS))).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        if i["keep"] is None:
            f = np.ones((T, 1), F)
        else:
            rows = np.minimum(np.arange(T), i["keep"].size - 1) if wrong == "keep by row" else np.arange(T) // c.per
            f = (i["keep"][rows] / F(BN_SURVIVAL))[:, None].astype(F)
        xh = (y - mean) * inv
        zpre = g * xh + b
        z = (hardswish(zpre).astype(F) if c.act else zpre) * f
        if i["res"] is not None:
            z = i["res"] + z
        if c.out in ("f32", "both"):
            r["z32"] = z
        if c.out in ("bf16", "both"):
            r["z16"] = bf16r(z) if store else z
        dz = i["dz"]
        if wrong == "bf16 dz read as fp32" and c.dzbf:
            bits = torch.from_numpy(dz).to(torch.bfloat16).view(torch.int16).numpy().reshape(-1)
            as32 = bits.view(np.float32) if bits.size % 2 == 0 else np.zeros(0, F)
            dz = np.zeros(T * C, F)
            dz[:as32.size] = as32
            dz = dz.reshape(T, C)
        dzp = dz
        if c.act:
            dzp = dzp * hardswish_grad(xh if wrong == "hs' at x^" else zpre).astype(F)
        dzp = (dzp * f).astype(F)
        dg_, ok = _groups(dzp, T)
        xg, _ = _groups(xh.astype(F), T)
        sd, sdx = (np.zeros((dg_.shape[0], BN_GROUPS, C), F) for _ in range(2))
        for s in range(dg_.shape[1]):
            v = ok[:, s]
            sd, sdx = np.where(v, sd + dg_[:, s], sd), np.where(v, dg_[:, s] * xg[:, s] + sdx, sdx)
        for k in range(1, BN_GROUPS):
            sd[:, 0], sdx[:, 0] = sd[:, 0] + sd[:, k], sdx[:, 0] + sdx[:, k]
        sD, sDX = _lanes64(sd[:, 0].astype(np.float64)), _lanes64(sdx[:, 0].astype(np.float64))
        div = float(dg_.shape[0] * BN_CHUNK) if wrong == "mean over the padded rows" else float(T)
        m1, m2 = (sD / div).astype(F), (sDX / div).astype(F)
        k = g * inv
        dy = k * (dzp - m1 - xh * m2) if c.training else k * dzp
    r.update(dgamma=sDX.astype(F), dbeta=sD.astype(F), dy=bf16r(dy) if store else dy)
    return r


def cs_emul(c: CsCase, i, wrong=None):
    T, N = c.T, c.N
    rpc, chunks = colsum_split(T)
    back = i["back"]
    flat = back.reshape(-1)
    ld = N if wrong == "ld ignored" else c.ld
    a = np.zeros((chunks, 4, N), F)
    with np.errstate(invalid="ignore"):
        for ch in range(chunks):
            r1 = (ch + 1) * rpc if wrong == "past T" else min(T, (ch + 1) * rpc)
            for rl in range(4):
                for r in range(ch * rpc + rl, r1, 4):
                    a[ch, rl] = a[ch, rl] + flat[r * ld:r * ld + N]
        partial = (a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3])
        return reduce_rows(partial, i["out0"], c.beta, per_partial=wrong == "beta per partial")
