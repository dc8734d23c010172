"""Fused Sinkhorn attention at its tile, slot and walk edges: geometry, case tables, inputs, the fp64 reference and a plain restatement
of what the kernel pair does (test infrastructure, no kernels).  Builds on peaked_ref.py; the house pattern of attn_edges_ref.py.

The kernels: noise_robust_vit_amd/csrc/nrv_sinkhorn.hip, one forward and one backward per NP = 32 ceil(N / 32) <= 256 at dh = 64.
  forward    16 waves x one 16-query tile; the head's P0 in registers; K and V as LDS images, two image pairs and two b vectors that
             alternate with `it & 1` while one workgroup per CU walks the heads blockIdx.x, + gridDim.x, ..
  backward   8 waves x SK_TPW = 2 query tiles; P7 / dS go through an LDS chunk of CH = 128 queries (slot u = 0: queries 0..127,
             slot u = 1: the NP - 128 queries behind them) for dV = P7^T dO and dK = dS^T Q; with three image slots (NP <= 224) the
             walk is persistent as well, K and V swap slots on odd `it`, and the next head's K image lands in the slot V has left.
             At NP = 256 there are two slots and grid = heads.
Padding: keys >= N are masked in the LAST TWO key tiles (NP - N < 32); queries >= N get inv = 0 in the forward and lse = +inf, a = 0 in
the backward; rows >= N of every LDS image read as zero; the saved vectors are [B, H, 7, N] with row stride N.

What the cases are for.  A whole-tensor norm cannot see one wrong key tile, one wrong query tile of one head, or a head that got its
neighbour's K image: each is a few per cent of the norm.  `check` is per row (peaked_ref.per_row_rel), on every head, and reports the
head, the row and -- for a walk case -- the pass `head // grid` of the worst row.  The inputs put key N - 1 twelve nats below the rest
for every query (N >= 8): b3 of that key is ~ 1e5, it sits on the pad boundary, and its dk / dv rows are as large as any other key's.

  EDGE_CASES    B = H = 2; N in {32k-31, 32k-17, 32k-16, 32k-15, 32k-1, 32k} for k = 1..8, and N = 2, 3, 5  (51 values)
  SCALE_CASES   N in {3, 49, 130, 197, 256} at scale 0.1, 0.2, 0.0625 (every other test of the pair uses 0.125)
  WALK_SPECS    3 cus + 7 heads as (heads, 1) and (ceil(heads / 5), 5) at N = 17, 33: `it` = 0, 1, 2 for every workgroup, 3 for seven;
                ceil(2.25 cus) + 3 heads at N = 129, 197 (forward and backward) and N = 225 (forward only: NP = 256, two slots)

`restated` is the kernels' arithmetic in plain torch on the padded NP x NP layout, with at most one of MISTAKES switched on; the host
test shows that each mistake puts a named case over a bound of `check`, and that the stale-image mistake is invisible to every case
whose workgroups make at most two passes: the many-head tests that existed before (270 and 276 heads on 256 CUs) among them.
"""
from __future__ import annotations

import functools
import math
import os
import re
from collections import namedtuple
from typing import Optional

import torch

import peaked_ref as PR
from peaked_ref import EMULATION_BOUND, PER_ROW_BOUND, heads, per_row_rel  # noqa: F401  (re-exported for the two tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "noise_robust_vit_amd", "csrc", "nrv_sinkhorn.hip")

DH = 64
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
SK_WAVES = 16                 # forward: one 16-query tile per wave
SK_TPW = 2                    # backward: query tiles per wave
BWD_WAVES = SK_WAVES // SK_TPW
CH = 16 * BWD_WAVES           # queries per chunk slot of the backward
LDS_BYTES = 160 * 1024
NOMINAL_CUS = 256             # the host test's stand-in for multi_processor_count (an MI355X has 256)
REF_HEADS = 64                # the reference is evaluated in chunks of at most this many heads
WEAK_NATS = 12.0              # key N - 1, for N >= MIN_PEAKED_N
MIN_PEAKED_N = 8
O_BOUND = 2.0 ** -6           # x the tensor's maximum, per o row               } the figures of
LSE_TOL = 1e-4                # x max(1, |lse|_max)                             } tests/test_peaked_attn_gpu.py
SCAL_TOL = 1e-3               # element-wise relative, the seven saved vectors  }
KERNEL_ROUNDING_BOUND = PER_ROW_BOUND / 2     # restated(kernel_rounding=True) against fp64, per row (host test): the other half of the
                              # GPU bound is for what the restatement leaves exact (fp32 sums in another order, v_exp_f32, the MFMAs)
ONE_KEY_STEPS = 8             # N = 1: the seven normalisation steps and the softmax backward each leave at most one fp32 rounding of G
FP32_BOUND = 1e-5             # restated() in fp32 against fp64, per row: the figure of tests/test_peaked_ref_host.py for torch fp32

# family: edge | scale | walk;  kind: the edge kind (EDGE_KINDS), "" otherwise;  fwd_only: the backward is not run (walk, NP = 256)
Case = namedtuple("Case", "family B N H scale kind fwd_only")
WalkSpec = namedtuple("WalkSpec", "heads_rule per_sample N fwd_only")      # heads_rule: "3x+7" | "2.25x+3";  per_sample: H (1 or 5)


# ---- geometry, restated from the source -------------------------------------------------------------------------------------------
def np_of(N: int) -> int:
    return 32 * ((N + 31) // 32)


def nt_of(N: int) -> int:
    return np_of(N) // 16


def fwd_lds(NP: int):
    """SkFwdLds<NP>: (TWO, BYTES)"""
    img, vec = 2 * NP * 128, (2 + SK_WAVES) * NP * 4
    two = 2 * img + vec <= LDS_BYTES
    return two, (2 if two else 1) * img + vec


def bwd_lds(NP: int):
    """SkBwdLds<NP, SK_TPW>: (THREE, BYTES).  3 NP 128 + (5 + 8) NP 4 + 128 (2 NP + 32) = 692 NP + 4096."""
    rs, vec = NP * 2 + 32, (5 + BWD_WAVES) * NP * 4
    three = 3 * NP * 128 + vec + CH * rs <= LDS_BYTES
    return three, (3 if three else 2) * NP * 128 + vec + CH * rs


def grids(N: int, nheads: int, cus: int):
    """(forward grid, backward grid) of launch_sk_fwd / launch_sk_bwd: persistent (grid = cus) where the next head's images have room."""
    NP = np_of(N)
    return (cus if fwd_lds(NP)[0] and nheads > cus else nheads), (cus if bwd_lds(NP)[0] and nheads > cus else nheads)


def passes(N: int, nheads: int, cus: int):
    """(forward, backward): the largest number of heads one workgroup walks"""
    return tuple(-(-nheads // g) for g in grids(N, nheads, cus))


# what the host test reads back out of nrv_sinkhorn.hip: (pattern, the groups it must capture).  A constant changed later fails there
# instead of quietly moving the cases off their edges.
SOURCE_FACTS = (
    (r"constexpr int SK_THREADS = (\d+);", ("1024",)),
    (r"constexpr int SK_WAVES = (\d+);", (str(SK_WAVES),)),
    (r"constexpr int SK_TPW = (\d+);", (str(SK_TPW),)),
    (r"int np_of\(int N\) \{ return \(N \+ (\d+)\) / (\d+) \* (\d+); \}", ("31", "32", "32")),
    (r"static constexpr int IMG = (\d+) \* NP \* (\d+);", ("2", "128")),
    (r"static constexpr int VEC = \((\d+) \+ SK_WAVES\) \* NP \* (\d+);", ("2", "4")),
    (r"static constexpr bool TWO = (\d+) \* IMG \+ VEC <= (\d+) \* (\d+);", ("2", "160", "1024")),
    (r"static constexpr int WAVES = (\d+) / TPW;", ("16",)),
    (r"static constexpr int CH = (\d+) \* WAVES;", ("16",)),
    (r"static constexpr int RS = NP \* (\d+) \+ (\d+);", ("2", "32")),
    (r"static constexpr int VEC = \((\d+) \+ WAVES\) \* NP \* (\d+);", ("5", "4")),
    (r"static constexpr bool THREE = (\d+) \* NP \* (\d+) \+ VEC \+ CH \* RS <= (\d+) \* (\d+);", ("3", "128", "160", "1024")),
    (r"const int grid = SkFwdLds<NP>::(TWO) && heads > sk_cus\(\) \? sk_cus\(\) : heads;", ("TWO",)),
    (r"const int grid = SkBwdLds<NP, TPW>::(THREE) && heads > sk_cus\(\) \? sk_cus\(\) : heads;", ("THREE",)),
    (r"if \(kt >= NP / 16 - (\d+)\) p0\[kt\]\[e\] = \(kt \* 16 \+ 4 \* g \+ e < N\)", ("2",)),        # forward: pad mask, last two tiles
    (r"if \(kt >= NT - (\d+)\) pv = \(kt \* 16 \+ 4 \* g \+ e < N\) \? pv : 0\.f;", ("2",)),           # backward: the same
    (r"float\* scal = p\.scal \+ \(long long\)bh \* (\d+) \* (N);", ("7", "N")),
    (r"const bool odd = THREE && \(it & (\d+)\);", ("1",)),
    (r"const int cur = L::TWO \? \(it & (\d+)\) : 0;", ("1",)),
    (r"if \(!\(scale > 0\.f\)\) return (NRV_ERR_SHAPE);", ("NRV_ERR_SHAPE",)),
)
DISPATCH_NP = (32, 64, 96, 128, 160, 192, 224, 256)


def source_text() -> str:
    with open(SOURCE) as f:
        return f.read()


def source_problems(text: str):
    out = []
    for rx, want in SOURCE_FACTS:
        found = [tuple(m.groups()) for m in re.finditer(rx, text)]
        if not found:
            out.append(f"nrv_sinkhorn.hip no longer matches {rx!r}")
        elif any(f != tuple(want) for f in found):
            out.append(f"{rx!r} captures {found}, the geometry here was derived from {tuple(want)}")
    nps = tuple(int(m.group(1)) for m in re.finditer(r"case \d+: \{ constexpr int NPV = (\d+); return CALL; \}", text)) + \
        tuple(int(m.group(1)) for m in re.finditer(r"default: \{ constexpr int NPV = (\d+); return CALL; \}", text))
    if nps != DISPATCH_NP:
        out.append(f"NRV_SK_DISPATCH instantiates NP = {nps}, the case table was written for {DISPATCH_NP}")
    return out


# ---- the case tables --------------------------------------------------------------------------------------------------------------
# per NP = 32 k: the offsets from 32 k and what each puts on an edge
EDGE_KINDS = {
    -31: "first_n",               # the first N of the NP: one real key in tile NT - 2, tile NT - 1 all padding, one query in the last active wave
    -17: "pad_tile_after_partial",  # tile NT - 1 all padding behind a partial tile NT - 2
    -16: "pad_tile_after_full",   # tile NT - 1 all padding behind a full one
    -15: "one_key_last_tile",     # one real key (and one real query) in tile NT - 1
    -1: "one_pad_key",            # one padding key
    0: "full",                    # N = NP: nothing padded
}
TINY_NS = (2, 3, 5)


def _edge_cases():
    out = []
    for k in range(1, 9):
        for off, kind in EDGE_KINDS.items():
            out.append(Case("edge", 2, 32 * k + off, 2, DH ** -0.5, kind, False))
    out += [Case("edge", 2, N, 2, DH ** -0.5, "tiny", False) for N in TINY_NS]
    return tuple(sorted(out, key=lambda c: c.N))


EDGE_CASES = _edge_cases()
SCALE_NS = (3, 49, 130, 197, 256)
SCALES = (0.1, 0.2, 0.0625)
SCALE_CASES = tuple(Case("scale", 2, N, 2, s, "", False) for N in SCALE_NS for s in SCALES)
WALK_SPECS = (
    WalkSpec("3x+7", 1, 17, False), WalkSpec("3x+7", 5, 17, False), WalkSpec("3x+7", 1, 33, False), WalkSpec("3x+7", 5, 33, False),
    WalkSpec("2.25x+3", 1, 129, False), WalkSpec("2.25x+3", 1, 197, False), WalkSpec("2.25x+3", 1, 225, True),
)
WRAPPER_CASES = tuple(c for c in EDGE_CASES if c.N in (17, 129, 225))     # wave 0 and 1 only; both chunk slots; the two-slot backward

# "change that case's inputs, not the bound": (N, scale) of the cases whose first draw left a row outside EMULATION_BOUND or
# KERNEL_ROUNDING_BOUND on the CPU, and the number of the draw that stays inside both (tests/test_sinkhorn_edges_ref_host.py asserts
# both for every case as drawn here).
RESEEDED: dict = {}


def walk_heads(rule: str, cus: int) -> int:
    return 3 * cus + 7 if rule == "3x+7" else math.ceil(2.25 * cus) + 3


def walk_case(spec: WalkSpec, cus: int) -> Case:
    n = walk_heads(spec.heads_rule, cus)
    B = -(-n // spec.per_sample)
    return Case("walk", B, spec.N, spec.per_sample, DH ** -0.5, "", spec.fwd_only)


def spec_id(s: WalkSpec) -> str:
    return f"walk-{s.heads_rule}-H{s.per_sample}-N{s.N}" + ("-fwd" if s.fwd_only else "")


def case_id(c: Case) -> str:
    s = f"{c.family}-B{c.B}-H{c.H}-N{c.N}-NP{np_of(c.N)}"
    if c.kind:
        s += f"-{c.kind}"
    if c.family == "scale":
        s += f"-scale{c.scale:g}"
    return s + ("-fwd" if c.fwd_only else "")


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(B: int, N: int, H: int, scale: float) -> dict:
    seed = 3000 + 7 * N + 100003 * RESEEDED.get((N, scale), 0)
    weak = ((N - 1, WEAK_NATS),) if N >= MIN_PEAKED_N else ()
    qkv = PR.peaked_qkv(B, N, H, DH, weak, seed=seed)
    dout = torch.randn(B * N, H * DH, generator=torch.Generator().manual_seed(11)).to(torch.bfloat16)   # test_peaked_attn_gpu._dout
    return {"qkv": qkv, "dout": dout}


def inputs(c: Case) -> dict:
    """qkv bf16 [B*N, 3*H*64], dout bf16 [B*N, H*64].  Shared by every test of the case: do not modify."""
    return _inputs(c.B, c.N, c.H, c.scale)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def _reference_uncached(c: Case, emulate: bool, device) -> dict:
    """peaked_ref.attention_reference + peaked_ref.sinkhorn_scalings in fp64, in chunks of at most REF_HEADS heads (whole samples)."""
    i = inputs(c)
    B, N, H = c.B, c.N, c.H
    step = max(1, REF_HEADS // H)
    parts = {n: [] for n in ("o", "dq", "dk", "dv", "lse", "scal")}
    for b0 in range(0, B, step):
        nb = min(step, B - b0)
        qkv, dout = i["qkv"][b0 * N:(b0 + nb) * N], i["dout"][b0 * N:(b0 + nb) * N]
        r = PR.attention_reference(qkv, dout, nb, N, H, DH, c.scale, emulate_bf16=emulate, device=device)
        for n in ("o", "dq", "dk", "dv", "lse"):
            parts[n].append(r[n].cpu())
        if not emulate:
            q, k, _ = heads(qkv.to(r["o"].device).double(), nb, N, H, DH)
            av, bv = PR.sinkhorn_scalings(q @ k.transpose(-1, -2) * c.scale)
            scal = torch.empty(nb, H, 7, N, dtype=torch.float64, device=av.device)
            scal[:, :, 0::2], scal[:, :, 1::2] = av, bv
            parts["scal"].append(scal.cpu())
        del r
    return {n: torch.cat(p) for n, p in parts.items() if p}


_small_reference = functools.lru_cache(maxsize=None)(_reference_uncached)
_walk_reference = functools.lru_cache(maxsize=2)(_reference_uncached)        # hundreds of heads each: only the latest are kept


def reference(c: Case, emulate_bf16: bool = False, device=None) -> dict:
    """o, dq, dk, dv [B,H,N,64], lse [B,H,N], scal [B,H,7,N] (a1 b1 a2 b2 a3 b3 a4; not with emulate_bf16), fp64 on the CPU, computed
    once and shared: do not modify.  `device`: where the evaluation runs (the GPU test passes its device for the walk cases)."""
    return (_walk_reference if c.family == "walk" else _small_reference)(c, emulate_bf16, device)


# ---- the kernels, restated --------------------------------------------------------------------------------------------------------
MISTAKES = (
    "pad_mask_last_tile_only",    # keys >= N masked in tile NT - 1 only: the zero K rows of tile NT - 2 enter the softmax with score 0
    "pad_queries_counted",        # inv = 1 / l for the padded query lanes of the active waves too: copies of row N - 1 in the column sums
    "contract_full_tiles_only",   # dK / dV contract over the queries of the full 16-query tiles only
    "second_chunk_dropped",       # chunk slot u = 1 (queries >= 128) left out of dK / dV
    "scal_stride_np",             # the seven saved vectors written with row stride NP (and read with N)
    "ds_without_scale",           # dS = P0 (G - sum G P0), the scale forgotten
    "p0_fp16",                    # the backward's resident P0 as fp16: the historic defect (tests/test_peaked_attn_gpu.py)
    "stale_k_image",              # from pass 2 on, the K image of pass it - 2: a slot not refilled after the swap
)


def _inv_or_zero(x):
    return torch.where(x > 0, 1.0 / x.clamp_min(torch.finfo(x.dtype).tiny), torch.zeros_like(x))


def _ratio_or_zero(num, den):
    return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(num))


def _pad_rows(x, NP):
    """[G, N, d] -> [G, NP, d]: rows >= N of an LDS image read as zero"""
    out = x.new_zeros(x.shape[0], NP, x.shape[2])
    out[:, :x.shape[1]] = x
    return out


def _clamp_rows(x, NP):
    """[G, N, d] -> [G, NP, d]: the per-lane fragment loads of a padded query read row N - 1"""
    N = x.shape[1]
    return x[:, torch.arange(NP).clamp_max(N - 1)]


def pad_key_mask(N: int, NP: int, mistake: Optional[str] = None) -> torch.Tensor:
    """[NP] bool: the keys the kernels mask -- key >= N, tested in the last two key tiles only"""
    key = torch.arange(NP)
    first_tested = NP // 16 - (1 if mistake == "pad_mask_last_tile_only" else 2)
    return (key >= N) & (key // 16 >= first_tested)


def sinkhorn_from_scores(S: torch.Tensor, N: int, sc: float, mistake: Optional[str] = None):
    """The forward's scores-only part.  S [G, NP, NP]: raw scores on the padded layout (query rows >= N hold anything finite), sc =
    scale log2(e).  -> P0 [G,NP,NP], lse [G,NP] and the seven vectors a1 b1 a2 b2 a3 b3 a4 [G,7,NP], as the forward holds them."""
    NP = S.shape[-1]
    nqt = (N + 15) // 16
    S = S.masked_fill(pad_key_mask(N, NP, mistake), float("-inf"))
    m = S.amax(dim=-1, keepdim=True) * sc               # the maximum of the RAW scores, then the scale: sc > 0
    p = torch.exp2(S * sc - m)
    l = p.sum(dim=-1, keepdim=True)
    row = torch.arange(NP)
    counted = (row < 16 * nqt) if mistake == "pad_queries_counted" else (row < N)
    P0 = p / l * counted[:, None].to(S.dtype)
    lse = ((m + torch.log2(l)) * LN2)[..., 0]
    b = torch.ones_like(S[:, 0])
    vecs = []
    for _ in range(3):
        a = _inv_or_zero((P0 * b[:, None, :]).sum(dim=-1))
        b = _inv_or_zero((P0 * a[:, :, None]).sum(dim=-2))
        vecs += [a, b]
    vecs.append(_inv_or_zero((P0 * b[:, None, :]).sum(dim=-1)))
    return P0, lse, torch.stack(vecs, dim=1)


def _forward(q, k, v, N, NP, scale, mistake, rnd):
    S = _clamp_rows(q, NP) @ _pad_rows(k, NP).transpose(-1, -2)
    P0, lse, vecs = sinkhorn_from_scores(S, N, scale * LOG2E, mistake)
    P7 = rnd(P0 * vecs[:, 5, None, :] * vecs[:, 6, :, None])
    return rnd(P7 @ _pad_rows(v, NP))[:, :N], lse[:, :N], vecs[:, :, :N]


def _backward(q, k_img, v, dO, lse, scal, N, NP, scale, mistake, rnd, rnd_p0):
    """k_img: what the K image slot holds (P0 and dQ = dS K read it); scal [G,7,N], lse [G,N] as saved."""
    G_, dt = q.shape[0], q.dtype
    sc = scale * LOG2E
    row = torch.arange(NP)
    ok = row < N
    S = _clamp_rows(q, NP) @ _pad_rows(k_img, NP).transpose(-1, -2)
    lse2 = torch.full((G_, NP), float("inf"), dtype=dt)
    lse2[:, :N] = lse * LOG2E
    P0 = torch.exp2(S * sc - lse2[:, :, None]).masked_fill(pad_key_mask(N, NP, mistake), 0.0)
    P0 = rnd_p0(P0)
    av = torch.zeros(G_, 5, NP, dtype=dt)                # a0 = 1, a1 .. a4; 0 for a padded query
    bv = torch.zeros(G_, 4, NP, dtype=dt)                # b0 = 1, b1 .. b3; 0 for a padded key
    av[:, 0, :N], bv[:, 0, :N] = 1.0, 1.0
    av[:, 1:, :N], bv[:, 1:, :N] = scal[:, 0::2], scal[:, 1::2]
    contracted = torch.ones(NP, dtype=torch.bool)        # the queries dK / dV contract over: both chunk slots, every 32-query step
    if mistake == "contract_full_tiles_only":
        contracted = row < 16 * (N // 16)
    elif mistake == "second_chunk_dropped":
        contracted = row < CH
    cq = contracted[None, :, None].to(dt)
    dOp = _pad_rows(dO, NP)
    P7 = rnd(P0 * bv[:, 3, None, :] * av[:, 4, :, None])
    dv = rnd((P7 * cq).transpose(-1, -2) @ dOp)[:, :N]
    Gm = _clamp_rows(dO, NP) @ _pad_rows(v, NP).transpose(-1, -2)
    for t in (3, 2, 1, 0):
        r = (P0 * Gm * bv[:, t, None, :]).sum(dim=-1) * av[:, t + 1]
        f = _ratio_or_zero(av[:, t + 1], av[:, t])
        Gm = Gm * f[:, :, None] - (r * f)[:, :, None]
        if t == 0:
            break
        c = (P0 * Gm * av[:, t, :, None]).sum(dim=-2)
        ratio = _ratio_or_zero(bv[:, t], bv[:, t - 1])
        Gm = Gm * ratio[:, None, :] - (c * bv[:, t] * ratio)[:, None, :]
    sd = (P0 * Gm).sum(dim=-1, keepdim=True)
    s_ = 1.0 if mistake == "ds_without_scale" else scale
    dS = rnd(P0 * (Gm * s_ - sd * s_))
    dq = rnd(dS @ _pad_rows(k_img, NP))[:, :N]
    dk = rnd((dS * cq).transpose(-1, -2) @ _pad_rows(q, NP))[:, :N]
    return dq, dk, dv


def stale_source(nheads: int, grid: int) -> torch.Tensor:
    """[nheads]: the head whose K image the stale-image mistake reads for head bh -- bh itself in passes 0 and 1, bh - 2 grid after"""
    bh = torch.arange(nheads)
    return torch.where(bh // grid >= 2, bh - 2 * grid, bh)


def restated(c: Case, mistake: Optional[str] = None, kernel_rounding: bool = False, cus: int = NOMINAL_CUS,
             dtype: torch.dtype = torch.float32) -> dict:
    """The kernel pair in plain torch (fp32) on the padded layout: P = diag(a) P0 diag(b) with the kernels' masks, the seven saved
    vectors, and the backward walk of the file header with its chunked contraction over queries.  Same result dict as `reference`.
    `kernel_rounding`: P0 resident as bf16 in the backward, and P7 (into P7 V and P7^T dO), dS and the bf16 outputs rounded to bf16.
    `mistake`: one of MISTAKES; `cus` gives the grids of the two launches to the one that needs them."""
    assert mistake is None or mistake in MISTAKES, mistake
    i = inputs(c)
    B, N, H, scale = c.B, c.N, c.H, c.scale
    NP, nheads = np_of(N), c.B * c.H
    q, k, v = (t.reshape(nheads, N, DH).to(dtype) for t in heads(i["qkv"], B, N, H, DH))
    dO = heads(i["dout"], B, N, H, DH)[0].reshape(nheads, N, DH).to(dtype)
    rnd = (lambda t: t.to(torch.bfloat16).to(dtype)) if kernel_rounding else (lambda t: t)
    rnd_p0 = (lambda t: t.to(torch.float16).to(dtype)) if mistake == "p0_fp16" else rnd
    gf, gb = grids(N, nheads, cus)
    kf = k[stale_source(nheads, gf)] if mistake == "stale_k_image" else k
    kb = k[stale_source(nheads, gb)] if mistake == "stale_k_image" else k
    out = {n: [] for n in ("o", "lse", "scal")}
    for h0 in range(0, nheads, REF_HEADS):
        s = slice(h0, h0 + REF_HEADS)
        for n, t in zip(("o", "lse", "scal"), _forward(q[s], kf[s], v[s], N, NP, scale, mistake, rnd)):
            out[n].append(t)
    res = {n: torch.cat(p) for n, p in out.items()}
    if mistake == "scal_stride_np":                      # head bh writes row r at bh 7 N + r NP; the heads in order; read back with stride N
        flat = torch.full((nheads * 7 * N + 7 * NP,), float("nan"), dtype=dtype)
        for bh in range(nheads):
            for r in range(7):
                flat[bh * 7 * N + r * NP: bh * 7 * N + r * NP + N] = res["scal"][bh, r]
        res["scal"] = flat[:nheads * 7 * N].reshape(nheads, 7, N).clone()
    if not c.fwd_only:
        out = {n: [] for n in ("dq", "dk", "dv")}
        for h0 in range(0, nheads, REF_HEADS):
            s = slice(h0, h0 + REF_HEADS)
            got = _backward(q[s], kb[s], v[s], dO[s], res["lse"][s], res["scal"][s], N, NP, scale, mistake, rnd, rnd_p0)
            for n, t in zip(("dq", "dk", "dv"), got):
                out[n].append(t)
        res.update({n: torch.cat(p) for n, p in out.items()})
    return {n: t.reshape((B, H) + tuple(t.shape[1:])) for n, t in res.items()}


# ---- the check --------------------------------------------------------------------------------------------------------------------
def _at(err: torch.Tensor, H: int, grid: Optional[int]) -> str:
    """where the largest entry of err [B, H, rows] sits"""
    flat = int(torch.argmax(torch.nan_to_num(err, nan=float("inf")).reshape(-1)))
    rows = err.shape[-1]
    bh, row = divmod(flat, rows)
    s = f"head {bh} (b {bh // H}, h {bh % H}) row {row}"
    return s + (f" pass {bh // grid}" if grid else "")


def check(c: Case, got: dict, ref: Optional[dict] = None, grid: Optional[dict] = None, where: Optional[dict] = None) -> dict:
    """error / bound of every tensor of `got` against the fp64 reference:
      dq, dk, dv   per-row relative L2 over PER_ROW_BOUND; no row is skipped, a reference row of norm zero gives inf
      o            max |err| of every row over O_BOUND x the tensor's maximum
      lse          |err| over LSE_TOL max(1, |lse|_max)
      scal         element-wise relative error of the seven saved vectors over SCAL_TOL
    N = 1: o must equal v and dv must equal dO bit for bit (else inf); dq and dk are exactly zero in the definition and a cancellation in
    fp32, bounded by ONE_KEY_STEPS x the one-key expression of attn_edges_ref.check, 2 dh 2^-24 |dO| |v| scale |k or q|.
    `grid`: {"fwd": .., "bwd": ..} for a walk case; `where` (a dict) receives, per tensor, the head, the row and the pass of the worst
    entry.  A tensor that is not finite everywhere gives inf."""
    ref = reference(c) if ref is None else ref
    i = inputs(c)
    grid = grid or {}
    names = ("o", "lse", "scal") + (() if c.fwd_only else ("dq", "dk", "dv"))
    out = {}

    def note(name, err, g):
        if where is not None:
            where[name] = _at(err, c.H, g)

    for name in names:
        g, r = got[name].detach().cpu().double(), ref[name]
        assert g.shape == r.shape, (name, g.shape, r.shape)
        gr = grid.get("fwd" if name in ("o", "lse", "scal") else "bwd")
        if not bool(torch.isfinite(g).all()):
            out[name] = float("inf")
            note(name, (~torch.isfinite(g)).double().reshape(c.B, c.H, -1), None)
            continue
        if name == "o":
            err = (g - r).abs().amax(dim=-1)
            out[name] = (err.max() / (O_BOUND * r.abs().max())).item()
        elif name == "lse":
            err = (g - r).abs()
            out[name] = (err.max() / (LSE_TOL * max(1.0, r.abs().max().item()))).item()
        elif name == "scal":
            err = ((g - r).abs() / r.abs()).amax(dim=-2)
            out[name] = err.max().item() / SCAL_TOL
        else:
            err = per_row_rel(g, r)
            out[name] = err.max().item() / PER_ROW_BOUND
        note(name, err, gr)
    if c.N == 1:
        q, k, v = heads(i["qkv"].double(), c.B, 1, c.H, DH)
        dO = heads(i["dout"].double(), c.B, 1, c.H, DH)[0]
        if not torch.equal(got["o"].detach().cpu().double(), v):
            out["o"] = float("inf")
        if not torch.equal(got["dv"].detach().cpu().double(), dO):
            out["dv"] = float("inf")
        for name, other in (("dq", k), ("dk", q)):
            assert bool((ref[name] == 0).all())
            g = got[name].detach().cpu().double()
            cancel = ONE_KEY_STEPS * 2 * DH * 2.0 ** -24 * dO.norm(dim=-1) * v.norm(dim=-1) * c.scale * other.norm(dim=-1)
            out[name] = (g.norm(dim=-1) / cancel).max().item() if bool(torch.isfinite(g).all()) else float("inf")
    return {n: (x if x == x else float("inf")) for n, x in out.items()}
