"""Softmax attention at its tile, mask-word and batch-sum edges: inputs, case lists, an fp64 reference and a plain restatement of the
kernels' index rules (test infrastructure, no kernels).  Builds on peaked_ref.py.

The kernels: csrc/nrv_attn.hip (single pass, dh 64, N <= 256, one instantiation per count NT of 16-key tiles) and
csrc/nrv_attn_gen.hip (streaming over 64-key tiles: KS = 1..4 for dh 32 / 64 / 80|96 / 128, KS = 5, 6 for the wide heads, and MEM = true
with memory keys behind the token keys and a bit mask of W = ceil(Nk / 32) words per query).

Whole-tensor checks on randn cannot see one wrong mask bit or one padding key in the softmax: either moves a row by ~ 1 / Nk of its
weight.  The builders here make such a mistake O(1) in the rows it touches:
  all-negative   every real key 8 nats down for every query (peaked_qkv, qc = 8): a zero padding key (score 0, v = 0) that is let
                 into the softmax takes most of the row
  loud keys      key j 8 nats ABOVE the rest for every query, at the positions {0, 31, 32, 63, 64, Nq-1, Nq, Nk-1} that exist (bit 31 /
                 bit 0 of a mask word, row 63 / row 0 of a key tile, the last token key, the first and the last memory key); the mask
                 removes them for even queries and admits them for odd ones
  structural     on a random 70 % mask: one fully masked query in the last (partial) 64-query tile, one query whose whole first 64-key
                 tile is masked, one whose whole last tile is masked, one with exactly two admitted keys
A query that admits the loud keys has nearly all its weight on two to eight keys, and its dq is a difference of a few large terms.  Two
things keep such rows well conditioned (both on the CPU, before any kernel: tests/test_attn_edges_ref_host.py): the queries' spread
across u is halved (LOUD_Q_SPREAD), and dO carries + v_j / - v_j of the loud keys (`_conditioned_dout`).  Without them the rounding of
o to bf16 alone, which the backward reads in delta = rowsum(dO o), moves one such dq row in ten by more than the GPU bound.
The reference applies the mask with masked_fill(-FLT_MAX) as learnable_memory_vit.py does, so a fully masked row is uniform over the
Nk keys and carries no score gradient.

Rows that are exactly zero in the definition must be exactly zero from a kernel (`check`): the dq row of a fully masked query and the
pad columns of a wide head.  One kind of zero row is a cancellation and not a structure: with ONE key, P = 1 and dS = P (dP - delta) =
dO.v - dO.o with o = v, two fp32 sums of the same dh products in different orders.  There (Nk = 1) dq and dk are bounded absolutely by
what those two sums can differ by: 2 dh 2^-24 |dO| |v| for dS, times scale |k| (dq) or scale |q| (dk).
"""
from __future__ import annotations

import functools
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

import peaked_ref as PR
from peaked_ref import EMULATION_BOUND, PER_ROW_BOUND, heads, per_row_rel  # noqa: F401  (re-exported for the two tests)

FLT_MAX = float(torch.finfo(torch.float32).max)
GT = 64                       # keys (queries) of a streamed tile
LOUD_Q_SPREAD = 0.5           # the loud builder halves the queries' component across u: the scores of two loud keys then differ by
                              # ~ N(0, 0.7) and not N(0, 1.4), so a row that admits them does not put everything on one of them
KERNEL_ROUNDING_BOUND = PER_ROW_BOUND / 2     # restated(kernel_rounding=True) against fp64, per row (host test): the other half of
                              # the GPU bound is for what the restatement leaves exact (fp32 sums, exp2, P rounded before it is normalised)
MEM_SUM_GROUP = 16            # samples per group of the shared-memory batch sum
NATS = 8.0                    # the all-negative keys are this far down, the loud keys this far up
LOUD_QC = 8.0                 # the loud builder's query offset along u (peaked_qkv's qc).  At 4 the loud keys carry twice the common
                              # component along u, the bf16 rounding of dS no longer cancels in it, and the emulated dq rows of the
                              # queries that admit them reach 1.28e-2 of fp64, over EMULATION_BOUND
LSE_TOL = 1e-4                # x max(1, |lse|_max): fp32 from bf16 operands (test_peaked_attn_gpu.py)
STREAM_DH = (32, 64, 80, 96, 128)
MASK_SHAPES = ("2d", "1h", "b1", "bh")          # [Nq,Nk], [1,H,Nq,Nk], [B,1,Nq,Nk], [B,H,Nq,Nk]
LAYOUT_ROWMAJOR, LAYOUT_BLOCKED = 0, 3          # include/nrv.h: 3 = NRV_ATTN_QKV_BLOCKED | NRV_ATTN_OUT_BLOCKED

# family: single | stream | wide | mem | sum;  width: the true head width (147 stored as 152, else dh);  mask: None or one of
# MASK_SHAPES;  build: "neg" | "loud" | "plain" (randn, nothing peaked: the batch sum without a mask, where every query would admit
# every loud key and the other keys' dk rows would be e^-8 of them);  entry: the C entry points that run it ("attn" | "mem" | "wide");
# layout: nrv_attn_* only
Case = namedtuple("Case", "family B Nq M H dh width shared mask build entry layout")


def single_pass_nt(N: int) -> int:
    """launch_fwd_fat / launch_bwd_fat: the instantiated count of 16-key tiles for N tokens."""
    nt = (N + 15) // 16
    return nt + (nt & 1) if nt <= 12 else (nt if nt in (13, 14) else 16)


def stream_ks(dh: int) -> int:
    """ks_of / wide_ks: 32-feature steps of the head dim (0: not a streaming head dim)."""
    if dh in STREAM_DH:
        return {32: 1, 64: 2, 80: 3, 96: 3, 128: 4}[dh]
    return 0 if (dh & 7) or dh <= 128 or dh > 192 else (5 if dh <= 160 else 6)


def _single_pass_ns():
    ns = {1}
    for NT in (2, 4, 6, 8, 10, 12, 13, 14, 16):
        ns |= {16 * NT, 16 * NT - 15}                       # no padding at all; one real key in the last tile
        if NT % 2 == 0 and NT != 14:
            ns |= {16 * (NT - 1), 16 * (NT - 2) + 1}        # the last tile all padding behind a full one / behind a one-key one
    return sorted(ns)


SINGLE_PASS_NS = _single_pass_ns()
SINGLE_PASS_CASES = tuple(Case("single", 2, N, 0, 2, 64, 64, True, None, "neg", "attn", lay)
                          for N in SINGLE_PASS_NS for lay in (LAYOUT_ROWMAJOR, LAYOUT_BLOCKED))
STREAM_CASES = tuple(Case("stream", 2, N, 0, 2, dh, dh, True, None, "neg", "mem", 0)
                     for dh in STREAM_DH for N in (1, 63, 64, 65, 129)) + (
    Case("stream", 2, 257, 0, 2, 64, 64, True, None, "neg", "attn", 0),)          # N > 256 at dh 64: nrv_attn_fwd's own dispatch
WIDE_CASES = tuple(Case("wide", 2, N, 0, 2, dh, 147 if dh == 152 else dh, True, None, "neg", "wide", 0)
                   for dh in (136, 152, 160, 168, 192) for N in (1, 64, 65, 129))
_MEM_SHAPES = ((17, 0), (33, 0), (31, 1), (32, 1), (63, 1), (64, 1), (60, 10), (65, 63), (90, 6), (70, 70))
MEM_CASES = tuple(Case("mem", 2, Nq, M, 2, STREAM_DH[i % 5], STREAM_DH[i % 5], i % 2 == 0, MASK_SHAPES[i % 4], "loud", "mem", 0)
                  for i, (Nq, M) in enumerate(_MEM_SHAPES))
SUM_CASES = tuple(Case("sum", B, 17, 3, 1, 32, 32, True, mask, "loud" if mask else "plain", "mem", 0)
                  for B in (16, 17, 35) for mask in ("b1", None)) + (
    Case("sum", 17, 17, 3, 1, 32, 32, False, "b1", "loud", "mem", 0),)
ALL_CASES = SINGLE_PASS_CASES + STREAM_CASES + WIDE_CASES + MEM_CASES + SUM_CASES


def _shape_key(c: Case):
    return (c.B, c.Nq, c.M, c.H, c.dh, c.shared, c.mask, c.build)


# "A case that does not stay inside gets other inputs, not another bound": the shapes whose first draw left a row outside
# EMULATION_BOUND (the reference's emulate_bf16 switch) or KERNEL_ROUNDING_BOUND (restated(kernel_rounding=True)) on the CPU, and the
# number of the draw that stays inside both.  tests/test_attn_edges_ref_host.py asserts both bounds for every case as drawn here.
RESEEDED = {
    (2, 17, 0, 2, 64, True, None, "neg"): 1,         # draw 0: a dq row at 1.5e-2 under kernel rounding
    (2, 65, 0, 2, 96, True, None, "neg"): 1,         # the same
    (16, 17, 3, 1, 32, True, "b1", "loud"): 1,
    (16, 17, 3, 1, 32, True, None, "plain"): 2,
    (35, 17, 3, 1, 32, True, "b1", "loud"): 47,      # 595 query rows and 595 key rows, every second one on two to four keys
    (35, 17, 3, 1, 32, True, None, "plain"): 1,
}


def case_id(c: Case) -> str:
    s = f"{c.family}-B{c.B}-N{c.Nq}"
    if c.M:
        s += f"+{c.M}{'s' if c.shared else 'p'}"
    s += f"-H{c.H}-dh{c.dh}"
    if c.mask:
        s += f"-{c.mask}"
    if c.family == "single":
        s += f"-NT{single_pass_nt(c.Nq)}-lay{c.layout}"
    elif c.entry == "attn":
        s += "-attn"
    return s


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def loud_positions(Nq: int, M: int):
    Nk = Nq + M
    return sorted({j for j in (0, 31, 32, 63, 64, Nq - 1, Nq, Nk - 1) if 0 <= j < Nk})


def structural_rows(Nq: int, Nk: int) -> dict:
    """query index of each structural row (absent where the shape has no such row: a first / last key tile needs a second tile, and a
    row keeps at least two admitted keys unless it is the fully masked one)."""
    t0 = GT * ((Nq - 1) // GT)
    rows = {"full": t0 + (Nq - 1 - t0) // 2, "two": 1}
    if Nk - GT >= 8:
        rows["first_tile"] = 3
    if Nk > GT:
        rows["last_tile"] = 6
    return rows


def two_keys(Nq: int, M: int):
    """the two keys that the two-key query admits: ordinary ones, the second as far back as the loud positions leave room"""
    loud = loud_positions(Nq, M)
    return [5, max(j for j in range(6, Nq + M - 1) if j not in loud)]


def build_mask(c: Case, seed: int) -> torch.Tensor:
    B, H, Nq, Nk = c.B, c.H, c.Nq, c.Nq + c.M
    shape = {"2d": (Nq, Nk), "1h": (1, H, Nq, Nk), "b1": (B, 1, Nq, Nk), "bh": (B, H, Nq, Nk)}[c.mask]
    m = torch.rand(shape, generator=torch.Generator().manual_seed(seed)) < 0.7
    odd = (torch.arange(Nq) % 2 == 1)
    for j in loud_positions(Nq, c.M):
        m[..., j] = odd
    rows = structural_rows(Nq, Nk)
    two = two_keys(Nq, c.M)
    assert len(set(rows.values())) == len(rows)
    if "first_tile" in rows:
        m[..., rows["first_tile"], :GT] = False
    if "last_tile" in rows:
        m[..., rows["last_tile"], GT * ((Nk - 1) // GT):] = False
    m[..., rows["two"], :] = False
    m[..., rows["two"], two] = True
    m[..., rows["full"], :] = False
    admitted = m.sum(dim=-1)
    assert bool(((admitted >= 2) | (admitted == 0)).all())           # one admitted key alone: dq is a cancellation, not a structure
    assert int((admitted == 0).sum()) == m.numel() // (Nq * Nk)      # the fully masked query, once per mask plane
    assert bool((m.sum(dim=-2) >= 1).all())                          # every key is seen by some query: no zero dk / dv row
    return m


def _pad_heads(t: torch.Tensor, parts: int, H: int, width: int, dh: int) -> torch.Tensor:
    out = torch.zeros(t.shape[0], parts * H, dh, dtype=t.dtype)
    out[..., :width] = t.reshape(t.shape[0], parts * H, width)
    return out.reshape(t.shape[0], parts * H * dh)


def _conditioned_dout(c: Case, qkv, mkv, dout) -> torch.Tensor:
    """A row that puts its weight on two or three keys has dS_j = P_j (dO.v_j - delta), a few scalars that a random dO leaves within
    the bf16 error of o in delta = rowsum(dO o) for about one row in ten (dq is then a cancellation: up to 0.4 relative from that
    rounding point alone, measured with `restated(kernel_rounding=True)`).  So every dO row gets + sum_j s_j v_j over the loud keys
    of its (batch, head), s_j = +1, -1, +1 .. in key order, and the two-key query's row + v_a - v_b of its two keys: dO.v_j then
    differs by ~ 2 dh between any two neighbouring loud keys.  The keys, the values and the mask stay as described above."""
    B, Nq, M, H, w = c.B, c.Nq, c.M, c.H, c.width
    v = heads(qkv.double(), B, Nq, H, w)[2]                                               # [B, H, Nq, w]
    if M > 0:
        mv = mkv.double().reshape(-1, M, 2, H, w)[:, :, 1].permute(0, 2, 1, 3)            # [(1 | B), H, M, w]
        v = torch.cat([v, mv.expand(B, -1, -1, -1)], dim=2)
    loud = loud_positions(Nq, M)
    sign = torch.tensor([(-1.0) ** i for i in range(len(loud))], dtype=torch.float64)
    add = (sign[:, None] * v[:, :, loud]).sum(dim=2, keepdim=True).expand(B, H, Nq, w).clone()
    if c.mask:
        a, b = two_keys(Nq, M)
        add[:, :, structural_rows(Nq, Nq + M)["two"]] = v[:, :, a] - v[:, :, b]
    d = heads(dout.double(), B, Nq, H, w)[0] + add
    return d.permute(0, 2, 1, 3).reshape(B * Nq, H * w).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _inputs(c: Case) -> dict:
    B, Nq, M, H, dh, w = c.B, c.Nq, c.M, c.H, c.dh, c.width
    seed = 1000 + 7 * Nq + 3 * M + dh + B + 100003 * RESEEDED.get(_shape_key(c), 0)
    scale = w ** -0.5
    g = torch.Generator().manual_seed(seed + 1)
    if c.build == "neg":
        qkv = PR.peaked_qkv(B, Nq, H, w, [(j, NATS) for j in range(Nq)], qc=8.0, seed=seed)
    elif c.build == "plain":
        qkv = PR.peaked_qkv(B, Nq, H, w, (), seed=seed)
    else:
        qkv = PR.peaked_qkv(B, Nq, H, w, [(j, -NATS) for j in loud_positions(Nq, M) if j < Nq], qc=LOUD_QC, seed=seed)
        x = qkv.double().reshape(B * Nq, 3, H, w)
        u = torch.full((w,), w ** -0.5, dtype=torch.float64)
        along = (x[:, 0] @ u)[..., None] * u
        x[:, 0] = along + LOUD_Q_SPREAD * (x[:, 0] - along)
        qkv = x.reshape(B * Nq, 3 * H * w).to(torch.bfloat16)
    dout = torch.randn(B * Nq, H * w, generator=g).to(torch.bfloat16)
    mkv = None
    if M > 0:
        Bm = 1 if c.shared else B
        x = torch.randn(Bm, M, 2, H, w, generator=g, dtype=torch.float64)
        u = torch.full((w,), w ** -0.5, dtype=torch.float64)
        x[:, :, 0] -= (x[:, :, 0] @ u)[..., None] * u
        for j in loud_positions(Nq, M):
            if j >= Nq and c.build == "loud":
                x[:, j - Nq, 0] += NATS / (scale * LOUD_QC) * u
        mkv = x.reshape(Bm * M, 2 * H * w).to(torch.bfloat16)
    if c.build == "loud":
        dout = _conditioned_dout(c, qkv, mkv, dout)
    if w != dh:                                                # the zero pad columns of an odd head width (147 stored as 152)
        qkv, dout = _pad_heads(qkv, 3, H, w, dh), _pad_heads(dout, 1, H, w, dh)
    mask = build_mask(c, seed + 2) if c.mask else None
    return {"qkv": qkv, "dout": dout, "mkv": mkv, "mask": mask, "scale": scale}


def inputs(c: Case) -> dict:
    """qkv bf16 [B*Nq, 3*H*dh], dout bf16 [B*Nq, H*dh], mkv bf16 [(1 | B)*M, 2*H*dh] or None, mask bool or None, scale.  Shared by
    every test of the case (and by both layouts of a single-pass case): do not modify."""
    return _inputs(c._replace(layout=0, entry="attn", family=""))


# ---- the mask words ---------------------------------------------------------------------------------------------------------------
def pack_bits(mask: torch.Tensor, Nq: int, Nk: int):
    """bool mask of one of MASK_SHAPES -> (int32 words [mb*mh*Nq, W], batch stride, head stride) as kernels.mask_pack lays them out:
    bit (key & 31) of word key >> 5, strides in words, 0 = broadcast."""
    m = mask.reshape((1,) * (4 - mask.dim()) + tuple(mask.shape)).numpy()
    mb, mh = m.shape[:2]
    W = (Nk + 31) // 32
    padded = np.zeros((mb, mh, Nq, W * 32), dtype=np.uint64)
    padded[..., :Nk] = m
    words = (padded.reshape(mb, mh, Nq, W, 32) << np.arange(32, dtype=np.uint64)).sum(axis=-1).astype(np.uint32)
    bits = torch.from_numpy(words.view(np.int32).reshape(mb * mh * Nq, W).copy())
    return bits, (mh * Nq * W if mb > 1 else 0), (Nq * W if mh > 1 else 0)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def attention_mem_reference(qkv, dout, B, Nq, H, dh, scale, *, mkv=None, M=0, shared=True, mask=None, dtype=torch.float64,
                            emulate_bf16=False) -> dict:
    """Softmax attention of the Nq token queries over the Nq token keys + M memory keys, by autograd in `dtype`: o, dq, dk, dv
    [B,H,Nq,dh], lse and `full` (every key masked) [B,H,Nq], dmem_k / dmem_v [(1 | B), H, M, dh] (summed over the batch when the
    memories are shared).  `mask`: bool, broadcastable to [B,H,Nq,Nk], applied with masked_fill(-FLT_MAX).  `emulate_bf16` as in
    peaked_ref.attention_reference: P, dS and the bf16 outputs (o, dq, dk, dv) are rounded to bf16, and nothing else."""
    x = qkv.detach().cpu().to(dtype).requires_grad_(True)
    q, k, v = heads(x, B, Nq, H, dh)
    mem = None
    if M > 0:
        mem = mkv.detach().cpu().to(dtype).requires_grad_(True)
        mk, mv = mem.reshape(-1, M, 2, H, dh).permute(2, 0, 3, 1, 4)
        k = torch.cat([k, mk.expand(B, -1, -1, -1)], dim=2)
        v = torch.cat([v, mv.expand(B, -1, -1, -1)], dim=2)
    S = (q @ k.transpose(-1, -2)) * scale
    if emulate_bf16:
        S = PR._RoundGrad.apply(S)
    full = torch.zeros(B, H, Nq, dtype=torch.bool)
    if mask is not None:
        keep = mask.detach().cpu().reshape((1,) * (4 - mask.dim()) + tuple(mask.shape)).expand(B, H, Nq, Nq + M)
        S = S.masked_fill(~keep, -FLT_MAX)
        full = ~keep.any(dim=-1)
    P = torch.softmax(S, dim=-1)
    o = (PR._round_st(P) if emulate_bf16 else P) @ v
    o.backward(heads(dout.detach().cpu().to(dtype), B, Nq, H, dh)[0])
    res = {"o": o.detach(), "lse": torch.logsumexp(S.detach(), dim=-1), "full": full}
    res["dq"], res["dk"], res["dv"] = heads(x.grad, B, Nq, H, dh)
    if M > 0:
        res["dmem_k"], res["dmem_v"] = mem.grad.reshape(-1, M, 2, H, dh).permute(2, 0, 3, 1, 4)
    if emulate_bf16:
        for name in ("o", "dq", "dk", "dv"):
            res[name] = res[name].to(torch.bfloat16).to(dtype)
    return res


@functools.lru_cache(maxsize=None)
def _reference(c: Case, emulate: bool) -> dict:
    i = inputs(c)
    return attention_mem_reference(i["qkv"], i["dout"], c.B, c.Nq, c.H, c.dh, i["scale"], mkv=i["mkv"], M=c.M, shared=c.shared,
                                   mask=i["mask"], emulate_bf16=emulate)


def reference(c: Case, emulate_bf16: bool = False) -> dict:
    """The fp64 reference of a case, computed once and shared: do not modify."""
    return _reference(c._replace(layout=0, entry="attn", family=""), emulate_bf16)


# ---- the kernels' index rules, restated -------------------------------------------------------------------------------------------
MISTAKES = ("mask_bit", "w1_past_W", "mem_row", "pad_le", "uniform_padded", "mask_bstride", "sum_remainder", "sum_pass2")


def _gather(flat: np.ndarray, idx: np.ndarray, beyond: int) -> np.ndarray:
    """flat[idx] with `beyond` for an index outside the buffer (what a restated mistake reads there is not defined)."""
    inside = (idx >= 0) & (idx < flat.size)
    return np.where(inside, flat[np.where(inside, idx, 0)], np.uint32(beyond))


def admitted_by_words(bits, bs, hs, B, H, Nq, Nk, mistake=None) -> torch.Tensor:
    """[B,H,Nq,Nkp] bool, Nkp = Nk rounded up to 64: mask_words + the bit test of the streaming kernels.  Per 64-key tile k0: w0 =
    word (k0 >> 5) of the query's row, w1 = the next one or 0 when there is none; key k0 + r reads bit r & 31 of w0 (r < 32) or w1."""
    W = (Nk + 31) // 32
    Nkp = GT * ((Nk + GT - 1) // GT)
    flat = bits.numpy().view(np.uint32).reshape(-1)
    if mistake == "mask_bstride" and bs == 0:
        bs = (H if hs else 1) * Nq * W                      # the stride of a mask that had a batch dimension
    b, h, q = np.meshgrid(np.arange(B), np.arange(H), np.arange(Nq), indexing="ij")
    row = b * bs + h * hs + q * W
    out = np.zeros((B, H, Nq, Nkp), dtype=bool)
    r = np.arange(32)
    shift = r + 1 if mistake == "mask_bit" else r
    for k0 in range(0, Nk, GT):
        wi = k0 >> 5
        w0 = _gather(flat, row + wi, 0)
        if wi + 1 < W:
            w1 = _gather(flat, row + wi + 1, 0)
        else:                                               # the mistake reads the next row's first word, or whatever lies past the buffer
            w1 = _gather(flat, row + wi + 1, 0xFFFFFFFF) if mistake == "w1_past_W" else np.zeros_like(w0)
        for half, w in enumerate((w0, w1)):
            bit = (w[..., None].astype(np.uint64) >> shift.astype(np.uint64)) & 1          # a shift by 32 leaves nothing
            out[..., k0 + 32 * half:k0 + 32 * half + 32] = bit.astype(bool)
    return torch.from_numpy(out)


def batch_sum_restated(dmem: torch.Tensor, mistake=None) -> torch.Tensor:
    """mem_batch_sum_kernel, two launches: groups of MEM_SUM_GROUP samples summed in place into each group's first sample, then the
    group leaders into the output.  dmem [B, ...] per sample -> [...]."""
    d = dmem.clone()
    B = d.shape[0]
    groups = (B + MEM_SUM_GROUP - 1) // MEM_SUM_GROUP
    if mistake == "sum_remainder":
        groups = B // MEM_SUM_GROUP
    for y in range(groups):
        first = y * MEM_SUM_GROUP
        n = min(MEM_SUM_GROUP, B - first)
        acc = d[first].clone()
        for j in range(1, n):
            acc = acc + d[first + j]
        d[first] = acc
    stride = 1 if mistake == "sum_pass2" else MEM_SUM_GROUP
    acc = d[0].clone()
    for j in range(1, groups):
        acc = acc + d[j * stride]
    return acc


def restated(c: Case, mistake: Optional[str] = None, kernel_rounding: bool = False) -> dict:
    """The streaming kernels' forward and backward written out in fp64 with their index rules -- key source (token row or memory
    row), mask word and bit, the padding test, the uniform weight of a fully masked row, the two-level batch sum -- and at most one
    of MISTAKES switched on.  Same result dict as attention_mem_reference.  The arithmetic is exact; only the indices are restated.
    `kernel_rounding`: the rounding points of `emulate_bf16` (P into P.V and into P^T dO, dS, the bf16 outputs) AND the one that
    switch does not have: delta = rowsum(dO o) is formed from the bf16 o, as the backward kernels read it."""
    assert mistake is None or mistake in MISTAKES, mistake
    i = inputs(c)
    B, Nq, M, H, dh, scale = c.B, c.Nq, c.M, c.H, c.dh, i["scale"]
    Nk = Nq + M
    Nkp = GT * ((Nk + GT - 1) // GT)
    q, k, v = heads(i["qkv"].double(), B, Nq, H, dh)
    dO = heads(i["dout"].double(), B, Nq, H, dh)[0]
    # key_row: key j < Nq is token row j, Nq <= j < Nk is memory row b * mstride + j - Nq, beyond: zero
    K = torch.zeros(B, H, Nkp + 1, dh, dtype=torch.float64)
    V = torch.zeros_like(K)
    K[:, :, :Nq], V[:, :, :Nq] = k, v
    if M > 0:
        rows = i["mkv"].double().reshape(-1, 2, H, dh)
        rows = torch.cat([rows, torch.zeros(1, 2, H, dh, dtype=torch.float64)])             # what lies past the buffer
        mstride = 0 if c.shared else M
        for b in range(B):
            for j in range(Nq, Nk):
                r = min(b * mstride + j - Nq + (1 if mistake == "mem_row" else 0), rows.shape[0] - 1)
                K[b, :, j], V[b, :, j] = rows[r, 0], rows[r, 1]
    K, V = K[:, :, :Nkp], V[:, :, :Nkp]
    if i["mask"] is not None:
        bits, bs, hs = pack_bits(i["mask"], Nq, Nk)
        keep = admitted_by_words(bits, bs, hs, B, H, Nq, Nk, mistake)
    else:
        keep = torch.ones(B, H, Nq, Nkp, dtype=torch.bool)
    key = torch.arange(Nkp)
    valid = (key <= Nk) if mistake == "pad_le" else (key < Nk)
    neg_inf = torch.tensor(float("-inf"), dtype=torch.float64)
    # forward: a masked score is -FLT_MAX, a padding key -inf; a row that keeps m = -FLT_MAX is fully masked
    raw = (q @ K.transpose(-1, -2)) * scale
    s = torch.where(keep, raw, torch.tensor(-FLT_MAX, dtype=torch.float64))
    s = torch.where(valid, s, torch.tensor(-FLT_MAX, dtype=torch.float64) if mistake == "uniform_padded" else neg_inf)
    m = s.amax(dim=-1, keepdim=True)
    p = torch.exp(s - m)
    l = p.sum(dim=-1, keepdim=True)
    rnd = (lambda t: t.to(torch.bfloat16).double()) if kernel_rounding else (lambda t: t)
    o = rnd(rnd(p / l) @ V)
    full = (m == -FLT_MAX)[..., 0]
    lse = torch.where(full, torch.tensor(-FLT_MAX, dtype=torch.float64), (m + torch.log(l))[..., 0])
    # backward: P from the saved lse; masked pairs carry no score gradient; a fully masked row has P = 1 / Nk and no gradient at all
    uni = 1.0 / (Nkp if mistake == "uniform_padded" else Nk)
    lse_b = torch.where(full, torch.tensor(float("inf"), dtype=torch.float64), lse)[..., None]
    P = torch.where(keep, torch.exp(raw - lse_b), (full.double() * uni)[..., None].expand_as(raw))
    P = torch.where(valid, P, torch.zeros((), dtype=torch.float64))
    delta = (dO * o).sum(dim=-1, keepdim=True)
    dS = rnd(torch.where(keep & valid, P * (dO @ V.transpose(-1, -2) - delta), torch.zeros((), dtype=torch.float64)))
    res = {"o": o, "lse": lse, "full": full, "dq": rnd(scale * dS @ K)}
    dK, dV = scale * dS.transpose(-1, -2) @ q, rnd(P).transpose(-1, -2) @ dO
    res["dk"], res["dv"] = rnd(dK[:, :, :Nq]), rnd(dV[:, :, :Nq])
    if M > 0:
        for name, t in (("dmem_k", dK), ("dmem_v", dV)):
            t = t[:, :, Nq:Nk]                                                              # per sample [B, H, M, dh]
            res[name] = batch_sum_restated(t, mistake)[None] if c.shared else t
    return res


# ---- the check --------------------------------------------------------------------------------------------------------------------
def gradient_names(c: Case):
    return ("dq", "dk", "dv") + (("dmem_k", "dmem_v") if c.M > 0 else ())


def check(c: Case, got: dict, ref: Optional[dict] = None) -> dict:
    """error / bound of every tensor of `got` (o, lse, dq, dk, dv [, dmem_k, dmem_v], shaped as the reference's) against the fp64
    reference: per-row relative L2 over PER_ROW_BOUND for o and every gradient row (no row is skipped; a reference row that is exactly
    zero must be exactly zero, else the ratio is inf -- see the module docstring for the one-key cancellation), |lse - ref| over
    LSE_TOL max(1, |lse|_max) on the rows that keep a key and exactly -FLT_MAX (else inf) on the fully masked ones."""
    ref = reference(c) if ref is None else ref
    i = inputs(c)
    out = {}
    for name in ("o",) + gradient_names(c):
        g, r = got[name].detach().cpu().double(), ref[name]
        assert g.shape == r.shape, (name, g.shape, r.shape)
        if not bool(torch.isfinite(g).all()):
            out[name] = float("inf")
            continue
        err = per_row_rel(g, r)
        if c.Nq + c.M == 1 and name in ("dq", "dk"):
            q, k, v = heads(i["qkv"].double(), c.B, c.Nq, c.H, c.dh)
            dO = heads(i["dout"].double(), c.B, c.Nq, c.H, c.dh)[0]
            assert bool((r == 0).all())
            cancel = 2 * c.dh * 2.0 ** -24 * dO.norm(dim=-1) * v.norm(dim=-1) * i["scale"] * (k if name == "dq" else q).norm(dim=-1)
            out[name] = (g.norm(dim=-1) / cancel).max().item()
            continue
        out[name] = err.max().item() / PER_ROW_BOUND
        if c.width != c.dh and bool((g[..., c.width:] != 0).any()):
            out[name] = float("inf")                                                          # a pad column of a wide head
    g, r, full = got["lse"].detach().cpu().double(), ref["lse"], ref["full"]
    assert g.shape == r.shape
    ratio = 0.0
    if bool((~full).any()):
        ratio = ((g - r).abs()[~full].max() / (LSE_TOL * max(1.0, r[~full].abs().max().item()))).item()
    if bool(full.any()) and not bool((g[full] == -FLT_MAX).all()):
        ratio = float("inf")
    out["lse"] = ratio if ratio == ratio else float("inf")
    return out
