"""The strided batched GEMM (csrc/nrv_bgemm.hip) per element: the case table, the fp64 reference, the bound, the inputs and an
fp32 emulation of the kernel's arithmetic.  tests/test_bgemm_ref_host.py holds the table against the real dispatch
(kernels.bgemm_plan) and proves the bound on the emulation; tests/test_bgemm_paths_gpu.py runs the table on the device.

The kernel computes  C[g1,g2] = alpha * A[g1,g2] . B[g1,g2]  with every operand addressed as
base + g1 * b1 + g2 * b2 + row * rs + col * cs (elements), operands rounded to bf16 when they are staged, bf16 MFMA with fp32
accumulation in K-steps of 32.  Its address paths: each operand is staged by 16-byte vectors or element by element
(`bg_vec_ok`), k-fast or row-fast, fp32 or bf16; two vector operands run `bg_loop_vec<AF32,BF32>` (register double buffer),
every other pairing runs `bg_stage`, whose vector branch has tail code of its own; C goes out as 4-column vector stores
(fp32 / bf16) or element by element.

Reference and bound.  ref = alpha * sum_k a_k b_k in fp64 on the bf16-rounded operands: the products are exact (8 x 8 mantissa
bits), so all the kernel can lose is the K - 1 fp32 additions and the product with alpha: K + 1 operations counted with K + 1,
each at most 2^-23 of the running sum of magnitudes, times the slack factor 2 of tests/rvt_ref.py:

    bound = 2 (K + 1) 2^-23 |alpha| sum_k |a_k b_k|          (+ 2^-8 |ref| for a bf16 output: one rounding of the fp32 value)

Nonzero operand magnitudes lie in [2^-6, 4]: no product is subnormal, nothing overflows.

Inputs.  Every operand lives in a flat storage larger than what it addresses, pre-filled with NaN; only the addressed elements
are written.  Gaps between rows and batches and the space behind the last element stay NaN, so a read outside the addressed
set poisons a result even when it is multiplied by a staged zero.  C's storage is pre-filled with one NaN bit pattern
(SENTINEL_F32 / SENTINEL_BF16) that every element the kernel must not write still has to hold afterwards.

    random    bf16 operands are bf16-exact; fp32 operands carry full mantissas (the rounding at staging matters)
    select_a  row m of A is one-hot (1.0) at k = (5 m + 3) mod K, B random, alpha = 0.5: C[m, n] = 0.5 bf16(B[k(m), n]) exactly
    select_b  column n of B is one-hot at k = (5 n + 3) mod K, A random, alpha = 0.5: C[m, n] = 0.5 bf16(A[m, k(n)]) exactly
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import Optional

import torch

BF16 = 2.0 ** -8
U32 = 2.0 ** -23
TILE, KSTEP = 64, 32                         # csrc/nrv_bgemm.hip BG_T, BG_K
SENTINEL_F32 = 0x7FC0BEEF                    # as int32: a quiet NaN with a payload no arithmetic produces
SENTINEL_BF16 = 0x7FC5                       # as int16
KINDS = ("random", "select_a", "select_b")
SELECT_ALPHA = 0.5
DIMS_MN = (1, 7, 64, 65, 71, 130)
DIMS_K = (1, 8, 31, 32, 33, 36, 40, 67, 97, 130)
FAKE_BASE = {"a": 0x10000000, "b": 0x20000000, "c": 0x30000000}        # allocation bases of the plan query's made-up addresses
TAIL_PAD = 37                                # NaN elements behind the last addressed one

# layout -> (dtype, staging the plan must report, fast direction); "rows" are m for A and n for B
LAYOUTS = {
    "L1": ("bf16", True, "k"),      # k unit, everything else even
    "L2": ("bf16", True, "row"),    # row unit, even k stride
    "L3": ("bf16", False, "k"),     # k unit, odd row stride
    "L4": ("bf16", False, "row"),   # row unit, odd k stride
    "L5": ("bf16", False, "k"),     # L1's strides, odd element offset
    "L6": ("bf16", False, "k"),     # L1's strides, odd b1 or b2
    "L7": ("f32", True, "k"),       # k unit, odd row stride: rows are only dword-aligned
    "L8": ("f32", True, "row"),     # row unit, odd k stride
    "L9": ("f32", False, None),     # no unit stride
    "L10": ("bf16", False, None),   # no unit stride
    "L11": ("bf16", False, "k"),    # K = 1, both strides 1: the s_row == 1 && s_k == 1 branch of bg_vec_ok
}
VECTOR_KINDS = ("L1", "L2", "L7", "L8")
# C form -> (dtype, c_vec the plan must report)
C_FORMS = {
    "f32_vec": ("f32", True),           # unit column stride: 16-byte stores at dword-aligned addresses
    "bf16_vec": ("bf16", True),         # unit column stride, even row / batch strides and offset: 8-byte stores
    "f32_T": ("f32", False),            # c_rs = 1, c_cs = ld: a transposed write
    "bf16_odd_rs": ("bf16", False),     # element stores forced by an odd row stride
    "bf16_odd_off": ("bf16", False),    # element stores forced by an odd element offset
}


@dataclass(frozen=True)
class Operand:
    layout: str                     # key of LAYOUTS (A, B) or C_FORMS (C)
    dtype: str                      # "bf16" | "f32"
    off: int                        # element offset of element (0, 0) of batch (0, 0) inside the storage
    strides: tuple                  # (rs, cs, b1, b2) in elements, as nrv_bgemm takes them (A [M, K], B [K, N], C [M, N])

    @property
    def torch_dtype(self):
        return torch.bfloat16 if self.dtype == "bf16" else torch.float32

    @property
    def vec(self) -> int:
        return 4 if self.dtype == "f32" else 8


@dataclass(frozen=True)
class Case:
    name: str
    edge: str                       # what this record is in the table for
    G1: int
    G2: int
    M: int
    N: int
    K: int
    alpha: float
    a: Operand
    b: Operand
    c: Operand
    plan: tuple                     # (a_vec, b_vec, c_vec, tiles_m, tiles_n) the dispatch must give
    real: Optional[str] = None      # the model call this record restates

    def dims(self, side):
        """(rows, cols) of the operand as a matrix"""
        return {"a": (self.M, self.K), "b": (self.K, self.N), "c": (self.M, self.N)}[side]

    def staging(self, side):
        """(s_row, s_k) of an input operand: the strides along the tile's rows (m / n) and along k"""
        rs, cs = getattr(self, side).strides[:2]
        return (rs, cs) if side == "a" else (cs, rs)

    def rows(self, side):
        return self.M if side == "a" else self.N

    @property
    def path(self):
        return "loop" if self.plan[0] and self.plan[1] else "stage"


def _ev(x):
    return x + (x & 1)


def _od(x):
    return x + 1 - (x & 1)


def _operand(layout, side, rows, K, G1, G2, bcast=False, odd="b2"):
    """An A (side "a", rows = M) or B (side "b", rows = N) operand in one of LAYOUTS, with gaps between rows and between batches."""
    dtype = LAYOUTS[layout][0]
    if layout in ("L1", "L5", "L6"):
        s_row, s_k, off = _ev(K + 2), 1, 2                 # off 2: a bf16 vector that is dword- but not 16-byte-aligned
        span = s_row * rows
    elif layout == "L2":
        s_row, s_k, off = 1, _ev(rows + 2), 6
        span = s_k * K
    elif layout in ("L3", "L7"):
        s_row, s_k, off = _od(K + 2), 1, 3 if layout == "L3" else 1
        span = s_row * rows
    elif layout in ("L4", "L8"):
        s_row, s_k, off = 1, _od(rows + 2), 4 if layout == "L4" else 3
        span = s_k * K
    elif layout == "L9":
        s_row, s_k, off = 2 * K + 3, 2, 2
        span = s_row * rows
    elif layout == "L10":
        s_row, s_k, off = 3, 3 * rows + 2, 4
        span = s_k * K
    elif layout == "L11":
        assert K == 1
        s_row, s_k, off = 1, 1, 2
        span = rows
    else:
        raise KeyError(layout)
    b2 = _ev(span + 6)
    b1 = _ev(b2 * G2 + 10)
    if bcast:                                              # one matrix per g1, shared by every g2
        b2, b1 = 0, _ev(span + 10)
    if layout == "L5":
        off = 5
    if layout == "L6":
        if odd == "b2":
            b2 += 1
        else:
            b1 += 1
    if layout in ("L3", "L4", "L9", "L10") and not bcast:  # nothing asks for even batch strides here: take odd ones
        b2, b1 = _od(b2), _od(b1 + 2)
    st = (s_row, s_k, b1, b2) if side == "a" else (s_k, s_row, b1, b2)
    return Operand(layout, dtype, off, st)


def _cform(form, M, N, G1, G2):
    dtype = C_FORMS[form][0]
    if form == "f32_vec":
        rs, cs, off = _od(N + 2), 1, 1                     # rows and base only dword-aligned
        span = rs * M
    elif form in ("bf16_vec", "bf16_odd_off"):
        rs, cs, off = _ev(N + 2), 1, 2 if form == "bf16_vec" else 3
        span = rs * M
    elif form == "bf16_odd_rs":
        rs, cs, off = _od(N + 2), 1, 2
        span = rs * M
    elif form == "f32_T":
        rs, cs, off = 1, M + 3, 2
        span = cs * N
    else:
        raise KeyError(form)
    b2 = _ev(span + 6)
    b1 = _ev(b2 * G2 + 10)
    if dtype == "f32":
        b2, b1 = _od(b2), _od(b1 + 2)
    return Operand(form, dtype, off, (rs, cs, b1, b2))


def _tiles(M, N):
    return (-(-M // TILE), -(-N // TILE))


def _case(name, edge, G, M, N, K, alpha, a, b, c, a_opt=None, b_opt=None):
    G1, G2 = G
    A = _operand(a, "a", M, K, G1, G2, **(a_opt or {}))
    B = _operand(b, "b", N, K, G1, G2, **(b_opt or {}))
    C = _cform(c, M, N, G1, G2)
    plan = (LAYOUTS[a][1], LAYOUTS[b][1], C_FORMS[c][1]) + _tiles(M, N)
    return Case(name, edge, G1, G2, M, N, K, alpha, A, B, C, plan)


def _real(name, edge, G, M, N, K, alpha, a, b, c, c_form):
    """A model call restated: a, b, c = (layout the strides realise, dtype, element offset, strides from the model's own helper)."""
    G1, G2 = G
    A, B = Operand(*a), Operand(*b)
    C = Operand(c_form, *c)
    plan = (LAYOUTS[A.layout][1], LAYOUTS[B.layout][1], C_FORMS[c_form][1]) + _tiles(M, N)
    return Case(name, edge, G1, G2, M, N, K, alpha, A, B, C, plan, real=name)


# the model call shapes at their smallest
REAL_B, REAL_H, REAL_N, REAL_DH = 2, 2, 67, 40            # composed Sinkhorn path: N odd (fp32 [N, N] rows dword-aligned), dh % 32 = 8
CAIT_N, CAIT_NK = 1, 17                                    # CaiT class attention: one query row, 1 + 16 keys, a bf16 A matrix
REAL_COMPOSED = ("S", "O", "dV", "dP", "dQ", "dK")
REAL_CAIT = ("S", "O", "dV", "dA", "dQ", "dK")


def _real_records():
    from noise_robust_vit_amd import cait
    from noise_robust_vit_amd.kernels import _composed_strides
    B, H, N, dh = REAL_B, REAL_H, REAL_N, REAL_DH
    scale = dh ** -0.5
    hq, hqT, ho, mat, matT = _composed_strides(N, H, dh)
    G = (B, H)
    v0 = 2 * H * dh
    recs = [
        # kernels.py _composed_scores / attn_composed_fwd / attn_composed_bwd
        _real("composed_S", "S = q k^T: both head slices k-fast, dh = 40 is one whole bf16 vector behind a full K-step; fp32 rows of 67",
              G, N, N, dh, scale, ("L1", "bf16", 0, hq), ("L1", "bf16", H * dh, hqT), ("f32", 0, mat), "f32_vec"),
        _real("composed_O", "O = P v: fp32 P with dword-aligned rows (K = 67: three K-steps, a 3-element tail) meets row-fast v",
              G, N, dh, N, 1.0, ("L7", "f32", 0, mat), ("L2", "bf16", v0, hq), ("bf16", 0, ho), "bf16_vec"),
        _real("composed_dV", "dV = P^T dO: fp32 row-fast staging, rows of 67 end in a 3-row tail",
              G, N, dh, N, 1.0, ("L8", "f32", 0, matT), ("L2", "bf16", 0, ho), ("bf16", v0, hq), "bf16_vec"),
        _real("composed_dP", "dP = dO v^T: the out-layout slice against a transposed head slice",
              G, N, N, dh, 1.0, ("L1", "bf16", 0, ho), ("L1", "bf16", v0, hqT), ("f32", 0, mat), "f32_vec"),
        _real("composed_dQ", "dQ = scale dS k", G, N, dh, N, scale, ("L7", "f32", 0, mat), ("L2", "bf16", H * dh, hq), ("bf16", 0, hq),
              "bf16_vec"),
        _real("composed_dK", "dK = scale dS^T q", G, N, dh, N, scale, ("L8", "f32", 0, matT), ("L2", "bf16", 0, hq),
              ("bf16", H * dh, hq), "bf16_vec"),
    ]
    n, Nk = CAIT_N, CAIT_NK
    inner = H * dh
    sq, skv, skvT, cm, cmT = cait._strides(n, Nk, H, dh)
    recs += [
        # cait.py LayerFn.forward / backward
        _real("cait_S", "CaiT S = q k^T with M = 1", G, n, Nk, dh, scale, ("L1", "bf16", 0, sq), ("L1", "bf16", 0, skvT), ("f32", 0, cm),
              "f32_vec"),
        _real("cait_O", "CaiT O = A v: the bf16 A has an odd row stride (Nk = 17) and stages by elements while v stages by vectors",
              G, n, dh, Nk, 1.0, ("L3", "bf16", 0, cm), ("L2", "bf16", inner, skv), ("bf16", 0, sq), "bf16_vec"),
        _real("cait_dV", "CaiT dV = A^T dO: K = 1, a row-unit bf16 A with an odd k stride", G, Nk, dh, n, 1.0, ("L4", "bf16", 0, cmT),
              ("L2", "bf16", 0, sq), ("bf16", inner, skv), "bf16_vec"),
        _real("cait_dA", "CaiT dA = dO v^T with M = 1", G, n, Nk, dh, 1.0, ("L1", "bf16", 0, sq), ("L1", "bf16", inner, skvT),
              ("f32", 0, cm), "f32_vec"),
        _real("cait_dQ", "CaiT dQ = scale dS k: M = 1, K = 17", G, n, dh, Nk, scale, ("L7", "f32", 0, cm), ("L2", "bf16", 0, skv),
              ("bf16", 0, sq), "bf16_vec"),
        _real("cait_dK", "CaiT dK = scale dS^T q: K = 1 through the double-buffered loop", G, Nk, dh, n, scale, ("L8", "f32", 0, cmT),
              ("L2", "bf16", 0, sq), ("bf16", 0, skv), "bf16_vec"),
    ]
    return recs


def _table():
    T = [
        # ---- bg_loop_vec: all four instantiations, every operand k-fast and row-fast in each dtype
        _case("loop_ff_rowfast_a", "<bf16,bf16> with a row-fast A: 65 rows = a 1-row tail behind a full tile; B k-fast over four K-steps "
              "with a 1-element tail", (1, 1), 65, 7, 97, 1.0, "L2", "L1", "f32_vec"),
        _case("loop_ft_k32", "<bf16,f32>: K = 32 exactly, no tail and no prefetch; fp32 B row-fast with 65 rows; N % 4 == 1 bf16 vector C",
              (1, 1), 64, 65, 32, -0.75, "L1", "L8", "bf16_vec"),
        _case("loop_tf_k32", "<f32,bf16>: K = 32 exactly; row-fast bf16 B with a 7-row tail", (1, 1), 7, 71, 32, 2.0, "L7", "L2", "bf16_vec"),
        _case("loop_ft_whole_tail", "<bf16,f32>: K = 40, a tail of whole vectors for the k-fast fp32 B; fp32 vector C with N % 4 == 0 across two batches",
              (1, 2), 71, 64, 40, 1.0, "L2", "L7", "f32_vec"),
        _case("loop_tt_k36", "<f32,f32>: K = 36, one whole fp32 vector behind a full K-step; row-fast A with 65 rows; 2 x 3 batches, all "
              "strides distinct", (2, 3), 65, 130, 36, 0.375, "L8", "L7", "f32_vec"),
        _case("loop_tt_k130", "<f32,f32>: K = 130, five K-steps and a 2-element tail; k-fast A, a single row-fast B column (N = 1)", (1, 1), 130, 1, 130, 1.0,
              "L7", "L8", "f32_T"),
        # ---- bg_stage's vector branch: each vector kind on each side against a scalar partner
        _case("mixed_a_L1", "vector A k-fast bf16: 65 rows, K = 33 (a 1-element tail)", (1, 1), 65, 7, 33, 1.0, "L1", "L5", "f32_vec"),
        _case("mixed_b_L1", "vector B k-fast bf16: K = 8, one whole vector and K < 32; A forced scalar by an odd b1", (2, 1), 7, 64, 8,
              1.5, "L6", "L1", "bf16_odd_rs", a_opt={"odd": "b1"}),
        _case("mixed_a_L2", "vector A row-fast bf16: 65 rows (a 1-row tail), K = 67", (1, 1), 65, 64, 67, 1.0, "L2", "L9", "f32_vec"),
        _case("mixed_b_L2", "vector B row-fast bf16: K = 40, a last K-step of 8", (1, 1), 7, 64, 40, 1.0, "L10", "L2", "bf16_vec"),
        _case("mixed_a_L7", "vector A k-fast fp32: K = 36, a whole-vector tail", (1, 2), 64, 7, 36, 1.0, "L7", "L3", "bf16_odd_off"),
        _case("mixed_b_L7", "vector B k-fast fp32: 65 rows, K = 97 (a 1-element tail)", (1, 1), 7, 65, 97, 1.0, "L4", "L7", "f32_vec"),
        _case("mixed_a_L8", "vector A row-fast fp32: K = 8, a single partial K-step", (1, 1), 64, 7, 8, 1.0, "L8", "L10", "bf16_vec"),
        _case("mixed_b_L8", "vector B row-fast fp32: 65 rows (a 1-row tail), K = 31 < 32", (1, 1), 7, 65, 31, 1.0, "L9", "L8", "f32_vec"),
        # ---- both operands element by element
        _case("scalar_L3_L4", "odd row stride x odd k stride; bf16 C forced to element stores by an odd row stride; a broadcast B (b2 = 0)",
              (2, 2), 65, 71, 33, 1.0, "L3", "L4", "bf16_odd_rs", b_opt={"bcast": True}),
        _case("scalar_L9_L10", "no unit stride on either side; a transposed fp32 write (c_rs = 1) across 2 x 1 batches", (2, 1), 71, 65, 31, 1.0, "L9", "L10",
              "f32_T"),
        _case("scalar_L5_L6", "an odd offset x an odd b2; bf16 C at an odd offset", (1, 2), 64, 71, 67, 1.0, "L5", "L6", "bf16_odd_off"),
        _case("outer_product", "K = 1 with both strides 1 on both operands", (1, 1), 71, 65, 1, 1.0, "L11", "L11", "f32_vec"),
        # ---- the workgroup index decomposition
        _case("grid_3x2_batched", "M = 130, N = 70: tiles_m = 3 != tiles_n = 2 under 2 x 2 batches", (2, 2), 130, 70, 33, 1.0, "L1", "L2",
              "bf16_vec"),
    ]
    return tuple(T + _real_records())


TABLE = _table()
BY_NAME = {c.name: c for c in TABLE}
assert len(BY_NAME) == len(TABLE)


# ----------------------------------------------------------------------------------------------
# what the table has to cover (tests/test_bgemm_ref_host.py asserts coverage_gaps(TABLE) == [] and that no record is spare)
# ----------------------------------------------------------------------------------------------
def layout_holds(case: Case, side: str) -> bool:
    """Do the operand's dtype, offset and strides realise the layout its record names?"""
    op = getattr(case, side)
    s_row, s_k = case.staging(side)
    b1, b2 = op.strides[2:]
    even = lambda *v: all(x % 2 == 0 for x in v)      # noqa: E731
    L = op.layout
    bf = op.dtype == "bf16"
    if L == "L1":
        return bf and s_k == 1 and s_row != 1 and even(s_row, b1, b2, op.off)
    if L == "L2":
        return bf and s_row == 1 and s_k != 1 and even(s_k, b1, b2, op.off)
    if L == "L3":
        return bf and s_k == 1 and s_row % 2 == 1 and s_row != 1
    if L == "L4":
        return bf and s_row == 1 and s_k % 2 == 1 and s_k != 1
    if L == "L5":
        return bf and s_k == 1 and s_row != 1 and even(s_row, b1, b2) and op.off % 2 == 1
    if L == "L6":
        return bf and s_k == 1 and s_row != 1 and even(s_row, op.off) and (b1 % 2 == 1 or b2 % 2 == 1)
    if L == "L7":
        return not bf and s_k == 1 and s_row % 2 == 1 and s_row != 1
    if L == "L8":
        return not bf and s_row == 1 and s_k % 2 == 1 and s_k != 1
    if L == "L9":
        return not bf and s_row != 1 and s_k != 1
    if L == "L10":
        return bf and s_row != 1 and s_k != 1
    if L == "L11":
        return case.K == 1 and s_row == 1 and s_k == 1
    return False


def cform_holds(case: Case) -> bool:
    c = case.c
    rs, cs, b1, b2 = c.strides
    f = c.layout
    if f == "f32_vec":
        return c.dtype == "f32" and cs == 1
    if f == "bf16_vec":
        return c.dtype == "bf16" and cs == 1 and all(x % 2 == 0 for x in (rs, b1, b2, c.off))
    if f == "f32_T":
        return c.dtype == "f32" and rs == 1 and cs != 1
    if f == "bf16_odd_rs":
        return c.dtype == "bf16" and cs == 1 and rs % 2 == 1 and c.off % 2 == 0
    if f == "bf16_odd_off":
        return c.dtype == "bf16" and cs == 1 and c.off % 2 == 1 and all(x % 2 == 0 for x in (rs, b1, b2))
    return False


def _has_gaps(case: Case, side: str) -> bool:
    """gaps between the rows (along the slow matrix direction) and between the batches of an operand; a record without a second
    batch has no gap between batches"""
    op = getattr(case, side)
    rows, cols = case.dims(side)
    rs, cs, b1, b2 = op.strides
    (fast_n, fast_s), (slow_n, slow_s) = sorted(((rows, rs), (cols, cs)), key=lambda t: t[1])
    row_gap = slow_n == 1 or slow_s > (fast_n - 1) * fast_s + 1
    span = (rows - 1) * rs + (cols - 1) * cs + 1
    levels = [(g, b) for g, b in ((case.G1, b1), (case.G2, b2)) if g > 1]
    return row_gap and bool(levels) and all(b > span for _, b in levels)          # at least one batch level really steps over a gap


def select_hits_both_ends(case: Case, side: str) -> bool:
    """does the one-hot index (5 r + 3) mod K reach 0 and K - 1 over the operand's rows?"""
    ks = {(5 * r + 3) % case.K for r in range(case.rows(side))}
    return 0 in ks and case.K - 1 in ks


def _edges(case: Case, side: str):
    """the dimension edges a vector staging kind sees in this record"""
    op = getattr(case, side)
    K, rows, V = case.K, case.rows(side), op.vec
    e = set()
    kfast = LAYOUTS[op.layout][2] == "k"
    if kfast and K % V:                                    # the vector runs along k: the tail code of the vector itself
        e.add("a K tail shorter than the vector")
    if kfast and K % KSTEP and K % V == 0:
        e.add("a K tail of whole vectors only")
    if not kfast and K % KSTEP:                            # the vector runs along the rows: K only decides which k of the step exist
        e.add("a partial last K-step")
    if rows % TILE == 1:
        e.add("rows % 64 == 1")
    if LAYOUTS[op.layout][2] == "row" and rows % V:
        e.add("a row tail shorter than the vector")
    if case.path == "loop":
        if K % KSTEP == 0:
            e.add("K % 32 == 0")
        if K > 2 * KSTEP:
            e.add("at least three K steps")
    return e


def conditions(table):
    """{condition: [names of the records that carry it]} for everything the table must cover."""
    cond = {}

    def need(key, names):
        cond[key] = list(names)

    sides = ("a", "b")
    for L in LAYOUTS:
        for s in sides:
            need(f"layout {L} as operand {s.upper()}", [c.name for c in table if getattr(c, s).layout == L])
    for af in ("bf16", "f32"):
        for bf in ("bf16", "f32"):
            need(f"bg_loop_vec<{af},{bf}>", [c.name for c in table if c.path == "loop" and (c.a.dtype, c.b.dtype) == (af, bf)])
    for L in VECTOR_KINDS:
        for s in sides:
            o = "b" if s == "a" else "a"
            need(f"loop path with {L} as operand {s.upper()}", [c.name for c in table if c.path == "loop" and getattr(c, s).layout == L])
            need(f"mixed pairing: vector {L} as operand {s.upper()} against a scalar partner",
                 [c.name for c in table if getattr(c, s).layout == L and not LAYOUTS[getattr(c, o).layout][1]])
        if LAYOUTS[L][2] == "k":
            all_edges = ["a K tail shorter than the vector", "a K tail of whole vectors only", "rows % 64 == 1"]
        else:
            all_edges = ["a partial last K-step", "a row tail shorter than the vector", "rows % 64 == 1"]
        for path in ("loop", "stage"):
            for e in all_edges + (["K % 32 == 0", "at least three K steps"] if path == "loop" else []):
                need(f"{L} in the {path} path sees {e}",
                     [c.name for c in table for s in sides if c.path == path and getattr(c, s).layout == L and e in _edges(c, s)])
        need(f"a one-hot {L} operand reaches k = 0 and k = K - 1",
             [c.name for c in table for s in sides if getattr(c, s).layout == L and select_hits_both_ends(c, s)])
    for x, y in (("L3", "L4"), ("L9", "L10"), ("L5", "L6")):
        need(f"both-scalar pairing {x} x {y}", [c.name for c in table if (c.a.layout, c.b.layout) == (x, y)])
    need("L6 by an odd b1", [c.name for c in table for s in sides if getattr(c, s).layout == "L6" and getattr(c, s).strides[2] % 2])
    need("L6 by an odd b2", [c.name for c in table for s in sides if getattr(c, s).layout == "L6" and getattr(c, s).strides[3] % 2])
    need("K < 32", [c.name for c in table if c.K < KSTEP])
    need("fp32 vector C store with N % 4 != 0", [c.name for c in table if c.c.layout == "f32_vec" and c.N % 4 and _has_gaps(c, "c")])
    need("fp32 vector C store with N % 4 == 0", [c.name for c in table if c.c.layout == "f32_vec" and c.N % 4 == 0 and _has_gaps(c, "c")])
    need("bf16 vector C store with N % 4 != 0", [c.name for c in table if c.c.layout == "bf16_vec" and c.N % 4 and _has_gaps(c, "c")])
    for f in ("f32_T", "bf16_odd_rs", "bf16_odd_off"):
        need(f"C form {f} with gaps", [c.name for c in table if c.c.layout == f and _has_gaps(c, "c")])
    need("G1 x G2 = 2 x 3 with all batch strides distinct",
         [c.name for c in table if (c.G1, c.G2) == (2, 3) and len({x for o in (c.a, c.b, c.c) for x in o.strides[2:]}) == 6])
    need("a broadcast operand (b2 = 0)", [c.name for c in table if c.G2 > 1 and 0 in (c.a.strides[3], c.b.strides[3])])
    need("tiles_m = 3 != tiles_n = 2 with G1, G2 > 1",
         [c.name for c in table if (c.M, c.N) == (130, 70) and c.plan[3:] == (3, 2) and c.G1 > 1 and c.G2 > 1])
    for v in DIMS_MN:
        need(f"M = {v}", [c.name for c in table if c.M == v])
        need(f"N = {v}", [c.name for c in table if c.N == v])
    for v in DIMS_K:
        need(f"K = {v}", [c.name for c in table if c.K == v])
    for fam, names in (("composed", REAL_COMPOSED), ("cait", REAL_CAIT)):
        for p in names:
            need(f"the model call {fam}_{p}", [c.name for c in table if c.real == f"{fam}_{p}"])
    return cond


def coverage_gaps(table):
    return [k for k, names in conditions(table).items() if not names]


# ----------------------------------------------------------------------------------------------
# inputs, reference, bound
# ----------------------------------------------------------------------------------------------
def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def index(case: Case, side: str) -> torch.Tensor:
    """int64 [G1, G2, rows, cols]: the storage element every matrix element lives in"""
    op = getattr(case, side)
    rows, cols = case.dims(side)
    rs, cs, b1, b2 = op.strides
    ar = torch.arange
    return (op.off + ar(case.G1)[:, None, None, None] * b1 + ar(case.G2)[None, :, None, None] * b2
            + ar(rows)[None, None, :, None] * rs + ar(cols)[None, None, None, :] * cs)


def numel(case: Case, side: str) -> int:
    return int(index(case, side).max()) + 1 + TAIL_PAD


def fake_address(case: Case, side: str) -> int:
    op = getattr(case, side)
    return FAKE_BASE[side] + op.off * (2 if op.dtype == "bf16" else 4)


def sentinel_storage(case: Case) -> torch.Tensor:
    n = numel(case, "c")
    if case.c.dtype == "f32":
        return torch.full((n,), SENTINEL_F32, dtype=torch.int32).view(torch.float32)
    return torch.full((n,), SENTINEL_BF16, dtype=torch.int16).view(torch.bfloat16)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _random_flat(n, dtype, gen):
    """magnitudes 2^u, u uniform in [-6, 2), random signs; bf16 storages hold bf16-exact values, fp32 ones full mantissas"""
    mag = torch.exp2(torch.rand(n, generator=gen, dtype=torch.float64) * 8.0 - 6.0)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    return (mag * sign).float().to(dtype)


def _one_hot(case: Case, side: str) -> torch.Tensor:
    rows, K = case.rows(side), case.K
    m = torch.zeros(rows, K)
    m[torch.arange(rows), (5 * torch.arange(rows) + 3) % K] = 1.0
    m = m if side == "a" else m.t()
    return m.expand(case.G1, case.G2, *m.shape)


@dataclass
class Inputs:
    case: Case
    kind: str
    alpha: float
    a: torch.Tensor                 # flat storages, NaN outside the addressed sets
    b: torch.Tensor
    ia: torch.Tensor                # index() of A, B, C
    ib: torch.Tensor
    ic: torch.Tensor
    ref: torch.Tensor               # fp64 [G1, G2, M, N]
    bound: torch.Tensor
    exact: Optional[torch.Tensor]   # select kinds: the result every addressed element must equal (C's dtype)


@functools.lru_cache(maxsize=None)
def inputs(name: str, kind: str) -> Inputs:
    case = BY_NAME[name]
    gen = _gen("bgemm", name, kind)
    stores, idx = {}, {}
    for side in ("a", "b"):
        op = getattr(case, side)
        ix = index(case, side)
        n = int(ix.max()) + 1 + TAIL_PAD
        vals = _random_flat(n, op.torch_dtype, gen)
        st = torch.full((n,), float("nan"), dtype=op.torch_dtype)
        if kind == "select_" + side:
            st[ix.reshape(-1)] = _one_hot(case, side).reshape(-1).to(op.torch_dtype)
        else:
            st[ix.reshape(-1)] = vals[ix.reshape(-1)]
        stores[side], idx[side] = st, ix
    alpha = case.alpha if kind == "random" else SELECT_ALPHA
    a = stores["a"][idx["a"]].to(torch.bfloat16).double()          # round-to-nearest-even, as f32_to_bf16 on staging
    b = stores["b"][idx["b"]].to(torch.bfloat16).double()
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    ref = alpha * (a @ b)
    bound = 2 * (case.K + 1) * U32 * abs(alpha) * (a.abs() @ b.abs())
    if case.c.dtype == "bf16":
        bound = bound + BF16 * ref.abs()
    exact = None
    if kind != "random":
        exact = ref.to(case.c.torch_dtype)
        assert torch.equal(exact.double(), ref)                    # a scaled copy of one bf16 value: representable in both types
    return Inputs(case, kind, alpha, stores["a"], stores["b"], idx["a"], idx["b"], index(case, "c"), ref, bound, exact)


def ratio(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """max over the elements of |got - ref| / bound (0 / 0 counts as 0); a non-finite result counts as inf."""
    got, ref, bound = got.detach().double().cpu(), ref.double().cpu(), bound.double().cpu()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def unwritten(case: Case, storage: torch.Tensor, ic: torch.Tensor) -> torch.Tensor:
    """bit patterns of every element of C's storage that no (g1, g2, m, n) addresses"""
    mask = torch.ones(storage.numel(), dtype=torch.bool)
    mask[ic.reshape(-1)] = False
    return bits(storage.cpu())[mask]


def sentinel_bits(case: Case) -> int:
    return SENTINEL_F32 if case.c.dtype == "f32" else SENTINEL_BF16


# ----------------------------------------------------------------------------------------------
# the kernel's arithmetic in fp32, with the mutations the host test seeds
# ----------------------------------------------------------------------------------------------
MUTATIONS = ("drop_last_k", "zero_row_tail", "swap_tiles", "moat")


def emulate(inp: Inputs, mutate: Optional[str] = None) -> torch.Tensor:
    """C's storage as the kernel leaves it: operands rounded to bf16, fp32 accumulation in K-steps of 32 with k ascending inside a
    step, the product with alpha, one rounding for a bf16 output, written tile by tile in the kernel's workgroup order.
    `mutate` (a wrong kernel, for the host test):
      drop_last_k    the K loop stops one k early
      zero_row_tail  a row-fast vector operand stages zeros for a row tail shorter than its vector
      swap_tiles     the workgroup index is decomposed with tiles_m and tiles_n exchanged
      moat           A's element (row 0, k = K) of every batch is read from memory although the matrix ends at K - 1; it meets
                     the zero B stages there"""
    case = inp.case
    G1, G2, M, N, K = case.G1, case.G2, case.M, case.N, case.K
    a = inp.a[inp.ia].to(torch.bfloat16).float()
    b = inp.b[inp.ib].to(torch.bfloat16).float()
    if mutate == "zero_row_tail":
        for side, t in (("a", a), ("b", b)):
            op = getattr(case, side)
            rows = case.rows(side)
            if LAYOUTS[op.layout][1] and LAYOUTS[op.layout][2] == "row" and rows % op.vec:
                if side == "a":
                    t[:, :, rows - rows % op.vec:, :] = 0.0
                else:
                    t[:, :, :, rows - rows % op.vec:] = 0.0
    kend = K - 1 if mutate == "drop_last_k" else K
    acc = torch.zeros(G1, G2, M, N, dtype=torch.float32)
    for k0 in range(0, K, KSTEP):
        for k in range(k0, min(k0 + KSTEP, kend)):
            acc = acc + a[:, :, :, k, None] * b[:, :, k, None, :]            # bf16 x bf16 is exact in fp32; one rounding per addition
    if mutate == "moat" and K % KSTEP:
        rs, cs = case.a.strides[:2]
        stray = inp.a[inp.ia[:, :, 0, 0] + K * cs].float()                    # [G1, G2]; the storage's tail pad keeps the index inside
        acc[:, :, 0, :] = acc[:, :, 0, :] + (stray * 0.0)[:, :, None]
    out = (acc * torch.tensor(inp.alpha, dtype=torch.float32)).to(case.c.torch_dtype)
    store = sentinel_storage(case)
    tm_n, tn_n = _tiles(M, N)
    if mutate == "swap_tiles":
        tm_n, tn_n = tn_n, tm_n
    for bid in range(G1 * G2 * tm_n * tn_n):
        tn, r = bid % tn_n, bid // tn_n
        tm, r = r % tm_n, r // tm_n
        g2, g1 = r % G2, r // G2
        m0, n0 = tm * TILE, tn * TILE
        if m0 >= M or n0 >= N:
            continue
        ix = inp.ic[g1, g2, m0:m0 + TILE, n0:n0 + TILE]
        store[ix.reshape(-1)] = out[g1, g2, m0:m0 + TILE, n0:n0 + TILE].reshape(-1)
    return store
