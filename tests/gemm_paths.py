"""The tile / kernel / epilogue variants of the NT and TN GEMMs, and the small shapes at which the tests reach each of them.

`nrv_gemm_nt_bf16` picks one of five tile configurations (Cfg256, Cfg320, Cfg192, Cfg128: 256 / 320 / 192 / 128 rows x 256
columns; Cfg384n: 384 x 128) and one of two kernels (gemm_nt8_kernel: phased K loop, persistent, workgroup b walks the tiles
b, b + grid, ...; gemm_nt_kernel: plain, one tile per workgroup) from the shape and the CUs it plans for.  At the 256 CUs of the
device only workload-sized operands reach most of the ten pairs.  Planned for 8 CUs (`nrv_set_reserved_cus(CUs - 8)`) the same
cost model picks every tile height at M <= 3100, N <= 600, and the persistent grid is 8 workgroups that walk two or three
tiles each.  `nrv_gemm_nt_plan` / `nrv_gemm_tn_plan` (include/nrv.h) answer what a launch would do; test_gemm_paths_host.py
asserts every record's plan with them, test_gemm_paths_gpu.py asserts it again on the device and then runs the record.

One record per variant under test:

    cus     the CUs the launch is planned for (the tests reserve the device's CUs minus this many)
    shape   (M, N, K) or (M, N, T)
    plan    what the query must answer: the record is only worth anything while it does

Every NT record: M is no multiple of the tile height and N no multiple of the tile width (ragged last tile row and column),
N % 8 == 0, three column tiles.  Each (tile, kernel) pair has two records: one with N % 64 != 0 (the last column tile holds
8 columns: one 16-byte chunk of a wave's first 64-column slab) and one with N % 64 == 0 for the 8-bit gelu' stream (N = 576:
a last 256-column tile of 64; N = 320 on 384 x 128: a last 128-column tile of 64, so the row-pair blocks of 64 columns end
inside a tile).  Plain records take K = 72 or 136 (a partial last K-step) and K = 128 (two whole K-steps, below the phased
minimum); phased records K = 192 (the minimum: the prologue's 1.5 K-steps meet the two peeled ones) and 256 or 320.  Phased
records have tiles > grid and tiles % grid != 0, so workgroups walk unequal tile counts; `passes` = tiles / planned CUs is
>= launch_paths.MIN_PASSES = 2.25 except for Cfg128: the cost model leaves the 128-row tile as soon as a taller one needs
no more rounds, and 15 tiles on 8 workgroups (1.875) is the most it takes at 8, 16 or 24 planned CUs.  The plain kernel has no
walk; its records keep the same tile counts so that the column-group tile order (groups of 4 tile columns) is the same.

A new tile configuration gets its records here first ("GEMM variant table"): the host test's coverage assertion
lists the (tile, kernel) pairs and fails until the table has both kinds of record for the new pair.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

MIN_PASSES = 2.25            # launch_paths.MIN_PASSES: two full walks of the grid and a quarter of a third

NT_TILES = ((256, 256), (320, 256), (192, 256), (128, 256), (384, 128))


@dataclass(frozen=True)
class NtPath:
    name: str
    cus: int
    M: int
    N: int
    K: int
    tile_m: int
    tile_n: int
    phased: bool
    tiles: int
    grid: int

    @property
    def plan(self) -> dict:
        return {"tile_m": self.tile_m, "tile_n": self.tile_n, "phased": self.phased, "tiles": self.tiles, "grid": self.grid}

    @property
    def passes(self) -> float:          # tiles per planned CU: the walk length of the phased kernel's busiest workgroups
        return self.tiles / self.cus

    @property
    def q8(self) -> bool:               # the 8-bit gelu' stream needs N % 64 == 0
        return self.N % 64 == 0

    @property
    def tiles_n(self) -> int:
        return -(-self.N // self.tile_n)


def _nt(M, N, K, tile_m, tile_n, phased, tiles, cus=8):
    kern = "phased" if phased else "plain"
    grid = min(tiles, cus) if phased else tiles
    return NtPath(f"{tile_m}x{tile_n}_{kern}_n{N}_k{K}", cus, M, N, K, tile_m, tile_n, phased, tiles, grid)


NT_TABLE: Tuple[NtPath, ...] = (
    #    M     N    K   tile      phased tiles         tiles / 8 CUs
    _nt(961, 520, 136, 128, 256, False, 24),         # 3.0
    _nt(961, 576, 128, 128, 256, False, 24),
    _nt(513, 520, 192, 128, 256, True, 15),          # 1.875: the most Cfg128 takes (module docstring)
    _nt(513, 576, 256, 128, 256, True, 15),
    _nt(1281, 520, 72, 192, 256, False, 21),         # 2.625
    _nt(1281, 576, 128, 192, 256, False, 21),
    _nt(1281, 520, 192, 192, 256, True, 21),
    _nt(1281, 576, 320, 192, 256, True, 21),
    _nt(1601, 520, 136, 256, 256, False, 21),        # 2.625
    _nt(1601, 576, 128, 256, 256, False, 21),
    _nt(1601, 520, 192, 256, 256, True, 21),
    _nt(1601, 576, 256, 256, 256, True, 21),
    _nt(2305, 520, 136, 320, 256, False, 24),        # 3.0
    _nt(2305, 576, 128, 320, 256, False, 24),
    _nt(3073, 392, 192, 320, 256, True, 20),         # 2.5
    _nt(3073, 448, 320, 320, 256, True, 20),
    _nt(2561, 264, 72, 384, 128, False, 21),         # 2.625
    _nt(2561, 320, 128, 384, 128, False, 21),
    _nt(2561, 264, 192, 384, 128, True, 21),
    _nt(2561, 320, 256, 384, 128, True, 21),
)

# Cfg128 on the phased kernel cannot reach MIN_PASSES (module docstring); every other phased record must
SHORT_WALK = {"128x256_phased_n520_k192": 1.875, "128x256_phased_n576_k256": 1.875}


@dataclass(frozen=True)
class TnPath:
    name: str
    cus: int
    M: int
    N: int
    T: int
    a_group: int        # 0, or the group size of the row remap of A (stride a_group + 1, offset 1: a class-token slot)
    beta: float
    dbias: bool
    ldc_pad: int        # the GPU test's C has leading dimension N + ldc_pad
    tiles: int
    splits: int
    kt_q: int
    kt_r: int
    phased: bool
    direct: bool
    reduce: bool

    @property
    def plan(self) -> dict:
        return {"tiles": self.tiles, "splits": self.splits, "kt_q": self.kt_q, "kt_r": self.kt_r, "phased": self.phased,
                "direct": self.direct, "reduce": self.reduce}


# 8 planned CUs: splits = 8 // tiles, so 5 tiles or more make a one-split plan without workload-sized T
TN_TABLE: Tuple[TnPath, ...] = (
    # phased + direct: the kernel stores into the caller's C (ldc > N); with dbias the reduction kernel runs for the sums alone
    TnPath("phased_direct", 8, 520, 520, 197, 0, 0.0, False, 24, 9, 1, 4, 0, True, True, False),
    TnPath("phased_direct_dbias", 8, 520, 520, 197, 0, 0.0, True, 24, 9, 1, 4, 0, True, True, True),
    # phased + slabs, 7 K-tiles over 2 splits: the first split takes one more (kt_r = 1); T = 7 x 64 - 5
    TnPath("phased_slabs_kt_r", 8, 520, 136, 443, 0, 0.0, True, 8, 3, 2, 3, 1, True, False, True),
    # plain + slabs: 5 K-tiles over 2 splits, kt_q = 2 < 3
    TnPath("plain_slabs_short", 8, 520, 136, 300, 0, 0.0, True, 8, 3, 2, 2, 1, False, False, True),
    # plain + direct: the row remap of A keeps the plain kernel; T = 3 groups of 65 rows
    TnPath("plain_direct_remap", 8, 520, 264, 195, 65, 0.0, False, 8, 6, 1, 4, 0, False, True, False),
    # beta = 1 on a one-split plan: slabs, and the reduction adds into C
    TnPath("one_split_beta1", 8, 520, 264, 197, 0, 1.0, True, 8, 6, 1, 4, 0, True, False, True),
)

TN_BRANCHES = {
    "phased + direct": lambda r: r.phased and r.direct and not r.dbias and r.ldc_pad > 0,
    "phased + direct + dbias": lambda r: r.phased and r.direct and r.dbias and r.ldc_pad > 0,
    "phased + slabs, kt_r != 0": lambda r: r.phased and not r.direct and r.kt_r != 0,
    "plain + slabs, kt_q < 3": lambda r: not r.phased and not r.direct and r.kt_q < 3,
    "plain + direct, a_group": lambda r: not r.phased and r.direct and r.a_group > 0,
    "beta = 1 on one split: slabs": lambda r: r.splits == 1 and r.beta == 1.0 and not r.direct,
}


@dataclass(frozen=True)
class TngPath:
    name: str
    cus: int
    T: int
    problems: Tuple[Tuple[int, int, bool], ...]      # (M, N, dbias)
    tiles: int
    slots: int          # nrv_gemm_tn_grouped_workspace / ((256 * 256 + 256) * 4); 0 = the grouped kernel refuses the group


# The grouped kernel runs W = planned CUs workgroups: F cohorts of one workgroup per tile (F <= W // tiles) and Wr = W - F x tiles
# remainder workgroups of segs_r partial-tile slots each; slots = F x tiles + Wr x segs_r.  With 6 tiles on 8 CUs F = 1, so
# slots > tiles says that remainder workgroups run (Wr = 2, 5 slots each); 70 K-steps make Lc >= 8.
TNG_TABLE: Tuple[TngPath, ...] = (
    TngPath("accepted_with_remainder", 8, 4475, ((264, 136, True), (264, 264, False)), 6, 16),
    TngPath("refused_more_tiles_than_cus", 8, 4475, ((520, 520, True), (264, 264, False)), 13, 0),
)

SLOT_BYTES = (256 * 256 + 256) * 4

# ---- the plans of the workload shapes at the device's own CU count, recorded from the cost model before the launch and the
# query shared one planning function: (reserved CUs, M, N, K, epilogue id, remap) -> (tile_m, tile_n, phased, tiles, grid).
# Epilogue ids: include/nrv.h (0 none, 1 bias, 3 bias + residual, 5 / 6 the 8-bit gelu' pair).
WORKLOAD_NT = {
    (0, 50432, 768, 768, 0, False): (320, 256, True, 474, 256),
    (0, 25216, 1024, 4096, 0, False): (256, 256, True, 396, 256),
    (0, 98760, 384, 384, 0, False): (384, 128, True, 774, 256),
    (16, 9000, 2304, 768, 0, False): (192, 256, True, 423, 240),
    (0, 50432, 384, 1536, 3, False): (256, 256, True, 394, 256),      # the allow_384n exception: fp32 residual, K >= 1024
    (0, 50432, 384, 1536, 0, False): (384, 128, True, 396, 256),      # ... and the same shape without it
    (0, 50176, 768, 768, 3, True): (256, 256, False, 588, 588),       # patch embedding: row remap, plain kernel
    # ViT-B/16, batch 256: qkv, proj, fc1, fc2, dX of qkv, dU, dX of fc1
    (0, 50432, 2304, 768, 1, False): (256, 256, True, 1773, 256),
    (0, 50432, 768, 768, 3, False): (320, 256, True, 474, 256),
    (0, 50432, 3072, 768, 5, False): (256, 256, True, 2364, 256),
    (0, 50432, 768, 3072, 3, False): (320, 256, True, 474, 256),
    (0, 50432, 768, 2304, 0, False): (320, 256, True, 474, 256),
    (0, 50432, 3072, 768, 6, False): (256, 256, True, 2364, 256),
    (0, 50432, 768, 3072, 0, False): (320, 256, True, 474, 256),
    # ViT-S/16, batch 256
    (0, 50432, 1152, 384, 1, False): (256, 256, True, 985, 256),
    (0, 50432, 384, 384, 3, False): (384, 128, True, 396, 256),
    (0, 50432, 1536, 384, 5, False): (256, 256, True, 1182, 256),
    (0, 50432, 384, 1152, 0, False): (384, 128, True, 396, 256),
    (0, 50432, 1536, 384, 6, False): (256, 256, True, 1182, 256),
    # ViT-L/16, batch 128
    (0, 25216, 3072, 1024, 1, False): (256, 256, True, 1188, 256),
    (0, 25216, 1024, 1024, 3, False): (256, 256, True, 396, 256),
    (0, 25216, 4096, 1024, 5, False): (320, 256, True, 1264, 256),
    (0, 25216, 1024, 4096, 3, False): (256, 256, True, 396, 256),
    (0, 25216, 1024, 3072, 0, False): (256, 256, True, 396, 256),
    (0, 25216, 4096, 1024, 6, False): (320, 256, True, 1264, 256),
}


def nt(name: str) -> NtPath:
    return next(r for r in NT_TABLE if r.name == name)


def tn(name: str) -> TnPath:
    return next(r for r in TN_TABLE if r.name == name)


def xcd_remap(bid: int, nwg: int) -> int:
    """nrv_common.hpp xcd_remap: position `bid` of the launch order -> tile id, so that the ids one XCD holds are consecutive."""
    q, r, xcd, idx = nwg >> 3, nwg & 7, bid & 7, bid >> 3
    start = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return start + idx


def tile_of(rec: NtPath, m: int, n: int):
    """(tile row, tile column, position t of the tile in the launch order, walk position t // grid) of output element (m, n).

    Both kernels turn position t (the workgroup index of the plain kernel; b, b + grid, ... for workgroup b of the persistent
    one) into tile id xcd_remap(t, tiles) and sweep the ids in column groups of 4 tile columns, row by row within a group;
    with at most 4 tile columns, as in every record here, that is the row-major order."""
    assert rec.tiles_n <= 4
    tr, tc = m // rec.tile_m, n // rec.tile_n
    tid = tr * rec.tiles_n + tc
    t = next(t for t in range(rec.tiles) if xcd_remap(t, rec.tiles) == tid)
    return tr, tc, t, t // rec.grid
