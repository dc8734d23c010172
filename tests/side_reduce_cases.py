"""The (weight gradient, dX GEMM) pairs at which the tests run the split-K reduction as a side job of the NT launch.

`nrv_gemm_tn_bf16_deferred` leaves a job (slabs and / or bias column sums to add up); `nrv_gemm_nt_bf16_side` gives it to the
late-starting workgroups of the persistent NT kernel when `nrv_gemm_nt_side_plan` admits it, and runs the stand-alone reduction
in front of the GEMM otherwise.  Both ways must give the bits of `nrv_gemm_tn_bf16` + `nrv_gemm_nt_bf16`.

One record per pair, planned for `cus` CUs (`nrv_set_reserved_cus`, as tests/gemm_paths.py):

    nt      (M, N, K, epilogue id) of the NT launch, and its plan (tile_m, tile_n, tiles, grid): always the phased kernel
    late    grid - tiles % grid: the workgroups that take shares
    tn      (M, N, T, beta) of the weight gradient; dbias: None (absent), 0.0 or 1.0 (dbias_beta); ldc_pad: C's ldc - N
    splits, kt_r, direct   the TN plan
    share   ceil(job_bytes / late), job_bytes = splits * M * N * 4 (0 for a direct plan: only the bias sums remain)
    admitted   share <= BYTES_PER_KSTEP * (K / 64) * tile_m / 256

All values are worked out by hand from the planning rules (csrc/nrv_gemm.hip nt_plan / tn_plan / nt_side_plan);
test_side_reduce_host.py asserts every one of them against the library, test_side_reduce_gpu.py once more on the device.

What the records cover between them: late = 1 and late = grid - 1; a chunk count that the shares do not divide, with a short
last share (17680 chunks on 3 shares of 5894) and with empty ones (16 chunks on 7 shares of 3: share 5 holds one, share 6 none;
8 bias rows on 7 shares of 2: shares 4 - 6 none); M N / 4 no multiple of 64; splits 1 (beta = 1), 2, 5, 8 and 19; kt_r != 0;
beta 0 and 1 with ldc > N; dbias absent, present and accumulated; a direct plan with a bias gradient; epilogue 0 on the 256-,
320- and 384 x 128-tiles and epilogue 6 (the 8-bit gelu' stream); a rejected job; a launch that leaves nothing pending.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

BYTES_PER_KSTEP = 40 * 1024        # csrc/nrv_gemm.hip NT_SIDE_BYTES_PER_KSTEP (profiles/r19_nt_side_reduce.txt)


@dataclass(frozen=True)
class Pair:
    name: str
    cus: int
    nt: Tuple[int, int, int, int]               # M, N, K, epilogue id
    nt_plan: Tuple[int, int, int, int]          # tile_m, tile_n, tiles, grid
    late: int
    tn: Tuple[int, int, int, float]             # M, N, T, beta
    dbias: Optional[float]
    ldc_pad: int
    splits: int
    kt_r: int
    direct: bool
    share: int
    admitted: bool

    @property
    def job_bytes(self) -> int:
        return 0 if self.direct else self.splits * self.tn[0] * self.tn[1] * 4

    @property
    def pending(self) -> bool:
        return not self.direct or self.dbias is not None


PAIRS: Tuple[Pair, ...] = (
    # 2 splits of 4 + 3 K-tiles; 520 x 136 / 4 = 17680 chunks = 276.25 x 64 on 3 shares of 5894 (the last 2 short);
    # 565760 B / 3 = 188587 <= 40 KiB x 5 K-steps = 204800
    Pair("late3_splits2_kt_r", 8, (1601, 520, 320, 0), (256, 256, 21, 8), 3, (520, 136, 443, 0.0), 0.0, 8, 2, 1, False, 188587, True),
    # the same job on a launch of 3 K-steps: 188587 > 122880, the reduction runs on its own
    Pair("rejected_short_k", 8, (1601, 520, 192, 0), (256, 256, 21, 8), 3, (520, 136, 443, 0.0), 0.0, 8, 2, 1, False, 188587, False),
    # 15 tiles on 8 workgroups: one late workgroup takes the whole job, 5 x 136 x 136 x 4 = 369920 <= 40 KiB x 10 = 409600
    Pair("late1_splits5_beta1", 8, (1200, 520, 640, 0), (256, 256, 15, 8), 1, (136, 136, 320, 1.0), None, 4, 5, 0, False, 369920, True),
    # 9 tiles of 384 x 128 (4 x 2 waves) on 8: 7 late workgroups for 16 chunks and 8 bias rows
    Pair("late7_empty_shares", 8, (3083, 72, 192, 0), (384, 128, 9, 8), 7, (8, 8, 320, 1.0), 1.0, 4, 5, 0, False, 183, True),
    # the 320-row tile; 9 K-tiles on 8 splits (the first takes 2); 591872 / 4 = 147968 <= 40 KiB x 3 x 320 / 256 = 153600
    Pair("tile320_splits8", 8, (3073, 392, 192, 0), (320, 256, 20, 8), 4, (136, 136, 515, 0.0), 0.0, 0, 8, 1, False, 147968, True),
    # epilogue 6 reads the 8-bit stream; one split with beta = 1 goes through a slab; 549120 / 3 = 183040 <= 40 KiB x 5 = 204800
    Pair("epi6_one_split_beta1", 8, (1601, 576, 320, 6), (256, 256, 21, 8), 3, (520, 264, 197, 1.0), 1.0, 8, 1, 0, False, 183040, True),
    # a direct plan: the kernel stored C itself (ldc > N), only the bias sums are left
    Pair("direct_bias_only", 8, (1601, 520, 192, 0), (256, 256, 21, 8), 3, (520, 520, 197, 0.0), 0.0, 24, 1, 0, True, 0, True),
    # ... and without a bias gradient nothing is pending
    Pair("nothing_pending", 8, (1601, 520, 192, 0), (256, 256, 21, 8), 3, (520, 520, 197, 0.0), None, 24, 1, 0, True, 0, True),
    # 24 planned CUs and one tile: 19 splits of one K-tile (wave g sums the slabs g, g + 4, ...: five rounds, the last ragged);
    # 19 x 136 x 136 x 4 = 1405696 / 3 = 468566 (rounded up) <= 40 KiB x 12 = 491520
    Pair("splits19_24cus", 24, (3743, 520, 768, 0), (256, 256, 45, 24), 3, (136, 136, 1155, 0.0), 0.0, 4, 19, 0, False, 468566, True),
)

# launches without late workgroups: (cus, M, N, K, epilogue, remap) and why
NO_LATE = (
    (8, 1601, 520, 128, 0, False, "plain kernel: two K-steps"),
    (8, 1601, 520, 192, 3, True, "row remap: plain kernel"),
    (8, 513, 264, 192, 0, False, "tiles <= grid"),
    (8, 1800, 520, 192, 0, False, "tiles % grid == 0"),
)


def pair(name: str) -> Pair:
    return next(p for p in PAIRS if p.name == name)
