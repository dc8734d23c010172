"""The grid caps of the row and elementwise kernels, and the shapes at which the GPU tests make them wrap.

Every kernel listed here walks its work with `for (i = first; i < n; i += gridDim.x * ...)` under a capped grid.  Below
`threshold = cap x items per workgroup` items each thread (or wave) runs the loop body once; above it the loop continues, which
is what every batch-256 training step does.  One record per entry point:

    source     file under noise_robust_vit_amd/csrc
    cap_name   the cap as the source writes it (a constant's name, or the literal)
    cap        its value
    group      work items per workgroup (threads, or waves x rows per wave)
    per_item   elements per work item (the vector width; a row kernel counts rows: 1)
    threshold  cap x group items: the largest launch that makes one pass
    wrapped    the shape test_launch_paths_gpu.py runs; items(wrapped) >= 2.25 x threshold and no multiple of it, so every
               launch makes two full passes and a partial third

test_launch_paths_host.py reads `cap` and `group` back out of the source through the regular expressions below, so a cap that
is raised later fails there instead of quietly turning the GPU tests into one-pass tests again.

Not in the table:
  * nrv_pcn.hip's elementwise kernels (dw_bwd_da, se_apply, ls_add, dgelu_rows): PCN_GRID_CAP = 65535 x 8 workgroups of 256
    threads x 4 elements wrap above 5.4e8 elements, which neither a test of a few seconds nor the workload reaches.
  * bn_bwd_apply_kernel (8192 x 256 elements, wrapped by test_bn_rows_gpu.py's 12544 x 640), nrv_sumsq_f32 (1024 x 256 x 4,
    wrapped by test_optim_gpu.py), the talking-heads kernels, and the persistent GEMM / attention walks, which their own
    tests already run over several passes.
  * the persistent walk of the fused Sinkhorn pair (nrv_sinkhorn.hip: one workgroup per CU, the K / V image slots alternating
    with `it & 1`).  Its older many-head tests use 270 and 276 heads on 256 CUs, two passes at the most, so no slot was ever
    reused.  The walk cases of tests/sinkhorn_edges_ref.py (WALK_SPECS, run by test_sinkhorn_edges_gpu.py) hold it to the
    standard of this table: 3 cus + 7 heads at N = 17 and 33, as (heads, 1) and as (ceil(heads / 5), 5), and
    ceil(2.25 cus) + 3 heads at N = 129, 197 and (forward only) 225, with cus read from the device and every head checked
    per row; test_sinkhorn_edges_ref_host.py asserts the pass counts for several CU counts.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "noise_robust_vit_amd", "csrc")

MIN_PASSES = 2.25            # two full passes and at least a quarter of a third


def pad8(n: int) -> int:
    return (n + 7) // 8 * 8


def conv_out(n: int, ks: int, stride: int, pad: int) -> int:
    return (n + 2 * pad - ks) // stride + 1


@dataclass(frozen=True)
class LaunchPath:
    name: str
    source: str
    cap_name: str
    cap: int
    cap_regex: str                                   # finds the cap in the source: one group named `cap`
    group: int
    group_facts: Tuple[Tuple[str, Tuple[str, ...]], ...]   # (regex, the groups it must capture): what `group` follows from
    per_item: int
    unit: str
    wrapped: Dict[str, int]
    items: Callable[[Dict[str, int]], int] = field(compare=False)

    @property
    def threshold(self) -> int:                      # items of a one-pass launch, at most
        return self.cap * self.group

    @property
    def threshold_elements(self) -> int:
        return self.threshold * self.per_item

    @property
    def wrapped_items(self) -> int:
        return self.items(self.wrapped)

    @property
    def passes(self) -> float:
        return self.wrapped_items / self.threshold


# ---- facts shared by several records ---------------------------------------------------------------------------------------
_LN_GROUP = ((r"constexpr int LN_THREADS = (\d+);", ("256",)),
             (r"constexpr int LN_WAVES = LN_THREADS / (\d+);", ("64",)),
             (r"int ln_lpr\(int dim\) \{ return dim <= (\d+) \? (\d+) : (\d+); \}", ("512", "32", "64")),
             # a wave takes 64 / lanes-per-row rows at a time, in both grid formulas and both kernels
             (r"nrv_cdiv\(rows, LN_WAVES \* \((\d+) / ln_lpr\(dim\)\)\)", ("64",)),
             (r"row0 \+= \(long long\)gridDim\.x \* (LN_WAVES \* RPW)\)", ("LN_WAVES * RPW",)))
_LNP_GROUP = ((r"constexpr int LNP_THREADS = (\d+);", ("256",)),
              (r"constexpr int LNP_WAVES = LNP_THREADS / (\d+);", ("64",)),
              (r"r \+= \(long long\)gridDim\.x \* (LNP_WAVES)\)", ("LNP_WAVES",)))
_UNFOLD_ITEMS = r"grid_for\(\(long long\)g\.B \* g\.Ho \* g\.Wo \* \(g\.KP >> 3\), (\d+), grid_cap\)"
_FOLD_ITEMS = r"grid_for\(\(long long\)g\.B \* g\.H \* g\.W \* g\.ld, (\d+), grid_cap\)"


def _rows(s):
    return s["rows"]


def _n_over(v):
    return lambda s: s["n"] // v


def _unfold_items(s):            # one item = 8 consecutive features of one output token
    return s["B"] * conv_out(s["H"], s["ks"], s["stride"], s["pad"]) * conv_out(s["W"], s["ks"], s["stride"], s["pad"]) * \
        (pad8(s["ks"] * s["ks"] * s["C"]) // 8)


def _fold_items(s):              # one item = one element of dx, rows ld wide
    return s["B"] * s["H"] * s["W"] * s.get("ld", s["C"])


def _grid_for(kernel: str, items: str) -> str:
    """`<kernel>..., dim3(grid_for(<items>, BLOCK, CAP))` of a launch line; BLOCK is group 1, CAP the group `cap`."""
    return re.escape(kernel) + r"\)?, dim3\(grid_for\(" + re.escape(items) + r", (\d+), (?P<cap>\d+)\)\)"


TABLE: List[LaunchPath] = [
    # LayerNorm: 4 waves per workgroup, one row per wave (dim > 512) or two (dim <= 512).  Row counts are odd (the last pair
    # of the two-row form is incomplete) and odd modulo the 4 waves (some waves walk one row more than others).
    LaunchPath("layernorm_fwd", "nrv_norm.hip", "LN_FWD_BLOCKS", 4096, r"constexpr int LN_FWD_BLOCKS = (?P<cap>\d+);",
               4, _LN_GROUP + ((r"if \(g > (LN_FWD_BLOCKS)\) g = (LN_FWD_BLOCKS);", ("LN_FWD_BLOCKS", "LN_FWD_BLOCKS")),),
               1, "row (dim > 512)", {"rows": 38915}, _rows),
    LaunchPath("layernorm_fwd_half_wave", "nrv_norm.hip", "LN_FWD_BLOCKS", 4096, r"constexpr int LN_FWD_BLOCKS = (?P<cap>\d+);",
               8, _LN_GROUP, 1, "row (dim <= 512)", {"rows": 75777}, _rows),
    LaunchPath("layernorm_bwd", "nrv_norm.hip", "LN_BWD_BLOCKS", 1024, r"constexpr int LN_BWD_BLOCKS = (?P<cap>\d+);",
               4, _LN_GROUP + ((r"if \(g > (LN_BWD_BLOCKS)\) g = (LN_BWD_BLOCKS);", ("LN_BWD_BLOCKS", "LN_BWD_BLOCKS")),),
               1, "row (dim > 512)", {"rows": 9731}, _rows),
    LaunchPath("layernorm_bwd_half_wave", "nrv_norm.hip", "LN_BWD_BLOCKS", 1024, r"constexpr int LN_BWD_BLOCKS = (?P<cap>\d+);",
               8, _LN_GROUP, 1, "row (dim <= 512)", {"rows": 19463}, _rows),
    # AdamW: 256 threads x 4 elements; n % 4 = 3 leaves a scalar tail
    LaunchPath("adamw_flat", "nrv_optim.hip", "8192", 8192, r"if \(blocks > (?P<cap>\d+)\) blocks = (\d+);",
               256, ((r"constexpr int OPT_THREADS = (\d+);", ("256",)),
                     (r"if \(blocks > (\d+)\) blocks = (\d+);", ("8192", "8192")),
                     (r"long long blocks = \(n4 \+ (OPT_THREADS) - 1\) / (OPT_THREADS);", ("OPT_THREADS", "OPT_THREADS"))),
               4, "4 parameters", {"n": 19000003}, _n_over(4)),
    LaunchPath("cast_bf16", "nrv_misc.hip", "4096", 4096, _grid_for("cast_kernel", "n >> 2"), 256,
               ((_grid_for("cast_kernel", "n >> 2"), ("256", "4096")),), 4, "4 floats", {"n": 9937187}, _n_over(4)),
    LaunchPath("dropout_add", "nrv_misc.hip", "4096", 4096, _grid_for("dropout_add_kernel", "n >> 3"), 256,
               ((_grid_for("dropout_add_kernel", "n >> 3"), ("256", "4096")),), 8, "8 floats", {"n": 19874408}, _n_over(8)),
    LaunchPath("mask_mul", "nrv_misc.hip", "4096", 4096, _grid_for("mask_mul_kernel", "n >> 3"), 256,
               ((_grid_for("mask_mul_kernel", "n >> 3"), ("256", "4096")),), 8, "8 bf16", {"n": 19874408}, _n_over(8)),
    LaunchPath("mask_mul_f32", "nrv_misc.hip", "4096", 4096, _grid_for("mask_mul_f32_kernel", "n"), 256,
               ((_grid_for("mask_mul_f32_kernel", "n"), ("256", "4096")),), 1, "float", {"n": 2484301}, _n_over(1)),
    # gather / scatter: one wave per row, 4 waves; dim 260 also runs the wave's column loop twice
    LaunchPath("gather_rows", "nrv_misc.hip", "4096", 4096, _grid_for("(move_rows_kernel<false>", "rows_out"), 4,
               ((_grid_for("(move_rows_kernel<false>", "rows_out"), ("4", "4096")),
                (r"r < rows; r \+= \(long long\)gridDim\.x \* (\d+)\)", ("4",))),
               1, "row", {"rows": 38915, "rows_src": 50000, "dim": 260}, _rows),
    LaunchPath("scatter_rows", "nrv_misc.hip", "4096", 4096, _grid_for("(move_rows_kernel<true>", "rows_out"), 4,
               ((_grid_for("(move_rows_kernel<true>", "rows_out"), ("4", "4096")),
                (r"r < rows; r \+= \(long long\)gridDim\.x \* (\d+)\)", ("4",))),
               1, "row", {"rows": 38915, "rows_src": 50000, "dim": 260}, _rows),
    LaunchPath("patch_unfold", "nrv_misc.hip", "4096", 4096, r"const int grid = grid_for\(total, (\d+), (?P<cap>\d+)\);", 256,
               ((r"const int grid = grid_for\(total, (\d+), (\d+)\);", ("256", "4096")),), 8, "8 features",
               {"B": 7, "C": 3, "H": 944, "W": 976, "p": 16},
               lambda s: s["B"] * (s["H"] // s["p"]) * (s["W"] // s["p"]) * (pad8(s["C"] * s["p"] * s["p"]) // 8)),
    # the shared unfold / fold pair under its two caps
    LaunchPath("conv_unfold", "nrv_misc.hip", "CONV_GRID_CAP", 4096, r"constexpr int CONV_GRID_CAP = (?P<cap>\d+)", 256,
               ((_UNFOLD_ITEMS, ("256",)), (r"launch_unfold<UF_TAP_MAJOR>\([^;]*, (\w+_GRID_CAP),", ("CONV_GRID_CAP",))),
               8, "8 features", {"B": 5, "C": 8, "H": 460, "W": 476, "ks": 3, "stride": 2, "pad": 1}, _unfold_items),
    LaunchPath("conv_fold", "nrv_misc.hip", "CONV_GRID_CAP", 4096, r"constexpr int CONV_GRID_CAP = (?P<cap>\d+)", 256,
               ((_FOLD_ITEMS, ("256",)), (r"launch_fold<UF_TAP_MAJOR, false>\([^;]*, (\w+_GRID_CAP),", ("CONV_GRID_CAP",))),
               1, "float of dx", {"B": 5, "C": 8, "H": 244, "W": 252, "ks": 5, "stride": 2, "pad": 2}, _fold_items),
    LaunchPath("soft_split_fwd", "nrv_misc.hip", "SPLIT_GRID_CAP", 16384, r"SPLIT_GRID_CAP = (?P<cap>\d+);", 256,
               ((_UNFOLD_ITEMS, ("256",)), (r"launch_unfold<UF_CHANNEL_MAJOR>\([^;]*, (\w+_GRID_CAP),", ("SPLIT_GRID_CAP",))),
               8, "8 features", {"B": 9, "C": 3, "H": 944, "W": 952, "ks": 7, "stride": 4, "pad": 2}, _unfold_items),
    LaunchPath("soft_split_bwd", "nrv_misc.hip", "SPLIT_GRID_CAP", 16384, r"SPLIT_GRID_CAP = (?P<cap>\d+);", 256,
               ((_FOLD_ITEMS, ("256",)), (r"launch_fold<UF_CHANNEL_MAJOR, true>\([^;]*, (\w+_GRID_CAP),", ("SPLIT_GRID_CAP",))),
               1, "float of dx", {"B": 2, "C": 3, "H": 768, "W": 776, "ks": 7, "stride": 4, "pad": 2, "ld": 8}, _fold_items),
    LaunchPath("sd_add", "nrv_window_attn.hip", "4096", 4096, _grid_for("sd_add_kernel", "n4"), 256,
               ((_grid_for("sd_add_kernel", "n4"), ("256", "4096")),), 4, "4 floats",
               {"samples": 13, "rows_per_sample": 7993, "dim": 96}, lambda s: s["samples"] * s["rows_per_sample"] * s["dim"] // 4),
    LaunchPath("sd_scale_bf16", "nrv_window_attn.hip", "4096", 4096, _grid_for("sd_scale_kernel", "n4"), 256,
               ((_grid_for("sd_scale_kernel", "n4"), ("256", "4096")),), 4, "4 floats",
               {"samples": 13, "rows_per_sample": 7993, "dim": 96}, lambda s: s["samples"] * s["rows_per_sample"] * s["dim"] // 4),
    # T is a multiple of 8 for the per-sample `keep` variant
    LaunchPath("bn_apply", "nrv_bn.hip", "8192", 8192, _grid_for("bn_apply_kernel", "T * C / 4"), 256,
               ((_grid_for("bn_apply_kernel", "T * C / 4"), ("256", "8192")),), 4, "4 floats",
               {"T": 950008, "C": 20}, lambda s: s["T"] * s["C"] // 4),
    # one wave per row, 4 waves; n = 147 of ld = 152 columns: the last 64-lane step of a row is partial
    LaunchPath("layernorm_pad_fwd", "nrv_t2t.hip", "8192", 8192,
               r"nrv_layernorm_pad_fwd\((?:[^}]|\}(?!\n))*?const int grid = grid_for\(rows, LNP_WAVES, (?P<cap>\d+)\);", 4,
               _LNP_GROUP, 1, "row", {"rows": 75777, "n": 147}, _rows),
    LaunchPath("layernorm_pad_bwd", "nrv_t2t.hip", "8192", 8192,
               r"nrv_layernorm_pad_bwd\((?:[^}]|\}(?!\n))*?const int grid = grid_for\(rows, LNP_WAVES, (?P<cap>\d+)\);", 4,
               _LNP_GROUP, 1, "row", {"rows": 75777, "n": 147}, _rows),
]

# further shapes that wrap the same launches through other template instantiations (source kind, width): checked like `wrapped`
ALSO_WRAPPED: Dict[str, List[Dict[str, int]]] = {
    "conv_unfold": [{"B": 5, "C": 3, "H": 690, "W": 694, "ks": 3, "stride": 2, "pad": 1},       # NCHW fp32, KP 27 -> 32
                    {"B": 2, "C": 20, "H": 452, "W": 460, "ks": 3, "stride": 2, "pad": 1}],     # NCHW bf16, generic path
}

# the LayerNorm widths of the wrapped cases -> (lanes per row, chunks per lane as dispatched): J = 6 and 8 of the 64-lane
# form, partly empty last chunks (1792 under 8; 2056, 3072 under 16; 520 under 3), idle lanes of the 32-lane form (96)
LN_DIMS = {96: (32, 1), 520: (64, 3), 1536: (64, 6), 1792: (64, 8), 2048: (64, 8), 2056: (64, 16), 3072: (64, 16)}


def get(name: str) -> LaunchPath:
    for r in TABLE:
        if r.name == name:
            return r
    raise KeyError(name)


def shapes_of(rec: LaunchPath) -> List[Dict[str, int]]:
    return [rec.wrapped] + ALSO_WRAPPED.get(rec.name, [])


def _groups(m) -> Tuple[str, ...]:
    return tuple(g for g in m.groups())


def problems(rec: LaunchPath, text: str) -> List[str]:
    """What is wrong with `rec` against the source text of rec.source; empty when the table and the source agree and the
    wrapped shape still wraps.  Every message names the record."""
    out = []
    caps = [int(m.group("cap")) for m in re.finditer(rec.cap_regex, text)]
    if not caps:
        return [f"{rec.name}: the cap {rec.cap_name} was not found in {rec.source} (pattern {rec.cap_regex!r})"]
    if any(c != rec.cap for c in caps):
        out.append(f"{rec.name}: the table says {rec.cap_name} = {rec.cap}, {rec.source} says {caps}")
    for rx, want in rec.group_facts:
        found = [_groups(m) for m in re.finditer(rx, text)]
        if not found:
            out.append(f"{rec.name}: {rec.source} no longer matches {rx!r}")
        elif any(f != tuple(want) for f in found):
            out.append(f"{rec.name}: {rx!r} captures {found} in {rec.source}, the table was derived from {tuple(want)}")
    threshold = max(caps) * rec.group            # of the source as it is now
    for shape in shapes_of(rec):
        items = rec.items(shape)
        if items < MIN_PASSES * threshold:
            out.append(f"{rec.name}: {shape} is {items} items = {items / threshold:.3f} passes of {threshold}; "
                       f"the GPU test needs {MIN_PASSES}")
        if items % threshold == 0:
            out.append(f"{rec.name}: {shape} is a multiple of the threshold {threshold}: no partial last pass")
    return out


def source_text(rec: LaunchPath, csrc: str = CSRC) -> str:
    with open(os.path.join(csrc, rec.source)) as f:
        return f.read()


def doubled_cap(rec: LaunchPath, text: str) -> str:
    """The source text with the record's cap set to twice its value (every place the cap pattern finds it)."""
    pieces, last = [], 0
    for m in re.finditer(rec.cap_regex, text):
        pieces += [text[last:m.start("cap")], str(2 * int(m.group("cap")))]
        last = m.end("cap")
    return "".join(pieces) + text[last:]
