"""CPU: the geometry, case tables, inputs and bounds of tests/sinkhorn_edges_ref.py, before any kernel is involved.

  * geometry: the restated formulas (NP, NT, the LDS budgets that decide TWO / THREE, the grids) agree with the constants read back
    out of nrv_sinkhorn.hip, and the table holds every (NP, edge kind) pair, N <= 16, N = 1, both chunk-slot regimes and the two-slot
    backward; the walk cases make three passes (and a fourth for seven heads) where the many-head tests that existed made two;
  * definition: `restated()` in fp32, with no mistake in it, is the fp64 reference to FP32_BOUND per row on every edge and scale case,
    and its scores-only part reproduces tests/golden/sinkhorn_unit.npz (the reference implementation's own output);
  * rounding alone: the reference's emulate_bf16 switch stays within EMULATION_BOUND per row (o within 2^-6), and
    `restated(kernel_rounding=True)` within KERNEL_ROUNDING_BOUND, on every edge, scale and walk case as drawn: the GPU bound of 3e-2
    is 3 x and 2 x what the formats cost on these inputs.  No case needed other inputs (RESEEDED is empty);
  * mistakes: each of the eight, switched on alone in the restatement, puts the named cases over a bound of `check`; the stale-image
    mistake changes NOTHING in any case whose workgroups make at most two passes (every edge and scale case, and the head counts of the
    two many-head tests that existed before, 270 and 276 on 256 CUs) and fails every walk case.

Measured here (worst row over the 51 edge, 15 scale and 7 walk cases, against fp64): emulate_bf16 dq 4.8e-3, dk 5.8e-3, dv 4.5e-3,
o 6.1e-3 of the maximum; kernel rounding dq 8.3e-3, dk 6.9e-3, dv 6.7e-3, o 6.1e-3; restated fp32 1.7e-6 per row, lse 1.3e-7
max(1, |lse|), saved vectors 1.2e-6 relative.  Worst error / bound per mistake: see test_one_mistake_is_over_a_bound_of_check.
"""
import math

import numpy as np
import pytest
import torch

import peaked_ref as PR
import sinkhorn_edges_ref as R

SMALL = R.EDGE_CASES + R.SCALE_CASES
WALK = tuple(R.walk_case(s, R.NOMINAL_CUS) for s in R.WALK_SPECS)


def _worst(r: dict) -> float:
    return max(r.values())


def _walk_grid(c):
    return dict(zip(("fwd", "bwd"), R.grids(c.N, c.B * c.H, R.NOMINAL_CUS)))


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def test_geometry_agrees_with_the_source():
    text = R.source_text()
    assert R.source_problems(text) == []
    # the check itself: a changed constant, a mask moved to one tile, a changed slot budget are each reported
    for old, new in (("constexpr int SK_TPW = 2;", "constexpr int SK_TPW = 1;"),
                     ("if (kt >= NT - 2) pv =", "if (kt >= NT - 1) pv ="),
                     ("3 * NP * 128 + VEC + CH * RS <= 160 * 1024", "3 * NP * 128 + VEC + CH * RS <= 64 * 1024"),
                     ("case 7: { constexpr int NPV = 224; return CALL; }", "case 7: { constexpr int NPV = 256; return CALL; }")):
        assert old in text
        assert R.source_problems(text.replace(old, new)) != [], old
    for N in range(1, 257):
        NP = R.np_of(N)
        assert NP == 32 * math.ceil(N / 32) and NP in R.DISPATCH_NP and 0 <= NP - N < 32 and R.nt_of(N) == NP // 16
    assert R.BWD_WAVES == 8 and R.CH == 128
    for NP in R.DISPATCH_NP:
        two, fbytes = R.fwd_lds(NP)
        three, bbytes = R.bwd_lds(NP)
        assert two and fbytes == 584 * NP <= R.LDS_BYTES
        assert three == (692 * NP + 4096 <= 160 * 1024) == (NP <= 224)
        assert bbytes == (692 if three else 564) * NP + 4096 <= R.LDS_BYTES
    # three slots: both launches persistent; NP = 256: the forward alone
    assert R.grids(197, 1000, 256) == (256, 256) and R.grids(225, 1000, 256) == (256, 1000) and R.grids(197, 256, 256) == (256, 256)
    assert R.grids(197, 4, 256) == (4, 4) and R.passes(197, 3072, 256) == (12, 12)


def test_case_tables_reach_what_they_claim():
    ns = [c.N for c in R.EDGE_CASES]
    assert len(ns) == len(set(ns)) == 51 and all(c.B == 2 and c.H == 2 and c.scale == 0.125 and not c.fwd_only for c in R.EDGE_CASES)
    for k in range(1, 9):
        NP = 32 * k
        kinds = {c.kind: c.N for c in R.EDGE_CASES if R.np_of(c.N) == NP and c.kind != "tiny"}
        assert kinds == {"first_n": NP - 31, "pad_tile_after_partial": NP - 17, "pad_tile_after_full": NP - 16,
                         "one_key_last_tile": NP - 15, "one_pad_key": NP - 1, "full": NP}, NP
        NT = NP // 16
        assert (kinds["first_n"] - 1) // 16 == NT - 2 and kinds["first_n"] % 16 == 1                     # one real key in tile NT - 2
        assert 16 * (NT - 2) < kinds["pad_tile_after_partial"] < 16 * (NT - 1)                           # tile NT - 2 partial, NT - 1 padding
        assert kinds["pad_tile_after_full"] == 16 * (NT - 1) and kinds["one_key_last_tile"] == 16 * (NT - 1) + 1
    assert {c.N for c in R.EDGE_CASES if c.kind == "tiny"} == {2, 3, 5}
    assert {1, 2, 3, 5, 15, 16} == {n for n in ns if n <= 16}                                            # only wave 0 active
    second_slot = {R.np_of(n): R.np_of(n) - R.CH for n in ns if R.np_of(n) > R.CH}
    assert second_slot == {160: 32, 192: 64, 224: 96, 256: 128}                                          # rows of chunk slot u = 1
    assert sum(R.np_of(n) <= R.CH for n in ns) == 27                                                     # the slot is skipped
    assert sum(not R.bwd_lds(R.np_of(n))[0] for n in ns) == 6                                            # the two-slot backward
    assert [(c.N, c.scale) for c in R.SCALE_CASES] == [(N, s) for N in (3, 49, 130, 197, 256) for s in (0.1, 0.2, 0.0625)]
    assert all(c.scale != 0.125 and c.B == 2 and c.H == 2 for c in R.SCALE_CASES)
    assert len({R.case_id(c) for c in SMALL}) == len(SMALL)
    assert [c.N for c in R.WRAPPER_CASES] == [17, 129, 225]


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_walk_cases_make_a_third_pass_on_any_cu_count(cus):
    for s in R.WALK_SPECS:
        c = R.walk_case(s, cus)
        nheads = c.B * c.H
        fwd, bwd = R.passes(c.N, nheads, cus)
        gf, gb = R.grids(c.N, nheads, cus)
        if s.heads_rule == "3x+7":
            assert nheads >= 3 * cus + 7 and nheads - (3 * cus + 7) < c.H and (c.B, c.H) in ((nheads, 1), (-(-(3 * cus + 7) // 5), 5))
            assert (fwd, bwd) == (4, 4) and 0 < nheads - 3 * gf < gf                  # it = 3 for a few workgroups only
        else:
            assert nheads == math.ceil(2.25 * cus) + 3 and nheads % cus != 0 and c.H == 1
            assert fwd == 3 and bwd == (1 if s.fwd_only else 3)
            assert s.fwd_only == (not R.bwd_lds(R.np_of(c.N))[0])
        assert gf == cus and gb == (nheads if s.fwd_only else cus)
    assert {(s.heads_rule, s.per_sample, s.N) for s in R.WALK_SPECS} == {("3x+7", 1, 17), ("3x+7", 5, 17), ("3x+7", 1, 33), ("3x+7", 5, 33),
                                                                        ("2.25x+3", 1, 129), ("2.25x+3", 1, 197), ("2.25x+3", 1, 225)}
    # what existed before: 270 and 276 heads on 256 CUs never reach it = 2
    assert R.passes(197, 270, 256) == (2, 2) and R.passes(197, 276, 256) == (2, 2)


def test_inputs_put_the_last_key_twelve_nats_down():
    for c in SMALL + WALK[:1]:
        i = R.inputs(c)
        assert i["qkv"].dtype == torch.bfloat16 and tuple(i["qkv"].shape) == (c.B * c.N, 3 * c.H * R.DH)
        assert tuple(i["dout"].shape) == (c.B * c.N, c.H * R.DH)
        if c.N < R.MIN_PEAKED_N:
            continue
        q, k, _ = R.heads(i["qkv"].double(), c.B, c.N, c.H, R.DH)
        s = q @ k.transpose(-1, -2) * R.DH ** -0.5                  # the builder's nats are at the builder's scale
        gap = s[..., :-1].mean() - s[..., -1].mean()
        assert abs(gap.item() - R.WEAK_NATS) < 0.5, (R.case_id(c), gap)
    # b3 of that key is large and sits on the pad boundary
    ref = R.reference(next(c for c in R.EDGE_CASES if c.N == 207))
    assert ref["scal"][:, :, 5, -1].min().item() > 1e3 * ref["scal"][:, :, 5, :-1].median().item()


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def test_restatement_without_a_mistake_is_the_reference():
    worst = {}
    for c in SMALL:
        r = R.check(c, R.restated(c))
        for n, x in r.items():
            worst[n] = max(worst.get(n, 0.0), x)
        for n in ("dq", "dk", "dv"):
            assert r[n] <= (1.0 if c.N == 1 else R.FP32_BOUND / R.PER_ROW_BOUND), (R.case_id(c), n, r)
        assert r["o"] <= R.FP32_BOUND / R.O_BOUND and r["lse"] <= 1e-2 and r["scal"] <= 1e-2, (R.case_id(c), r)
    print("restated fp32, worst error / bound of check:", {k: f"{v:.2e}" for k, v in worst.items()})


def test_no_reference_row_is_zero_except_the_one_key_cancellation():
    for c in SMALL:
        ref = R.reference(c)
        for n in ("dq", "dk", "dv"):
            zero = ref[n].norm(dim=-1) == 0
            assert bool(zero.all()) if (c.N == 1 and n != "dv") else not bool(zero.any()), (R.case_id(c), n)


def test_scores_only_part_reproduces_the_golden_unit_vector(golden_dir):
    g = np.load(f"{golden_dir}/sinkhorn_unit.npz")
    s, want = torch.from_numpy(g["scores"]), torch.from_numpy(g["out"])
    N = s.shape[-1]
    NP = R.np_of(N)
    S = torch.zeros(s.numel() // (N * N), NP, NP)
    S[:, :N, :N] = s.reshape(-1, N, N)
    S[:, N:] = S[:, N - 1:N]                                        # a padded query lane holds row N - 1
    P0, lse, vecs = R.sinkhorn_from_scores(S, N, R.LOG2E)
    P7 = (P0 * vecs[:, 5, None, :] * vecs[:, 6, :, None])
    assert bool((P7[:, N:] == 0).all()) and bool((P7[:, :, N:] == 0).all())
    assert (P7[:, :N, :N].reshape(want.shape) - want).abs().max().item() < 1e-6
    assert (lse[:, :N].reshape(s.shape[:-1]) - torch.logsumexp(s, dim=-1)).abs().max().item() < 1e-5
    av, bv = PR.sinkhorn_scalings(s.double())
    assert ((vecs[:, 0::2, :N].reshape(av.shape) - av).abs() / av).max().item() < 1e-5
    assert ((vecs[:, 1::2, :N].reshape(bv.shape) - bv).abs() / bv).max().item() < 1e-5


# ---- rounding alone ---------------------------------------------------------------------------------------------------------------
def _rounding_figures(c):
    ref = R.reference(c)
    emu = R.reference(c, emulate_bf16=True)
    kr = R.restated(c, kernel_rounding=True)
    names = () if c.fwd_only else ("dq", "dk", "dv")
    fig = {}
    for tag, got in (("emulate_bf16", emu), ("kernel rounding", kr)):
        for n in names:
            fig[tag, n] = R.per_row_rel(got[n], ref[n]).max().item() if c.N > 1 or n == "dv" else 0.0
        fig[tag, "o"] = ((got["o"].double() - ref["o"]).abs().amax(dim=-1).max() / ref["o"].abs().max()).item()
    return fig


def _assert_rounding(c, fig):
    for (tag, n), e in fig.items():
        bound = R.O_BOUND if n == "o" else (R.EMULATION_BOUND if tag == "emulate_bf16" else R.KERNEL_ROUNDING_BOUND)
        assert e <= bound, (R.case_id(c), tag, n, e)


def test_rounding_at_the_kernels_points_stays_inside_the_emulation_bounds():
    worst = {}
    for c in SMALL:
        fig = _rounding_figures(c)
        for key, e in fig.items():
            worst[key] = max(worst.get(key, 0.0), e)
        _assert_rounding(c, fig)
        kr = R.check(c, R.restated(c, kernel_rounding=True))       # and the whole check, N = 1 rules included
        assert _worst(kr) <= 1.0, (R.case_id(c), kr)
    print("worst row over the edge and scale cases: " + "  ".join(f"{t} {n} {e:.2e}" for (t, n), e in sorted(worst.items())))


# ---- the walk cases: rounding, and the stale image -------------------------------------------------------------------------------
@pytest.mark.parametrize("c", WALK, ids=R.case_id)
def test_walk_case_rounding_and_the_stale_image(c):
    """Every head of a walk case: inside the rounding bounds as drawn, and over every bound of `check` with the stale K image -- the
    worst row of every tensor in a head of pass >= 2.  Measured error / bound: o 46 .. 78, lse 1.1e3 .. 5.0e3, saved vectors 890 ..
    4.3e3, dq 160 .. 229, dk 115 .. 141, dv 73 .. 105."""
    _assert_rounding(c, _rounding_figures(c))
    grid, where = _walk_grid(c), {}
    clean = R.check(c, R.restated(c), grid=grid)
    assert _worst(clean) <= 1e-2, (R.case_id(c), clean)
    r = R.check(c, R.restated(c, "stale_k_image"), grid=grid, where=where)
    print(R.case_id(c), "stale K image, error / bound", {k: f"{v:.3g}" for k, v in r.items()}, where)
    assert min(r.values()) > 1.0, (R.case_id(c), r)
    assert all(int(w.rsplit("pass ", 1)[1]) >= 2 for w in where.values()), where


def test_stale_image_is_invisible_with_two_or_fewer_passes():
    """Why the suite could not have seen it: with at most two passes per workgroup the mistake reads every head's own image."""
    for nheads in (4, 256, 270, 276, 512):
        assert torch.equal(R.stale_source(nheads, min(nheads, 256)), torch.arange(nheads)), nheads
    assert not torch.equal(R.stale_source(513, 256), torch.arange(513))
    for c in SMALL:
        assert max(R.passes(c.N, c.B * c.H, R.NOMINAL_CUS)) == 1
    for c in SMALL[::6]:
        a, b = R.restated(c), R.restated(c, "stale_k_image")
        for n in a:
            assert torch.equal(a[n], b[n]), (R.case_id(c), n)
    # the many-head shape of tests/test_peaked_attn_gpu.py (45 x 6 = 270 heads, N = 197), all heads, bit for bit
    B, N, H, _, _ = PR.MANY_HEADS_CASE
    c = R.Case("walk", B, N, H, R.DH ** -0.5, "", False)
    assert R.passes(N, B * H, 256) == (2, 2)
    a, b = R.restated(c), R.restated(c, "stale_k_image")
    for n in a:
        assert torch.equal(a[n], b[n]), n


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------
def _np_partial(c):
    return c.N % 32 != 0


# mistake -> (the cases it must put over a bound, the tensor that shows it there -- None: any)
MUST_FAIL = {
    # the zero K rows of tile NT - 2 enter the softmax with score 0: where that tile has a padding key
    "pad_mask_last_tile_only": (lambda c: c.N % 32 != 0 and c.N % 32 < 16, None),
    # copies of row N - 1 in the column sums: where the last active wave has a padded query lane
    "pad_queries_counted": (lambda c: c.N % 16 != 0, "scal"),
    "contract_full_tiles_only": (lambda c: c.N % 16 != 0, None),
    "second_chunk_dropped": (lambda c: c.N > R.CH, "dk"),
    "scal_stride_np": (_np_partial, "scal"),
    "ds_without_scale": (lambda c: c.N > 1, "dq"),
    # the weak key's P0 entries, e^-12 / N and below, are under fp16's 2^-14 normal range (N = 15, 16: from 2.7 x the bound upwards)
    "p0_fp16": (lambda c: c.family == "edge" and c.N >= 15, None),
}


@pytest.mark.parametrize("mistake", sorted(MUST_FAIL))
def test_one_mistake_is_over_a_bound_of_check(mistake):
    """Worst error / bound over the edge and scale cases.  Measured (cases over a bound of the 66; the figures of those):
        pad_mask_last_tile_only   28   lse / saved vectors 13 .. 6.5e5 (N = 1: o is no longer v); the others have no padding key in tile NT - 2
        pad_queries_counted       47   saved vectors 58 .. 4.1e6; the others have N % 16 == 0
        contract_full_tiles_only  47   dk / dv 14 .. 39 (N = 1: dv is no longer dO)
        second_chunk_dropped      33   dk 16 .. 46: every N > 128, no other
        scal_stride_np            55   NaN in the saved vectors: every N that is no multiple of 32
        ds_without_scale          65   dq 233 = (1 / scale - 1) / 3e-2 at scale 0.125, 133 .. 500 at the other scales; N = 1 has dS = 0
        p0_fp16                   54   2.7 .. 23 on all 47 edge cases from N = 15 on (asserted); 7 scale cases, 33 at scale 0.2 (the weak
                                       key's rows are lost outright); N <= 5 has no weak key
    Every case the mistake cannot touch stays where the restatement without it is."""
    must, tensor = MUST_FAIL[mistake]
    hit = {}
    for c in SMALL:
        r = R.check(c, R.restated(c, mistake))
        if must(c):
            assert _worst(r) > 1.0, (mistake, R.case_id(c), r)
            if tensor is not None:
                assert r[tensor] > 1.0, (mistake, R.case_id(c), tensor, r)
            hit[R.case_id(c)] = _worst(r)
        elif mistake != "p0_fp16":                                  # (fp16 costs the other cases something, not everything)
            assert _worst(r) <= 1e-2, (mistake, R.case_id(c), r)
    finite = [v for v in hit.values() if v < math.inf]
    print(f"{mistake}: {len(hit)} of {len(SMALL)} cases over a bound, error / bound {min(hit.values()):.3g} .. {max(hit.values()):.3g}"
          + (f" (largest finite {max(finite):.3g})" if finite else ""))
    assert hit
    assert set(MUST_FAIL) | {"stale_k_image"} == set(R.MISTAKES)


def test_check_rules():
    c = next(k for k in R.EDGE_CASES if k.N == 33)
    ref = R.reference(c)
    same = {k: v.clone() for k, v in ref.items()}
    assert _worst(R.check(c, same)) == 0.0
    where = {}
    got = {k: v.clone() for k, v in ref.items()}
    got["dk"][1, 0, 32] *= 1.05                                     # one row of one head, 5 %: 1 / 132 of the tensor
    r = R.check(c, got, where=where)
    assert 1.6 < r["dk"] < 1.7 and where["dk"] == "head 2 (b 1, h 0) row 32" and max(v for k, v in r.items() if k != "dk") == 0.0
    got = {k: v.clone() for k, v in ref.items()}
    got["scal"][0, 1, 5, 32] *= 1.002
    assert 1.9 < R.check(c, got)["scal"] < 2.1
    got = {k: v.clone() for k, v in ref.items()}
    got["o"][0, 0, 7, 3] = float("nan")
    assert R.check(c, got)["o"] == math.inf
    one = R.EDGE_CASES[0]
    assert one.N == 1
    i = R.inputs(one)
    q, k, v = R.heads(i["qkv"].double(), one.B, 1, one.H, R.DH)
    dO = R.heads(i["dout"].double(), one.B, 1, one.H, R.DH)[0]
    ref = R.reference(one)
    assert torch.equal(ref["o"], v) and torch.equal(ref["dv"], dO) and bool((ref["dq"] == 0).all()) and bool((ref["dk"] == 0).all())
    got = {k_: v_.clone() for k_, v_ in ref.items()}
    assert _worst(R.check(one, got)) == 0.0
    slip = 2.0 ** -24 * (dO * v).abs().sum(dim=-1, keepdim=True)    # one fp32 rounding of |dO|.|v|
    got["dq"] = one.scale * slip * k
    assert 0 < R.check(one, got)["dq"] < 1.0
    got["dq"] = 1e-3 * one.scale * (dO * v).sum(dim=-1, keepdim=True) * k
    assert R.check(one, got)["dq"] > 1.0
    got = {k_: v_.clone() for k_, v_ in ref.items()}
    got["dv"][0, 0, 0, 5] += 2.0 ** -10                             # bit for bit
    assert R.check(one, got)["dv"] == math.inf
