"""CPU: the inputs, case lists and bounds of tests/attn_edges_ref.py, before any kernel is involved.

  * the case lists reach what they claim: every single-pass NT, every streaming KS, W = 1 and an odd W, a memory key at bit 31 and at
    bit 0 of a mask word and at row 63 and row 0 of a key tile, every mask shape with both kinds of memory, B across 16 with and
    without a remainder;
  * the restatement of the kernels' index rules, with no mistake in it, IS the fp64 reference (1e-9 per row);
  * rounding at the kernels' documented points costs at most EMULATION_BOUND per row (the reference's emulate_bf16 switch: P, dS, the
    bf16 outputs) and at most KERNEL_ROUNDING_BOUND with the one point that switch lacks (delta = rowsum(dO o) read from the bf16 o),
    so the GPU bound of 3e-2 is 3 x and 2 x what the format costs on these inputs;
  * each index mistake, switched on alone in the restatement, puts a listed case over the GPU bound (printed: the worst error / bound).

Measured (worst row over all cases, relative L2 against fp64): emulate_bf16 o 4.8e-3, dq 7.8e-3, dk 8.9e-3, dv 4.3e-3, memory rows
5.3e-3; kernel rounding o 4.8e-3, dq 1.37e-2, dk 1.35e-2, dv 4.3e-3, memory rows 8.2e-3.
Worst error / bound per mistake: see test_one_index_mistake_is_over_the_gpu_bound.  The eighth mistake of the list, w1 not zeroed past
the last mask word, turns out to change no result at all: test_w1_past_the_last_word_cannot_be_seen_in_a_result says why and asserts it.
"""
import math

import numpy as np
import pytest
import torch

import attn_edges_ref as R


def _shapes(cases):
    """one case per distinct set of inputs (the two layouts of a single-pass case share theirs)"""
    seen, out = set(), []
    for c in cases:
        if R._shape_key(c) not in seen:
            seen.add(R._shape_key(c))
            out.append(c)
    return out


def _worst(ratios: dict) -> float:
    return max(ratios.values())


# ---- the case lists ---------------------------------------------------------------------------------------------------------------
def test_case_lists_reach_what_they_claim():
    assert len(R.SINGLE_PASS_NS) == 32 and len(R.SINGLE_PASS_CASES) == 64
    assert {R.single_pass_nt(c.Nq) for c in R.SINGLE_PASS_CASES} == {2, 4, 6, 8, 10, 12, 13, 14, 16}
    assert {c.layout for c in R.SINGLE_PASS_CASES} == {0, 3}
    for NT in (2, 4, 6, 8, 10, 12, 13, 14, 16):
        ns = {c.Nq for c in R.SINGLE_PASS_CASES if R.single_pass_nt(c.Nq) == NT}
        assert {16 * NT, 16 * NT - 15} <= ns, NT                       # no padding; one real key in the last tile
        if NT % 2 == 0 and NT != 14:
            assert {16 * (NT - 1), 16 * (NT - 2) + 1} <= ns, NT        # a last tile of padding only, behind a full / a one-key tile
    assert 1 in R.SINGLE_PASS_NS and all(c.dh == 64 and c.Nq <= 256 for c in R.SINGLE_PASS_CASES)
    assert {R.stream_ks(c.dh) for c in R.STREAM_CASES} == {1, 2, 3, 4} and {R.stream_ks(c.dh) for c in R.WIDE_CASES} == {5, 6}
    for dh in R.STREAM_DH:
        assert {c.Nq for c in R.STREAM_CASES if c.dh == dh and c.entry == "mem"} == {1, 63, 64, 65, 129}
    assert [c for c in R.STREAM_CASES if c.entry == "attn"] == [R.Case("stream", 2, 257, 0, 2, 64, 64, True, None, "neg", "attn", 0)]
    for dh in (136, 152, 160, 168, 192):
        assert {c.Nq for c in R.WIDE_CASES if c.dh == dh} == {1, 64, 65, 129}
    assert {c.width for c in R.WIDE_CASES if c.dh == 152} == {147}
    # memory + mask
    W = {(c.Nq + c.M + 31) // 32 for c in R.MEM_CASES}
    assert 1 in W and any(w > 1 and w % 2 for w in W) and any(w % 2 == 0 for w in W)
    first_mem = {c.Nq for c in R.MEM_CASES if c.M > 0}
    assert {31, 32, 63, 64} <= first_mem                               # bit 31 / bit 0 of a word, row 63 / row 0 of a key tile
    assert any(c.Nq < 64 < c.Nq + c.M for c in R.MEM_CASES)            # memory rows on both sides of a tile seam
    assert {c.mask for c in R.MEM_CASES} == set(R.MASK_SHAPES) and {c.dh for c in R.MEM_CASES} == set(R.STREAM_DH)
    assert {(c.shared, c.mask) for c in R.MEM_CASES if c.M > 0} >= {(True, "b1"), (True, "2d"), (False, "1h"), (False, "bh")}
    assert all(c.B == 2 and c.H == 2 for c in R.SINGLE_PASS_CASES + R.STREAM_CASES + R.WIDE_CASES + R.MEM_CASES)
    # batch sum: one full group, a remainder of one, two groups and a remainder of three; with and without a mask; per sample once
    shared = [c for c in R.SUM_CASES if c.shared]
    assert {(c.B, c.mask is None) for c in shared} == {(B, m) for B in (16, 17, 35) for m in (False, True)}
    assert {c.B % R.MEM_SUM_GROUP for c in shared} == {0, 1, 3} and max(-(-c.B // R.MEM_SUM_GROUP) for c in shared) == 3
    assert [(c.B, c.shared) for c in R.SUM_CASES if not c.shared] == [(17, False)]
    assert len({R.case_id(c) for c in R.ALL_CASES}) == len(R.ALL_CASES)


@pytest.mark.parametrize("c", R.MEM_CASES + R.SUM_CASES[:1], ids=R.case_id)
def test_masks_hold_the_loud_keys_and_the_structural_rows(c):
    i = R.inputs(c)
    Nq, Nk = c.Nq, c.Nq + c.M
    m = i["mask"].reshape((1,) * (4 - i["mask"].dim()) + tuple(i["mask"].shape))
    assert m.shape[0] == (c.B if c.mask in ("b1", "bh") else 1) and m.shape[1] == (c.H if c.mask in ("1h", "bh") else 1)
    rows = R.structural_rows(Nq, Nk)
    special = set(rows.values())
    for j in R.loud_positions(Nq, c.M):
        for q in range(Nq):
            if q not in special:
                assert bool((m[..., q, j] == bool(q % 2)).all()), (q, j)
    assert not bool(m[..., rows["full"], :].any()) and rows["full"] >= 64 * ((Nq - 1) // 64)
    assert bool((m[..., rows["two"], :].sum(dim=-1) == 2).all())
    if "first_tile" in rows:
        assert not bool(m[..., rows["first_tile"], :64].any()) and bool(m[..., rows["first_tile"], 64:].any())
    if "last_tile" in rows:
        assert not bool(m[..., rows["last_tile"], 64 * ((Nk - 1) // 64):].any())
    assert any("first_tile" in R.structural_rows(k.Nq, k.Nq + k.M) for k in R.MEM_CASES)
    # every query scores every loud key ~ 8 nats above the best other key's typical score
    q, k, _ = R.heads(i["qkv"].double(), c.B, Nq, c.H, c.dh)
    s = q @ k.transpose(-1, -2) * i["scale"]
    loud = [j for j in R.loud_positions(Nq, c.M) if j < Nq]
    rest = [j for j in range(Nq) if j not in loud]
    gap = s[..., loud].mean() - s[..., rest].mean()
    assert abs(gap.item() - R.NATS) < 0.5, gap


def test_pack_bits_is_bit_key_and_31_of_word_key_shift_5():
    g = torch.Generator().manual_seed(3)
    m = torch.rand(2, 3, 5, 70, generator=g) < 0.5
    bits, bs, hs = R.pack_bits(m, 5, 70)
    assert (bs, hs) == (3 * 5 * 3, 5 * 3) and tuple(bits.shape) == (30, 3)
    words = bits.numpy().view(np.uint32)
    flat = m.reshape(-1, 70)
    for r in range(30):
        for k in range(70):
            assert bool((int(words[r, k >> 5]) >> (k & 31)) & 1) == bool(flat[r, k])
        assert int(words[r, 2]) >> 6 == 0                               # the bits past Nk are zero
    assert R.pack_bits(m[0, 0], 5, 70)[1:] == (0, 0) and R.pack_bits(m[:1], 5, 70)[1:] == (0, 15) and R.pack_bits(m[:, :1], 5, 70)[1:] == (15, 0)


# ---- the restatement and the bounds -----------------------------------------------------------------------------------------------
def test_restatement_without_a_mistake_is_the_reference():
    for c in _shapes(R.ALL_CASES):
        r = R.check(c, R.restated(c))
        assert _worst(r) <= 1e-9 / R.PER_ROW_BOUND, (R.case_id(c), r)


def test_rounding_at_the_kernels_points_stays_inside_the_emulation_bounds():
    worst = {"emulate_bf16": {}, "kernel rounding": {}}
    bad = []
    for c in _shapes(R.ALL_CASES):
        ref = R.reference(c)
        for tag, got, bound in (("emulate_bf16", R.reference(c, emulate_bf16=True), R.EMULATION_BOUND),
                                ("kernel rounding", R.restated(c, kernel_rounding=True), R.KERNEL_ROUNDING_BOUND)):
            for name in ("o",) + R.gradient_names(c):
                e = R.per_row_rel(got[name], ref[name]).max().item()
                key = "memory rows" if name.startswith("dmem") else name
                worst[tag][key] = max(worst[tag].get(key, 0.0), e)
                if not e <= bound:
                    bad.append((R.case_id(c), tag, name, e))
    for tag, w in worst.items():
        print(f"{tag}: worst row over all cases " + "  ".join(f"{k} {v:.2e}" for k, v in w.items()))
    assert not bad, bad


def test_check_rules_for_zero_rows_and_fully_masked_lse():
    c = R.MEM_CASES[6]
    ref = R.reference(c)
    full_q = R.structural_rows(c.Nq, c.Nq + c.M)["full"]
    assert bool(ref["full"][:, :, full_q].all()) and int(ref["full"].sum()) == c.B * c.H
    assert bool((ref["dq"][:, :, full_q] == 0).all()) and bool((ref["lse"][ref["full"]] == -R.FLT_MAX).all())
    mean_v = torch.cat([R.heads(R.inputs(c)["qkv"].double(), c.B, c.Nq, c.H, c.dh)[2],
                        R.inputs(c)["mkv"].double().reshape(1, c.M, 2, c.H, c.dh)[:, :, 1].permute(0, 2, 1, 3).expand(c.B, -1, -1, -1)], dim=2).mean(dim=2)
    assert (ref["o"][:, :, full_q] - mean_v).abs().max().item() < 1e-12            # uniform over the Nk keys
    got = {k: v.clone() for k, v in ref.items()}
    assert _worst(R.check(c, got)) == 0.0
    got["dq"][0, 1, full_q, 3] = 1e-30                                              # a zero row must be exactly zero
    assert R.check(c, got)["dq"] == math.inf
    got = {k: v.clone() for k, v in ref.items()}
    got["lse"][0, 0, full_q] = -R.FLT_MAX * (1 - 2.0 ** -24)
    assert R.check(c, got)["lse"] == math.inf
    got = {k: v.clone() for k, v in ref.items()}
    got["dk"][1, 0, 7] = float("nan")
    assert R.check(c, got)["dk"] == math.inf
    w = R.WIDE_CASES[5]                                                             # dh 152, width 147: a pad column
    assert w.width == 147
    got = {k: v.clone() for k, v in R.reference(w).items()}
    assert bool((got["dv"][..., 147:] == 0).all()) and _worst(R.check(w, got)) == 0.0
    got["dv"][0, 0, 3, 150] = 1e-30
    assert R.check(w, got)["dv"] == math.inf
    one = R.STREAM_CASES[0]                                                         # one key: dq and dk are a cancellation
    assert one.Nq == 1
    got = {k: v.clone() for k, v in R.reference(one).items()}
    assert bool((got["dq"] == 0).all()) and bool((got["dk"] == 0).all())
    i = R.inputs(one)
    q, k, v = R.heads(i["qkv"].double(), one.B, 1, one.H, one.dh)
    dO = R.heads(i["dout"].double(), one.B, 1, one.H, one.dh)[0]
    slip = 2.0 ** -24 * (dO * v).abs().sum(dim=-1, keepdim=True)                    # one fp32 rounding of |dO|.|v|
    got["dq"] = i["scale"] * slip * k
    assert 0 < R.check(one, got)["dq"] < 1.0
    got["dq"] = 1e-3 * i["scale"] * (dO * v).sum(dim=-1, keepdim=True) * k          # a thousandth of one of the two sums: far too much
    assert R.check(one, got)["dq"] > 1.0


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------
_MASKED = [c for c in R.MEM_CASES + R.SUM_CASES if c.mask]
_SHARED_SUM = [c for c in R.SUM_CASES if c.shared]
_NEG = _shapes(R.SINGLE_PASS_CASES + R.STREAM_CASES + R.WIDE_CASES)
WHERE = {
    "mask_bit": _MASKED,                                         # key j read from bit (j & 31) + 1
    "mem_row": [c for c in R.MEM_CASES + R.SUM_CASES if c.M],    # memory row j - Nq + 1
    "pad_le": _NEG,                                              # key <= Nk instead of key < Nk
    "uniform_padded": _MASKED,                                   # a fully masked row spread over the padded key count
    "mask_bstride": [c for c in _MASKED if c.mask in ("2d", "1h")],   # a broadcast mask stepped per sample
    "sum_remainder": _SHARED_SUM,                                # the last, partial group of samples dropped
    "sum_pass2": _SHARED_SUM,                                    # pass 2 over samples 0, 1, 2 .. instead of 0, 16, 32 ..
}


@pytest.mark.parametrize("mistake", sorted(WHERE))
def test_one_index_mistake_is_over_the_gpu_bound(mistake):
    """Worst error / GPU bound over the cases a mistake can touch.  Measured (cases over the bound, smallest .. largest figure of them):
        mask_bit        14 of 14    5.0e+3 .. 9.4e+3   (the lse of a row that gains or loses a loud key)
        mask_bstride     6 of 6     3e+41              (sample 1 reads past the words: every row fully masked, lse -FLT_MAX)
        mem_row         15 of 15    504 .. 8.7e+3
        pad_le          61 of 74    1.0e+4             (lse; every o row >= 0.5 relative; the 13 others have N % 64 == 0: no padding row)
        uniform_padded  12 of 14    8.3 .. 24.5        (o and dv of the fully masked row; the 2 others have Nk % 64 == 0)
        sum_remainder    4 of 6     3.5 .. 15.9        (B = 16 has no remainder group)
        sum_pass2        4 of 6     3.2 .. 36.5        (B = 16 has one group)"""
    per_case = {R.case_id(c): R.check(c, R.restated(c, mistake)) for c in WHERE[mistake]}
    worst = {k: _worst(v) for k, v in per_case.items()}
    finite = [v for r in per_case.values() for v in r.values() if v < math.inf]
    hit = [v for v in worst.values() if v > 1.0]
    print(f"{mistake}: {len(hit)} of {len(worst)} cases over the bound, error / bound {min(hit):.3g} .. {max(hit):.3g} (largest finite figure "
          f"{max(finite):.3g})" + ("; per case " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()) if len(worst) <= 8 else ""))
    assert max(worst.values()) > 1.0, worst
    if mistake == "pad_le":                                      # every case whose last 64-key tile has a padding row is taken over
        for c in WHERE[mistake]:
            r = per_case[R.case_id(c)]
            if c.Nq % R.GT:
                assert r["o"] > 1.0 and r["lse"] > 1.0, (R.case_id(c), r)
                ref, got = R.reference(c), R.restated(c, mistake)
                assert R.per_row_rel(got["o"], ref["o"]).min().item() >= 0.5 and (got["lse"] - ref["lse"]).min().item() >= 1.0
            else:
                assert _worst(r) <= 1e-9
    if mistake == "mask_bit":
        assert min(worst.values()) > 1.0, worst                  # every masked case
    if mistake == "uniform_padded":                              # every masked case whose key count is no multiple of the tile
        for c in WHERE[mistake]:
            assert (worst[R.case_id(c)] > 1.0) == ((c.Nq + c.M) % R.GT != 0), (R.case_id(c), per_case[R.case_id(c)])
    if mistake in ("sum_remainder", "sum_pass2"):
        for c in WHERE[mistake]:
            r = per_case[R.case_id(c)]
            assert (min(r["dmem_k"], r["dmem_v"]) > 1.0) == (c.B > R.MEM_SUM_GROUP), (R.case_id(c), r)
            assert max(r[n] for n in ("o", "lse", "dq", "dk", "dv")) <= 1e-9


def test_w1_past_the_last_word_cannot_be_seen_in_a_result():
    """mask_words zeroes w1 when the tile's second word does not exist.  Every key that word would cover is >= 32 W >= Nk: a padding key,
    which the `< Nk` test removes in the forward and in dQ and whose dK / dV lanes are never stored.  So reading anything there -- the
    next query's first word, or all ones past the end of the buffer -- changes no result bit: what the guard prevents is the read past
    the mask buffer itself, which no comparison of results can show.  Asserted here so that the claim is not only stated."""
    touched = 0
    for c in _MASKED:
        W = (c.Nq + c.M + 31) // 32
        touched += W % 2
        a, b = R.restated(c), R.restated(c, "w1_past_W")
        for name in a:
            assert torch.equal(a[name], b[name]), (R.case_id(c), name)
    assert touched >= 5                                          # cases with an odd W, where the last tile has no second word
