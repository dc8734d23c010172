"""CPU: tests/gemm_epi_ref.py judged on itself.  The fp64 definitions are torch's GELU and its derivative; the operand range
conditions hold for every record of tests/gemm_paths.py; both restatements of the GELU stay inside the counted bounds (worst
error / bound printed, and not below 0.02: a bound that loose would not be a counted one; bf16 stores are held to the
interval of gemm_epi_ref's docstring, and the figure against 2^-9 |ref| (1 + 2^-8) + delta, which nearest-even itself exceeds, is
printed: 1.969 for g, 1.984 for g'); and every wrong kernel of
gemm_epi_ref.MISTAKES / TN_MISTAKES -- an edit of the restatement -- fails the shared judge on exactly the checks EXPECT names.

The last two tests are the gap the exact dense operands close: a K element dropped for the rows m with m % K != k, and the token
rows t >= M dropped from the weight gradient, both PASS the one-hot placement inputs of test_gemm_paths_gpu.py (A with its 1 at
m % K; A = [I; 0]) and fail the dense operands."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_epi_ref as R  # noqa: E402
import gemm_paths as GP  # noqa: E402
from gemm_epi_ref import (BF16, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_Q8, EPI_BIAS_RESIDUAL, EPI_DGELU, EPI_DGELU_Q8,  # noqa: E402
                          EPI_NONE, F32)

# a small record of its own for the mistake table: two column tiles (256 + 64 columns), M > 2 K, N % 64 == 0
HOST = GP._nt(193, 320, 72, 128, 256, False, 4)


def test_epilogue_ids_are_the_librarys():
    from noise_robust_vit_amd import _lib
    assert (_lib.EPI_NONE, _lib.EPI_BIAS, _lib.EPI_BIAS_GELU, _lib.EPI_BIAS_RESIDUAL, _lib.EPI_DGELU, _lib.EPI_BIAS_GELU_Q8,
            _lib.EPI_DGELU_Q8) == (EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESIDUAL, EPI_DGELU, EPI_BIAS_GELU_Q8, EPI_DGELU_Q8)


def test_fp64_definitions_are_torchs_gelu():
    u = torch.cat([R.LADDER.double(), torch.linspace(-10.0, 10.0, 4001, dtype=torch.float64)]).requires_grad_(True)
    g = torch.nn.functional.gelu(u)
    dg, = torch.autograd.grad(g.sum(), u)
    assert float((R.gelu64(u.detach()) - g.detach()).abs().max()) <= 1e-12
    assert float((R.dgelu64(u.detach()) - dg).abs().max()) <= 1e-12
    c, s = R.nt_ref64(torch.tensor([[2.0]]), EPI_BIAS_GELU, torch.tensor([0.5]))
    assert float(c) == float(R.gelu64(torch.tensor(2.5))) and float(s) == float(R.dgelu64(torch.tensor(2.5)))
    assert float(R.nt_ref64(torch.tensor([[3.0]]), EPI_DGELU_Q8, aux=torch.tensor([[228]], dtype=torch.uint8))[0]) == 3.0


def test_q8_layout_round_trips():
    for M, N, ld in ((7, 64, 64), (6, 128, 160), (1, 192, 192)):
        q = torch.randint(0, 255, (M, N), generator=R._gen("q8", M, N)).to(torch.uint8)
        flat = R.q8_store(q, ld)
        assert torch.equal(R.q8_load(flat, M, N, ld), q)
        assert int((flat != 255).sum()) <= M * N                      # nothing else is written
        offs = R.q8_offset(torch.arange(M)[:, None], torch.arange(N)[None, :], ld).reshape(-1)
        assert len(set(offs.tolist())) == M * N and int(offs.max()) < (M + 1) // 2 * 2 * ld
    # include/nrv.h by hand: byte (3, 70) of a stream with ld = 160 lies in pair 1, block 1, second row, column 6
    assert R.q8_offset(3, 70, 160) == 1 * 320 + 128 + 64 + 6
    # remap_row: group 65 with a class-token slot
    assert [R.remap_row(m, 65, 66, 1) for m in (0, 64, 65, 194)] == [1, 65, 67, 197]


# ---------------------------------------------------------------------------------------------- range conditions
@pytest.mark.parametrize("name", [r.name for r in GP.NT_TABLE])
def test_nt_operand_conditions(name):
    rec = GP.nt(name)
    ops = R.dense_exact(rec)
    acc = ops["acc"]
    assert torch.equal(acc.double(), ops["A"].double() @ ops["B"].double().t()), "the fp32 accumulator is not the fp64 one"
    assert float(acc.abs().max()) <= 128 and float((acc + ops["bias"] + ops["aux32"]).abs().max()) <= 256
    assert torch.equal(ops["aux16"].float(), ops["aux32"])
    for epi, aux in ((EPI_NONE, None), (EPI_BIAS, None), (EPI_BIAS_RESIDUAL, ops["aux32"]), (EPI_DGELU, ops["auxg"])):
        ref, _ = R.nt_ref64(acc, epi, ops["bias"], aux)
        got, _ = R.epilogue(acc, epi, F32, ops["bias"], aux)
        assert torch.equal(got.double(), ref), f"epilogue {epi} is not exact in fp32"
        if epi != EPI_DGELU:
            assert torch.equal(R.epilogue(acc, epi, BF16, ops["bias"], aux)[0].double(), ref), f"epilogue {epi}: not exact in bf16"
    fr = R.fractional_aux(rec, ops)
    x64 = acc.double() + ops["bias"].double() + fr["aux32"].double()
    x32, _ = R.epilogue(acc, EPI_BIAS_RESIDUAL, F32, ops["bias"], fr["aux32"])
    assert torch.equal(x32.double(), x64), "(acc + bias) + aux is not exact in fp32"
    band, odd = fr["band"], fr["odd"]
    assert torch.equal(fr["aux32"], torch.round(fr["aux32"] * 4096) / 4096)
    assert float((x32.to(BF16).float() != x32)[:, ~band].float().mean()) > 0.9, "most sums must not be bf16 numbers"
    # the band: the last 8-column chunk of the ragged column tile, both halves in every column tile, and exact ties
    assert bool(band[rec.N - 8:].all()) and bool(odd[rec.N - 4:].all()) and not bool(odd[rec.N - 8:rec.N - 4].any())
    for n0 in range(0, rec.N, rec.tile_n):
        cols = slice(n0, min(rec.N, n0 + rec.tile_n))
        assert bool((band & ~odd)[cols].any()) and bool((band & odd)[cols].any())
    bits = x32[:, band].contiguous().view(torch.int32)
    assert bool(((bits & 0xFFFF) == 0x8000).all()), "not half way between two bf16 numbers"
    assert torch.equal(((bits >> 16) & 1).bool(), odd[band][None, :].expand(rec.M, -1)), "parity of the neighbour nearer zero"
    for with_bias in (False, True):
        lad = R.gelu_ladder(rec, with_bias)
        assert torch.equal(lad["acc"], R.accumulate(lad["A"], lad["B"]))
        u32 = lad["acc"] + lad["bias"]
        assert torch.equal(u32.double(), lad["acc"].double() + lad["bias"].double()), "u is not exact in fp32"
        assert set(lad["acc"].unique().tolist()) == set(R.LADDER.tolist()), "a ladder value no element sees"
    gd = R.gelu_dense(rec)
    assert torch.equal(gd["acc"].double(), gd["A"].double() @ gd["B"].double().t())
    u32 = gd["acc"] + gd["bias"]
    assert torch.equal(u32.double(), gd["acc"].double() + gd["bias"].double())
    assert float((u32.abs() <= 6.5).float().mean()) >= 0.9
    assert float((gd["A"].float() != 0).float().mean()) > 0.1 and float((gd["B"].float() != 0).float().mean()) > 0.2


def test_ladder_is_what_the_issue_lists():
    L = R.LADDER
    assert 0.0 in L.tolist()
    for s in (1.0, -1.0):
        for v in (2.0 ** -20, 2.0 ** -7, 6.0, 8.0, 10.0):
            assert s * v in L.tolist()
        for b in range(-6, 3):
            assert int(((L * s >= 2.0 ** b) & (L * s < 2.0 ** (b + 1))).sum()) >= 8, (s, b)
    fb = R.fractional_bias(4096, "x")
    assert torch.equal(fb, torch.round(fb * 1024) / 1024) and float(fb.min()) >= -0.5 and float(fb.max()) < 0.5


def _tn_cases():
    for rec in GP.TN_TABLE:
        yield rec.name, rec.M, rec.N, rec.T, rec.a_group
    for rec in GP.TNG_TABLE:
        for i, (M, N, _) in enumerate(rec.problems):
            yield f"{rec.name}[{i}]", M, N, rec.T, 0


@pytest.mark.parametrize("name,M,N,T,a_group", list(_tn_cases()))
def test_tn_operand_conditions(name, M, N, T, a_group):
    ops = R.tn_dense(M, N, T, a_group, name)
    c, db = R.tn_ref(ops["dY"], ops["X"], ops["c0"], ops["db0"], 1.0, 1.0, a_group, T)
    rows = R.tn_rows(T, a_group)
    absum = ops["dY"][rows].double().abs().t() @ ops["X"].double().abs() + ops["c0"].double().abs()
    assert float(absum.max()) < 2 ** 24 and float(c.abs().max()) < 2 ** 24         # every partial sum in every order
    assert ops["dY"].shape[0] == (T if not a_group else T // a_group * (a_group + 1)) and int(rows.max()) < ops["dY"].shape[0]
    for splits in (1, 2):
        kt = -(-T // 64)
        c32, db32 = R.tn_restated(ops["dY"], ops["X"], ops["c0"], ops["db0"], 1.0, 1.0, splits, kt // splits, kt % splits, a_group, T)
        assert torch.equal(c32.double(), c) and torch.equal(db32.double(), db)


# ---------------------------------------------------------------------------------------------- the bounds hold for the restatement
def _gelu_inputs(rec):
    return {"ladder": R.gelu_ladder(rec, False), "ladder_bias": R.gelu_ladder(rec, True), "gelu_dense": R.gelu_dense(rec)}


def test_restated_gelu_within_the_counted_bounds():
    """gelu_both, gelu_both4 contracted and not: g, g', their bf16 forms and the byte, over the ladder (with and without bias)
    and the dense case of three records.  The worst error / bound is printed per quantity."""
    worst, reported = {}, {}
    for rec in (HOST, GP.nt("128x256_phased_n576_k256"), GP.nt("320x256_phased_n448_k320")):
        for kind, ops in _gelu_inputs(rec).items():
            u = ops["acc"] + ops["bias"]
            g64, dg64, dg_, ddg_ = R.gelu_bounds(u)
            for what, fn in (("gelu_both", R.gelu_both), ("gelu_both4", R.gelu_both4),
                             ("gelu_both4 uncontracted", lambda x: R.gelu_both4(x, contract=False))):
                g, dg = fn(u)
                figs = {"g fp32": R.ratio((g.double() - g64).abs(), dg_),
                        "g' fp32": R.ratio((dg.double() - dg64).abs(), ddg_),
                        "g' byte": R.ratio((R.q8_pack4(dg).double() - R.q8_ref64(u)).abs(), R.q8_bound(ddg_))}
                for k, v in figs.items():
                    worst[(what, k)] = max(worst.get((what, k), 0.0), v)
                # bf16: the interval check, and the reported figure (gemm_epi_ref's docstring)
                for k, got, ref, delta in (("g bf16", R.pack_bf16x2(g), g64, dg_), ("g' bf16", R.pack_bf16x2(dg), dg64, ddg_)):
                    assert not bool(R.bf16_outside(got, ref, delta).any()), (what, k, kind)
                    key = (what, k + " (reported)")
                    reported[key] = max(reported.get(key, 0.0), R.ratio((got.double() - ref).abs(), R.bf16_bound(ref, delta)))
    for (what, k), v in sorted({**worst, **reported}.items()):
        print(f"{what:24s} {k:18s} worst error / bound {v:.3f}")
    assert all(v <= 1.0 for v in worst.values()), worst
    assert all(v >= 0.02 for v in worst.values()), ("a bound more than 50 x the restatement's error is not a counted one", worst)
    assert all(1.0 < v <= 2.0 for v in reported.values()), reported        # nearest-even itself: up to 2^-8 |ref|
    # the decode: the two rounded constants and the fma, each at most U of a term below 1.27
    q = torch.arange(0, 255, dtype=torch.uint8)
    assert float((R.q8_unpack4(q).double() - (q.double() - 26.0) / 202.0).abs().max()) <= 3 * 1.27 * 2.0 ** -24


# ---------------------------------------------------------------------------------------------- wrong kernels
def nt_cases(rec):
    """{case name: (ops, epilogue, out dtype, aux)} -- the launches of tests/test_gemm_epi_edges_gpu.py on one record"""
    de = R.dense_exact(rec)
    cases = {}
    for odt, on in ((F32, "f32"), (BF16, "bf16")):
        cases[f"dense_exact/NONE/{on}"] = (de, EPI_NONE, odt, None)
        cases[f"dense_exact/BIAS/{on}"] = (de, EPI_BIAS, odt, None)
        cases[f"dense_exact/RESIDUAL_aux32/{on}"] = (de, EPI_BIAS_RESIDUAL, odt, de["aux32"])
        cases[f"dense_exact/RESIDUAL_aux16/{on}"] = (de, EPI_BIAS_RESIDUAL, odt, de["aux16"])
        cases[f"dense_exact/DGELU/{on}"] = (de, EPI_DGELU, odt, de["auxg"])
    cases["dense_exact/DGELU_Q8/bf16"] = (de, EPI_DGELU_Q8, BF16, de["auxq"])
    fr = R.fractional_aux(rec, de)
    cases["fractional_aux/RESIDUAL_aux32/bf16"] = (fr, EPI_BIAS_RESIDUAL, BF16, fr["aux32"])
    for kind, ops in _gelu_inputs(rec).items():
        cases[f"{kind}/GELU/f32"] = (ops, EPI_BIAS_GELU, F32, None)
        cases[f"{kind}/GELU/bf16"] = (ops, EPI_BIAS_GELU, BF16, None)
        cases[f"{kind}/GELU_Q8/bf16"] = (ops, EPI_BIAS_GELU_Q8, BF16, None)
    return cases


def nt_failures(cases, mistake):
    """the checks `case:check` the restatement with `mistake` fails"""
    out = set()
    for name, (ops, epi, odt, aux) in cases.items():
        acc = R.accumulate(ops["A"], ops["B"], mistake)
        c, stream = R.epilogue(acc, epi, odt, ops["bias"], aux, mistake)
        out |= {f"{name}:{k}" for k in R.failed(R.judge_nt(ops, epi, odt, aux, c, stream))}
    return out


@pytest.fixture(scope="module")
def host_cases():
    return nt_cases(HOST)


GELU_KINDS = ("ladder", "ladder_bias", "gelu_dense")
ALL_GELU_OUT = {f"{k}/{e}/{o}:out" for k in GELU_KINDS for e, o in (("GELU", "f32"), ("GELU", "bf16"), ("GELU_Q8", "bf16"))}
ALL_GELU_STREAM = {f"{k}/{e}:stream" for k in GELU_KINDS for e in ("GELU/f32", "GELU/bf16", "GELU_Q8/bf16")}
BIASED = ("ladder_bias", "gelu_dense")
Q8_STREAM = {f"{k}/GELU_Q8/bf16:stream" for k in GELU_KINDS}
BF16_EXACT = {f"dense_exact/{e}/bf16:out" for e in ("NONE", "BIAS", "RESIDUAL_aux32", "RESIDUAL_aux16", "DGELU", "DGELU_Q8")}
TIES = "fractional_aux/RESIDUAL_aux32/bf16:"

# mistake -> (the named check it must fail, every check it fails).  Integer results are bf16 numbers, so a wrong ROUNDING passes
# every dense_exact launch but DGELU's (integer x bf16 needs rounding) and shows in the GELU launches only through their bounds.
EXPECT = {
    "tanh_gelu": ("ladder/GELU/f32:out", ALL_GELU_OUT | ALL_GELU_STREAM),
    "bias_after_gelu": ("ladder_bias/GELU/f32:out", {c for c in ALL_GELU_OUT if c.split("/")[0] in BIASED}),
    "dgelu_without_u_phi": ("ladder/GELU/bf16:stream", ALL_GELU_STREAM),
    "dgelu_from_acc_without_bias": ("ladder_bias/GELU/bf16:stream", {c for c in ALL_GELU_STREAM if c.split("/")[0] in BIASED}),
    "bf16_truncate": (TIES + "ties_even_above", None),
    # integer x bf16 (16 bits) and the sums of multiples of 2^-12 hold ties of their own
    "bf16_round_half_up": (TIES + "ties_even_below", {TIES + "ties_even_below", TIES + "off_band", "dense_exact/DGELU/bf16:out"}),
    "residual_rounded_to_bf16": (TIES + "off_band", {TIES + "off_band", TIES + "ties_even_below", TIES + "ties_even_above"}),
    "bias_rounded_to_bf16": ("ladder_bias/GELU/f32:out", {c for c in ALL_GELU_OUT | ALL_GELU_STREAM if c.split("/")[0] in BIASED}),
    "dgelu_q8_rounded_twice": ("dense_exact/DGELU_Q8/bf16:out", {"dense_exact/DGELU_Q8/bf16:out"}),
    "q8_zero_25.5": ("ladder/GELU_Q8/bf16:stream", Q8_STREAM),
    "q8_scale_200": ("ladder/GELU_Q8/bf16:stream", Q8_STREAM),
    "q8_decode_200": ("dense_exact/DGELU_Q8/bf16:out", {"dense_exact/DGELU_Q8/bf16:out"}),
    "k_dropped_off_diagonal": ("dense_exact/NONE/f32:out", None),
}


def test_the_restatement_passes_every_case(host_cases):
    assert nt_failures(host_cases, None) == set()


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_each_wrong_kernel_fails_its_named_case(host_cases, mistake):
    named, every = EXPECT[mistake]
    got = nt_failures(host_cases, mistake)
    print(mistake, sorted(got))
    assert named in got, f"{mistake} passes {named}"
    if every is not None:
        assert got == every, f"{mistake}: unexpected {sorted(got - every)}, missing {sorted(every - got)}"
    if mistake == "bf16_truncate":
        # truncation is wrong wherever a result is not a bf16 number: the odd ties by name, never the even ones (the even
        # neighbour is the nearer-zero one there), and no integer result
        assert TIES + "ties_even_below" not in got and not (got & (BF16_EXACT - {"dense_exact/DGELU/bf16:out", "dense_exact/DGELU_Q8/bf16:out"}))
    if mistake == "k_dropped_off_diagonal":
        assert {c.split(":")[0] for c in got} >= {c for c in host_cases if c.split("/")[0] in ("dense_exact", "fractional_aux", "gelu_dense")}
        assert not any(c.startswith("ladder") for c in got), "the ladder's A is one-hot too: it cannot see a dropped K element"


def test_one_hot_placement_passes_a_dropped_k_element_dense_fails():
    """test_nt_placement_is_exact's operands (A one-hot at m % K, B = an integer pattern) against the kernel that skips K element
    5 for the rows m % K != 5: bit-equal.  The dense exact operands of the same record: not."""
    rec = HOST
    M, N, Kd = rec.M, rec.N, rec.K
    A = R.one_hot_A(M, Kd)
    B = (torch.arange(N * Kd, dtype=F32).reshape(N, Kd) % 13 - 6).to(BF16)
    want = B.float()[:, torch.arange(M) % Kd].t()
    assert torch.equal(R.accumulate(A, B), want)
    assert torch.equal(R.accumulate(A, B, "k_dropped_off_diagonal"), want), "the one-hot input would have noticed"
    de = R.dense_exact(rec)
    bad = R.accumulate(de["A"], de["B"], "k_dropped_off_diagonal") != de["acc"]
    assert float(bad.float().mean()) > 0.3, "the dense input does not notice"


TN_EXPECT = {"beta_per_slab": "phased_slabs_kt_r with beta = 1", "dbias_beta_ignored": "every record with dbias",
             "token_tail_dropped": "accepted_with_remainder[0]"}


@pytest.mark.parametrize("mistake", R.TN_MISTAKES)
def test_each_wrong_tn_kernel_fails_its_named_case(mistake):
    assert mistake in TN_EXPECT
    failing = set()
    for rec in GP.TN_TABLE:
        ops = R.tn_dense(rec.M, rec.N, rec.T, rec.a_group, rec.name)
        for beta in sorted({rec.beta, 1.0}):
            c, db = R.tn_ref(ops["dY"], ops["X"], ops["c0"], ops["db0"], beta, 1.0, rec.a_group, rec.T)
            c32, db32 = R.tn_restated(ops["dY"], ops["X"], ops["c0"], ops["db0"], beta, 1.0, rec.splits, rec.kt_q, rec.kt_r,
                                      rec.a_group, rec.T, mistake)
            if not torch.equal(c32.double(), c):
                failing.add((rec.name, beta, "C"))
            if rec.dbias and not torch.equal(db32.double(), db):
                failing.add((rec.name, beta, "dbias"))
    grp = GP.TNG_TABLE[0]
    M, N, _ = grp.problems[0]
    ops = R.tn_dense(M, N, grp.T, 0, f"{grp.name}[0]")
    c, db = R.tn_ref(ops["dY"], ops["X"], None, None, 0.0, 0.0)
    c32, db32 = R.tn_restated(ops["dY"], ops["X"], None, None, 0.0, 0.0, mistake=mistake)
    if not (torch.equal(c32.double(), c) and torch.equal(db32.double(), db)):
        failing.add((f"{grp.name}[0]", 0.0, "C+dbias"))
    print(mistake, sorted(failing))
    two_split = {r.name for r in GP.TN_TABLE if r.splits > 1}
    if mistake == "beta_per_slab":
        assert failing == {(n, 1.0, "C") for n in two_split} and "phased_slabs_kt_r" in two_split
    elif mistake == "dbias_beta_ignored":
        assert failing == {(r.name, b, "dbias") for r in GP.TN_TABLE if r.dbias for b in {r.beta, 1.0}}
    else:
        # no single record has a token t >= M (T < M in all of them): only the grouped problem can see this one
        assert all(r.T < r.M for r in GP.TN_TABLE) and failing == {(f"{grp.name}[0]", 0.0, "C+dbias")}


def test_identity_rows_pass_a_dropped_token_tail_dense_fails():
    """test_tn_grouped_record's exact operands (A = [I; 0], B an integer pattern) against the kernel that drops the token rows
    t >= M: bit-equal in C and dbias.  The dense exact operands: not."""
    grp = GP.TNG_TABLE[0]
    T = grp.T
    for M, N, _ in grp.problems:
        A1 = torch.zeros(T, M, dtype=BF16)
        A1[torch.arange(M), torch.arange(M)] = 1.0
        B1 = (torch.arange(T * N, dtype=F32).reshape(T, N) % 11 - 5).to(BF16)
        c, db = R.tn_restated(A1, B1, None, None, 0.0, 0.0, mistake="token_tail_dropped")
        assert torch.equal(c, B1.float()[:M]) and torch.equal(db, torch.ones(M)), "the identity input would have noticed"
        ops = R.tn_dense(M, N, T, 0, "tail", M, N)
        c, db = R.tn_restated(ops["dY"], ops["X"], None, None, 0.0, 0.0, mistake="token_tail_dropped")
        c64, db64 = R.tn_ref(ops["dY"], ops["X"])
        assert float((c.double() != c64).float().mean()) > 0.5 and float((db.double() != db64).float().mean()) > 0.5
