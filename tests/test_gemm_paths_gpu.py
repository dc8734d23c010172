"""GPU: every record of tests/gemm_paths.py -- all five NT tile configurations on both kernels with every epilogue, output and
aux type, and every TN / grouped-TN branch -- at small shapes, with the launches planned for 8 CUs.

The module fixture reserves the device's CUs minus 8 (`nrv_set_reserved_cus`) and restores 0.  Every test first asks the library
what it would launch (`nrv_gemm_nt_plan` / `nrv_gemm_tn_plan`) and compares with the record, so that on a part with another CU
count a test fails instead of quietly covering another variant.

NT, per record:
  * placement, exact: A is one-hot (row m has its 1 at column m % K), B holds small integers in an asymmetric pattern, so
    C[m, n] = B[n, m % K] bit for bit in fp32 and bf16;
  * values: random bf16 operands against the float64 product of the same values, per element:
        fp32 out          |c - ref| <= 1e-5 sqrt(K) max|ref|                  (test_kernels_gpu.py: test_gemm_nt_plain, ..._persistent_...)
        bf16 out          |c - ref| <= |ref| 2^-8 + 1e-3 max|ref|             (test_gemm_nt_plain)
        GELU, bf16 out    |c - ref| <= |ref| 2^-7 + 2e-3 max|ref|             (..._persistent_workgroups_every_tile_every_time)
        gelu' bf16 stream |u - ref| <= |ref| 2^-8 + 3e-4     bf16 rounding + the erf approximation test_gemm_nt_gelu_stream_8bit allows
        gelu' byte stream |u - ref| <= 0.5 / 202 + 3e-4, h bit-equal to the bf16-stream epilogue's (test_gemm_nt_gelu_stream_8bit)
    The error of torch's own fp32 product against the same float64 reference is printed as a control; the fp32 bound was at
    least 400 x that control on every record when the table was made (MI355X), so no record documents a tight bound
    here: tests/gemm_epi_ref.py and test_gemm_epi_edges_gpu.py pin the same records per element, bit for bit on exact integer
    accumulators and within counted bounds for the GELU epilogues.
  * sentinels: C, aux_out and the byte stream live in padded allocations, operands have leading dimensions above K and N;
    nothing outside [0:M, 0:N] changes (odd M: the second row of the last byte-stream pair stays untouched);
  * a second launch of a phased record is bit-identical.
A failure names the first bad element's tile (row, column), its position in the launch order, the walk (position // grid) of
its workgroup and the offset inside the tile, and counts the bad tiles per walk: a broken later walk reads differently from a
broken ragged tail.

TN, per record: float64 reference at 2e-5 sqrt(T) of the tile's max (test_gemm_tn's bound, applied per 256 x 256 tile), dbias
against float64 column sums at 1e-5 sqrt(T), beta = 1, sentinels around C with ldc > N, the exact one-hot check (A = [I; 0], so
C is a row block of B) and a bit-identical second launch.  The grouped launch gets the same checks per problem and is compared
with the single launches."""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_paths as GP  # noqa: E402
from noise_robust_vit_amd import _lib  # noqa: E402
from noise_robust_vit_amd import kernels as K  # noqa: E402
from noise_robust_vit_amd._lib import (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_Q8, EPI_BIAS_RESIDUAL, EPI_DGELU,  # noqa: E402
                                       EPI_DGELU_Q8, EPI_NONE)

pytestmark = pytest.mark.gpu

PLANNED = 8
PADR, PADC, S = 5, 24, 512.0          # sentinel rows / columns / value (exact in bf16)
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def planned8(dev):
    """Every launch of this module is planned for 8 CUs."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert cus - PLANNED >= 0
    prev = K.set_reserved_cus(cus - PLANNED)
    try:
        assert prev == 0, f"reservation was {prev}, not 0"
        yield cus
    finally:
        K.set_reserved_cus(0)


def rnd(shape, dev, seed, scale=1.0, dtype=BF16):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)


def wide(t, extra):
    """The same values with a leading dimension `extra` elements above the width."""
    big = torch.zeros(t.shape[0], t.shape[1] + extra, dtype=t.dtype, device=t.device)
    big[:, :t.shape[1]] = t
    return big[:, :t.shape[1]]


def padded(M, N, dtype, dev, padc=PADC):
    big = torch.full((M + 2 * PADR, N + padc), S, dtype=dtype, device=dev)
    return big, big[PADR:PADR + M, :N]


def assert_untouched_outside(big, M, N, what, rec=None):
    """Only [0:M, 0:N] of the padded allocation changed.  The report gives the first changed sentinel in C's coordinates and,
    for an NT record, the tile beside it (the one whose range check let the store through) with its walk."""
    guard = big.clone()
    guard[PADR:PADR + M, :N] = S
    bad = guard != S
    if bool(bad.any()):
        r, c = (int(v) for v in bad.nonzero()[0])
        m, n = r - PADR, c
        msg = f"{what}: wrote outside [0:{M}, 0:{N}]: {int(bad.sum())} sentinels changed, first at row {m}, column {n}"
        if rec is not None:
            tr, tc, t, walk = GP.tile_of(rec, min(max(m, 0), M - 1), min(n, N - 1))
            msg += f", beside tile (row {tr}, column {tc}), launch position {t}, walk {walk} of workgroup {t % rec.grid}"
        raise AssertionError(msg)


# ---------------------------------------------------------------------------------------------- failure reports
def where_bad_nt(bad, rec):
    """`bad`: bool [M, N].  First bad element by tile, launch position, walk and offset; bad tiles per walk."""
    idx = bad.nonzero()
    m, n = int(idx[0, 0]), int(idx[0, 1])
    tr, tc, t, walk = GP.tile_of(rec, m, n)
    tiles = {(int(a) // rec.tile_m, int(b) // rec.tile_n) for a, b in idx[:: max(1, len(idx) // 4096)].tolist()}
    per_walk = {}
    for a, b in tiles:
        w = GP.tile_of(rec, a * rec.tile_m, b * rec.tile_n)[3]
        per_walk[w] = per_walk.get(w, 0) + 1
    return (f"{rec.name}: {len(idx)} of {bad.numel()} elements bad; first at ({m}, {n}) = tile (row {tr}, column {tc}), launch "
            f"position {t}, walk {walk} of workgroup {t % rec.grid}, offset ({m - tr * rec.tile_m}, {n - tc * rec.tile_n}) in the "
            f"tile; bad tiles per walk {dict(sorted(per_walk.items()))}")


def assert_same_nt(got, ref, rec, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype
    if not torch.equal(got, ref):
        raise AssertionError(what + " " + where_bad_nt((got != ref) | got.isnan(), rec))


def assert_within_nt(got, ref, bound, rec, what):
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        raise AssertionError(f"{what}: worst error {float(err[bad].max()):.3e} (bound at that element "
                             f"{float((bound if bound.dim() else bound.expand_as(err))[bad][err[bad].argmax()]):.3e}); "
                             + where_bad_nt(bad, rec))


def test_report_names_tile_walk_and_offset():
    rec = GP.nt("192x256_phased_n520_k192")
    bad = torch.zeros(rec.M, rec.N, dtype=torch.bool)
    bad[0:192, 256:300] = True                              # tile id 1: launch position 8, the second walk of workgroup 0
    msg = where_bad_nt(bad, rec)
    assert "first at (0, 256) = tile (row 0, column 1), launch position 8, walk 1 of workgroup 0, offset (0, 0)" in msg, msg
    assert "bad tiles per walk {1: 1}" in msg, msg
    bad = torch.zeros(rec.M, rec.N, dtype=torch.bool)
    bad[rec.M - 1, rec.N - 8:] = True                       # the ragged corner: last tile row, last tile column
    msg = where_bad_nt(bad, rec)
    assert "tile (row 6, column 2)" in msg and "offset (128, 0)" in msg, msg


# ---------------------------------------------------------------------------------------------- NT
def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def q8_rows(qbig, M, N, ld):
    """The byte stream's rows [M, N] out of its row-pair storage (include/nrv.h), and the pairs themselves."""
    ME = (M + 1) // 2 * 2
    pairs = qbig[PADR:PADR + ME].reshape(ME // 2, 2 * ld)
    q = pairs[:, :2 * N].reshape(ME // 2, N // 64, 2, 64).permute(0, 2, 1, 3).reshape(ME, N)[:M]
    return q, pairs


@pytest.fixture(scope="module")
def nt_operands(dev):
    """Per record: random operands with their own leading dimensions and the float64 accumulator, computed once."""
    cache = {}

    def get(rec):
        if rec.name not in cache:
            A = wide(rnd((rec.M, rec.K), dev, 70, 0.5), 8)
            B = wide(rnd((rec.N, rec.K), dev, 71, 0.2), 16)
            bias = rnd((rec.N,), dev, 72, 1.0, F32)
            acc = A.double() @ B.double().t()
            cache.clear()                                   # one record's operands at a time
            cache[rec.name] = (A, B, bias, acc)
        return cache[rec.name]
    return get


@pytest.mark.parametrize("name", [r.name for r in GP.NT_TABLE])
def test_nt_placement_is_exact(dev, planned8, name):
    rec = GP.nt(name)
    M, N, Kd = rec.M, rec.N, rec.K
    assert K.gemm_nt_plan(M, N, Kd) == rec.plan, "another variant would run on this device"
    col = torch.arange(M, device=dev) % Kd
    A = torch.zeros(M, Kd + 8, dtype=BF16, device=dev)
    A[torch.arange(M, device=dev), col] = 1.0
    B = wide((torch.arange(N * Kd, device=dev, dtype=F32).reshape(N, Kd) % 13 - 6).to(BF16), 16)
    want = B.float()[:, col].t().contiguous()
    for odt in (F32, BF16):
        big, out = padded(M, N, odt, dev)
        K.gemm_nt(A[:, :Kd], B, out=out)
        assert_same_nt(out.contiguous(), want.to(odt), rec, f"one-hot A, {odt}:")
        assert_untouched_outside(big, M, N, f"{name} {odt}", rec)
        if rec.phased:
            big2, out2 = padded(M, N, odt, dev)
            K.gemm_nt(A[:, :Kd], B, out=out2)
            assert torch.equal(big, big2), f"{name} {odt}: a second launch differs"


def _nt_case(rec, ops, dev, epi, odt, adt=None):
    """One launch into padded allocations: (C big, C view, aux_out big | None, aux_out view | None, float64 reference, aux)."""
    A, B, bias, acc = ops
    M, N = rec.M, rec.N
    big, out = padded(M, N, odt, dev)
    aux = ubig = u = None
    if epi == EPI_BIAS_RESIDUAL:
        aux = wide(rnd((M, N), dev, 73, 1.0, adt), 16)
        ref = acc + bias.double() + aux.double()
    elif epi == EPI_DGELU:
        aux = wide(rnd((M, N), dev, 74, 1.0), 8)
        ref = acc * aux.double()
    elif epi == EPI_BIAS_GELU:
        ubig, u = padded(M, N, BF16, dev)
        ref = gelu64(acc + bias.double())
    elif epi == EPI_BIAS:
        ref = acc + bias.double()
    else:
        ref = acc
    K.gemm_nt(A, B, epilogue=epi, bias=bias if epi in (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESIDUAL) else None, aux=aux, aux_out=u,
              out=out)
    return big, out, ubig, u, ref, aux


NT_CASES = [(EPI_NONE, None), (EPI_BIAS, None), (EPI_BIAS_GELU, None), (EPI_BIAS_RESIDUAL, F32), (EPI_BIAS_RESIDUAL, BF16),
            (EPI_DGELU, None)]


@pytest.mark.parametrize("name", [r.name for r in GP.NT_TABLE])
def test_nt_values_epilogues_and_sentinels(dev, planned8, nt_operands, name):
    rec = GP.nt(name)
    M, N, Kd = rec.M, rec.N, rec.K
    ops = nt_operands(rec)
    A, B, bias, acc = ops
    control = float((A.float() @ B.float().t() - acc).abs().max())
    fp32_bound = 1e-5 * math.sqrt(Kd) * float(acc.abs().max())
    print(f"{name}: torch fp32 max error {control:.3e}, fp32 bound {fp32_bound:.3e} = {fp32_bound / max(control, 1e-30):.1f} x")
    for epi, adt in NT_CASES:
        assert K.gemm_nt_plan(M, N, Kd, epi) == rec.plan, "another variant would run on this device"
        for odt in (F32, BF16):
            what = f"{name} epilogue {epi} out {odt} aux {adt}"
            big, out, ubig, u, ref, _ = _nt_case(rec, ops, dev, epi, odt, adt)
            top = ref.abs().max()
            if odt == F32:
                bound = 1e-5 * math.sqrt(Kd) * top
            elif epi == EPI_BIAS_GELU:
                bound = ref.abs() * 2.0 ** -7 + 2e-3 * top
            else:
                bound = ref.abs() * 2.0 ** -8 + 1e-3 * top
            assert_within_nt(out, ref, bound, rec, what)
            assert_untouched_outside(big, M, N, what, rec)
            if u is not None:
                dref = dgelu64(acc + bias.double())
                assert_within_nt(u, dref, dref.abs() * 2.0 ** -8 + 3e-4, rec, what + " gelu' stream")
                assert_untouched_outside(ubig, M, N, what + " gelu' stream", rec)
            if rec.phased:
                big2, _, ubig2, _, _, _ = _nt_case(rec, ops, dev, epi, odt, adt)
                assert torch.equal(big, big2) and (ubig is None or torch.equal(ubig, ubig2)), what + ": a second launch differs"


@pytest.mark.parametrize("name", [r.name for r in GP.NT_TABLE if r.q8])
def test_nt_gelu_byte_stream(dev, planned8, nt_operands, name):
    rec = GP.nt(name)
    M, N, Kd = rec.M, rec.N, rec.K
    A, B, bias, acc = nt_operands(rec)
    assert K.gemm_nt_plan(M, N, Kd, EPI_BIAS_GELU_Q8) == rec.plan and K.gemm_nt_plan(M, N, Kd, EPI_DGELU_Q8) == rec.plan
    h16 = K.gemm_nt(A, B, out_dtype=BF16, epilogue=EPI_BIAS_GELU, bias=bias)
    ld, ME = N + 32, (M + 1) // 2 * 2
    runs = []
    for _ in range(2 if rec.phased else 1):
        qbig = torch.full((ME + 2 * PADR, ld), 255, dtype=torch.uint8, device=dev)
        big, out = padded(M, N, BF16, dev)
        K.gemm_nt(A, B, epilogue=EPI_BIAS_GELU_Q8, bias=bias, aux_out=qbig[PADR:PADR + ME, :N], out=out)
        runs.append((big, qbig))
    big, qbig = runs[0]
    assert all(torch.equal(big, b2) and torch.equal(qbig, q2) for b2, q2 in runs[1:]), f"{name}: a second launch differs"
    assert_same_nt(big[PADR:PADR + M, :N].contiguous(), h16, rec, "h of the byte-stream epilogue vs the bf16-stream epilogue:")
    assert_untouched_outside(big, M, N, name, rec)
    q, pairs = q8_rows(qbig, M, N, ld)
    guard = qbig.clone()
    guard[PADR:PADR + ME].reshape(ME // 2, 2 * ld)[:, :2 * N] = 255
    assert bool((guard == 255).all()), f"{name}: the byte stream was written outside its block"
    assert M % 2 == 1 and bool((pairs[-1, :2 * N].reshape(N // 64, 2, 64)[:, 1] == 255).all()), "second row of the last pair"
    g = (q.double() - 26.0) / 202.0
    dref = dgelu64(acc + bias.double())
    assert_within_nt(g, dref, torch.tensor(0.5 / 202 + 3e-4, device=dev, dtype=torch.float64), rec, f"{name} decoded gelu'")
    # the backward epilogue multiplies by the decoded value; bf16 out: the bf16 bound of the module docstring
    ref = acc * g
    runs = []
    for _ in range(2 if rec.phased else 1):
        big, out = padded(M, N, BF16, dev)
        K.gemm_nt(A, B, epilogue=EPI_DGELU_Q8, aux=qbig[PADR:PADR + ME, :N], out=out)
        runs.append(big)
    assert all(torch.equal(runs[0], b2) for b2 in runs[1:]), f"{name}: a second DGELU_Q8 launch differs"
    assert_within_nt(runs[0][PADR:PADR + M, :N], ref, ref.abs() * 2.0 ** -8 + 1e-3 * ref.abs().max(), rec, f"{name} DGELU_Q8")
    assert_untouched_outside(runs[0], M, N, name + " DGELU_Q8", rec)


# ---------------------------------------------------------------------------------------------- TN
def tile_errors(c, ref, T, what):
    """test_gemm_tn's bound per 256 x 256 tile: max error <= 2e-5 sqrt(T) x the tile's max |ref|."""
    M, N = ref.shape
    for m0 in range(0, M, 256):
        for n0 in range(0, N, 256):
            r = ref[m0:m0 + 256, n0:n0 + 256]
            e = float((c[m0:m0 + 256, n0:n0 + 256].double() - r).abs().max()) / max(float(r.abs().max()), 1e-30)
            assert e < 2e-5 * math.sqrt(T), f"{what}: tile ({m0 // 256}, {n0 // 256}) relative error {e:.3e}"


def tn_rows(rec, t, dev):
    """Row of A that token t reads (the class-token remap of the record, or the identity) and the rows A needs."""
    if rec.a_group == 0:
        return t, rec.T
    g = rec.a_group
    return t // g * (g + 1) + t % g + 1, rec.T // g * (g + 1)


def tn_launch(rec, A, B, dev, c0=None):
    M, N = rec.M, rec.N
    big, out = padded(M, N, F32, dev, rec.ldc_pad)
    if c0 is not None:
        out.copy_(c0)
    db = torch.full((M + 16,), S, device=dev) if rec.dbias else None
    g = rec.a_group
    K.gemm_tn(A, B, out=out, beta=rec.beta, a_group=g, a_group_stride=g + 1 if g else 0, a_row_offset=1 if g else 0, T=rec.T,
              dbias=None if db is None else db[:M], dbias_beta=0.0)
    return big, out, db


@pytest.mark.parametrize("name", [r.name for r in GP.TN_TABLE])
def test_tn_record(dev, planned8, name):
    rec = GP.tn(name)
    M, N, T = rec.M, rec.N, rec.T
    assert K.gemm_tn_plan(M, N, T, rec.a_group > 0, rec.beta, rec.dbias) == rec.plan, "another variant would run on this device"
    rows, arows = tn_rows(rec, torch.arange(T, device=dev), dev)
    A = wide(rnd((arows, M), dev, 40), 8)                   # rows the remap skips hold values too: they must not be read
    B = wide(rnd((T, N), dev, 41), 8)
    ref = A[rows].double().t() @ B.double()
    c0 = rnd((M, N), dev, 42, 1.0, F32) if rec.beta else None
    big, out, db = tn_launch(rec, A, B, dev, c0)
    tile_errors(out, ref + c0.double() if rec.beta else ref, T, name)
    assert_untouched_outside(big, M, N, name)
    if rec.dbias:
        sums = A[rows].double().sum(0)
        e = float((db[:M].double() - sums).abs().max() / sums.abs().max())
        assert e < 1e-5 * math.sqrt(T), f"{name}: dbias relative error {e:.3e}"
        assert bool((db[M:] == S).all()), f"{name}: dbias written behind M"
    big2, _, db2 = tn_launch(rec, A, B, dev, c0)
    assert torch.equal(big, big2) and (db is None or torch.equal(db, db2)), f"{name}: a second launch differs"
    # exact: token t holds its 1 in column t (T < M), so C[:T] = B and the rows behind are zero
    assert T < M
    A1 = torch.zeros(arows, M + 8, dtype=BF16, device=dev)
    A1[rows, torch.arange(T, device=dev)] = 1.0
    B1 = wide((torch.arange(T * N, device=dev, dtype=F32).reshape(T, N) % 11 - 5).to(BF16), 8)
    want = torch.zeros(M, N, device=dev)
    want[:T] = B1.float()
    if rec.beta:
        c0 = torch.round(c0 * 4)                            # small integers: the sum stays exact
        want = want + c0
    big, out, db = tn_launch(rec, A1[:, :M], B1, dev, c0)
    bad = out != want
    assert not bool(bad.any()), (f"{name}: one-hot A: {int(bad.sum())} bad, first at {bad.nonzero()[0].tolist()} "
                                 f"(tile {[int(v) // 256 for v in bad.nonzero()[0]]}, K-tile of row {int(bad.nonzero()[0][0]) // 64})")
    assert_untouched_outside(big, M, N, name + " one-hot")
    if rec.dbias:
        assert torch.equal(db[:M], (torch.arange(M, device=dev) < T).float())


# ---------------------------------------------------------------------------------------------- grouped TN
def grouped_bytes(rec):
    arr = (_lib.TnProblem * len(rec.problems))()
    for i, (M, N, _) in enumerate(rec.problems):
        arr[i] = _lib.TnProblem(None, M, None, N, None, N, M, N, 0.0, None, 0.0)
    return int(_lib.load().nrv_gemm_tn_grouped_workspace(ctypes.addressof(arr), len(rec.problems), rec.T))


@pytest.mark.parametrize("name", [r.name for r in GP.TNG_TABLE])
def test_tn_grouped_record(dev, planned8, name):
    rec = next(r for r in GP.TNG_TABLE if r.name == name)
    T = rec.T
    assert grouped_bytes(rec) == rec.slots * GP.SLOT_BYTES, "another plan on this device"
    probs, bigs, refs = [], [], []
    for i, (M, N, bias) in enumerate(rec.problems):
        A = wide(rnd((T, M), dev, 140 + 2 * i), 8)
        B = wide(rnd((T, N), dev, 141 + 2 * i), 8)
        big, out = padded(M, N, F32, dev, 8)
        probs.append(dict(A=A, B=B, out=out, beta=0.0, dbias=True if bias else None))
        bigs.append(big)
        refs.append((A.double().t() @ B.double(), A.double().sum(0)))
    outs = K.gemm_tn_grouped(probs)
    for (c, db), (rc, rdb), big, (M, N, bias) in zip(outs, refs, bigs, rec.problems):
        tile_errors(c, rc, T, f"{name} [{M}, {N}]")
        assert_untouched_outside(big, M, N, f"{name} [{M}, {N}]")
        if bias:
            e = float((db.double() - rdb).abs().max() / rdb.abs().max())
            assert e < 1e-5 * math.sqrt(T), f"{name}: dbias relative error {e:.3e}"
    first = [(c.clone(), None if db is None else db.clone()) for c, db in outs]
    for (c, db), (c1, db1) in zip(K.gemm_tn_grouped(probs), first):
        assert torch.equal(c, c1) and (db is None or torch.equal(db, db1)), f"{name}: a second launch differs"
    # the single launches: fp32 sums in another order (test_gemm_tn_grouped_agrees_with_the_single_launches' bound)
    for q, (c1, db1) in zip(probs, first):
        cs, dbs = K.gemm_tn(q["A"], q["B"], want_dbias=True)
        assert float((c1 - cs).abs().max() / cs.abs().max()) < 1e-5
        assert db1 is None or float((db1 - dbs).abs().max() / dbs.abs().max()) < 1e-5
    # beta = 1 accumulates into C and dbias
    probs3 = [dict(A=q["A"], B=q["B"], out=c.clone(), beta=1.0, dbias=None if db is None else db.clone(), dbias_beta=1.0)
              for q, (c, db) in zip(probs, first)]
    for (c3, db3), (rc, rdb) in zip(K.gemm_tn_grouped(probs3), refs):
        tile_errors(c3, 2 * rc, T, f"{name} beta = 1")
        assert db3 is None or float((db3.double() - 2 * rdb).abs().max() / rdb.abs().max()) < 2e-5 * math.sqrt(T)
    # exact: A = [I; 0] rows, small-integer B
    probs1, wants = [], []
    for M, N, bias in rec.problems:
        A1 = torch.zeros(T, M + 8, dtype=BF16, device=dev)
        A1[torch.arange(M, device=dev), torch.arange(M, device=dev)] = 1.0
        B1 = wide((torch.arange(T * N, device=dev, dtype=F32).reshape(T, N) % 11 - 5).to(BF16), 8)
        probs1.append(dict(A=A1[:, :M], B=B1, dbias=True if bias else None))
        wants.append(B1.float()[:M].contiguous())
    for (c, db), want, (M, N, bias) in zip(K.gemm_tn_grouped(probs1), wants, rec.problems):
        bad = c != want
        assert not bool(bad.any()), f"{name} [{M}, {N}]: one-hot A: {int(bad.sum())} bad, first at {bad.nonzero()[0].tolist()}"
        assert db is None or torch.equal(db, torch.ones(M, device=dev))
