"""GPU: the NT / TN GEMM epilogues per element on exact accumulators (tests/gemm_epi_ref.py), on every record of
tests/gemm_paths.py, planned for 8 CUs as test_gemm_paths_gpu.py plans them (its fixture, its padded sentinel allocations, its
leading dimensions and its failure report are imported, not copied).

Per NT record, after `gemm_nt_plan == rec.plan` for the epilogue under test:
  * bit for bit (`torch.equal` against gemm_epi_ref.epilogue on the exact integer accumulator, computed on the device in fp32),
    fp32 and bf16 out: dense_exact under NONE, BIAS, BIAS_RESIDUAL (fp32 and bf16 aux), DGELU (a random bf16 operand) and, where
    N % 64 == 0, DGELU_Q8 (random bytes in the row-pair layout); gelu_dense under BIAS (u = acc + bias is what the GELU tests
    take for known); fractional_aux under BIAS_RESIDUAL with bf16 out, the tie band judged by name;
  * within the counted bounds: gelu_ladder (bias 0 and the fractional bias) and gelu_dense under BIAS_GELU, fp32 and bf16 out,
    the gelu' bf16 stream, and on the N % 64 == 0 records the byte stream with h bit-equal to the bf16-stream epilogue's.
    The worst error / bound per quantity is printed (DESIGN.md holds the MI355X figures);
  * every launch runs twice into fresh sentinel allocations and both must be bit-identical, nothing outside [0:M, 0:N] changed.
The epilogue_remap path (out_group / aux_row_mod, plain 256 x 256 kernel): dense_exact bit for bit with both aux row rules and the
fractional residual with its ties at the remapped row; the library takes the remap with BIAS_RESIDUAL only, so BIAS_GELU there
must be refused with nothing written.
Per TN record and grouped-TN group: dense exact operands, integer start values in C (padding columns and guard rows around it)
and dbias (guard behind it) with dbias_beta = 1 and the record's beta, and again with beta = 1; `torch.equal` against the
integer reference; the deferred form + flush_reduce and the grouped launch give the same buffers as the direct single calls.
All inputs are finite."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_epi_ref as R  # noqa: E402
import gemm_paths as GP  # noqa: E402
import test_gemm_paths_gpu as TP  # noqa: E402
from noise_robust_vit_amd import kernels as K  # noqa: E402
from noise_robust_vit_amd._lib import NrvError  # noqa: E402
from gemm_epi_ref import (BF16, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_Q8, EPI_BIAS_RESIDUAL, EPI_DGELU, EPI_DGELU_Q8,  # noqa: E402
                          EPI_NONE, F32)
from test_gemm_paths_gpu import planned8  # noqa: E402,F401   (the module-scoped 8-CU reservation, restored in its `finally`)

pytestmark = pytest.mark.gpu

PADR, S = TP.PADR, TP.S
NT_NAMES = [r.name for r in GP.NT_TABLE]
ODT = ((F32, "f32"), (BF16, "bf16"))


def on_dev(ops, dev):
    """the operand dict on the device; A and B with the leading dimensions of test_gemm_paths_gpu.py"""
    d = {k: v.to(dev) for k, v in ops.items()}
    d["A"], d["B"] = TP.wide(d["A"], 8), TP.wide(d["B"], 16)
    return d


def q8_buffer(M, N, dev, rows=None):
    """the byte stream's padded allocation (ld = N + 32, 255 everywhere) and its [ME, N] view; `rows` [M, N] stored in it"""
    ld, ME = N + 32, (M + 1) // 2 * 2
    qbig = torch.full((ME + 2 * PADR, ld), 255, dtype=torch.uint8, device=dev)
    if rows is not None:
        qbig[PADR:PADR + ME] = R.q8_store(rows, ld).reshape(ME, ld)
    return qbig, qbig[PADR:PADR + ME, :N]


def launch(rec, d, epi, odt, aux=None, stream=False):
    """one launch into fresh padded allocations: (C big, C [M, N], stream big | None, stream rows [M, N] | None)"""
    M, N = rec.M, rec.N
    big, out = TP.padded(M, N, odt, d["A"].device)
    sbig = srows = sview = None
    if stream and epi == EPI_BIAS_GELU_Q8:
        sbig, sview = q8_buffer(M, N, big.device)
    elif stream:
        sbig, sview = TP.padded(M, N, BF16, big.device)
    has_bias = epi in (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_Q8, EPI_BIAS_RESIDUAL)
    K.gemm_nt(d["A"], d["B"], epilogue=epi, bias=d["bias"] if has_bias else None, aux=aux, aux_out=sview, out=out)
    if stream and epi == EPI_BIAS_GELU_Q8:
        ld, ME = N + 32, (M + 1) // 2 * 2
        srows, pairs = TP.q8_rows(sbig, M, N, ld)
        guard = sbig.clone()
        guard[PADR:PADR + ME].reshape(ME // 2, 2 * ld)[:, :2 * N] = 255
        assert bool((guard == 255).all()), f"{rec.name}: the byte stream was written outside its block"
        assert M % 2 == 1 and bool((pairs[-1, :2 * N].reshape(N // 64, 2, 64)[:, 1] == 255).all()), "second row of the last pair"
    elif stream:
        srows = sview.contiguous()
        TP.assert_untouched_outside(sbig, M, N, f"{rec.name} epilogue {epi} gelu' stream", rec)
    TP.assert_untouched_outside(big, M, N, f"{rec.name} epilogue {epi} out {odt}", rec)
    return big, out.contiguous(), sbig, srows


def run(rec, d, epi, odt, what, aux=None, aux_rows=None, stream=False, figures=None):
    """plan, two launches that must agree bit for bit, the shared judge; a failure names tile, launch position and walk"""
    assert K.gemm_nt_plan(rec.M, rec.N, rec.K, epi) == rec.plan, "another variant would run on this device"
    big, out, sbig, srows = launch(rec, d, epi, odt, aux, stream)
    big2, _, sbig2, _ = launch(rec, d, epi, odt, aux, stream)
    assert torch.equal(big, big2) and (sbig is None or torch.equal(sbig, sbig2)), what + ": a second launch differs"
    res = R.judge_nt(d, epi, odt, aux if aux_rows is None else aux_rows, out, srows)
    for check, (bad, fig) in res.items():
        if fig is not None and figures is not None:
            key = (what.split(" ", 1)[1], check)
            figures[key] = max(figures.get(key, 0.0), fig)
        if bool(bad.any()):
            raise AssertionError(f"{what} [{check}]" + (f" worst error / bound {fig:.3f}" if fig is not None else "") + ": "
                                 + TP.where_bad_nt(bad, rec))
    return out, srows


# ---------------------------------------------------------------------------------------------- NT, bit for bit
@pytest.mark.parametrize("name", NT_NAMES)
def test_nt_linear_epilogues_bit_for_bit(dev, planned8, name):
    rec = GP.nt(name)
    d = on_dev(R.dense_exact(rec), dev)
    aux32, aux16, auxg = TP.wide(d["aux32"], 16), TP.wide(d["aux16"], 16), TP.wide(d["auxg"], 8)
    for odt, on in ODT:
        run(rec, d, EPI_NONE, odt, f"{name} dense_exact/NONE/{on}")
        run(rec, d, EPI_BIAS, odt, f"{name} dense_exact/BIAS/{on}")
        run(rec, d, EPI_BIAS_RESIDUAL, odt, f"{name} dense_exact/RESIDUAL_aux32/{on}", aux32)
        run(rec, d, EPI_BIAS_RESIDUAL, odt, f"{name} dense_exact/RESIDUAL_aux16/{on}", aux16)
        run(rec, d, EPI_DGELU, odt, f"{name} dense_exact/DGELU/{on}", auxg)
    if rec.q8:
        _, qview = q8_buffer(rec.M, rec.N, dev, d["auxq"])
        run(rec, d, EPI_DGELU_Q8, BF16, f"{name} dense_exact/DGELU_Q8/bf16", qview, aux_rows=d["auxq"])
    g = on_dev(R.gelu_dense(rec), dev)                      # u = acc + bias of the GELU tests, on its own
    for odt, on in ODT:
        run(rec, g, EPI_BIAS, odt, f"{name} gelu_dense/BIAS/{on}")


@pytest.mark.parametrize("name", NT_NAMES)
def test_nt_fractional_residual_and_ties(dev, planned8, name):
    """(acc + bias) + aux exact in fp32 and no bf16 number: the one rounding of the store is nearest-even.  The tie band names
    what else it could be: round-half-up fails `ties_even_below`, truncation `ties_even_above`."""
    rec = GP.nt(name)
    d = on_dev(R.fractional_aux(rec), dev)
    aux = TP.wide(d["aux32"], 16)
    run(rec, d, EPI_BIAS_RESIDUAL, BF16, f"{name} fractional_aux/RESIDUAL_aux32/bf16", aux)
    run(rec, d, EPI_BIAS_RESIDUAL, F32, f"{name} fractional_aux/RESIDUAL_aux32/f32", aux)


# ---------------------------------------------------------------------------------------------- NT, the GELU epilogues
def quantity(case, check):
    """the DESIGN.md column of a judged check: `case` is kind/epilogue/out type"""
    _, epi, on = case.split("/")
    if check == "stream":
        return "Q8 byte" if epi == "GELU_Q8" else "gelu' bf16 (reported)"
    return "GELU fp32" if on == "f32" else "GELU bf16 (reported)"


@pytest.mark.parametrize("name", NT_NAMES)
def test_nt_gelu_epilogues_within_counted_bounds(dev, planned8, name):
    rec = GP.nt(name)
    figures = {}
    for kind, ops in (("ladder", R.gelu_ladder(rec, False)), ("ladder_bias", R.gelu_ladder(rec, True)),
                      ("gelu_dense", R.gelu_dense(rec))):
        d = on_dev(ops, dev)
        run(rec, d, EPI_BIAS_GELU, F32, f"{name} {kind}/GELU/f32", stream=True, figures=figures)
        h16, _ = run(rec, d, EPI_BIAS_GELU, BF16, f"{name} {kind}/GELU/bf16", stream=True, figures=figures)
        if rec.q8:
            hq, q = run(rec, d, EPI_BIAS_GELU_Q8, BF16, f"{name} {kind}/GELU_Q8/bf16", stream=True, figures=figures)
            TP.assert_same_nt(hq, h16, rec, f"{name} {kind}: h of the byte-stream epilogue vs the bf16-stream epilogue:")
    worst = {}
    for (case, check), v in figures.items():
        worst[quantity(case, check)] = max(worst.get(quantity(case, check), 0.0), v)
    print(f"{name}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


# ---------------------------------------------------------------------------------------------- NT, the row remap
REMAP = ((3, 65, 136, 72, 1), (9, 65, 264, 136, 6))         # groups, rows per group, N, K, tiles = workgroups of the plain kernel


@pytest.mark.parametrize("groups,G,N,Kd,tiles", REMAP)
def test_nt_remap_path_bit_for_bit(dev, planned8, groups, G, N, Kd, tiles):
    """epilogue_remap: result row m goes to row (m // G)(G + 1) + m % G + 1 of C (a class-token slot in front of every group);
    aux is read at row m % G (aux_row_mod) or at the remapped row.  The rows the remap skips keep their sentinels."""
    M = groups * G
    plan = {"tile_m": 256, "tile_n": 256, "phased": False, "tiles": tiles, "grid": tiles}
    assert K.gemm_nt_plan(M, N, Kd, EPI_BIAS_RESIDUAL, remap=True) == plan, "another variant would run on this device"
    rec = GP._nt(M, N, Kd, 256, 256, False, tiles)
    d = on_dev(R.dense_exact(rec), dev)
    m = torch.arange(M, device=dev)
    orow = R.remap_row(m, G, G + 1, 1)
    rows_out = groups * (G + 1)
    fr = R.fractional_aux(rec)                              # integer results hide a wrong rounding: the ties again, on this path
    band, odd = fr["band"].to(dev), fr["odd"].to(dev)
    d["frac"] = fr["aux32"].to(dev)
    for odt, on in ODT:
        for adt, an in ((F32, "aux32"), (BF16, "aux16"), (F32, "frac")):
            for row_mod in (G, 0):
                if an == "frac" and row_mod:
                    continue                                # a tie is made per element: no broadcast row
                table = TP.wide(torch.full((rows_out, N), 7.0, dtype=adt, device=dev), 16)     # 7: a row read by mistake shows
                if row_mod:
                    table[:G] = d[an][:G]
                    aux_rows = d[an][m % G]
                else:
                    table[orow] = d[an]
                    aux_rows = d[an]
                want, _ = R.epilogue(d["acc"], EPI_BIAS_RESIDUAL, odt, d["bias"], aux_rows)
                expect, _ = TP.padded(rows_out, N, odt, dev)
                expect[PADR + orow, :N] = want
                bigs = []
                for _ in range(2):
                    big, out = TP.padded(rows_out, N, odt, dev)
                    K.gemm_nt(d["A"], d["B"], epilogue=EPI_BIAS_RESIDUAL, bias=d["bias"], aux=table, aux_row_mod=row_mod, out=out,
                              out_group=G, out_group_stride=G + 1, out_row_offset=1)
                    bigs.append(big)
                what = f"remap {M} x {N} x {Kd} {on} {an} aux_row_mod {row_mod}"
                assert torch.equal(bigs[0], bigs[1]), what + ": a second launch differs"
                bad = bigs[0] != expect
                if an == "frac":
                    got = bigs[0][PADR + orow, :N] != want
                    assert not bool(got[:, band & ~odd].any()), what + ": ties with the even neighbour nearer zero (round-half-up?)"
                    assert not bool(got[:, band & odd].any()), what + ": ties with the even neighbour farther (truncation?)"
                assert not bool(bad.any()), (f"{what}: {int(bad.sum())} elements of the padded C differ, first at (row, column) "
                                             f"{[int(v) for v in bad.nonzero()[0]]} of the allocation ({PADR} guard rows in front)")
    # the library takes the remap with BIAS_RESIDUAL only: the scalar gelu_both of epilogue_remap is unreachable from the C ABI
    with pytest.raises(NrvError):
        K.gemm_nt_plan(M, N, Kd, EPI_BIAS_GELU, remap=True)
    lad = on_dev(R.gelu_ladder(rec, True), dev)
    big, out = TP.padded(rows_out, N, BF16, dev)
    with pytest.raises(NrvError):
        K.gemm_nt(lad["A"], lad["B"], epilogue=EPI_BIAS_GELU, bias=lad["bias"], out=out, out_group=G, out_group_stride=G + 1,
                  out_row_offset=1)
    torch.cuda.synchronize()
    assert bool((big == S).all()), "a refused launch wrote"


# ---------------------------------------------------------------------------------------------- TN
def tn_buffers(M, N, ldc_pad, ops, dev, with_dbias):
    big, out = TP.padded(M, N, F32, dev, ldc_pad)
    out.copy_(ops["c0"])
    db = None
    if with_dbias:
        db = torch.full((M + 16,), S, device=dev)
        db[:M] = ops["db0"]
    return big, out, db


def tn_check(name, big, out, db, c64, db64, M, N):
    bad = out.double() != c64
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} elements of C differ from the integer reference, first at "
                                 f"{bad.nonzero()[0].tolist()} (tile {[int(v) // 256 for v in bad.nonzero()[0]]})")
    TP.assert_untouched_outside(big, M, N, name)
    if db is not None:
        bad = db[:M].double() != db64
        assert not bool(bad.any()), f"{name}: dbias differs at {bad.nonzero().reshape(-1)[:8].tolist()} ({int(bad.sum())} of {M})"
        assert bool((db[M:] == S).all()), f"{name}: dbias written behind M"


@pytest.mark.parametrize("name", [r.name for r in GP.TN_TABLE])
def test_tn_record_bit_for_bit(dev, planned8, name):
    rec = GP.tn(name)
    M, N, T, g = rec.M, rec.N, rec.T, rec.a_group
    ops = {k: v.to(dev) for k, v in R.tn_dense(M, N, T, g, name).items()}
    A, B = TP.wide(ops["dY"], 8), TP.wide(ops["X"], 8)
    kw = dict(a_group=g, a_group_stride=g + 1 if g else 0, a_row_offset=1 if g else 0, T=T, dbias_beta=1.0)
    for beta in sorted({rec.beta, 1.0}):
        plan = rec.plan if beta == rec.beta else dict(rec.plan, direct=False, reduce=True)
        assert K.gemm_tn_plan(M, N, T, g > 0, beta, rec.dbias) == plan, "another variant would run on this device"
        c64, db64 = R.tn_ref(ops["dY"], ops["X"], ops["c0"], ops["db0"], beta, 1.0, g, T)
        runs = []
        for deferred in (False, False, True):
            big, out, db = tn_buffers(M, N, rec.ldc_pad, ops, dev, rec.dbias)
            if deferred:
                pend = K.gemm_tn(A, B, out=out, beta=beta, dbias=None if db is None else db[:M], defer=True, **kw)[-1]
                assert pend.pending == plan["reduce"]
                K.flush_reduce(pend)
            else:
                K.gemm_tn(A, B, out=out, beta=beta, dbias=None if db is None else db[:M], **kw)
            runs.append((big, db))
            tn_check(f"{name} beta {beta}" + (" deferred + flush_reduce" if deferred else ""), big, out, db, c64, db64, M, N)
        for big, db in runs[1:]:
            assert torch.equal(big, runs[0][0]) and (db is None or torch.equal(db, runs[0][1])), \
                f"{name} beta {beta}: the second or the deferred launch differs from the first"


@pytest.mark.parametrize("name", [r.name for r in GP.TNG_TABLE])
def test_tn_grouped_bit_for_bit(dev, planned8, name):
    rec = next(r for r in GP.TNG_TABLE if r.name == name)
    T = rec.T
    assert TP.grouped_bytes(rec) == rec.slots * GP.SLOT_BYTES, "another plan on this device"
    all_ops = [{k: v.to(dev) for k, v in R.tn_dense(M, N, T, 0, f"{name}[{i}]").items()} for i, (M, N, _) in enumerate(rec.problems)]
    for beta in (0.0, 1.0):
        probs, bufs = [], []
        for ops, (M, N, bias) in zip(all_ops, rec.problems):
            big, out, db = tn_buffers(M, N, 8, ops, dev, bias)
            probs.append(dict(A=TP.wide(ops["dY"], 8), B=TP.wide(ops["X"], 8), out=out, beta=beta,
                              dbias=None if db is None else db[:M], dbias_beta=1.0))
            bufs.append((big, out, db))
        K.gemm_tn_grouped(probs)
        for q, ops, (big, out, db), (M, N, bias) in zip(probs, all_ops, bufs, rec.problems):
            c64, db64 = R.tn_ref(ops["dY"], ops["X"], ops["c0"], ops["db0"], beta, 1.0)
            tn_check(f"{name} [{M}, {N}] beta {beta}", big, out, db, c64, db64, M, N)
            big1, out1, db1 = tn_buffers(M, N, 8, ops, dev, bias)
            K.gemm_tn(q["A"], q["B"], out=out1, beta=beta, dbias=None if db1 is None else db1[:M], dbias_beta=1.0)
            assert torch.equal(big1, big) and (db is None or torch.equal(db1, db)), f"{name} [{M}, {N}]: the single launch differs"
        probs2, bufs2 = [], []
        for q, ops, (M, N, bias) in zip(probs, all_ops, rec.problems):
            big, out, db = tn_buffers(M, N, 8, ops, dev, bias)
            probs2.append(dict(q, out=out, dbias=None if db is None else db[:M]))
            bufs2.append((big, db))
        K.gemm_tn_grouped(probs2)
        for (big, _, db), (big2, db2) in zip(bufs, bufs2):
            assert torch.equal(big, big2) and (db is None or torch.equal(db, db2)), f"{name}: a second grouped launch differs"
