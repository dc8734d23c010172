"""GPU: the split-K reduction as a side job of the NT launch that follows gives the bits of the three separate launches.

Per record of tests/side_reduce_cases.py, planned for its CU count (`nrv_set_reserved_cus`, restored in a `finally`): the plans are
asserted on the device first; then `gemm_tn` + `gemm_nt` and `gemm_tn(defer=True)` + `gemm_nt(side=...)` run on equal inputs and
the NT result, the whole C buffer (padding columns of ldc > N and a guard region behind the last row included) and the whole
dbias buffer (guard included) are compared with `torch.equal`: the sum order is that of the stand-alone reduction, so nothing
needs a tolerance.  `fused` must say what the record's admission says, and a rejected job gives the same bits, as does the
stand-alone `flush_reduce` of a third deferred launch.  A deferred launch whose token is dropped leaves C and dbias untouched."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import side_reduce_cases as SC  # noqa: E402
from noise_robust_vit_amd import kernels as K  # noqa: E402
from noise_robust_vit_amd._lib import EPI_DGELU_Q8  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, S = 256, 512.0               # guard elements behind C and behind dbias, sentinel value
BF16, F32 = torch.bfloat16, torch.float32


def rnd(shape, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF16).to(dev)


class planned:
    def __init__(self, dev, cus):
        self.reserve = torch.cuda.get_device_properties(dev).multi_processor_count - cus

    def __enter__(self):
        assert self.reserve >= 0
        prev = K.set_reserved_cus(self.reserve)
        if prev != 0:
            K.set_reserved_cus(0)
            raise AssertionError(f"reservation was {prev}, not 0")

    def __exit__(self, *exc):
        K.set_reserved_cus(0)


def grad_buffers(rec, dev):
    """(flat C buffer, its [M, N] view with ldc = N + ldc_pad, flat dbias buffer | None, its [M] view | None): every element
    that the launches must not touch holds the sentinel, C and dbias themselves a start value that beta = 1 adds to."""
    Mw, Nw, _, _ = rec.tn
    ldc = Nw + rec.ldc_pad
    flat = torch.full((Mw * ldc + GUARD,), S, dtype=F32, device=dev)
    view = flat[:Mw * ldc].view(Mw, ldc)[:, :Nw]
    view.copy_(torch.arange(Mw * Nw, device=dev, dtype=F32).reshape(Mw, Nw) % 7 - 3.0)
    if rec.dbias is None:
        return flat, view, None, None
    bflat = torch.full((Mw + GUARD,), S, dtype=F32, device=dev)
    bflat[:Mw] = torch.arange(Mw, device=dev, dtype=F32) % 5 - 2.0
    return flat, view, bflat, bflat[:Mw]


def guards_intact(rec, flat, bflat):
    Mw, Nw, _, _ = rec.tn
    ldc = Nw + rec.ldc_pad
    assert bool((flat[Mw * ldc:] == S).all()), "guard behind C"
    if rec.ldc_pad:
        assert bool((flat[:Mw * ldc].view(Mw, ldc)[:, Nw:] == S).all()), "padding columns of C"
    if bflat is not None:
        assert bool((bflat[Mw:] == S).all()), "guard behind dbias"


@pytest.mark.parametrize("rec", SC.PAIRS, ids=lambda r: r.name)
def test_side_job_gives_the_bits_of_the_separate_launches(dev, rec):
    M, N, Kk, epi = rec.nt
    Mw, Nw, T, beta = rec.tn
    A, B = rnd((M, Kk), dev, 1, 0.5), rnd((N, Kk), dev, 2, 0.5)
    aux = None
    if epi == EPI_DGELU_Q8:
        g = torch.Generator(device="cpu").manual_seed(3)
        aux = torch.randint(0, 256, ((M + 1) // 2 * 2, N), generator=g, dtype=torch.uint8).to(dev)
    dY, X = rnd((T, Mw), dev, 4), rnd((T, Nw), dev, 5)
    kw = dict(beta=beta, dbias_beta=rec.dbias or 0.0)
    with planned(dev, rec.cus):
        nt = K.gemm_nt_plan(M, N, Kk, epi)
        tn = K.gemm_tn_plan(Mw, Nw, T, beta=beta, dbias=rec.dbias is not None)
        sp = K.gemm_nt_side_plan(M, N, Kk, epi, False, rec.job_bytes)
        assert nt["phased"] and (nt["tile_m"], nt["tile_n"], nt["tiles"], nt["grid"]) == rec.nt_plan
        assert (tn["splits"], tn["kt_r"], tn["direct"]) == (rec.splits, rec.kt_r, rec.direct)
        assert sp == {"late": rec.late, "share_bytes": rec.share, "admitted": rec.admitted}

        # the three separate launches
        c0, cv0, b0, bv0 = grad_buffers(rec, dev)
        K.gemm_tn(dY, X, out=cv0, dbias=bv0, **kw)
        out0 = K.gemm_nt(A, B, epilogue=epi, aux=aux)
        # deferred + NT with the job
        c1, cv1, b1, bv1 = grad_buffers(rec, dev)
        pend = K.gemm_tn(dY, X, out=cv1, dbias=bv1, defer=True, **kw)[-1]
        assert pend.pending == rec.pending
        out1 = K.gemm_nt(A, B, epilogue=epi, aux=aux, side=pend)
        assert pend.fused == (rec.admitted if rec.pending else None)
        assert not pend.pending
        # deferred + the stand-alone reduction of the job
        c2, cv2, b2, bv2 = grad_buffers(rec, dev)
        pend2 = K.gemm_tn(dY, X, out=cv2, dbias=bv2, defer=True, **kw)[-1]
        K.flush_reduce(pend2)
        K.flush_reduce(pend2)               # a consumed token runs nothing
        torch.cuda.synchronize()
    assert torch.equal(out1, out0)
    assert torch.equal(c1, c0) and torch.equal(c2, c0)
    if b0 is not None:
        assert torch.equal(b1, b0) and torch.equal(b2, b0)
    guards_intact(rec, c1, b1)
    guards_intact(rec, c0, b0)
    # and the result is a weight gradient: per element against the fp64 product of the same values
    ref = dY[:T].double().t() @ X[:T].double()
    start = (torch.arange(Mw * Nw, device=dev, dtype=torch.float64).reshape(Mw, Nw) % 7 - 3.0) * beta
    # bf16 products are exact in fp32; each of the <= T + splits + 1 fp32 additions rounds a partial sum that is at most
    # sum |a b| (+ |start|) with relative error <= 2^-23 (round to nearest gives 2^-24; 2^-23 also covers an adder that truncates): the
    # bound below, per element
    nadd = T + rec.splits + 1
    mag = dY[:T].double().abs().t() @ X[:T].double().abs() + start.abs()
    assert bool(((cv1.double() - start - ref).abs() <= nadd * 2.0 ** -23 * mag + 1e-30).all())
    if bv1 is not None:
        bstart = (torch.arange(Mw, device=dev, dtype=torch.float64) % 5 - 2.0) * (rec.dbias or 0.0)
        bref = dY[:T].double().sum(0)
        bmag = dY[:T].double().abs().sum(0) + bstart.abs()
        assert bool(((bv1.double() - bstart - bref).abs() <= nadd * 2.0 ** -23 * bmag + 1e-30).all())


def test_a_dropped_token_never_runs(dev):
    """A deferred launch whose token is dropped leaves C as the launch left it: no reduction is issued behind the caller's back."""
    rec = SC.pair("late3_splits2_kt_r")
    Mw, Nw, T, beta = rec.tn
    dY, X = rnd((T, Mw), dev, 4), rnd((T, Nw), dev, 5)
    with planned(dev, rec.cus):
        c, cv, b, bv = grad_buffers(rec, dev)
        before_c, before_b = c.clone(), b.clone()
        pend = K.gemm_tn(dY, X, out=cv, dbias=bv, beta=beta, defer=True)[-1]
        assert pend.pending
        del pend
        torch.cuda.synchronize()
    assert torch.equal(c, before_c) and torch.equal(b, before_b)
