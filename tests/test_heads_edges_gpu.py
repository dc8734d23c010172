"""GPU: the talking-heads and re-attention kernels (csrc/nrv_talking_heads.hip, csrc/nrv_reattn.hip, helpers in csrc/nrv_heads.hpp)
per element against the fp64 references and derived bounds of tests/heads_ref.py, on the cases and inputs
tests/test_heads_ref_host.py proves the bounds on.  Method of test_twins_kernels_gpu.py, through the C ABI with raw pointers so that
the test owns every buffer: every input (the H x H matrices, gamma and beta too) sits in a NaN-filled storage with 512 elements of
moat on each side, so a read outside it poisons the result; every output is a view inside such a storage, which must stay NaN
around the view and hold no NaN inside it; the workspace has the size its entry point reports, is filled with NaN bytes before
every call (a partial no workgroup wrote reads as NaN) and is moated; every call runs twice with bit-identical results; every
output is compared as error / bound <= 1, the H x H and [H] gradients per entry."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_ref as R  # noqa: E402

from noise_robust_vit_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
MOAT = 512                        # elements of NaN in front of and behind every input, output and the workspace (doubles)
EPS = ctypes.c_float(R.EPS)
DT = {torch.float32: _lib.NRV_F32, torch.bfloat16: _lib.NRV_BF16}


def _kinds(cases, all_kinds):
    return [(c, "random") for c in cases] + [(c, k) for c in all_kinds for k in R.KINDS[1:]]


FUSED = _kinds(R.FUSED_CASES + R.ROW_WALK_CASES, R.FUSED_ALL_KINDS)
FLAT = _kinds(R.FLAT_CASES + R.TILE_WALK_CASES, R.FLAT_ALL_KINDS)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


class Out:
    """a view of `shape` in the middle of a NaN-filled storage"""

    def __init__(self, shape, dtype, dev):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * MOAT,), float("nan"), dtype=dtype, device=dev)
        self.v = self.buf[MOAT:MOAT + n].view(shape)
        self.ptr = self.v.data_ptr()

    def check(self):
        n = self.v.numel()
        assert bool(torch.isnan(self.buf[:MOAT]).all()) and bool(torch.isnan(self.buf[MOAT + n:]).all()), "written outside the view"
        assert not bool(torch.isnan(self.v).any()), "an element was not written, or read NaN from outside an input"


def _in(t, dev):
    o = Out(t.shape, t.dtype, dev)
    o.v.copy_(t)
    return o


class Workspace:
    """the bytes the `_workspace` entry point asks for, all ones (NaN as doubles), between two moats of the same"""

    def __init__(self, nbytes, dev):
        assert nbytes > 0 and nbytes % 8 == 0
        self.n = nbytes
        self.buf = torch.full((nbytes + 16 * MOAT,), 0xFF, dtype=torch.uint8, device=dev)
        self.ptr = self.buf.data_ptr() + 8 * MOAT

    def check(self):
        assert bool((self.buf[:8 * MOAT] == 0xFF).all()) and bool((self.buf[8 * MOAT + self.n:] == 0xFF).all()), "workspace overrun"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _twice(call):
    """call() -> tuple of Out (and Workspace): two runs, moats intact, no NaN, equal bits; the first run's views"""
    runs = [call() for _ in range(2)]
    torch.cuda.synchronize()
    for o in runs[0] + runs[1]:
        o.check()
    outs = [[o.v for o in r if isinstance(o, Out)] for r in runs]
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*outs)), "reruns differ"
    return outs[0]


def _dev_inputs(i, dev):
    return {k: _in(t, dev) for k, t in i.items()}


def _assert(tag, rs):
    print(tag, "error / bound:", {n: round(r, 4) for n, r in rs.items()})
    assert all(r <= 1.0 for r in rs.values()), (tag, rs)


def _ratios(ref, got):
    return {n: R.ratio(t, ref[n], ref[n + "_bound"]) for n, t in got.items()}


# ---- the eight entry points on moated buffers ----------------------------------------------------
def th_fwd(lib, d, shape, dtype, dev):
    def call():
        P, A = Out(shape, torch.float32, dev), Out(shape, dtype, dev)
        assert lib.nrv_th_softmax_fwd(d["S"].ptr, d["W1"].ptr, d["W2"].ptr, P.ptr, A.ptr, DT[dtype], *shape, None) == 0
        return P, A
    return _twice(call)


def th_bwd(lib, d, P, shape, dev):
    H = shape[1]
    n = lib.nrv_th_softmax_bwd_workspace(*shape)

    def call():
        dS, dW1, dW2, ws = Out(shape, torch.float32, dev), Out((H, H), torch.float32, dev), Out((H, H), torch.float32, dev), Workspace(n, dev)
        assert lib.nrv_th_softmax_bwd(d["dA"].ptr, P.data_ptr(), d["S"].ptr, d["W1"].ptr, d["W2"].ptr, dS.ptr, dW1.ptr, dW2.ptr, ws.ptr,
                                      ctypes.c_size_t(n), *shape, None) == 0
        return dS, dW1, dW2, ws
    return _twice(call)


def mix_fwd(lib, x, W, shape, dtype, dev):
    def call():
        out = Out(shape, dtype, dev)
        assert lib.nrv_head_mix_fwd(x.ptr, W.ptr, out.ptr, DT[dtype], *shape, None) == 0
        return (out,)
    return _twice(call)[0]


def mix_bwd(lib, dout, x, W, shape, dev):
    H = shape[1]
    n = lib.nrv_head_mix_bwd_workspace(*shape)

    def call():
        din, dW, ws = Out(shape, torch.float32, dev), Out((H, H), torch.float32, dev), Workspace(n, dev)
        assert lib.nrv_head_mix_bwd(dout.ptr, x.ptr, W.ptr, din.ptr, dW.ptr, ws.ptr, ctypes.c_size_t(n), *shape, None) == 0
        return din, dW, ws
    return _twice(call)


def ra_fwd(lib, d, shape, dtype, dev):
    def call():
        P, A = Out(shape, torch.float32, dev), Out(shape, dtype, dev)
        assert lib.nrv_reattn_softmax_fwd(d["S"].ptr, d["W"].ptr, d["gamma"].ptr, d["beta"].ptr, P.ptr, A.ptr, DT[dtype], *shape, EPS, None) == 0
        return P, A
    return _twice(call)


def ra_norm_fwd(lib, P, d, shape, dtype, dev):
    def call():
        A = Out(shape, dtype, dev)
        assert lib.nrv_reattn_norm_fwd(P.ptr, d["W"].ptr, d["gamma"].ptr, d["beta"].ptr, A.ptr, DT[dtype], *shape, EPS, None) == 0
        return (A,)
    return _twice(call)[0]


def ra_bwd(lib, d, P_ptr, shape, dev, fused):
    H = shape[1]
    n = (lib.nrv_reattn_softmax_bwd_workspace if fused else lib.nrv_reattn_norm_bwd_workspace)(*shape)
    fn = lib.nrv_reattn_softmax_bwd if fused else lib.nrv_reattn_norm_bwd

    def call():
        dx, dW, ws = Out(shape, torch.float32, dev), Out((H, H), torch.float32, dev), Workspace(n, dev)
        dg, db = Out((H,), torch.float32, dev), Out((H,), torch.float32, dev)
        assert fn(d["dA"].ptr, P_ptr, d["W"].ptr, d["gamma"].ptr, dx.ptr, dW.ptr, dg.ptr, db.ptr, ws.ptr, ctypes.c_size_t(n), *shape, EPS, None) == 0
        return dx, dW, dg, db, ws
    return _twice(call)


# ---- fused row kernels ---------------------------------------------------------------------------
@pytest.mark.parametrize("case,kind", FUSED, ids=str)
def test_th_softmax(lib, dev, case, kind):
    i = R.inputs(*case, kind)
    d = _dev_inputs(i, dev)
    P, A = th_fwd(lib, d, case, torch.float32, dev)
    P16, A16 = th_fwd(lib, d, case, torch.bfloat16, dev)
    assert torch.equal(P16, P)
    f, fb = R.th_fwd_ref(i["S"], i["W1"], i["W2"], P), R.th_fwd_ref(i["S"], i["W1"], i["W2"], P, bf=True)
    rs = dict(_ratios(f, {"P": P, "A": A}), A_bf16=R.ratio(A16, fb["A"], fb["A_bound"]))
    dS, dW1, dW2 = th_bwd(lib, d, P, case, dev)
    rs.update(_ratios(R.th_bwd_ref(i["dA"], P, i["S"], i["W1"], i["W2"]), {"dS": dS, "dW1": dW1, "dW2": dW2}))
    _assert(f"th_softmax {case} {kind}", rs)
    if case[3] == 1:                                                      # softmax over one key is the constant 1
        assert bool((P == 1).all()) and not bool(dS.any())
    if kind == "identity":
        assert torch.equal(A, P)                                          # 1 * p + 0 * the others, exactly


@pytest.mark.parametrize("case,kind", FUSED, ids=str)
def test_reattn_softmax(lib, dev, case, kind):
    i = R.inputs(*case, kind)
    d = _dev_inputs(i, dev)
    P, A = ra_fwd(lib, d, case, torch.float32, dev)
    P16, A16 = ra_fwd(lib, d, case, torch.bfloat16, dev)
    assert torch.equal(P16, P)
    s = R.ra_softmax_ref(i["S"])
    f, fb = R.ra_norm_fwd_ref(P, i["W"], i["gamma"], i["beta"]), R.ra_norm_fwd_ref(P, i["W"], i["gamma"], i["beta"], bf=True)
    rs = {"P": R.ratio(P, s["P"], s["P_bound"]), "A": R.ratio(A, f["A"], f["A_bound"]), "A_bf16": R.ratio(A16, fb["A"], fb["A_bound"])}
    dS, dW, dg, db = ra_bwd(lib, d, P.data_ptr(), case, dev, fused=True)
    rs.update(_ratios(R.ra_bwd_ref(i["dA"], P, i["W"], i["gamma"]), {"dS": dS, "dW": dW, "dgamma": dg, "dbeta": db}))
    _assert(f"reattn_softmax {case} {kind}", rs)
    if case[3] == 1:
        assert bool((P == 1).all()) and not bool(dS.any())
    if case[1] == 1:                                                      # the LayerNorm over one head leaves beta
        beta = i["beta"].to(dev).view(1, 1, 1, 1).expand_as(A)
        assert torch.equal(A, beta) and torch.equal(A16, beta.to(torch.bfloat16))
        assert not bool(dS.any()) and not bool(dW.any()) and not bool(dg.any())


# ---- flat kernels -----------------------------------------------------------------------------
@pytest.mark.parametrize("case,kind", FLAT, ids=str)
def test_head_mix(lib, dev, case, kind):
    i = R.inputs(*case, kind)
    d = _dev_inputs(i, dev)
    out = mix_fwd(lib, d["S"], d["W1"], case, torch.float32, dev)
    out16 = mix_fwd(lib, d["S"], d["W1"], case, torch.bfloat16, dev)
    f, fb = R.mix_fwd_ref(i["S"], i["W1"]), R.mix_fwd_ref(i["S"], i["W1"], bf=True)
    rs = {"out": R.ratio(out, f["out"], f["out_bound"]), "out_bf16": R.ratio(out16, fb["out"], fb["out_bound"])}
    din, dW = mix_bwd(lib, d["dA"], d["S"], d["W1"], case, dev)
    rs.update(_ratios(R.mix_bwd_ref(i["dA"], i["S"], i["W1"]), {"din": din, "dW": dW}))
    _assert(f"head_mix {case} {kind}", rs)
    assert torch.equal(out16, out.to(torch.bfloat16))                     # one rounding of the same fp32 value
    if kind == "identity":
        assert torch.equal(out, d["S"].v) and torch.equal(din, d["dA"].v)


@pytest.mark.parametrize("case,kind", FLAT, ids=str)
def test_reattn_norm(lib, dev, case, kind):
    i = R.inputs(*case, kind)
    d = _dev_inputs(i, dev)
    Pc = torch.softmax(i["S"], -1)
    P = _in(Pc, dev)
    A = ra_norm_fwd(lib, P, d, case, torch.float32, dev)
    A16 = ra_norm_fwd(lib, P, d, case, torch.bfloat16, dev)
    f, fb = R.ra_norm_fwd_ref(Pc, i["W"], i["gamma"], i["beta"]), R.ra_norm_fwd_ref(Pc, i["W"], i["gamma"], i["beta"], bf=True)
    rs = {"A": R.ratio(A, f["A"], f["A_bound"]), "A_bf16": R.ratio(A16, fb["A"], fb["A_bound"])}
    dP, dW, dg, db = ra_bwd(lib, d, P.ptr, case, dev, fused=False)
    rs.update(_ratios(R.ra_bwd_ref(i["dA"], Pc, i["W"], i["gamma"], softmax=False), {"dP": dP, "dW": dW, "dgamma": dg, "dbeta": db}))
    _assert(f"reattn_norm {case} {kind}", rs)
    assert torch.equal(A16, A.to(torch.bfloat16))
    if case[1] == 1:
        beta = i["beta"].to(dev).view(1, 1, 1, 1).expand_as(A)
        assert torch.equal(A, beta) and not bool(dP.any()) and not bool(dW.any()) and not bool(dg.any())


# ---- the grid cap of the flat forwards ------------------------------------------------------------
@pytest.mark.parametrize("case", R.GRID_CAP_CASES, ids=str)
def test_flat_forwards_past_the_grid_cap(lib, dev, case):
    """more than 65 536 x 256 items: the grid-stride loop wraps.  H = 1 is exact: head_mix is the fp32 product w x, reattn_norm
    gives beta.  A position the loop skipped stays NaN; one written twice shows in the moat or in the rerun"""
    B, H, Nq, Nk = case
    assert H == 1 and B * (Nq * Nk // R.vec(Nq * Nk)) > 65536 * R.TH_THREADS
    g = R._gen("grid cap", case)
    x = _in(torch.randn(B, 1, Nq, Nk, generator=g), dev)
    W, gamma, beta = (_in(t, dev) for t in (torch.tensor([[0.7310585]]), torch.tensor([1.25]), torch.tensor([-0.3125])))
    d = {"W": W, "gamma": gamma, "beta": beta}
    want = x.v * W.v.view(1, 1, 1, 1)
    for dtype in (torch.float32, torch.bfloat16):
        out = mix_fwd(lib, x, W, case, dtype, dev)
        assert torch.equal(out, want.to(dtype))
        del out
        A = ra_norm_fwd(lib, x, d, case, dtype, dev)
        assert bool((A == beta.v.to(dtype)).all())
        del A
    del x, want
    torch.cuda.empty_cache()
