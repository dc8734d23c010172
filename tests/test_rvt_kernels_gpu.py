"""GPU: the RvT kernels (csrc/nrv_rvt.hip) per element against the fp64 references and derived bounds of tests/rvt_ref.py, on
the inputs tests/test_rvt_ref_host.py proves the bounds on.  Method of test_pcn_edges_gpu.py: outputs are pre-filled with NaN,
every element is compared, elements a kernel must not write still hold the sentinel (the class rows of the conv's output, the
gap columns of a strided u), untouched elements of the in-place rotation are bit-identical, and every kernel runs twice with
bit-identical results.  The grids are exact (no capped grid-stride loop), so no multi-pass shape is needed."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rvt_ref as R  # noqa: E402

from noise_robust_vit_amd import kernels as K  # noqa: E402

pytestmark = pytest.mark.gpu
CONV_SHAPES = [(ks, H, W, C, lead) for ks in (3, 5, 7) for (H, W) in R.CONV_PLANES for C, lead in ((8, 0), (72, 1))]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


@pytest.mark.parametrize("case", R.ROTARY_CASES)
def test_rotary(dev, case):
    B, H, dh, dr, g, lead = case
    qkv, sin, cos, N = R.rotary_inputs(case)
    s, c = sin.to(dev), cos.to(dev)
    for sign, fn in ((1.0, K.rotary_fwd), (-1.0, K.rotary_bwd)):
        ref, bound = R.rotary_ref(qkv, sin, cos, N, lead, H, dh, sign)
        runs = [fn(qkv.to(dev).clone(), s, c, B, N, lead, H, dh) for _ in range(2)]
        assert torch.equal(runs[0], runs[1])
        got = runs[0].cpu()
        r = R.ratio(got, ref, bound)
        print("rotary", case, sign, "error / bound", r)
        assert r <= 1.0
        t, q = got.reshape(B, N, 3 * H, dh), qkv.reshape(B, N, 3 * H, dh)
        assert torch.equal(t[:, :, 2 * H:], q[:, :, 2 * H:]), "the v block changed"
        assert torch.equal(t[:, :lead], q[:, :lead]), "a class row changed"
        assert torch.equal(t[..., dr:], q[..., dr:]), "features behind dr changed"


@pytest.mark.parametrize("ks,H,W,C,lead", CONV_SHAPES)
@pytest.mark.parametrize("kind", ["random", "impulse_a", "impulse_d"])
def test_dwconv(dev, ks, H, W, C, lead, kind):
    a, w, dout = R.conv_inputs(ks, H, W, C, lead, kind)
    B = R.CONV_B
    ad, wd, dd = a.to(dev), w.to(dev), dout.to(dev)
    ref, bound = R.conv_fwd_ref(a, w, ks, H, W, lead)
    outs = [K.dwconv_fwd(ad, wd, B, H, W, lead, out=_nan(a.shape, torch.bfloat16, dev)) for _ in range(2)]
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    r = R.ratio(outs[0], ref, bound)                       # NaN in ref = the class rows: they must still hold the sentinel
    da_ref, da_bound, dw_ref, dw_bound = R.conv_bwd_ref(a, w, dout, ks, H, W, lead)
    runs = [K.dwconv_bwd(ad, wd, dd, B, H, W, lead, da=_nan(a.shape, torch.bfloat16, dev), dw=_nan(w.shape, torch.float32, dev))
            for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    r2 = R.ratio(runs[0][0], da_ref, da_bound)             # the class rows of da: exact zeros (zero bound)
    r3 = R.ratio(runs[0][1], dw_ref, dw_bound)
    print("conv", (ks, H, W, C, lead, kind), "error / bound: out", r, "da", r2, "dw", r3)
    assert r <= 1.0 and r2 <= 1.0 and r3 <= 1.0
    if lead:
        assert float(runs[0][0].view(B, lead + H * W, C)[:, :lead].abs().max()) == 0.0


def test_dwconv_fresh_output_has_zero_class_rows(dev):
    a, w, _ = R.conv_inputs(5, 3, 5, 72, 1)
    out = K.dwconv_fwd(a.to(dev), w.to(dev), R.CONV_B, 3, 5, 1)
    assert float(out.view(R.CONV_B, 16, 72)[:, 0].abs().max()) == 0.0


@pytest.mark.parametrize("case", R.GEGLU_CASES)
def test_geglu(dev, case):
    rows, hidden, ld = case
    u, dh = R.geglu_inputs(case)
    # u as a strided view: the columns behind 2 * hidden are NaN and must neither be read into a result nor be written
    buf = _nan((rows, ld), torch.bfloat16, dev)
    buf[:, :2 * hidden] = u.to(dev)[:, :2 * hidden]
    uv = buf[:, :2 * hidden]
    ref, bound = R.geglu_fwd_ref(u, hidden)
    hs = [K.geglu_fwd(uv, hidden) for _ in range(2)]
    assert torch.equal(hs[0], hs[1])
    r = R.ratio(hs[0], ref, bound)
    dref, dbound = R.geglu_bwd_ref(u, dh, hidden)
    dus = [K.geglu_bwd(uv, dh.to(dev), out=_nan((rows, 2 * hidden), torch.bfloat16, dev)) for _ in range(2)]
    assert torch.equal(dus[0], dus[1])
    r2 = R.ratio(dus[0], dref, dbound)
    print("geglu", case, "error / bound: h", r, "du", r2)
    assert r <= 1.0 and r2 <= 1.0
    assert bool(torch.isnan(buf[:, 2 * hidden:]).all()) and torch.equal(buf[:, :2 * hidden], u.to(dev)[:, :2 * hidden])
