"""GPU: the PiT kernels (csrc/nrv_pit.hip, nrv_unfold_patches in csrc/nrv_misc.hip) per element against the fp64 references and
derived bounds of tests/pit_ref.py, on the inputs tests/test_pit_ref_host.py proves the bounds on.  Method of
test_rvt_kernels_gpu.py: outputs are pre-filled with NaN, every element is compared as error / bound <= 1, the class rows of dx
are exact zeros, the class rows of x (random) are never read into a result, and every kernel runs twice with bit-identical
results.  The pool kernels' grids are exact and have no spatial tile; the unfold's capped grid-stride loop gets one shape that
it walks in two full passes and a partial one."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pit_ref as R  # noqa: E402

from noise_robust_vit_amd import kernels as K  # noqa: E402

pytestmark = pytest.mark.gpu
POOL_SHAPES = [(H, W, C, lead) for (H, W) in R.POOL_PLANES for C in R.POOL_C for lead in (0, 1)]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def _nan(shape, dtype, dev):
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device=dev)


@pytest.mark.parametrize("H,W,C,lead", POOL_SHAPES)
@pytest.mark.parametrize("kind", R.POOL_KINDS)
def test_pool_dwconv(dev, H, W, C, lead, kind):
    x, w, bias, dout = R.pool_inputs(H, W, C, lead, kind)
    B, Ho, Wo = R.POOL_B, R.pool_out(H), R.pool_out(W)
    xd, wd, bd, dd = x.to(dev), w.to(dev), bias.to(dev), dout.to(dev)
    ref, bound = R.pool_fwd_ref(x, w, bias, H, W, lead)
    outs = [K.pool_dwconv_fwd(xd, wd, bd, B, H, W, lead, out=_nan((B * Ho * Wo, 2 * C), torch.bfloat16, dev)) for _ in range(2)]
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    r = R.ratio(outs[0], ref, bound)
    dx_ref, dx_bound, dw_ref, dw_bound, db_ref, db_bound = R.pool_bwd_ref(x, w, dout, H, W, lead)
    runs = [K.pool_dwconv_bwd(xd, wd, dd, B, H, W, lead, dx=_nan(x.shape, torch.float32, dev), dw=_nan((2 * C, 9), torch.float32, dev),
                              dbias=_nan((2 * C,), torch.float32, dev)) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    r2 = R.ratio(runs[0][0], dx_ref, dx_bound)             # the class rows of dx: exact zeros (zero bound)
    r3 = R.ratio(runs[0][1], dw_ref, dw_bound)
    r4 = R.ratio(runs[0][2], db_ref, db_bound)
    print("pool", (H, W, C, lead, kind), "error / bound: out", r, "dx", r2, "dw", r3, "dbias", r4)
    assert r <= 1.0 and r2 <= 1.0 and r3 <= 1.0 and r4 <= 1.0
    if lead:
        assert float(runs[0][0].view(B, lead + H * W, C)[:, :lead].abs().max()) == 0.0


def test_pool_dwconv_takes_the_conv2d_weight_shape(dev):
    """w [2C, 1, 3, 3] as the module holds it; dw comes back in that shape"""
    H, W, C, lead = 3, 5, 8, 1
    x, w, bias, dout = R.pool_inputs(H, W, C, lead)
    w4 = w.reshape(2 * C, 1, 3, 3).to(dev)
    out = K.pool_dwconv_fwd(x.to(dev), w4, bias.to(dev), R.POOL_B, H, W, lead)
    assert torch.equal(out, K.pool_dwconv_fwd(x.to(dev), w.to(dev), bias.to(dev), R.POOL_B, H, W, lead))
    _, dw, db = K.pool_dwconv_bwd(x.to(dev), w4, dout.to(dev), R.POOL_B, H, W, lead)
    assert dw.shape == w4.shape and db.shape == (2 * C,)


@pytest.mark.parametrize("ks,stride", R.UNFOLD_CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_unfold_patches(dev, ks, stride, dtype):
    img = R.unfold_input(ks, stride, dtype)
    ref = R.unfold_ref(img, ks, stride)
    outs = [K.unfold_patches(img.to(dev), ks, stride, out=_nan(ref.shape, torch.bfloat16, dev)) for _ in range(2)]
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    assert torch.equal(outs[0].cpu().view(torch.int16), ref.view(torch.int16))
    F = R.UNFOLD_C * ks * ks
    assert float(outs[0][:, F:].abs().max()) == 0.0 if F % 8 else ref.shape[1] == F


def test_unfold_patches_over_several_grid_passes(dev):
    """ks = 16 at a size whose work items exceed two passes of the capped grid (R.UNFOLD_BIG); the reference runs on the device"""
    B, C, S, ks, stride = R.UNFOLD_BIG
    img = torch.randn(B, C, S, S, generator=R._gen("unfold.big")).to(dev)
    ref = torch.nn.functional.unfold(img, ks, stride=stride).transpose(1, 2).reshape(-1, C * ks * ks).to(torch.bfloat16)
    out = K.unfold_patches(img, ks, stride, out=_nan(ref.shape, torch.bfloat16, dev))
    assert out.shape[0] * (out.shape[1] // 8) > 2 * 16384 * 256
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
