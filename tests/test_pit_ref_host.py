"""CPU: the bounds of tests/pit_ref.py hold for the fp32 emulation of each PiT kernel's arithmetic on the very inputs
tests/test_pit_kernels_gpu.py uses (ratio error / bound <= 1, printed), and three wrong kernels each exceed them: the channel map
o % C instead of o / 2, a stride-2 window origin off by one, and swapped ky / kx.  The bounds are wide enough for the arithmetic
and tight enough to see a wrong kernel."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pit_ref as R  # noqa: E402

POOL_SHAPES = [(H, W, C, lead) for (H, W) in R.POOL_PLANES for C in R.POOL_C for lead in (0, 1)]


@pytest.mark.parametrize("H,W,C,lead", POOL_SHAPES)
@pytest.mark.parametrize("kind", R.POOL_KINDS)
def test_pool_bounds_hold_for_the_emulation(H, W, C, lead, kind):
    x, w, bias, dout = R.pool_inputs(H, W, C, lead, kind)
    ref, bound = R.pool_fwd_ref(x, w, bias, H, W, lead)
    r = R.ratio(R.pool_fwd_emul(x, w, bias, H, W, lead), ref, bound)
    dx, bdx, dw, bdw, db, bdb = R.pool_bwd_ref(x, w, dout, H, W, lead)
    r2 = R.ratio(R.pool_dx_emul(w, dout, H, W, lead, C), dx, bdx)
    ew, eb = R.pool_dw_emul(x, dout, H, W, lead)
    r3, r4 = R.ratio(ew, dw, bdw), R.ratio(eb, db, bdb)
    print("pool", (H, W, C, lead, kind), "error / bound: out", r, "dx", r2, "dw", r3, "dbias", r4)
    assert r <= 1.0 and r2 <= 1.0 and r3 <= 1.0 and r4 <= 1.0
    assert ref.shape == (R.POOL_B * R.pool_out(H) * R.pool_out(W), 2 * C) and dx.shape == x.shape


def test_the_fp64_reference_is_the_reference_modules_convolution():
    """pool_fwd_ref / pool_bwd_ref against autograd through nn.Conv2d(C, 2C, 3, stride 2, padding 1, groups = C) in fp64"""
    H, W, C, lead = 3, 5, 8, 1
    x, w, bias, dout = R.pool_inputs(H, W, C, lead)
    conv = torch.nn.Conv2d(C, 2 * C, 3, stride=2, padding=1, groups=C).double()
    with torch.no_grad():
        conv.weight.copy_(w.double().reshape(2 * C, 1, 3, 3))
        conv.bias.copy_(bias.double())
    p = R._planes(x, H, W, lead).clone().requires_grad_(True)
    y = conv(p)
    y.backward(R._planes(dout, R.pool_out(H), R.pool_out(W), 0))
    ref, _ = R.pool_fwd_ref(x, w, bias, H, W, lead)
    dx, _, dw, _, db, _ = R.pool_bwd_ref(x, w, dout, H, W, lead)
    assert torch.allclose(R._rows(y.detach()), ref, rtol=0, atol=1e-12)
    assert torch.allclose(R._rows(p.grad, lead, 0.0), dx, rtol=0, atol=1e-12)
    assert torch.allclose(conv.weight.grad.reshape(2 * C, 9), dw, rtol=0, atol=1e-12) and torch.allclose(conv.bias.grad, db, rtol=0, atol=1e-12)


# the one-hot input is a one in every channel of its token: it sees a wrong window or tap order, not a wrong channel map
@pytest.mark.parametrize("wrong,kind", [(dict(chan="mod"), "random"), (dict(origin=0), "random"), (dict(origin=0), "impulse_x"),
                                        (dict(swap=True), "random"), (dict(swap=True), "impulse_x")])
def test_a_wrong_kernel_exceeds_the_pool_bound(wrong, kind):
    H, W, C, lead = 9, 6, 8, 1
    x, w, bias, _ = R.pool_inputs(H, W, C, lead, kind)
    ref, bound = R.pool_fwd_ref(x, w, bias, H, W, lead)
    assert R.ratio(R.pool_fwd_emul(x, w, bias, H, W, lead), ref, bound) <= 1.0
    assert R.ratio(R.pool_fwd_emul(x, w, bias, H, W, lead, **wrong), ref, bound) > 1.0


@pytest.mark.parametrize("ks,stride", R.UNFOLD_CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_unfold_emulation_equals_the_reference(ks, stride, dtype):
    img = R.unfold_input(ks, stride, dtype)
    ref = R.unfold_ref(img, ks, stride)
    H, W = R.unfold_shape(ks, stride)
    assert (H - ks) % stride == 1 and (W - ks) % stride == 1 and ref.shape[0] == R.UNFOLD_B * 3 * 4
    assert ref.shape[1] % 8 == 0 and ref.shape[1] - R.UNFOLD_C * ks * ks < 8
    assert torch.equal(R.unfold_emul(img, ks, stride).view(torch.int16), ref.view(torch.int16))


def test_the_big_unfold_shape_runs_two_full_passes_and_a_partial_one():
    B, C, S, ks, stride = R.UNFOLD_BIG
    g = (S - ks) // stride + 1
    items = B * g * g * ((C * ks * ks + 7) // 8)
    lap = 16384 * 256
    assert ks == 16 and 2 * lap < items < 3 * lap and items % lap
