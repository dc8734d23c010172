"""CPU: the bounds of tests/rvt_ref.py hold for the fp32 emulation of each RvT kernel's arithmetic on the very inputs
tests/test_rvt_kernels_gpu.py uses (ratio error / bound <= 1, printed), and a wrong tap order, swapped sin / cos tables and a
swapped GEGLU half each exceed them: the bounds are wide enough for the arithmetic and tight enough to see a wrong kernel."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rvt_ref as R  # noqa: E402

CONV_SHAPES = [(ks, H, W, C, lead) for ks in (3, 5, 7) for (H, W) in R.CONV_PLANES for C, lead in ((8, 0), (72, 1))]


@pytest.mark.parametrize("case", R.ROTARY_CASES)
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_rotary_bound_holds_for_the_emulation(case, sign):
    B, H, dh, dr, g, lead = case
    qkv, sin, cos, N = R.rotary_inputs(case)
    ref, bound = R.rotary_ref(qkv, sin, cos, N, lead, H, dh, sign)
    got = R.rotary_emul(qkv, sin, cos, N, lead, H, dh, sign)
    r = R.ratio(got, ref, bound)
    print("rotary", case, sign, "error / bound", r)
    assert r <= 1.0
    # untouched elements are bit-identical: zero bound there
    t = got.reshape(B, N, 3 * H, dh)
    q = qkv.reshape(B, N, 3 * H, dh)
    assert torch.equal(t[:, :, 2 * H:], q[:, :, 2 * H:]) and torch.equal(t[:, :lead], q[:, :lead]) and torch.equal(t[..., dr:], q[..., dr:])
    assert R.ratio(R.rotary_emul(qkv, sin, cos, N, lead, H, dh, sign, swap=True), ref, bound) > 1.0


@pytest.mark.parametrize("ks,H,W,C,lead", CONV_SHAPES)
@pytest.mark.parametrize("kind", ["random", "impulse_a", "impulse_d"])
def test_conv_bounds_hold_for_the_emulation(ks, H, W, C, lead, kind):
    a, w, dout = R.conv_inputs(ks, H, W, C, lead, kind)
    ref, bound = R.conv_fwd_ref(a, w, ks, H, W, lead)
    r = R.ratio(R.conv_emul(a, w, ks, H, W, lead), ref, bound)
    da, bda, dw, bdw = R.conv_bwd_ref(a, w, dout, ks, H, W, lead)
    r2 = R.ratio(R.conv_emul(dout, w, ks, H, W, lead, flip=True), da, bda)
    r3 = R.ratio(R.conv_dw_emul(a, dout, ks, H, W, lead), dw, bdw)
    print("conv", (ks, H, W, C, lead, kind), "error / bound: out", r, "da", r2, "dw", r3)
    assert r <= 1.0 and r2 <= 1.0 and r3 <= 1.0


@pytest.mark.parametrize("ks", [3, 5, 7])
def test_a_wrong_tap_order_exceeds_the_conv_bound(ks):
    H, W = R.CONV_PLANES[-1]
    a, w, dout = R.conv_inputs(ks, H, W, 8, 1)
    ref, bound = R.conv_fwd_ref(a, w, ks, H, W, 1)
    transposed = torch.arange(ks * ks).reshape(ks, ks).t().reshape(-1)           # kx, ky instead of ky, kx
    assert R.ratio(R.conv_emul(a, w, ks, H, W, 1, order=transposed), ref, bound) > 1.0
    da, bda, _, _ = R.conv_bwd_ref(a, w, dout, ks, H, W, 1)
    assert R.ratio(R.conv_emul(dout, w, ks, H, W, 1, flip=False), torch.where(da == 0, da, da), bda) > 1.0     # unflipped taps


@pytest.mark.parametrize("case", R.GEGLU_CASES)
def test_geglu_bounds_hold_for_the_emulation(case):
    rows, hidden, ld = case
    u, dh = R.geglu_inputs(case)
    ref, bound = R.geglu_fwd_ref(u, hidden)
    r = R.ratio(R.geglu_fwd_emul(u, hidden), ref, bound)
    dref, dbound = R.geglu_bwd_ref(u, dh, hidden)
    r2 = R.ratio(R.geglu_bwd_emul(u, dh, hidden), dref, dbound)
    print("geglu", case, "error / bound: h", r, "du", r2)
    assert r <= 1.0 and r2 <= 1.0
    assert R.ratio(R.geglu_fwd_emul(u, hidden, swap=True), ref, bound) > 1.0
