"""CPU: what the model ports share through encoder.py -- the conv stems' feature order, the parameter holders and the run guard."""
import pytest
import torch

import port_checks as PC
from noise_robust_vit_amd import encoder as E


def _im2col(x, ks, stride, pad, KP, swap=False):
    """Plain torch im2col of x [B, C, H, W]: rows (b, oy, ox), features in (ky, kx, c) order, zero columns up to KP."""
    B, C, H, W = x.shape
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    xp = torch.nn.functional.pad(x, (pad, pad, pad, pad))
    taps = [xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            for ky, kx in ((b, a) if swap else (a, b) for a in range(ks) for b in range(ks))]
    cols = torch.stack(taps, dim=1).permute(0, 3, 4, 1, 2).reshape(B * Ho * Wo, ks * ks * C)      # [B, Ho, Wo, ks*ks, C]
    return torch.nn.functional.pad(cols, (0, KP - ks * ks * C)), Ho, Wo


def _wgrad_error(Co, Cin, ks, KP, swap):
    """max |conv_from_columns(dy^T cols) - autograd's conv2d weight gradient| in fp64, B = 2, 5 x 5 map, stride 2, pad 1."""
    torch.manual_seed(0)
    x = torch.randn(2, Cin, 5, 5, dtype=torch.float64)
    w = torch.randn(Co, Cin, ks, ks, dtype=torch.float64, requires_grad=True)
    cols, Ho, Wo = _im2col(x, ks, 2, 1, KP, swap)
    dy = torch.randn(2 * Ho * Wo, Co, dtype=torch.float64)                 # NHWC rows, as the stems' GEMMs see them
    y = torch.nn.functional.conv2d(x, w, stride=2, padding=1)
    y.backward(dy.reshape(2, Ho, Wo, Co).permute(0, 3, 1, 2))
    if not swap:                                                             # the forward product reads the same order
        rows = cols @ E.conv_to_columns(w.detach(), KP).t()
        assert float((rows - y.detach().permute(0, 2, 3, 1).reshape(-1, Co)).abs().max()) <= 1e-12
    return float((E.conv_from_columns(dy.t() @ cols, Cin, ks) - w.grad).abs().max())


CONV_CASES = [(8, 3, 3, 32), (16, 8, 3, 72), (8, 8, 7, 392), (8, 16, 1, 16)]     # (Co, Cin, ks, KP); 27 -> 32 is padded


@pytest.mark.parametrize("Co,Cin,ks,KP", CONV_CASES)
def test_conv_feature_order_round_trip_and_weight_gradient(Co, Cin, ks, KP):
    torch.manual_seed(1)
    w = torch.randn(Co, Cin, ks, ks, dtype=torch.float64)
    wc = E.conv_to_columns(w, KP)
    assert wc.shape == (Co, KP) and wc.is_contiguous() and not wc[:, ks * ks * Cin:].any()      # zero pad columns, if any
    assert torch.equal(E.conv_from_columns(wc, Cin, ks), w)
    assert _wgrad_error(Co, Cin, ks, KP, swap=False) <= 1e-12


def test_conv_feature_order_check_sees_a_ky_kx_swap():
    """The check above is not blind: an im2col in (kx, ky, c) order misses the bound by orders of magnitude."""
    for Co, Cin, ks, KP in CONV_CASES:
        if ks == 3:
            assert _wgrad_error(Co, Cin, ks, KP, swap=True) > 1e-3


def test_holders_refuse_a_direct_call_naming_their_class():
    from noise_robust_vit_amd import cait, deepvit, pit, rvt, twins_svt
    holders = [pit.Attention(64, heads=2, dim_head=32), pit.FeedForward(64, 128), deepvit.Residual(torch.nn.Identity()),
               deepvit.Attention(64, heads=2, dim_head=32), cait.LayerScale(64, torch.nn.Identity(), depth=1),
               cait.PreNorm(64, torch.nn.Identity()), rvt.GEGLU(), rvt.FeedForward(64, 128), twins_svt.PEG(64),
               twins_svt.PreNorm(64, torch.nn.Identity())]
    for h in holders:
        assert isinstance(h, E.Holder)
        with pytest.raises(NotImplementedError, match=f"^{type(h).__name__} holds parameters only"):
            h(torch.zeros(1, 4, 64))
    assert cait.PreNorm is pit.PreNorm is deepvit.PreNorm is rvt.PreNorm is E.PreNorm
    assert cait.FeedForward is pit.FeedForward is deepvit.FeedForward is E.FeedForward
    assert deepvit.Residual is twins_svt.Residual is E.Residual
    assert twins_svt.PreNorm is not E.PreNorm and rvt.FeedForward is not E.FeedForward       # their own: channel LN, GEGLU
    r = E.Rearrange('b c (h p1) (w p2) -> b (h w) (p1 p2 c)', p1=4, p2=4)
    assert repr(r) == "Rearrange('b c (h p1) (w p2) -> b (h w) (p1 p2 c)', p1=4, p2=4)" and not list(r.parameters())


def test_require_run_refuses_cpu_tensors_and_recording():
    from noise_robust_vit_amd._lib import NrvError
    x = torch.zeros(2, 3)
    with pytest.raises(NrvError, match="no CPU fallback"):
        E.require_run(x, "SomePort")
    E.require_run(PC.fake_cuda(x), "SomePort")
    with E.record_attention([]):
        with pytest.raises(NrvError, match="no CPU fallback"):            # the device check comes first
            E.require_run(x, "SomePort")
        with pytest.raises(NotImplementedError, match="recording is not implemented for SomePort"):
            E.require_run(PC.fake_cuda(x), "SomePort")
    E.require_run(PC.fake_cuda(x), "SomePort")


def test_kernel_constants_are_read_not_copied():
    from noise_robust_vit_amd import cct, kernels as K, rvt, t2t
    assert K.ATTN_FUSED_DH == (32, 64, 80, 96, 128) and K.SINKHORN_ITERS == 3
    assert [rvt._attention_kind(dh, False) for dh in (64, 72)] == ["softmax", "composed"]
    assert t2t._attention_kind(64) == "fused"
    with pytest.raises(NotImplementedError):
        cct.Attention(72, num_heads=1)
