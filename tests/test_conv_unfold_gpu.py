"""GPU: the stem's unfold / fold (nrv_conv_unfold / nrv_conv_fold) against F.unfold / F.fold, exactly (integer-valued data),
for the four stem geometries, and Conv2d_BN end to end against fp32 torch."""
import pytest
import torch
import torch.nn.functional as F

from noise_robust_vit_amd import kernels as K
from noise_robust_vit_amd import levit as L

pytestmark = pytest.mark.gpu

GEOMS = [(2, 3, 224, 224), (2, 16, 112, 112), (2, 32, 56, 56), (2, 64, 28, 28), (3, 8, 7, 9)]


def _perm(cols_unfold, C):
    """F.unfold's (c, ky, kx) feature order -> the kernel's (ky, kx, c)."""
    B, F9, L_ = cols_unfold.shape
    return cols_unfold.reshape(B, C, 9, L_).permute(0, 3, 2, 1).reshape(B * L_, 9 * C)


@pytest.mark.parametrize("B,C,H,W", GEOMS)
def test_unfold_and_fold_match_torch(dev, B, C, H, W):
    g = torch.Generator().manual_seed(C)
    x = torch.randint(-8, 9, (B, C, H, W), generator=g).float().to(dev)
    ref = _perm(F.unfold(x, 3, padding=1, stride=2), C)
    Ho, Wo = K.conv_out_size(H, 3, 2, 1), K.conv_out_size(W, 3, 2, 1)
    if C == 3:
        cols = K.conv_unfold(x, B, C, H, W, 3, 2, 1, nhwc=False)
        assert torch.equal(cols[:, 27:], torch.zeros_like(cols[:, 27:]))
    else:
        rows = x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
        cols = K.conv_unfold(rows, B, C, H, W, 3, 2, 1, nhwc=True)
    assert cols.shape == (B * Ho * Wo, (9 * C + 7) // 8 * 8)
    assert torch.equal(cols[:, :9 * C].float(), ref)
    d = torch.randint(-8, 9, (B * Ho * Wo, cols.shape[1]), generator=g).float().to(dev)
    dx = K.conv_fold(d.to(torch.bfloat16).contiguous(), B, C, H, W, 3, 2, 1)
    dcols = d[:, :9 * C].reshape(B, Ho * Wo, 3, 3, C).permute(0, 4, 2, 3, 1).reshape(B, 9 * C, Ho * Wo)
    fref = F.fold(dcols, (H, W), 3, padding=1, stride=2).permute(0, 2, 3, 1).reshape(B * H * W, C)
    assert torch.equal(dx, fref)


@pytest.mark.parametrize("train", [True, False])
def test_conv2d_bn_end_to_end(dev, train):
    torch.manual_seed(0)
    m = L.Conv2d_BN(16, 32, 3, 2, 1)
    with torch.no_grad():
        m.bn.weight.copy_(1 + 0.1 * torch.randn(32)); m.bn.bias.copy_(0.1 * torch.randn(32))
        m.bn.running_mean.copy_(0.1 * torch.randn(32)); m.bn.running_var.copy_(torch.rand(32) + 0.5)
    ref = L.Conv2d_BN(16, 32, 3, 2, 1)
    ref.load_state_dict(m.state_dict())
    m, ref = m.to(dev).train(train), ref.to(dev).train(train)
    x = torch.randn(4, 16, 56, 56, device=dev)
    y = m(x)
    yr = torch.nn.Sequential.forward(ref, x)           # the plain Conv2d -> BatchNorm2d of the reference
    assert ((y - yr).abs().max() / yr.abs().max()).item() < 2e-2
    if train:
        assert ((m.bn.running_var - ref.bn.running_var).abs().max() / ref.bn.running_var.abs().max()).item() < 1e-2
        g = torch.randn_like(yr)
        y.backward(g)
        yr.backward(g)
        for a, b in ((m.c.weight.grad, ref.c.weight.grad), (m.bn.weight.grad, ref.bn.weight.grad), (m.bn.bias.grad, ref.bn.bias.grad)):
            assert ((a - b).norm() / b.norm()).item() < 2e-2
