"""GPU: the tokens-to-token kernels (csrc/nrv_t2t.hip, nrv_attn_wide_* of nrv_attn_gen.hip) against torch.

soft split vs F.unfold: a copy, exact.  Its backward vs the autograd gradient of F.unfold: integer-valued data, so the fp32 sums
are exact in any order (the check of test_conv_unfold_gpu.py for nrv_conv_fold).  LayerNorm over n of ld columns vs F.layer_norm.
Wide-head attention vs fp32 torch on the same bf16 q / k / v with the bounds of test_kernels_gpu.py's streaming kernels.  Every
kernel: reruns are bit-identical, pad columns are zero, shapes outside the contract are refused."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from noise_robust_vit_amd import kernels as K  # noqa: E402
from noise_robust_vit_amd._lib import NrvError  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def rnd(shape, dev, seed, scale=1.0, dtype=torch.bfloat16):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)


# (B, C, H, W, ks, stride): the three T2T stages at 64 px and 224 px geometry, one channel, even kernel
SPLITS = [(2, 3, 64, 64, 7, 4), (2, 147, 16, 16, 3, 2), (1, 1323, 8, 8, 3, 2), (3, 1, 20, 20, 3, 2), (2, 9, 10, 10, 3, 2),
          (1, 3, 224, 224, 7, 4), (1, 147, 56, 56, 3, 2), (2, 5, 9, 9, 4, 3), (1, 2, 7, 7, 5, 1)]


@pytest.mark.parametrize("B,C,H,W,ks,stride", SPLITS)
def test_soft_split_and_its_backward_match_unfold(dev, B, C, H, W, ks, stride):
    pad = stride // 2
    g = torch.Generator().manual_seed(C + ks)
    img = torch.randint(-8, 9, (B, C, H, W), generator=g).float().to(dev)
    ref = F.unfold(img, ks, padding=pad, stride=stride).transpose(1, 2).reshape(-1, ks * ks * C)        # [B*L, C*k*k]
    Fd, Fp = ks * ks * C, K.pad8(ks * ks * C)
    Cp = K.pad8(C)
    rows = torch.zeros(B * H * W, Cp, device=dev)
    rows[:, :C] = img.permute(0, 2, 3, 1).reshape(-1, C)
    rows[:, C:] = 77.0                                             # pad columns of the source are never read
    got = [K.soft_split_fwd(img, B, C, H, W, ks, stride, pad, rows=False),
           K.soft_split_fwd(img.to(torch.bfloat16), B, C, H, W, ks, stride, pad, rows=False),
           K.soft_split_fwd(rows.to(torch.bfloat16), B, C, H, W, ks, stride, pad, rows=True)]
    for cols in got:
        assert cols.shape == (ref.shape[0], Fp) and cols.dtype == torch.bfloat16
        assert torch.equal(cols[:, :Fd].float(), ref)
        assert torch.equal(cols[:, Fd:], torch.zeros_like(cols[:, Fd:]))
    assert torch.equal(got[2], K.soft_split_fwd(rows.to(torch.bfloat16), B, C, H, W, ks, stride, pad, rows=True))
    # a random bf16 image goes through bit-exact (a copy)
    xb = rnd((B, C, H, W), dev, 5)
    cb = K.soft_split_fwd(xb, B, C, H, W, ks, stride, pad, rows=False)
    assert torch.equal(cb[:, :Fd], F.unfold(xb.float(), ks, padding=pad, stride=stride).transpose(1, 2).reshape(-1, Fd).to(torch.bfloat16))
    # backward: the autograd gradient of F.unfold on bf16 dcols, fp32
    d = torch.randint(-8, 9, (ref.shape[0], Fp), generator=g).float().to(dev)
    x = img.clone().requires_grad_(True)
    (F.unfold(x, ks, padding=pad, stride=stride).transpose(1, 2).reshape(-1, Fd) * d[:, :Fd]).sum().backward()
    want = x.grad.permute(0, 2, 3, 1).reshape(-1, C)
    dx = K.soft_split_bwd(d.to(torch.bfloat16), B, C, H, W, ks, stride, pad)
    assert dx.shape == (B * H * W, Cp) and dx.dtype == torch.float32
    assert torch.equal(dx[:, :C], want)
    assert torch.equal(dx[:, C:], torch.zeros_like(dx[:, C:]))
    assert torch.equal(dx, K.soft_split_bwd(d.to(torch.bfloat16), B, C, H, W, ks, stride, pad))
    # random (non-integer) dcols: fp32 summation order only
    dr = rnd((ref.shape[0], Fp), dev, 9)
    x.grad = None
    (F.unfold(x, ks, padding=pad, stride=stride).transpose(1, 2).reshape(-1, Fd) * dr[:, :Fd].float()).sum().backward()
    dxr = K.soft_split_bwd(dr, B, C, H, W, ks, stride, pad)
    want = x.grad.permute(0, 2, 3, 1).reshape(-1, C)
    assert (dxr[:, :C] - want).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item())


def test_soft_split_refuses_what_it_does_not_take(dev):
    img = torch.zeros(1, 3, 16, 16, device=dev)
    with pytest.raises(NrvError):
        K.soft_split_fwd(img, 1, 3, 16, 16, 9, 4, 2, rows=False)              # kernel above 7
    with pytest.raises(NrvError):
        K.soft_split_fwd(img, 1, 3, 16, 16, 3, 2, 3, rows=False)              # pad >= kernel
    with pytest.raises(NrvError):
        K.soft_split_fwd(torch.zeros(256, 8, device=dev), 1, 3, 16, 16, 3, 2, 1, rows=True)      # token rows must be bf16
    with pytest.raises(NrvError):
        K.soft_split_bwd(torch.zeros(64, 24, device=dev, dtype=torch.bfloat16), 1, 3, 16, 16, 3, 2, 1)   # needs 32 columns


@pytest.mark.parametrize("rows,n", [(37, 9), (3136, 147), (784, 1323), (5, 4096), (130, 81), (1, 147), (20000, 9)])
@pytest.mark.parametrize("xdt", [torch.float32, torch.bfloat16])
def test_layernorm_over_true_width(dev, rows, n, xdt):
    ld = K.pad8(n)
    x = torch.zeros(rows, ld, device=dev, dtype=xdt)
    x[:, :n] = rnd((rows, n), dev, 1, 2.0, torch.float32).add_(0.5).to(xdt)
    gamma = rnd((n,), dev, 2, 0.2, torch.float32) + 1.0
    beta = rnd((n,), dev, 3, 0.2, torch.float32)
    y, mean, rstd = K.layernorm_pad_fwd(x, n, gamma, beta, 1e-5)
    xr = x[:, :n].float().clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ref = F.layer_norm(xr, (n,), gr, br, 1e-5)
    assert y.shape == (rows, ld) and y.dtype == torch.bfloat16
    assert (y[:, :n].float() - ref).abs().max().item() <= 2 ** -8 * ref.abs().max().item() + 1e-5
    assert torch.equal(y[:, n:], torch.zeros_like(y[:, n:]))
    assert (mean - xr.mean(-1)).abs().max().item() <= 1e-5 and (rstd * xr.var(-1, unbiased=False).add(1e-5).sqrt() - 1).abs().max().item() <= 1e-4
    again = K.layernorm_pad_fwd(x, n, gamma, beta, 1e-5)
    assert all(torch.equal(a, b) for a, b in zip((y, mean, rstd), again))
    dy = torch.zeros(rows, ld, device=dev, dtype=torch.bfloat16)
    dy[:, :n] = rnd((rows, n), dev, 4)
    dres = torch.zeros(rows, ld, device=dev)
    dres[:, :n] = rnd((rows, n), dev, 5, 1.0, torch.float32)
    ref.backward(dy[:, :n].float())
    dx32, dx16, dg, db = K.layernorm_pad_bwd(dy, x, n, gamma, mean, rstd, dres=dres, want_f32=True, want_bf16=True)
    want = xr.grad + dres[:, :n]
    assert (dx32[:, :n] - want).abs().max().item() <= 1e-4 * max(1.0, want.abs().max().item())
    assert torch.equal(dx32[:, n:], torch.zeros_like(dx32[:, n:])) and torch.equal(dx16[:, n:], torch.zeros_like(dx16[:, n:]))
    assert torch.equal(dx16, dx32.to(torch.bfloat16))
    # column sums over `rows` terms in fp32, another order than torch's
    tol = 1e-5 * rows ** 0.5 + 1e-4
    assert (dg - gr.grad).abs().max().item() <= tol * max(1.0, gr.grad.abs().max().item())
    assert (db - br.grad).abs().max().item() <= tol * max(1.0, br.grad.abs().max().item())
    again = K.layernorm_pad_bwd(dy, x, n, gamma, mean, rstd, dres=dres, want_f32=True, want_bf16=True)
    assert all(torch.equal(a, b) for a, b in zip((dx32, dx16, dg, db), again))
    # without a residual gradient
    dx0, _, _, _ = K.layernorm_pad_bwd(dy, x, n, gamma, mean, rstd)
    assert (dx0[:, :n] - xr.grad).abs().max().item() <= 1e-4 * max(1.0, xr.grad.abs().max().item())


def test_layernorm_pad_refuses_what_it_does_not_take(dev):
    g, b = torch.ones(4097, device=dev), torch.zeros(4097, device=dev)
    with pytest.raises(NrvError):
        K.layernorm_pad_fwd(torch.zeros(4, 4104, device=dev), 4097, g, b, 1e-5)             # n above 4096
    with pytest.raises(NrvError):
        K.layernorm_pad_fwd(torch.zeros(4, 150, device=dev), 147, g[:147], b[:147], 1e-5)   # stride not a multiple of 8
    with pytest.raises(NrvError):
        K.layernorm_pad_fwd(torch.zeros(4, 152, device=dev), 147, g[:146], b[:147], 1e-5)


def attn_ref(qkv, B, N, H, dh, scale):
    q, k, v = qkv.float().reshape(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * scale
    o = torch.softmax(s, dim=-1) @ v
    return o.permute(0, 2, 1, 3).reshape(B * N, H * dh), torch.logsumexp(s, dim=-1)


# (B, N, H, dh, true width): stage 1 of T2T-ViT at 224 px (147 in 152), N off the 64-row tile, the smallest and the largest
# head dims, a single row, two heads
WIDE = [(1, 3136, 1, 152, 147), (2, 3136, 1, 160, 147), (2, 300, 1, 136, 136), (1, 777, 1, 192, 192), (2, 65, 2, 168, 168),
        (1, 1, 1, 152, 152), (3, 64, 1, 192, 190), (1, 1000, 2, 136, 130)]


@pytest.mark.parametrize("B,N,H,dh,true", WIDE)
def test_wide_head_attention(dev, B, N, H, dh, true):
    scale = true ** -0.5
    qkv = rnd((B * N, 3, H, dh), dev, 160, 1.0)
    qkv[..., true:] = 0                                            # the zero pad columns of an odd head width
    qkv = qkv.reshape(B * N, 3 * H * dh).contiguous()
    out, lse = K.attn_wide_fwd(qkv, B, N, H, dh, scale)
    qr = qkv.float().requires_grad_(True)
    ref_o, ref_lse = attn_ref(qr, B, N, H, dh, scale)
    assert (out.float() - ref_o).abs().max().item() < 2 ** -7 * ref_o.abs().max().item() + 1e-3
    assert (lse - ref_lse).abs().max().item() < 1e-4 * max(1.0, ref_lse.abs().max().item())
    pad = out.reshape(B * N, H, dh)[..., true:]
    assert torch.equal(pad, torch.zeros_like(pad))
    dout = rnd((B * N, H, dh), dev, 161, 1.0)
    dout[..., true:] = 0
    dout = dout.reshape(B * N, H * dh).contiguous()
    ref_o.backward(dout.float())
    dqkv = K.attn_wide_bwd(qkv, out, dout, lse, B, N, H, dh, scale)
    err = (dqkv.float() - qr.grad).abs().max().item() / qr.grad.abs().max().item()
    print(f"B {B} N {N} H {H} dh {dh}: dqkv max err / max {err:.3e}")
    assert err < 2e-2, err
    cos = F.cosine_similarity(dqkv.float().reshape(-1), qr.grad.reshape(-1), dim=0).item()
    assert cos > 0.9995, cos
    dpad = dqkv.reshape(B * N, 3, H, dh)[..., true:]
    assert torch.equal(dpad, torch.zeros_like(dpad))
    out2, lse2 = K.attn_wide_fwd(qkv, B, N, H, dh, scale)
    assert torch.equal(out, out2) and torch.equal(lse, lse2)
    assert torch.equal(dqkv, K.attn_wide_bwd(qkv, out, dout, lse, B, N, H, dh, scale))


def test_wide_head_attention_matches_the_composed_path(dev):
    """The path the stage-1 shape would take without the fused kernels: nrv_bgemm + softmax on the matrix + nrv_bgemm."""
    B, N, dh = 1, 784, 152
    qkv = rnd((B * N, 3 * dh), dev, 7, 1.0)
    o1, _ = K.attn_wide_fwd(qkv, B, N, 1, dh, 147 ** -0.5)
    o2, _ = K.attn_composed_fwd(qkv, B, N, 1, dh, 147 ** -0.5, 0)
    assert (o1.float() - o2.float()).abs().max().item() < 2 ** -6 * o2.float().abs().max().item()


@pytest.mark.parametrize("dh", [128, 64, 140, 200, 256])
def test_wide_head_attention_refuses_other_head_dims(dev, dh):
    qkv = torch.zeros(64, 3 * dh, device=dev, dtype=torch.bfloat16)
    with pytest.raises(NrvError):
        K.attn_wide_fwd(qkv, 1, 64, 1, dh, 1.0)
    o = torch.zeros(64, dh, device=dev, dtype=torch.bfloat16)
    with pytest.raises(NrvError):
        K.attn_wide_bwd(qkv, o, o, torch.zeros(1, 1, 64, device=dev), 1, 64, 1, dh, 1.0)
