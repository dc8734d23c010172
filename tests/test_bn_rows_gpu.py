"""GPU: batch norm over token rows (nrv_bn_stats / nrv_bn_apply / nrv_bn_bwd) against torch.nn.functional.batch_norm and its
autograd in fp64: statistics, running update, the apply variants, the backward, eval mode, and bit-identical reruns."""
import pytest
import torch
import torch.nn.functional as F

from noise_robust_vit_amd import kernels as K

pytestmark = pytest.mark.gpu


def _data(T, C, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    y = torch.randn(T, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)
    y[:, 0] = 1000.0 + 1.0 * torch.randn(T, generator=g)          # mean ~ 1e3 x the standard deviation
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    return y.to(dev), gamma.to(dev), beta.to(dev)


@pytest.mark.parametrize("T,C", [(1000, 16), (50176, 16), (6272, 128), (12544, 640)])
def test_stats_apply_and_running_update(dev, T, C):
    y, gamma, beta = _data(T, C, dev)
    rm = torch.randn(C, device=dev)
    rv = torch.rand(C, device=dev) + 0.5
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    mean, invstd, stat = K.bn_stats(y, 1e-5, 0.1, rm, rv)
    y64 = y.double()
    ref = F.batch_norm(y64, rm64, rv64, gamma.double(), beta.double(), True, 0.1, 1e-5)
    m64, v64 = y64.mean(0), y64.var(0, unbiased=False)
    assert torch.allclose(mean.double(), m64, rtol=0, atol=1e-6 * (m64.abs().max().item() + 1))
    assert ((invstd.double() - 1 / torch.sqrt(v64 + 1e-5)).abs() / (1 / torch.sqrt(v64 + 1e-5))).max() < 1e-5
    assert torch.equal(stat[0], torch.full_like(stat[0], float(T)))
    assert ((stat[2].double() / T - v64).abs() / v64).max() < 1e-5
    assert ((rm.double() - rm64).abs().max()) < 1e-4
    assert ((rv.double() - rv64).abs() / rv64).max() < 1e-5
    z32, z16 = K.bn_apply(y, mean, invstd, gamma, beta, want_f32=True)
    assert (z32.double() - ref).abs().max() < 2e-4 * ref.abs().max()
    assert torch.equal(z16, z32.to(torch.bfloat16))
    _, h16 = K.bn_apply(y, mean, invstd, gamma, beta, act=True)
    assert (h16.double() - F.hardswish(ref)).abs().max() < 1e-2 * ref.abs().max()
    res = torch.randn(T, C, device=dev)
    keep = (torch.arange(8, device=dev) % 3 != 0).float()
    o32, o16 = K.bn_apply(y, mean, invstd, gamma, beta, residual=res, keep=keep, survival=0.9, want_f32=True)
    f = (keep / 0.9).repeat_interleave(T // 8)[:, None].double()
    assert (o32.double() - (res.double() + ref * f)).abs().max() < 2e-4 * ref.abs().max()
    assert torch.equal(o16, o32.to(torch.bfloat16))


@pytest.mark.parametrize("T,C,act", [(1000, 16, True), (50176, 16, False), (6272, 128, True), (12544, 640, False)])
def test_backward_against_fp64_autograd(dev, T, C, act):
    y, gamma, beta = _data(T, C, dev, seed=1)
    mean, invstd, _ = K.bn_stats(y, 1e-5, 0.1)
    dz = torch.randn(T, C, device=dev)
    keep = None if act else (torch.arange(8, device=dev) % 4 != 1).float()
    dy, dg, db = K.bn_bwd(dz, y, mean, invstd, gamma, beta, eps=1e-5, act=act, keep=keep, survival=0.75)
    y64 = y.double().requires_grad_()
    g64 = gamma.double().requires_grad_()
    b64 = beta.double().requires_grad_()
    z = F.batch_norm(y64, None, None, g64, b64, True, 0.1, 1e-5)
    if act:
        z = F.hardswish(z)
    if keep is not None:
        z = z * (keep.double() / 0.75).repeat_interleave(T // 8)[:, None]
    z.backward(dz.double())
    for got, ref, tol in ((dy.double(), y64.grad, 1e-2), (dg.double(), g64.grad, 1e-4), (db.double(), b64.grad, 1e-4)):
        assert ((got - ref).norm() / ref.norm()).item() < tol
    again = K.bn_bwd(dz, y, mean, invstd, gamma, beta, eps=1e-5, act=act, keep=keep, survival=0.75)
    assert all(torch.equal(a, b) for a, b in zip((dy, dg, db), again))


def test_reruns_are_bit_identical_and_eval_mode(dev):
    y, gamma, beta = _data(50176, 128, dev, seed=2)
    a = K.bn_stats(y, 1e-5, 0.1)
    b = K.bn_stats(y, 1e-5, 0.1)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    rm, rv = torch.randn(128, device=dev), torch.rand(128, device=dev) + 0.5
    z32, _ = K.bn_apply(y, rm, rv, gamma, beta, eps=1e-5, scale_is_var=True, want_f32=True)
    ref = F.batch_norm(y.double(), rm.double(), rv.double(), gamma.double(), beta.double(), False, 0.1, 1e-5)
    assert (z32.double() - ref).abs().max() < 1e-4 * ref.abs().max()
    dz = torch.randn_like(y)
    dy, dg, db = K.bn_bwd(dz, y, rm, rv, gamma, beta, eps=1e-5, scale_is_var=True, training=False)
    k = gamma.double() / torch.sqrt(rv.double() + 1e-5)
    assert ((dy.double() - dz.double() * k).norm() / (dz.double() * k).norm()) < 1e-2
    assert ((db.double() - dz.double().sum(0)).abs().max()) < 1e-3
