"""nrv_window_attn_fwd / _bwd against fp32 (and fp64) torch on the same bf16 operands: windows 7 and 8, head dims 32 and 64,
shift 0 and 3, padded and unpadded maps, softmax and Sinkhorn; a peaked Sinkhorn case checked per key; bit-identical reruns."""
import pytest
import torch

import swin_ref

pytestmark = pytest.mark.gpu


def _case(dev, B, pH, pW, C, heads, window, seed, table_scale=0.5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = (torch.randn(B * pH * pW, 3 * C, generator=g) * 1.0).to(torch.bfloat16).to(dev)
    T = (2 * window[0] - 1) * (2 * window[1] - 1)
    table = (torch.randn(T, heads, generator=g) * table_scale).to(dev)
    dout = torch.randn(B * pH * pW, C, generator=g).to(torch.bfloat16).to(dev)
    return qkv, table, dout


def _ref(qkv, table, dout, B, pH, pW, C, heads, window, shift, robust, dtype=torch.float32):
    q = qkv.to(dtype).reshape(B, pH, pW, 3 * C).detach().requires_grad_(True)
    t = table.to(dtype).detach().requires_grad_(True)
    o = swin_ref.window_core(q, t, heads, window, shift, robust)
    (o * dout.to(dtype).reshape(B, pH, pW, C)).sum().backward()
    return o.reshape(B * pH * pW, C), q.grad.reshape(B * pH * pW, 3 * C), t.grad


def _rel_max(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()


def _rel_l2(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


GEOMS = [  # (B, pH, pW, C, heads, window, shift)
    (2, 14, 14, 64, 2, (7, 7), (0, 0)),
    (2, 14, 14, 64, 2, (7, 7), (3, 3)),
    (2, 21, 21, 32, 1, (7, 7), (3, 3)),       # padded grid of a 16 x 16 map
    (1, 14, 28, 128, 2, (7, 7), (3, 3)),      # dh 64
    (2, 16, 16, 64, 2, (8, 8), (0, 0)),
    (2, 16, 24, 64, 1, (8, 8), (4, 4)),       # window 8, dh 64
    (2, 7, 14, 64, 2, (7, 7), (0, 3)),        # one axis unshifted
]


@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("geom", GEOMS)
def test_window_attn_matches_fp32(dev, geom, robust):
    from noise_robust_vit_amd import kernels as K
    B, pH, pW, C, heads, window, shift = geom
    qkv, table, dout = _case(dev, B, pH, pW, C, heads, window, seed=hash((geom, robust)) % 1000)
    out, stats = K.window_attn_fwd(qkv, table, B, pH, pW, C, heads, window, shift, robust)
    dqkv, dtable = K.window_attn_bwd(qkv, table, dout, stats, B, pH, pW, C, heads, window, shift, robust)
    ro, rdq, rdt = _ref(qkv, table, dout, B, pH, pW, C, heads, window, shift, robust)
    assert _rel_max(out, ro) < 1e-2
    assert _rel_l2(out, ro) < 5e-3
    assert _rel_l2(dqkv, rdq) < 1e-2
    assert _rel_l2(dtable, rdt) < 5e-3


def test_peaked_sinkhorn_per_key_against_fp64(dev):
    """Keys whose scores lie 12-20 nats below the rest: Sinkhorn rescales their columns; every key's dK / dV row must hold."""
    from noise_robust_vit_amd import kernels as K
    B, pH, pW, C, heads, window, shift = 2, 14, 14, 32, 1, (7, 7), (3, 3)
    qkv, table, dout = _case(dev, B, pH, pW, C, heads, window, seed=5, table_scale=0.2)
    # a bias of -12..-20 on the relative offsets whose row difference is 3: those pairs are 12-20 nats down
    T = table.shape[0]
    dy = torch.arange(T, device=dev) // 13 - 6
    table[dy.abs() == 3] -= torch.linspace(12.0, 20.0, int((dy.abs() == 3).sum()), device=dev)[:, None]
    out, stats = K.window_attn_fwd(qkv, table, B, pH, pW, C, heads, window, shift, True)
    dqkv, dtable = K.window_attn_bwd(qkv, table, dout, stats, B, pH, pW, C, heads, window, shift, True)
    ro, rdq, rdt = _ref(qkv, table, dout, B, pH, pW, C, heads, window, shift, True, dtype=torch.float64)
    assert _rel_l2(out, ro) < 5e-3
    dk, dv = dqkv[:, C:2 * C].double(), dqkv[:, 2 * C:].double()
    rk, rv = rdq[:, C:2 * C], rdq[:, 2 * C:]
    ek = (dk - rk).norm(dim=1) / rk.norm(dim=1).clamp_min(1e-30)
    ev = (dv - rv).norm(dim=1) / rv.norm(dim=1).clamp_min(1e-30)
    assert ek.max().item() < 3e-2, ek.max().item()
    assert ev.max().item() < 3e-2, ev.max().item()
    assert _rel_l2(dtable, rdt) < 5e-3


@pytest.mark.parametrize("robust", [False, True])
def test_backward_is_bit_identical(dev, robust):
    from noise_robust_vit_amd import kernels as K
    B, pH, pW, C, heads, window, shift = 8, 14, 21, 64, 2, (7, 7), (3, 3)     # 48 windows: 6 partials per table entry
    qkv, table, dout = _case(dev, B, pH, pW, C, heads, window, seed=9)
    out, stats = K.window_attn_fwd(qkv, table, B, pH, pW, C, heads, window, shift, robust)
    a = K.window_attn_bwd(qkv, table, dout, stats, B, pH, pW, C, heads, window, shift, robust)
    b = K.window_attn_bwd(qkv, table, dout, stats, B, pH, pW, C, heads, window, shift, robust)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    out2, _ = K.window_attn_fwd(qkv, table, B, pH, pW, C, heads, window, shift, robust)
    assert torch.equal(out, out2)


def test_stochastic_depth_kernels(dev):
    from noise_robust_vit_amd import kernels as K
    B, n, D = 4, 49, 96
    x = torch.randn(B * n, D, device=dev)
    y = torch.randn(B * n, D, device=dev)
    keep = torch.tensor([1.0, 0.0, 1.0, 1.0], device=dev)
    out = K.sd_add(x, y, keep, 0.8)
    ref = x + y * (keep / 0.8).repeat_interleave(n)[:, None]
    assert torch.allclose(out, ref, rtol=1e-6, atol=1e-6)
    d = K.sd_scale_bf16(y, keep, 0.8)
    assert torch.equal(d, (y * (keep / 0.8).repeat_interleave(n)[:, None]).to(torch.bfloat16))
