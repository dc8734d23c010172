"""GPU: the PatchConvNet kernels (include/nrv.h, ABI 17) against fp32 PyTorch on the same bf16 operands, bit-identical reruns,
and NRV_ERR_SHAPE for shapes outside their range."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from noise_robust_vit_amd import _lib
from noise_robust_vit_amd import kernels as K

pytestmark = pytest.mark.gpu
dev = "cuda"


def _rel(a, b):
    a, b = a.detach().float().reshape(-1), b.detach().float().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(*shape, device=dev, generator=g) * scale).to(torch.bfloat16)


def _f(*shape, scale=1.0, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(*shape, device=dev, generator=g) * scale


def _nchw(rows, B, H, W):
    return rows.float().reshape(B, H, W, -1).permute(0, 3, 1, 2)


def _rows(nchw):
    return nchw.permute(0, 2, 3, 1).reshape(-1, nchw.shape[1])


@pytest.mark.parametrize("B,r,C", [(2, 4, 64), (3, 7, 384), (2, 14, 1024)])
def test_dwconv_fwd_bwd(B, r, C):
    a = _bf(B * r * r, C, seed=1)
    w, bias = _f(C, 1, 3, 3, scale=0.3, seed=2), _f(C, scale=0.1, seed=3)
    d, sq = K.dwconv3x3_fwd(a, w, bias, B, r, r)
    at = _nchw(a, B, r, r).requires_grad_(True)
    wt, bt = w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    dref = F.gelu(F.conv2d(at, wt, bt, padding=1, groups=C))
    assert _rel(d, _rows(dref)) < 1e-2
    assert _rel(sq, dref.sum((2, 3))) < 1e-4
    # backward with an SE gate s and a mean gradient, and the 1x1 conv's gelu' (bf16 stream)
    dg = _bf(B * r * r, C, seed=4)
    s, dmean = torch.sigmoid(_f(B, C, seed=5)), _f(B, C, seed=6)
    gs = (torch.rand(B * r * r, C, device=dev) + 0.1).to(torch.bfloat16)
    da, dw, db = K.dwconv3x3_bwd(a, w, bias, dg, s, dmean, B, r, r, gelu_stream=gs)
    L = (dref * _nchw(dg, B, r, r) * s[:, :, None, None]).sum() + (dref.mean((2, 3)) * dmean).sum()
    ga, gw, gb = torch.autograd.grad(L, (at, wt, bt))
    assert _rel(da, _rows(ga) * gs.float()) < 1e-2
    assert _rel(dw, gw) < 1e-4 and _rel(db, gb) < 1e-4
    # edge and corner tokens individually
    ref = _rows(ga) * gs.float()
    for p in (0, r - 1, r * (r - 1), r * r - 1):
        assert _rel(da[p], ref[p]) < 1e-2
    again = K.dwconv3x3_bwd(a, w, bias, dg, s, dmean, B, r, r, gelu_stream=gs)
    assert all(torch.equal(x, y) for x, y in zip((da, dw, db), again))
    assert all(torch.equal(x, y) for x, y in zip((d, sq), K.dwconv3x3_fwd(a, w, bias, B, r, r)))


@pytest.mark.parametrize("B", [1, 64])
def test_se(B):
    C, rd, HW = 384, 96, 49
    d = _bf(B * HW, C, seed=1)
    sq = d.float().reshape(B, HW, C).sum(1)
    wr, br = _f(rd, C, 1, 1, scale=0.05, seed=2), _f(rd, scale=0.1, seed=3)
    we, be = _f(C, rd, 1, 1, scale=0.1, seed=4), _f(C, scale=0.1, seed=5)
    s, hid = K.se_fwd(sq, HW, wr, br, we, be)
    P = [t.clone().requires_grad_(True) for t in (sq, wr, br, we, be)]
    h = F.relu(F.linear(P[0] / HW, P[1].reshape(rd, C), P[2]))
    sref = torch.sigmoid(F.linear(h, P[3].reshape(C, rd), P[4]))
    assert _rel(s, sref) < 1e-5 and _rel(hid, h) < 1e-5
    g = K.se_apply(d, s, HW)
    assert _rel(g, d.float().reshape(B, HW, C) * s[:, None]) < 1e-2
    dg = _bf(B * HW, C, seed=6)
    dmean, dwr, dbr, dwe, dbe = K.se_bwd(dg, d, sq, HW, s, hid, wr, we)
    L = ((dg.float().reshape(B, HW, C) * d.float().reshape(B, HW, C)).sum(1) * sref).sum()
    gs = torch.autograd.grad(L, P)
    assert _rel(dmean, gs[0] * HW) < 1e-4
    for x, y in zip((dwr, dbr, dwe, dbe), gs[1:]):
        assert _rel(x, y) < 1e-4
    again = K.se_bwd(dg, d, sq, HW, s, hid, wr, we)
    assert all(torch.equal(x, y) for x, y in zip((dmean, dwr, dbr, dwe, dbe), again))


@pytest.mark.parametrize("with_keep", [False, True])
def test_ls_add_bwd(with_keep):
    B, N, C = 4, 49, 384
    x, y, gamma = _f(B * N, C, seed=1), _f(B * N, C, seed=2), _f(C, scale=0.1, seed=3)
    keep = torch.tensor([1.0, 0.0, 1.0, 1.0], device=dev) if with_keep else None
    surv = 0.8 if with_keep else 1.0
    f = (keep / surv).repeat_interleave(N)[:, None] if with_keep else torch.ones(B * N, 1, device=dev)
    out = K.ls_add(x, y, gamma, keep, surv)
    assert _rel(out, x + f * gamma * y) < 1e-6
    dy = _f(B * N, C, seed=4)
    dz, dgamma = K.ls_bwd(dy, y, gamma, keep, surv)
    assert _rel(dz, dy * f * gamma) < 1e-2
    assert _rel(dgamma, (dy * f * y).sum(0)) < 1e-5
    dz2, dg2 = K.ls_bwd(dy, y, gamma, keep, surv)
    assert torch.equal(dz, dz2) and torch.equal(dgamma, dg2)


def test_dgelu_rows_both_streams():
    rows, C = 37, 128
    xn = _bf(rows, C, seed=1)
    w = _bf(C, C, scale=0.1, seed=2)
    bias = _f(C, scale=0.1, seed=3)
    u16 = torch.empty(rows, C, dtype=torch.bfloat16, device=dev)
    u8 = torch.empty(rows + 1, C, dtype=torch.uint8, device=dev)
    K.gemm_nt(xn, w, epilogue=_lib.EPI_BIAS_GELU, bias=bias, aux_out=u16)
    K.gemm_nt(xn, w, epilogue=_lib.EPI_BIAS_GELU_Q8, bias=bias, aux_out=u8)
    pre = (xn.float() @ w.float().t() + bias).requires_grad_(True)
    gp = torch.autograd.grad(F.gelu(pre).sum(), pre)[0]
    dx = _f(rows, C, seed=4)
    assert _rel(K.dgelu_rows(dx, u16), dx * gp) < 1e-2
    assert _rel(K.dgelu_rows(dx, u8), dx * gp) < 1e-2


@pytest.mark.parametrize("dh,Np,H", [(64, 16, 1), (384, 196, 1), (768, 196, 1), (1024, 1024, 1), (64, 196, 6), (64, 1024, 6)])
def test_cls_attn(dh, Np, H):
    B, C = 3, H * dh
    q, kc, vc = _bf(B, C, seed=1), _bf(B, C, seed=2), _bf(B, C, seed=3)
    kp, vp = _bf(B * Np, C, seed=4), _bf(B * Np, C, seed=5)
    scale = dh ** -0.5
    o, lse = K.cls_attn_fwd(q, kc, kp, vc, vp, B, H, Np, dh, scale)
    T = [t.float().requires_grad_(True) for t in (q, kc, kp, vc, vp)]
    k = torch.cat((T[1][:, None], T[2].reshape(B, Np, C)), 1).reshape(B, Np + 1, H, dh).transpose(1, 2)
    v = torch.cat((T[3][:, None], T[4].reshape(B, Np, C)), 1).reshape(B, Np + 1, H, dh).transpose(1, 2)
    s = torch.einsum("bhd,bhjd->bhj", T[0].reshape(B, H, dh), k) * scale
    oref = torch.einsum("bhj,bhjd->bhd", torch.softmax(s, -1), v).reshape(B, C)
    assert _rel(o, oref) < 1e-2
    assert _rel(lse, torch.logsumexp(s, -1).reshape(-1)) < 1e-5
    do = _bf(B, C, seed=6)
    grads = K.cls_attn_bwd(q, kc, kp, vc, vp, do, lse, B, H, Np, dh, scale)
    gref = torch.autograd.grad((oref * do.float()).sum(), T)
    for x, y in zip(grads, gref):
        assert _rel(x, y) < 2e-2
    again = K.cls_attn_bwd(q, kc, kp, vc, vp, do, lse, B, H, Np, dh, scale)
    assert all(torch.equal(x, y) for x, y in zip(grads, again))
    o2, l2 = K.cls_attn_fwd(q, kc, kp, vc, vp, B, H, Np, dh, scale)
    assert torch.equal(o, o2) and torch.equal(lse, l2)


def test_cls_attn_peaked():
    B, H, dh, Np = 2, 1, 384, 196
    q = torch.zeros(B, dh, device=dev); q[:, 0] = 1.0
    kp = _f(B * Np, dh, scale=0.1, seed=1); kp[5, 0] = 20.0 * dh ** 0.5       # one key 20 nats above the rest
    kc, vc, vp = _f(B, dh, scale=0.1, seed=2), _f(B, dh, seed=3), _f(B * Np, dh, seed=4)
    bf = [t.to(torch.bfloat16) for t in (q, kc, kp, vc, vp)]
    o, lse = K.cls_attn_fwd(*bf, B, H, Np, dh, dh ** -0.5)
    k = torch.cat((bf[1].float()[:, None], bf[2].float().reshape(B, Np, dh)), 1)
    v = torch.cat((bf[3].float()[:, None], bf[4].float().reshape(B, Np, dh)), 1)
    s = torch.einsum("bd,bjd->bj", bf[0].float(), k) * dh ** -0.5
    oref = torch.einsum("bj,bjd->bd", torch.softmax(s, -1), v)
    assert torch.isfinite(o.float()).all()
    assert _rel(o, oref) < 1e-2 and _rel(lse, torch.logsumexp(s, -1)) < 1e-5


def test_bad_shapes_are_refused():
    lib = _lib.load()
    t = torch.zeros(64, 1024, dtype=torch.bfloat16, device=dev)
    f = torch.zeros(4096 * 16, device=dev)
    p, fp = t.data_ptr(), f.data_ptr()
    s = ctypes.c_float(0.1)
    assert lib.nrv_cls_attn_fwd(p, 1024, p, 1024, p, 1024, p, 1024, p, 1024, p, 1024, fp, 2, 1, 4, 1032, s, None) == -2   # dh > 1024
    assert lib.nrv_cls_attn_fwd(p, 64, p, 64, p, 64, p, 64, p, 64, p, 64, fp, 2, 1, 4096, 60, s, None) == -2            # dh % 8
    assert lib.nrv_cls_attn_fwd(p, 64, p, 64, p, 64, p, 64, p, 64, p, 64, fp, 2, 1, 4096, 64, s, None) == -2            # Nk > 4096
    assert lib.nrv_cls_attn_bwd(p, 64, p, 64, p, 64, p, 64, p, 64, p, 64, fp, p, p, p, p, p, 2, 1, 4096, 64, s, None) == -2
    assert lib.nrv_cls_attn_fwd(p, 32, p, 64, p, 64, p, 64, p, 64, p, 64, fp, 2, 1, 4, 64, s, None) == -2               # ld < H dh
    assert lib.nrv_dwconv3x3_fwd(p, fp, fp, p, fp, 2, 4, 4, 12, None) == -2                                           # C % 8
    assert lib.nrv_dwconv3x3_bwd(p, fp, fp, p, fp, fp, p, _lib.NRV_U8, p, fp, fp, fp, 1 << 20, 1, 2, 2, 8, None) == -2   # q8: C % 64
    assert lib.nrv_se_fwd(fp, 16, fp, fp, fp, fp, fp, fp, 2, 8192, 16, None) == -2                                     # C > 4096
    assert lib.nrv_se_fwd(fp, 16, fp, fp, fp, fp, fp, fp, 2, 64, 2048, None) == -2                                     # rd > 1024
    assert lib.nrv_se_apply(p, fp, p, 2, 16, 12, None) == -2
    assert lib.nrv_ls_add_f32(fp, fp, fp, fp, ctypes.c_float(0.5), fp, 10, 3, 8, None) == -2                           # rows % per
    assert lib.nrv_ls_add_f32(fp, fp, fp, None, ctypes.c_float(1.0), fp, 10, 1, 6, None) == -2                         # C % 4
    assert lib.nrv_dgelu_rows(fp, p, _lib.NRV_U8, p, 4, 32, None) == -2                                                # q8: C % 64
    # refusals that return before any launch, each with real, correctly sized buffers
    u8 = lambda n: torch.zeros(max(int(n), 16), dtype=torch.uint8, device=dev)
    a, g = torch.zeros(5, 8, dtype=torch.bfloat16, device=dev), torch.zeros(4, 8, dtype=torch.bfloat16, device=dev)
    w, c8, c4 = torch.zeros(8, 9, device=dev), torch.zeros(8, device=dev), torch.zeros(4, 4, device=dev)
    need = lib.nrv_dwconv3x3_bwd_workspace(1, 2, 2, 8)
    ws = u8(need)
    dwb = lambda gs, gdt, nbytes: lib.nrv_dwconv3x3_bwd(a.data_ptr(), w.data_ptr(), c8.data_ptr(), g.data_ptr(), c8.data_ptr(), c8.data_ptr(), gs, gdt,
                                                        g.data_ptr(), w.data_ptr(), c8.data_ptr(), ws.data_ptr(), nbytes, 1, 2, 2, 8, None)
    assert need == 4 * 8 * 4 + 8 * 10 * 4 and dwb(None, _lib.NRV_BF16, need - 1) == -4            # workspace one byte short
    assert dwb(g.data_ptr(), _lib.NRV_F32, need) == -3                                             # stream dtype
    assert dwb(a.data_ptr() + 2, _lib.NRV_BF16, need) == -5                                        # stream pointer off by one bf16
    assert lib.nrv_dwconv3x3_fwd(a.data_ptr() + 2, w.data_ptr(), c8.data_ptr(), g.data_ptr(), c8.data_ptr(), 1, 2, 2, 8, None) == -5
    assert lib.nrv_dgelu_rows(fp, g.data_ptr(), _lib.NRV_F32, p, 4, 8, None) == -3
    assert lib.nrv_dgelu_rows(fp, g.data_ptr(), _lib.NRV_BF16, a.data_ptr() + 2, 4, 8, None) == -5
    need = lib.nrv_se_bwd_workspace(1, 8, 2)
    se = torch.zeros(2, 8, device=dev)
    assert need == (2 * 8 + 2) * 4 and lib.nrv_se_bwd(g.data_ptr(), g.data_ptr(), c8.data_ptr(), 1, c8.data_ptr(), c8.data_ptr(), se.data_ptr(),
                                                      se.data_ptr(), c8.data_ptr(), se.data_ptr(), c8.data_ptr(), se.data_ptr(), c8.data_ptr(),
                                                      u8(need).data_ptr(), need - 1, 1, 8, 2, None) == -4
    need = lib.nrv_ls_bwd_workspace(4, 4)
    assert need == 16 and lib.nrv_ls_bwd(c4.data_ptr(), c4.data_ptr(), c8.data_ptr(), None, ctypes.c_float(1.0), g.data_ptr(), c8.data_ptr(),
                                         u8(need).data_ptr(), need - 1, 4, 1, 4, None) == -4
    assert lib.nrv_cls_attn_fwd(p, 64, p, 64, None, 64, p, 64, p, 64, p, 64, fp, 2, 1, 4, 64, s, None) == -1           # kp NULL, Np > 0
    assert lib.nrv_cls_attn_bwd(p, 64, p, 64, p, 64, p, 64, None, 64, p, 64, fp, p, p, p, p, p, 2, 1, 4, 64, s, None) == -1
    assert lib.nrv_cls_attn_fwd(p, 68, p, 64, p, 64, p, 64, p, 64, p, 64, fp, 2, 1, 4, 64, s, None) == -2              # ld % 8
    assert lib.nrv_cls_attn_bwd(p, 64, p, 64, p, 64, p, 64, p, 64, p, 68, fp, p, p, p, p, p, 2, 1, 4, 64, s, None) == -2
    big = torch.zeros(65536, 8, dtype=torch.bfloat16, device=dev)                                                       # B > 65535
    bigsq = torch.zeros(65536, 8, device=dev)
    assert lib.nrv_dwconv3x3_fwd(big.data_ptr(), w.data_ptr(), c8.data_ptr(), big.data_ptr(), bigsq.data_ptr(), 65536, 1, 1, 8, None) == -2
