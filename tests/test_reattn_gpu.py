"""GPU: the re-attention kernels (csrc/nrv_reattn.hip) against a float64 torch evaluation of their formulas.

    P = softmax(S, -1)     M[b,g] = sum_h W[h,g] P[b,h]     x^ = (M - mean_g M) rsqrt(var_g M + eps)     A = x^ gamma + beta
    dbeta = sum dA,  dgamma = sum dA x^,  dx^ = dA gamma,  dM = rstd (dx^ - mean_g dx^ - x^ mean_g (dx^ x^)),
    dW = sum P dM,  dP = W-mix^T of dM,  dS = P (dP - <P, dP>)                                        (deepvit.py:47-53, 67-74)

Bound (the talking-heads test's, not tuned on these kernels): the same formulas are evaluated with torch in fp32 on the same
inputs; a kernel's max-norm relative error against float64 may be at most 4 x that fp32 evaluation's, with a floor of 8 * 2^-23,
plus 2^-8 on an output the kernel stores as bf16.  Both errors are printed per case.  rstd can reach 1 / sqrt(eps) = 316, which
would amplify the softmax's own rounding into the comparison: P is checked against the float64 softmax of S, and then all three
evaluations of A and of the backward read the kernel's own P."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from noise_robust_vit_amd import _lib
from noise_robust_vit_amd import kernels as K

pytestmark = pytest.mark.gpu

HEADS = (1, 2, 3, 4, 8, 12, 16)
SHAPES = ((1, 17), (16, 16), (197, 197), (196, 196), (1, 1024), (1, 1025))
FLOOR = 8 * 2.0 ** -23
BF16 = 2.0 ** -8
EPS = 1e-5


def _err(a, ref):
    ref = ref.double()
    return float((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _check(name, got, f32, f64, bf16=False):
    assert bool(torch.isfinite(got.float()).all()), name
    e_k, e_t = _err(got, f64), _err(f32, f64)
    bound = max(4 * e_t, FLOOR) + (BF16 if bf16 else 0.0)
    print(f"{name}: kernel {e_k:.3e}  torch fp32 {e_t:.3e}  bound {bound:.3e}")
    assert e_k <= bound, (name, e_k, e_t, bound)


def _inputs(B, H, Nq, Nk, dev, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 100 * H + Nq + Nk)
    S = (1.5 * torch.randn(B, H, Nq, Nk, generator=g)).to(dev)
    dA = torch.randn(B, H, Nq, Nk, generator=g).to(dev)
    W = (torch.randn(H, H, generator=g) / H ** 0.5).to(dev).contiguous()
    gamma = (1.0 + 0.5 * torch.randn(H, generator=g)).to(dev)
    beta = (0.5 * torch.randn(H, generator=g)).to(dev)
    return S, dA, W, gamma, beta


def _hv(v):
    return v.view(1, -1, 1, 1)


def _xhat(P, W, eps):
    M = torch.einsum("bhij,hg->bgij", P, W)
    d = M - M.mean(1, keepdim=True)
    rstd = torch.rsqrt((d * d).mean(1, keepdim=True) + eps)
    return d * rstd, rstd


def _fwd(P, W, gamma, beta, eps=EPS):
    return _xhat(P, W, eps)[0] * _hv(gamma) + _hv(beta)


def _bwd(dA, P, W, gamma, eps=EPS, softmax=True):
    """(dS or dP, dW, dgamma, dbeta) by the formulas of the module docstring"""
    xh, rstd = _xhat(P, W, eps)
    dxh = dA * _hv(gamma)
    dM = rstd * (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True))
    dP = torch.einsum("bgij,hg->bhij", dM, W)
    d = P * (dP - (P * dP).sum(-1, keepdim=True)) if softmax else dP
    return d, torch.einsum("bhij,bgij->hg", P, dM), (dA * xh).sum((0, 2, 3)), dA.sum((0, 2, 3))


def _d(*ts):
    return tuple(t.double() for t in ts)


def _fused(tag, S, dA, W, gamma, beta):
    """the fused pair on one set of inputs; returns what the kernels gave"""
    H = S.shape[1]
    P, A = K.reattn_softmax_fwd(S, W, gamma, beta, EPS, a_dtype=torch.float32)
    _check(tag + " P", P, torch.softmax(S, -1), torch.softmax(S.double(), -1))
    A64, A32 = _fwd(*_d(P, W, gamma, beta)), _fwd(P, W, gamma, beta)
    _check(tag + " A", A, A32, A64)
    P16, A16 = K.reattn_softmax_fwd(S, W, gamma, beta, EPS, a_dtype=torch.bfloat16)
    assert torch.equal(P16, P)
    _check(tag + " A(bf16)", A16, A32, A64, bf16=True)
    got = K.reattn_softmax_bwd(dA, P, W, gamma, EPS)
    if H > 1:
        r64, r32 = _bwd(*_d(dA, P, W, gamma)), _bwd(dA, P, W, gamma)
        for n, a, b, c in zip(("dS", "dW", "dgamma", "dbeta"), got, r32, r64):
            _check(f"{tag} {n}", a, b, c)
    again = K.reattn_softmax_bwd(dA, P, W, gamma, EPS)
    P2, A2 = K.reattn_softmax_fwd(S, W, gamma, beta, EPS, a_dtype=torch.float32)
    assert torch.equal(P2, P) and torch.equal(A2, A) and all(torch.equal(u, v) for u, v in zip(got, again))
    return P, A, got


def _flat(tag, P, dA, W, gamma, beta):
    H = P.shape[1]
    A = K.reattn_norm_fwd(P, W, gamma, beta, EPS, a_dtype=torch.float32)
    A64, A32 = _fwd(*_d(P, W, gamma, beta)), _fwd(P, W, gamma, beta)
    _check(tag + " A", A, A32, A64)
    _check(tag + " A(bf16)", K.reattn_norm_fwd(P, W, gamma, beta, EPS), A32, A64, bf16=True)
    got = K.reattn_norm_bwd(dA, P, W, gamma, EPS)
    if H > 1:
        r64, r32 = _bwd(*_d(dA, P, W, gamma), softmax=False), _bwd(dA, P, W, gamma, softmax=False)
        for n, a, b, c in zip(("dP", "dW", "dgamma", "dbeta"), got, r32, r64):
            _check(f"{tag} {n}", a, b, c)
    again = K.reattn_norm_bwd(dA, P, W, gamma, EPS)
    assert torch.equal(A, K.reattn_norm_fwd(P, W, gamma, beta, EPS, a_dtype=torch.float32))
    assert all(torch.equal(u, v) for u, v in zip(got, again))
    return A, got


def _one_head(A, got, dA, beta):
    """H = 1: the LayerNorm over one head leaves beta, and nothing but dbeta has a gradient"""
    d, dW, dg, db = got
    assert torch.equal(A, beta.view(1, 1, 1, 1).expand_as(A))
    assert not d.any() and not dW.any() and not dg.any()
    ref = dA.double().sum()
    assert abs(float(db[0]) - float(ref)) <= FLOOR * float(dA.double().abs().sum())


@pytest.mark.parametrize("Nq,Nk", SHAPES)
@pytest.mark.parametrize("H", HEADS)
def test_reattn_softmax_against_float64(dev, H, Nq, Nk):
    B = 3 if Nq > 1 else 2
    S, dA, W, gamma, beta = _inputs(B, H, Nq, Nk, dev)
    _, A, got = _fused(f"reattn_softmax H={H} {Nq}x{Nk}", S, dA, W, gamma, beta)
    if H == 1:
        _one_head(A, got, dA, beta)


@pytest.mark.parametrize("Nq,Nk", SHAPES)
@pytest.mark.parametrize("H", HEADS)
def test_reattn_norm_against_float64(dev, H, Nq, Nk):
    B = 3 if Nq > 1 else 2
    S, dA, W, gamma, beta = _inputs(B, H, Nq, Nk, dev, seed=1)
    P = torch.softmax(S, -1)
    A, got = _flat(f"reattn_norm H={H} {Nq}x{Nk}", P, dA, W, gamma, beta)
    if H == 1:
        _one_head(A, got, dA, beta)


def test_fused_backward_walks_rows(dev):
    """B * Nq = 1055 > 1024 workgroups: 31 of them own two rows"""
    _fused("row walk 5x4x211x17", *_inputs(5, 4, 211, 17, dev, seed=2))


def test_flat_backward_walks_tiles(dev):
    """5 * ceil(211 * 500 / 512) = 1035 > 1024 tiles"""
    S, dA, W, gamma, beta = _inputs(5, 4, 211, 500, dev, seed=3)
    _flat("tile walk 5x4x211x500", torch.softmax(S, -1), dA, W, gamma, beta)


@pytest.mark.parametrize("H,Nq,Nk", [(3, 16, 16), (4, 197, 197), (16, 1, 1025)])
def test_identity_mixing_is_layernorm_over_heads(dev, H, Nq, Nk):
    S, dA, _, _, _ = _inputs(2, H, Nq, Nk, dev, seed=4)
    W, gamma, beta = torch.eye(H, device=dev), torch.ones(H, device=dev), torch.zeros(H, device=dev)
    P, A = K.reattn_softmax_fwd(S, W, gamma, beta, EPS, a_dtype=torch.float32)

    def ln(p):
        return F.layer_norm(p.permute(0, 2, 3, 1), (H,), eps=EPS).permute(0, 3, 1, 2)

    tag = f"identity H={H} {Nq}x{Nk}"
    _check(tag + " fused A", A, ln(P), ln(P.double()))
    _check(tag + " flat A", K.reattn_norm_fwd(P, W, gamma, beta, EPS, a_dtype=torch.float32), ln(P), ln(P.double()))


@pytest.mark.parametrize("Nk", (17, 196))
def test_one_hot_rows_stay_finite(dev, Nk):
    """every key but one lies 120 nats below it: P is one-hot, and where all heads are zero var = 0, rstd = 1 / sqrt(eps), A = beta"""
    B, H, Nq = 2, 4, 5
    _, dA, W, gamma, beta = _inputs(B, H, Nq, Nk, dev, seed=5)
    hot = torch.randint(0, Nk, (B, H, Nq, 1), generator=torch.Generator().manual_seed(Nk)).to(dev)
    S = torch.full((B, H, Nq, Nk), -120.0, device=dev).scatter_(-1, hot, 0.0)
    P, A, _ = _fused(f"one-hot {Nk}", S, dA, W, gamma, beta)
    assert torch.equal(P, torch.zeros_like(P).scatter_(-1, hot, 1.0))
    cold = (P.sum(1, keepdim=True) == 0).expand_as(A)
    assert bool(cold.any()) and torch.equal(A[cold], _hv(beta).expand_as(A)[cold])
    _flat(f"one-hot flat {Nk}", P, dA, W, gamma, beta)


def test_shapes_outside_the_range_are_refused_without_a_launch(dev):
    lib = _lib.load()
    buf = torch.zeros(64, device=dev)
    p, big, eps = buf.data_ptr(), ctypes.c_size_t(1 << 30), ctypes.c_float(EPS)
    for H, Nk, e in ((17, 16, eps), (4, 1026, eps), (0, 16, eps), (4, 0, eps), (4, 16, ctypes.c_float(0.0))):
        assert lib.nrv_reattn_softmax_fwd(p, p, p, p, p, p, 0, 1, H, 1, Nk, e, None) == -2
        assert lib.nrv_reattn_softmax_bwd(p, p, p, p, p, p, p, p, p, big, 1, H, 1, Nk, e, None) == -2
        assert lib.nrv_reattn_norm_fwd(p, p, p, p, p, 0, 1, H, 1, Nk, e, None) == -2
        assert lib.nrv_reattn_norm_bwd(p, p, p, p, p, p, p, p, p, big, 1, H, 1, Nk, e, None) == -2
    with pytest.raises(NotImplementedError):
        K.reattn_softmax_fwd(torch.zeros(1, 17, 1, 8, device=dev), torch.eye(17, device=dev), torch.ones(17, device=dev),
                             torch.zeros(17, device=dev), EPS)
    with pytest.raises(NotImplementedError):
        K.reattn_norm_fwd(torch.zeros(1, 2, 1, 1026, device=dev), torch.eye(2, device=dev), torch.ones(2, device=dev),
                          torch.zeros(2, device=dev), EPS)
    with pytest.raises(_lib.NrvError):
        K.reattn_norm_fwd(torch.zeros(1, 2, 4, 8, device=dev).transpose(2, 3), torch.eye(2, device=dev), torch.ones(2, device=dev),
                          torch.zeros(2, device=dev), EPS)
    assert lib.nrv_reattn_softmax_bwd(p, p, p, p, p, p, p, p, p, ctypes.c_size_t(8), 4, 4, 16, 16, eps, None) == -4
    assert lib.nrv_reattn_norm_bwd(p, p, p, p, p, p, p, p, p, ctypes.c_size_t(8), 4, 4, 16, 16, eps, None) == -4
