"""GPU: the talking-heads kernels (csrc/nrv_talking_heads.hip) against a float64 torch evaluation of their formulas.

    T[b,g] = sum_h W1[h,g] S[b,h]     P = softmax(T, -1)     A[b,g] = sum_h W2[h,g] P[b,h]                  (cait.py:107-116)
    dP = W2-mix of dA,  dT = P (dP - <P, dP>),  dS = W1-mix of dT,  dW2 = sum P dA,  dW1 = sum S dT

Bound (not tuned on the kernels): the same formulas are evaluated with torch in fp32 on the same inputs; a kernel's max-norm
relative error against float64 may be at most 4 x that fp32 evaluation's (another summation order over <= 16 heads and <= 1025
keys), with a floor of 8 * 2^-23 for the cases torch evaluates exactly (H = 1, identity mixing), plus 2^-8 on an output the
kernel stores as bf16.  Both errors are printed per case."""
import ctypes

import pytest
import torch

from noise_robust_vit_amd import _lib
from noise_robust_vit_amd import kernels as K

pytestmark = pytest.mark.gpu

HEADS = (1, 2, 4, 8, 16)
SHAPES = ((1, 17), (1, 197), (16, 16), (196, 196), (197, 197), (577, 577), (1, 1025))
FLOOR = 8 * 2.0 ** -23
BF16 = 2.0 ** -8


def _err(a, ref):
    ref = ref.double()
    return float((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _check(name, got, f32, f64, bf16=False):
    e_k, e_t = _err(got, f64), _err(f32, f64)
    bound = max(4 * e_t, FLOOR) + (BF16 if bf16 else 0.0)
    print(f"{name}: kernel {e_k:.3e}  torch fp32 {e_t:.3e}  bound {bound:.3e}")
    assert e_k <= bound, (name, e_k, e_t, bound)


def _inputs(B, H, Nq, Nk, dev, seed=0, identity=False):
    g = torch.Generator().manual_seed(1000 * seed + 100 * H + Nq + Nk)
    S = (1.5 * torch.randn(B, H, Nq, Nk, generator=g)).to(dev)
    dA = torch.randn(B, H, Nq, Nk, generator=g).to(dev)
    if identity:
        W1 = W2 = torch.eye(H, device=dev)
    else:
        W1 = (torch.randn(H, H, generator=g) / H ** 0.5).to(dev)
        W2 = (torch.randn(H, H, generator=g) / H ** 0.5).to(dev)
    return S, dA, W1.contiguous(), W2.contiguous()


def _mix(x, W):
    return torch.einsum("bhij,hg->bgij", x, W)


def _mix_t(d, W):
    return torch.einsum("bgij,hg->bhij", d, W)


def _fwd(S, W1, W2):
    P = torch.softmax(_mix(S, W1), dim=-1)
    return P, _mix(P, W2)


def _bwd(dA, P, S, W1, W2):
    dP = _mix_t(dA, W2)
    dT = P * (dP - (P * dP).sum(-1, keepdim=True))
    return _mix_t(dT, W1), torch.einsum("bhij,bgij->hg", S, dT), torch.einsum("bhij,bgij->hg", P, dA)


def _batch(H, Nq, Nk):
    return 3 if H * Nq * Nk <= 1 << 20 else 1


@pytest.mark.parametrize("Nq,Nk", SHAPES)
@pytest.mark.parametrize("H", HEADS)
def test_th_softmax_against_float64(dev, H, Nq, Nk):
    B = _batch(H, Nq, Nk)
    S, dA, W1, W2 = _inputs(B, H, Nq, Nk, dev)
    tag = f"th_softmax H={H} {Nq}x{Nk}"
    P64, A64 = _fwd(S.double(), W1.double(), W2.double())
    P32, A32 = _fwd(S, W1, W2)
    P, A = K.th_softmax_fwd(S, W1, W2, a_dtype=torch.float32)
    _check(tag + " P", P, P32, P64)
    _check(tag + " A", A, A32, A64)
    P16, A16 = K.th_softmax_fwd(S, W1, W2, a_dtype=torch.bfloat16)
    assert torch.equal(P16, P)
    _check(tag + " A(bf16)", A16, A32, A64, bf16=True)
    # the backward takes P as an input: all three evaluations read the kernel's own P
    r64 = _bwd(dA.double(), P.double(), S.double(), W1.double(), W2.double())
    r32 = _bwd(dA, P, S, W1, W2)
    got = K.th_softmax_bwd(dA, P, S, W1, W2)
    for n, a, b, c in zip(("dS", "dW1", "dW2"), got, r32, r64):
        _check(f"{tag} {n}", a, b, c)
    again = K.th_softmax_bwd(dA, P, S, W1, W2)
    P2, A2 = K.th_softmax_fwd(S, W1, W2, a_dtype=torch.float32)
    assert torch.equal(P2, P) and torch.equal(A2, A) and all(torch.equal(u, v) for u, v in zip(got, again))


@pytest.mark.parametrize("Nq,Nk", SHAPES)
@pytest.mark.parametrize("H", HEADS)
def test_head_mix_against_float64(dev, H, Nq, Nk):
    B = _batch(H, Nq, Nk)
    x, dout, W, _ = _inputs(B, H, Nq, Nk, dev, seed=1)
    tag = f"head_mix H={H} {Nq}x{Nk}"
    o64, o32 = _mix(x.double(), W.double()), _mix(x, W)
    out = K.head_mix_fwd(x, W)
    _check(tag + " out", out, o32, o64)
    _check(tag + " out(bf16)", K.head_mix_fwd(x, W, out_dtype=torch.bfloat16), o32, o64, bf16=True)
    din, dW = K.head_mix_bwd(dout, x, W)
    _check(tag + " din", din, _mix_t(dout, W), _mix_t(dout.double(), W.double()))
    _check(tag + " dW", dW, torch.einsum("bhij,bgij->hg", x, dout), torch.einsum("bhij,bgij->hg", x.double(), dout.double()))
    din2, dW2 = K.head_mix_bwd(dout, x, W)
    assert torch.equal(out, K.head_mix_fwd(x, W)) and torch.equal(din, din2) and torch.equal(dW, dW2)


@pytest.mark.parametrize("H,Nq,Nk", [(1, 16, 16), (4, 197, 197), (16, 1, 1025)])
def test_identity_mixing_is_plain_softmax(dev, H, Nq, Nk):
    S, dA, W1, W2 = _inputs(2, H, Nq, Nk, dev, seed=2, identity=True)
    P, A = K.th_softmax_fwd(S, W1, W2, a_dtype=torch.float32)
    ref = torch.softmax(S.double(), dim=-1)
    tag = f"identity H={H} {Nq}x{Nk}"
    _check(tag + " P", P, torch.softmax(S, dim=-1), ref)
    assert torch.equal(A, P)                                # 1 * p + 0 * the others, exactly
    dS, _, _ = K.th_softmax_bwd(dA, P, S, W1, W2)
    Pd = P.double()
    d64 = Pd * (dA.double() - (Pd * dA.double()).sum(-1, keepdim=True))
    d32 = P * (dA - (P * dA).sum(-1, keepdim=True))
    _check(tag + " dS", dS, d32, d64)
    assert torch.equal(K.head_mix_fwd(S, W1), S)


def test_shapes_outside_the_range_are_refused_without_a_launch(dev):
    lib = _lib.load()
    buf = torch.zeros(64, device=dev)
    p = buf.data_ptr()
    for H, Nk in ((17, 16), (4, 1026), (0, 16), (4, 0)):
        assert lib.nrv_th_softmax_fwd(p, p, p, p, p, 0, 1, H, 1, Nk, None) == -2
        assert lib.nrv_th_softmax_bwd(p, p, p, p, p, p, p, p, p, ctypes.c_size_t(1 << 30), 1, H, 1, Nk, None) == -2
        assert lib.nrv_head_mix_fwd(p, p, p, 0, 1, H, 1, Nk, None) == -2
        assert lib.nrv_head_mix_bwd(p, p, p, p, p, p, ctypes.c_size_t(1 << 30), 1, H, 1, Nk, None) == -2
    with pytest.raises(NotImplementedError):
        K.th_softmax_fwd(torch.zeros(1, 17, 1, 8, device=dev), torch.eye(17, device=dev), torch.eye(17, device=dev))
    with pytest.raises(NotImplementedError):
        K.head_mix_fwd(torch.zeros(1, 2, 1, 1026, device=dev), torch.eye(2, device=dev))
    assert lib.nrv_th_softmax_bwd(p, p, p, p, p, p, p, p, p, ctypes.c_size_t(8), 4, 4, 16, 16, None) == -4      # workspace
