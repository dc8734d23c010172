"""fp32 PyTorch restatement of LeViT's forward (levit.py:57-528) -- the oracle of the GPU tests.

Written from the reference's equations, not copied: it walks a noise_robust_vit_amd.levit.LeViT for the structure and the
weights and computes everything with torch.nn.functional on fp32 copies (conv2d, batch_norm in the module's mode, the offset
bias gathered from attention_bias_idxs, softmax or Sinkhorn, Hardswish, drop-path with given keep masks).

    logits, loss, grads, buffers = levit_loss_and_grads(model, x, y, keeps=None, bf16_operands=False)

bf16_operands=True rounds every matrix-product and convolution operand to bf16 (what the HIP path feeds its GEMMs and attention
kernels) and computes the rest in fp32: the emulation the GPU tests use to attribute the model-level error to bf16 rounding.

grads: name -> fp32 gradient of every parameter; buffers: name -> the running statistics after the forward (updated in training).
keeps: list of fp32 [B] keep masks, one per Residual in forward order (drop-path), or None.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from noise_robust_vit_amd import levit as L


def _bn(h, P, Bf, pre, training, momentum, eps):
    return F.batch_norm(h, Bf[pre + ".running_mean"], Bf[pre + ".running_var"], P[pre + ".weight"], P[pre + ".bias"],
                        training, momentum, eps)


_ROUND = [False]


def _r(t):
    return t.to(torch.bfloat16).to(t.dtype) if _ROUND[0] else t


def _attend(q, k, v, bias, scale, robust):
    """q [B, H, Nq, kd], k [B, H, Nk, kd], v [B, H, Nk, d], bias [H, Nq, Nk] -> [B, H, Nq, d]."""
    q, k, v = _r(q), _r(k), _r(v)
    s = torch.einsum("bhid,bhjd->bhij", q, k) * scale + bias
    p = torch.softmax(s, dim=-1)
    if robust:
        for _ in range(3):
            p = p / p.sum(-1, keepdim=True)
            p = p / p.sum(-2, keepdim=True)
        p = p / p.sum(-1, keepdim=True)
    return torch.einsum("bhij,bhjd->bhid", p, v)


def levit_forward(model: L.LeViT, P: dict, Bf: dict, x: torch.Tensor, keeps=None):
    training = model.training
    names = {id(m): n for n, m in model.named_modules()}

    def lin_bn(t, lbn):
        pre = names[id(lbn)]
        y = _r(t) @ _r(P[pre + ".c.weight"]).t()
        shp = y.shape
        z = _bn(y.reshape(-1, shp[-1]), P, Bf, pre + ".bn", lbn.bn.training, lbn.bn.momentum, lbn.bn.eps)
        if lbn.bn.training:
            Bf[pre + ".bn.num_batches_tracked"] += 1
        return z.reshape(shp)

    h = x
    convs = model._convs
    for i, cbn in enumerate(convs):
        pre = names[id(cbn)]
        h = F.conv2d(_r(h), _r(P[pre + ".c.weight"]), stride=2, padding=1)
        h = _bn(h, P, Bf, pre + ".bn", cbn.bn.training, cbn.bn.momentum, cbn.bn.eps)
        if cbn.bn.training:
            Bf[pre + ".bn.num_batches_tracked"] += 1
        if i < len(convs) - 1:
            h = F.hardswish(h)
    B = h.shape[0]
    t = h.flatten(2).transpose(1, 2)
    r = h.shape[-1]
    ki = 0
    for blk in model.blocks:
        if isinstance(blk, L.AttentionSubsample):
            a = blk
            pre = names[id(a)]
            H, kd, d, s = a.num_heads, a.key_dim, a.d, a.stride
            kv = lin_bn(t, a.kv).view(B, r * r, H, kd + d)
            k, v = kv[..., :kd].permute(0, 2, 1, 3), kv[..., kd:].permute(0, 2, 1, 3)
            ts = t.view(B, r, r, -1)[:, ::s, ::s].reshape(B, -1, t.shape[-1])
            q = lin_bn(ts, a.q[1]).view(B, -1, H, kd).permute(0, 2, 1, 3)
            bias = P[pre + ".attention_biases"][:, Bf[pre + ".attention_bias_idxs"]]
            o = _attend(q, k, v, bias, kd ** -0.5, a.robust).transpose(1, 2).reshape(B, -1, H * d)
            t = lin_bn(F.hardswish(o), a.proj[1])
            r = a.resolution_
            continue
        m = blk.m
        if isinstance(m, L.Attention):
            pre = names[id(m)]
            H, kd, d = m.num_heads, m.key_dim, m.d
            qkv = lin_bn(t, m.qkv).view(B, r * r, H, 2 * kd + d)
            q, k, v = (qkv[..., :kd].permute(0, 2, 1, 3), qkv[..., kd:2 * kd].permute(0, 2, 1, 3),
                       qkv[..., 2 * kd:].permute(0, 2, 1, 3))
            bias = P[pre + ".attention_biases"][:, Bf[pre + ".attention_bias_idxs"]]
            o = _attend(q, k, v, bias, kd ** -0.5, m.robust).transpose(1, 2).reshape(B, -1, H * d)
            y = lin_bn(F.hardswish(o), m.proj[1])
        else:
            y = lin_bn(F.hardswish(lin_bn(t, m[0])), m[2])
        if training and blk.drop > 0:
            keep = keeps[ki]
            y = y * (keep.to(y.dtype).view(B, 1, 1) / (1 - blk.drop))
        ki += 1
        t = t + y
    pooled = t.mean(1)
    hp = names[id(model.head)]
    z = _bn(pooled, P, Bf, hp + ".bn", model.head.bn.training, model.head.bn.momentum, model.head.bn.eps)
    if model.head.bn.training:
        Bf[hp + ".bn.num_batches_tracked"] += 1
    return z @ P[hp + ".l.weight"].t() + P[hp + ".l.bias"]


def levit_loss_and_grads(model: L.LeViT, x: torch.Tensor, y: torch.Tensor, keeps=None, device=None, bf16_operands=False):
    device = device or x.device
    P = {n: p.detach().to(device=device, dtype=torch.float32).clone().requires_grad_(True) for n, p in model.named_parameters()}
    Bf = {n: b.detach().to(device).clone() for n, b in model.named_buffers()}
    _ROUND[0] = bf16_operands
    try:
        logits = levit_forward(model, P, Bf, x.to(device, torch.float32), keeps)
    finally:
        _ROUND[0] = False
    loss = F.cross_entropy(logits, y.to(device), label_smoothing=0.1)
    names = list(P)
    gs = torch.autograd.grad(loss, [P[n] for n in names], allow_unused=True)
    grads = {n: (torch.zeros_like(P[n]) if g is None else g) for n, g in zip(names, gs)}
    return logits.detach(), loss.detach(), grads, Bf
