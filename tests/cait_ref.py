"""fp32 PyTorch restatement of CaiT's forward (cait.py:95-232) -- the oracle of the GPU tests.

Written from the reference's equations: it walks a noise_robust_vit_amd.cait.CaiT for the structure and the weights and computes
everything with torch on fp32 copies (patch rearrangement, LayerScale, talking-heads attention with softmax or Sinkhorn, class
attention on cat(LN(cls), patches)).

    logits, loss, grads = cait_loss_and_grads(model, x, y, kept=None, bf16_operands=False)

bf16_operands=True rounds every matrix-product operand to bf16 -- the Linear layers' inputs and weights, q, k, v and the mixed
attention weights that meet v (what the HIP path feeds its GEMMs and nrv_bgemm) -- and computes the rest in fp32: the emulation
the GPU tests use to size their bounds.
kept: (patch layer indices, class layer indices) that survive layer dropout, or None for all.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

_ROUND = [False]


def _r(t):
    return t.to(torch.bfloat16).to(t.dtype) if _ROUND[0] else t


def _lin(x, w, b=None):
    return F.linear(_r(x), _r(w), b)


def sinkhorn(p, iters=3):
    for _ in range(iters):
        p = p / p.sum(-1, keepdim=True)
        p = p / p.sum(-2, keepdim=True)
    return p / p.sum(-1, keepdim=True)


def _layer(P, p, x, context, heads, scale, robust, eps):
    """x + scale_a attn(LN x, context), then + scale_f ff(LN .); p = the layer's key prefix."""
    D = x.shape[-1]
    a = p + "0.fn.fn."
    xn = F.layer_norm(x, (D,), P[p + "0.fn.norm.weight"], P[p + "0.fn.norm.bias"], eps[0])
    kv_in = xn if context is None else torch.cat((xn, context), dim=1)
    B, n, _ = xn.shape
    q = _lin(xn, P[a + "to_q.weight"])
    k, v = _lin(kv_in, P[a + "to_kv.weight"]).chunk(2, dim=-1)
    q, k, v = (t.reshape(B, t.shape[1], heads, -1).permute(0, 2, 1, 3) for t in (q, k, v))
    dots = torch.einsum("bhid,bhjd->bhij", _r(q), _r(k)) * scale
    dots = torch.einsum("bhij,hg->bgij", dots, P[a + "mix_heads_pre_attn"])
    attn = torch.softmax(dots, dim=-1)
    if robust:
        attn = sinkhorn(attn)
    attn = torch.einsum("bhij,hg->bgij", attn, P[a + "mix_heads_post_attn"])
    o = torch.einsum("bhij,bhjd->bhid", _r(attn), _r(v)).permute(0, 2, 1, 3).reshape(B, n, -1)
    x = x + P[p + "0.scale"] * _lin(o, P[a + "to_out.0.weight"], P[a + "to_out.0.bias"])
    f = p + "1.fn.fn.net."
    h = F.layer_norm(x, (D,), P[p + "1.fn.norm.weight"], P[p + "1.fn.norm.bias"], eps[1])
    h = _lin(F.gelu(_lin(h, P[f + "0.weight"], P[f + "0.bias"])), P[f + "3.weight"], P[f + "3.bias"])
    return x + P[p + "1.scale"] * h


def _transformer(model_t, P, prefix, x, context, kept):
    for i, (attn, ff) in enumerate(model_t.layers):
        if kept is not None and i not in kept:
            continue
        a = attn.fn.fn
        x = _layer(P, f"{prefix}.layers.{i}.", x, context, a.heads, a.scale, a.robust, (attn.fn.norm.eps, ff.fn.norm.eps))
    return x


def forward(model, P, img, kept=None):
    B, C, Hh, Ww = img.shape
    p = model.patch_size
    h, w = Hh // p, Ww // p
    x = img.reshape(B, C, h, p, w, p).permute(0, 2, 4, 3, 5, 1).reshape(B, h * w, p * p * C)     # b (h w) (p1 p2 c)
    x = _lin(x, P["to_patch_embedding.1.weight"], P["to_patch_embedding.1.bias"])
    x = x + P["pos_embedding"][:, :h * w]
    x = _transformer(model.patch_transformer, P, "patch_transformer", x, None, kept[0] if kept else None)
    cls = P["cls_token"].expand(B, -1, -1)
    cls = _transformer(model.cls_transformer, P, "cls_transformer", cls, x, kept[1] if kept else None)
    D = cls.shape[-1]
    f = F.layer_norm(cls[:, 0], (D,), P["mlp_head.0.weight"], P["mlp_head.0.bias"], model.mlp_head[0].eps)
    return F.linear(f, P["mlp_head.1.weight"], P["mlp_head.1.bias"])


def cait_loss_and_grads(model, x, y, kept=None, bf16_operands=False):
    P = {k: v.detach().float().clone().requires_grad_(True) for k, v in model.named_parameters()}
    _ROUND[0] = bf16_operands
    try:
        logits = forward(model, P, x.float(), kept)
        loss = F.cross_entropy(logits, y)
        grads = torch.autograd.grad(loss, list(P.values()), allow_unused=True)
    finally:
        _ROUND[0] = False
    return logits.detach(), loss.detach(), {k: (g if g is not None else torch.zeros_like(P[k])) for k, g in zip(P, grads)}
