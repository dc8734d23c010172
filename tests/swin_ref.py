"""fp32 restatement of the Swin Transformer forward (V1), written from the semantics, on a state_dict.

Used as the oracle of the GPU tests at sizes the reference fixture does not cover (full swin_t at 224 px), and checked
against that fixture on CPU.  Differentiable: gradients come from torch autograd.  `keeps` (optional) maps a block name
"features.<s>.<i>" to its two per-sample stochastic-depth keep vectors (attention branch, MLP branch) and `sd_probs` to p.
"""
import math

import torch
import torch.nn.functional as F


def _region(pos: torch.Tensor, extent: int, ws: int, s: int) -> torch.Tensor:
    """Shift region along one axis of the rolled map: 0 before extent - ws, 1 before extent - s, else 2; constant when s = 0."""
    if s == 0:
        return torch.full_like(pos, 2)
    return torch.where(pos < extent - ws, 0, torch.where(pos < extent - s, 1, 2))


def effective_geometry(H: int, W: int, window, shift):
    Wh, Ww = window
    pH, pW = math.ceil(H / Wh) * Wh, math.ceil(W / Ww) * Ww
    return pH, pW, (0 if Wh >= pH else shift[0]), (0 if Ww >= pW else shift[1])


def window_core(qkv, table, heads: int, window, shift, robust: bool):
    """qkv [B, pH, pW, 3C] of the padded map, (sh, sw) the effective shift -> attention output [B, pH, pW, C] (before proj)."""
    B, pH, pW, C3 = qkv.shape
    C = C3 // 3
    Wh, Ww = window
    sh, sw = shift
    # slot (i, j) of window (wy, wx) reads rolled position (wy*Wh + i, wx*Ww + j) = original ((.. + sh) % pH, (.. + sw) % pW)
    ry, rx = torch.arange(pH, device=qkv.device), torch.arange(pW, device=qkv.device)
    xr = qkv[:, (ry + sh) % pH][:, :, (rx + sw) % pW]
    nWy, nWx = pH // Wh, pW // Ww
    N = Wh * Ww
    dh = C // heads
    win = xr.reshape(B, nWy, Wh, nWx, Ww, C3).permute(0, 1, 3, 2, 4, 5).reshape(-1, N, 3, heads, dh).permute(2, 0, 3, 1, 4)
    q, k, v = win[0] * dh ** -0.5, win[1], win[2]
    s = q @ k.transpose(-2, -1)
    n = torch.arange(N, device=qkv.device)
    cy, cx = n // Ww, n % Ww
    rel = (cy[:, None] - cy[None, :] + Wh - 1) * (2 * Ww - 1) + (cx[:, None] - cx[None, :] + Ww - 1)
    s = s + table[rel].permute(2, 0, 1)[None]
    if sh + sw > 0:
        gy = torch.arange(nWy, device=qkv.device)[:, None] * Wh + cy[None, :]       # rolled row / column of every slot
        gx = torch.arange(nWx, device=qkv.device)[:, None] * Ww + cx[None, :]
        reg = (_region(gy, pH, Wh, sh)[:, None, :] * 3 + _region(gx, pW, Ww, sw)[None, :, :]).reshape(nWy * nWx, N)
        mask = torch.where(reg[:, :, None] != reg[:, None, :], -100.0, 0.0).to(s.dtype)
        s = (s.reshape(B, nWy * nWx, heads, N, N) + mask[None, :, None]).reshape(-1, heads, N, N)
    p = torch.softmax(s, dim=-1)
    if robust:
        for _ in range(3):
            p = p / p.sum(-1, keepdim=True)
            p = p / p.sum(-2, keepdim=True)
        p = p / p.sum(-1, keepdim=True)
    o = (p @ v).transpose(1, 2).reshape(B, nWy, nWx, Wh, Ww, C).permute(0, 1, 3, 2, 4, 5).reshape(B, pH, pW, C)
    return o[:, (ry - sh) % pH][:, :, (rx - sw) % pW]                          # inverse of the roll


def window_attention(x, wqkv, bqkv, wo, bo, table, heads: int, window, shift, robust: bool):
    """x [B, H, W, C] (already normalised) -> [B, H, W, C]: zero pad, qkv, window attention, proj, crop."""
    B, H, W, C = x.shape
    pH, pW, sh, sw = effective_geometry(H, W, window, shift)
    xp = x.new_zeros(B, pH, pW, C)
    xp[:, :H, :W] = x
    o = window_core(F.linear(xp, wqkv, bqkv), table, heads, window, (sh, sw), robust)
    return F.linear(o, wo, bo)[:, :H, :W]


def patch_merge(x, ln_w, ln_b, w, eps: float):
    B, H, W, C = x.shape
    xp = x.new_zeros(B, H + H % 2, W + W % 2, C)
    xp[:, :H, :W] = x
    parts = [xp[:, dy::2, dx::2] for dy, dx in ((0, 0), (1, 0), (0, 1), (1, 1))]
    return F.linear(F.layer_norm(torch.cat(parts, -1), (4 * C,), ln_w, ln_b, eps), w)


def forward(sd, embed_dim: int, depths, num_heads, window_size, patch: int, robust: bool, img, eps: float = 1e-5,
            keeps=None, sd_probs=None):
    x = F.conv2d(img, sd["features.0.0.weight"], sd["features.0.0.bias"], stride=patch).permute(0, 2, 3, 1)
    x = F.layer_norm(x, (embed_dim,), sd["features.0.2.weight"], sd["features.0.2.bias"], eps)
    f = 1
    for s, depth in enumerate(depths):
        C = embed_dim * 2 ** s
        for i in range(depth):
            pre = f"features.{f}.{i}."
            shift = [0, 0] if i % 2 == 0 else [w // 2 for w in window_size]
            k1 = k2 = None
            if keeps is not None and pre[:-1] in keeps:
                p = sd_probs[pre[:-1]]
                k1, k2 = [(k / (1.0 - p)).reshape(-1, 1, 1, 1) for k in keeps[pre[:-1]]]
            y = F.layer_norm(x, (C,), sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], eps)
            y = window_attention(y, sd[pre + "attn.qkv.weight"], sd[pre + "attn.qkv.bias"], sd[pre + "attn.proj.weight"],
                                 sd[pre + "attn.proj.bias"], sd[pre + "attn.relative_position_bias_table"], num_heads[s],
                                 window_size, shift, robust)
            x = x + (y if k1 is None else y * k1)
            y = F.layer_norm(x, (C,), sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], eps)
            y = F.linear(F.gelu(F.linear(y, sd[pre + "mlp.0.weight"], sd[pre + "mlp.0.bias"])), sd[pre + "mlp.3.weight"],
                         sd[pre + "mlp.3.bias"])
            x = x + (y if k2 is None else y * k2)
        f += 1
        if s < len(depths) - 1:
            x = patch_merge(x, sd[f"features.{f}.norm.weight"], sd[f"features.{f}.norm.bias"], sd[f"features.{f}.reduction.weight"], eps)
            f += 1
    x = F.layer_norm(x, (x.shape[-1],), sd["norm.weight"], sd["norm.bias"], eps)
    return F.linear(x.mean(dim=(1, 2)), sd["head.weight"], sd["head.bias"])


def loss_and_grads(sd, cfg: dict, img, y, **kw):
    """(logits, CE loss, {name: grad}) in fp32 on the device of the tensors."""
    p = {k: v.detach().clone().float().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    logits = forward(p, cfg["embed_dim"], cfg["depths"], cfg["num_heads"], cfg["window_size"], cfg["patch_size"][0],
                     cfg.get("robust", False), img, **kw)
    loss = F.cross_entropy(logits, y)
    loss.backward()
    return logits.detach(), loss.detach(), {k: v.grad for k, v in p.items() if v.grad is not None}
