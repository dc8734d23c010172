"""References for PiT.

1. The fp32 PyTorch restatement of PiT's forward (pit.py:20-186), the oracle of the GPU model tests.  Written from the
   reference's equations: it walks a noise_robust_vit_amd.pit.PiT for the structure and takes fp32 copies of its weights.

       logits, loss, grads = pit_loss_and_grads(model, x, y, autocast=False)

   Runs on the device of `x`.  autocast=True evaluates the same code under torch.autocast(bfloat16): the bf16 leg the GPU tests
   size their bounds with.

2. fp64 per-element references of the two kernel families (the pooled depthwise convolution, the overlapped patch unfold),
   the bound of each, an fp32 emulation of each kernel's arithmetic (tests/test_pit_ref_host.py shows the bounds hold for it
   and that wrong kernels break them) and the seeded inputs the GPU kernel test and the host test share.

   The bounds are derived, not tuned.  The forward's bf16 output is ONE rounding of an fp32 value: 2^-8 |ref| (a bf16 ulp
   relative to the value), plus what the fp32 arithmetic in front of it can lose: n fp32 operations on a sum of products lose
   at most n 2^-23 sum |products| (the standard gamma_n bound with a factor 2 of slack).  n = 10 for an output (nine taps and
   the bias), 8 for an element of dx (at most 2 x 2 windows times two output channels; fp32 output: no bf16 term) and
   B * Ho * Wo for a tap or bias gradient.  The unfold is a copy: exact equality with F.unfold rounded to bf16.
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as F

from rvt_ref import BF16, U32, _fma32, _gen, bf16, ratio, sinkhorn  # noqa: F401


# ----------------------------------------------------------------------------------------------
# 1. the model
# ----------------------------------------------------------------------------------------------
def _layer(P, p, x, heads, robust):
    D = x.shape[-1]
    a = p + "0."
    xn = F.layer_norm(x, (D,), P[a + "norm.weight"], P[a + "norm.bias"], 1e-5)
    B, n, _ = xn.shape
    q, k, v = (t.reshape(B, n, heads, -1).permute(0, 2, 1, 3) for t in F.linear(xn, P[a + "fn.to_qkv.weight"]).chunk(3, dim=-1))
    dots = torch.matmul(q, k.transpose(-1, -2)) * q.shape[-1] ** -0.5
    w = torch.softmax(dots.float(), dim=-1)
    if robust:
        w = sinkhorn(w)
    o = torch.matmul(w.to(v.dtype), v).permute(0, 2, 1, 3).reshape(B, n, -1)
    x = x + F.linear(o, P[a + "fn.to_out.0.weight"], P[a + "fn.to_out.0.bias"])
    f = p + "1."
    h = F.layer_norm(x, (D,), P[f + "norm.weight"], P[f + "norm.bias"], 1e-5)
    u = F.gelu(F.linear(h, P[f + "fn.net.0.weight"], P[f + "fn.net.0.bias"]))
    return x + F.linear(u, P[f + "fn.net.3.weight"], P[f + "fn.net.3.bias"])


def _pool(P, p, x):
    B, N, C = x.shape
    g = int(round((N - 1) ** 0.5))
    cls = F.linear(x[:, :1], P[p + "cls_ff.weight"], P[p + "cls_ff.bias"])
    plane = x[:, 1:].transpose(1, 2).reshape(B, C, g, g)
    t = F.conv2d(plane, P[p + "downsample.net.0.weight"], P[p + "downsample.net.0.bias"], stride=2, padding=1, groups=C)
    t = F.conv2d(t, P[p + "downsample.net.1.weight"], P[p + "downsample.net.1.bias"])
    return torch.cat((cls.to(t.dtype), t.flatten(2).transpose(1, 2)), dim=1)


def forward(model, P, img):
    p = model.patch_size
    B = img.shape[0]
    x = F.unfold(img, p, stride=p // 2).transpose(1, 2)
    x = F.linear(x, P["to_patch_embedding.2.weight"], P["to_patch_embedding.2.bias"])
    x = torch.cat((P["cls_token"].expand(B, -1, -1), x.to(P["cls_token"].dtype)), dim=1)
    x = x + P["pos_embedding"][:, :x.shape[1]]
    for si, stage in enumerate(model.layers):
        if hasattr(stage, "cls_ff"):
            x = _pool(P, f"layers.{si}.", x)
        else:
            for li, (attn, _) in enumerate(stage.layers):
                x = _layer(P, f"layers.{si}.layers.{li}.", x, attn.fn.heads, stage._meta.robust)
    x = x[:, 0]
    D = x.shape[-1]
    return F.linear(F.layer_norm(x, (D,), P["mlp_head.0.weight"], P["mlp_head.0.bias"], 1e-5), P["mlp_head.1.weight"], P["mlp_head.1.bias"])


def pit_loss_and_grads(model, x, y, autocast=False):
    P = {k: v.detach().to(x.device, torch.float32).clone().requires_grad_(model.training) for k, v in model.named_parameters()}
    ctx = torch.autocast(x.device.type, dtype=torch.bfloat16) if autocast else contextlib.nullcontext()
    with ctx:
        logits = forward(model, P, x.float())
    logits = logits.float()
    loss = F.cross_entropy(logits, y)
    grads = {}
    if model.training:
        loss.backward()
        grads = {k: v.grad for k, v in P.items()}
    return logits.detach(), loss.detach(), grads


# ----------------------------------------------------------------------------------------------
# 2. kernel references
# ----------------------------------------------------------------------------------------------
# ---- pooled depthwise conv ---------------------------------------------------------------------
# the kernels have no spatial tile (one thread per output token / input row, exact grids); (9, 6) runs several workgroups
POOL_PLANES = ((1, 1), (2, 3), (3, 5), (4, 4), (9, 6))
POOL_B = 3
POOL_C = (8, 72)
POOL_KINDS = ("random", "impulse_x", "impulse_d")


def pool_out(n: int) -> int:
    return (n - 1) // 2 + 1


def pool_inputs(H, W, C, lead, kind="random"):
    """(x fp32 rows [B*(lead + H*W), C], w fp32 [2C, 9], bias fp32 [2C], dout bf16 rows [B*Ho*Wo, 2C]), random.
    kind="impulse_x": x is zero but for a one at one patch token per sample (another token in every sample), all channels:
    the forward output holds bias + single taps, dw picks single values of dout.  kind="impulse_d": the same for dout: dx holds
    single taps (summed over the two output channels of a group), dw single values of x.  The class rows of x are random in
    every kind: they must not be read."""
    gen = _gen("pool", H, W, C, lead)
    Ho, Wo = pool_out(H), pool_out(W)
    x = torch.randn(POOL_B * (lead + H * W), C, generator=gen)
    w = torch.randn(2 * C, 9, generator=gen) / 3
    bias = torch.randn(2 * C, generator=gen) * 0.5
    dout = bf16(torch.randn(POOL_B * Ho * Wo, 2 * C, generator=gen))
    if kind == "impulse_x":
        x3 = x.reshape(POOL_B, lead + H * W, C)
        x3[:, lead:] = 0.0
        for b in range(POOL_B):
            x3[b, lead + (b * 7 + (H * W) // 2) % (H * W)] = 1.0
    elif kind == "impulse_d":
        d3 = torch.zeros(POOL_B, Ho * Wo, 2 * C)
        for b in range(POOL_B):
            d3[b, (b * 7 + (Ho * Wo) // 2) % (Ho * Wo)] = 1.0
        dout = bf16(d3.reshape(POOL_B * Ho * Wo, 2 * C))
    return x.contiguous(), w, bias, dout


def _planes(rows, H, W, lead, dtype=torch.float64):
    """[B*(lead + H*W), C] -> [B, C, H, W] of the patch rows"""
    C = rows.shape[1]
    return rows.to(dtype).reshape(POOL_B, lead + H * W, C)[:, lead:].reshape(POOL_B, H, W, C).permute(0, 3, 1, 2)


def _rows(planes, lead=0, fill=0.0):
    """[B, C, H, W] -> [B*(lead + H*W), C] with the class rows set to `fill`"""
    B, C, H, W = planes.shape
    out = torch.full((B, lead + H * W, C), fill, dtype=planes.dtype)
    out[:, lead:] = planes.permute(0, 2, 3, 1).reshape(B, H * W, C)
    return out.reshape(B * (lead + H * W), C)


def pool_fwd_ref(x, w, bias, H, W, lead):
    """(ref fp64 rows [B*Ho*Wo, 2C], bound)"""
    C = x.shape[1]
    p, k, b = _planes(x, H, W, lead), w.double().reshape(2 * C, 1, 3, 3), bias.double()
    ref = F.conv2d(p, k, b, stride=2, padding=1, groups=C)
    mag = F.conv2d(p.abs(), k.abs(), b.abs(), stride=2, padding=1, groups=C)
    return _rows(ref), _rows(BF16 * ref.abs() + 10 * U32 * mag)


def _windows(xp, ky, kx, Ho, Wo, chan="div"):
    """The input of tap (ky, kx) for every output token and output channel, [B, 2C, Ho, Wo], from the plane padded by one.
    chan="div": output channel o reads input channel o // 2 (PyTorch's grouping); "mod": o % C (a wrong kernel)."""
    win = xp[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2][:, :, :Ho, :Wo]
    return win.repeat_interleave(2, dim=1) if chan == "div" else win.repeat(1, 2, 1, 1)


def pool_bwd_ref(x, w, dout, H, W, lead):
    """(dx rows fp64 with zero class rows, its bound, dw fp64 [2C, 9], its bound, dbias fp64 [2C], its bound)"""
    C = x.shape[1]
    Ho, Wo = pool_out(H), pool_out(W)
    p, d, k = _planes(x, H, W, lead), _planes(dout, Ho, Wo, 0), w.double().reshape(2 * C, 1, 3, 3)
    op = (H - (2 * Ho - 1), W - (2 * Wo - 1))
    dx = F.conv_transpose2d(d, k, stride=2, padding=1, output_padding=op, groups=C)
    mag = F.conv_transpose2d(d.abs(), k.abs(), stride=2, padding=1, output_padding=op, groups=C)
    xp = F.pad(p, (1, 1, 1, 1))
    dw = torch.zeros(2 * C, 9, dtype=torch.float64)
    dwm = torch.zeros(2 * C, 9, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            t = d * _windows(xp, ky, kx, Ho, Wo)
            dw[:, ky * 3 + kx] = t.sum(dim=(0, 2, 3))
            dwm[:, ky * 3 + kx] = t.abs().sum(dim=(0, 2, 3))
    n = POOL_B * Ho * Wo
    return (_rows(dx, lead, 0.0), _rows(8 * U32 * mag, lead, 0.0), dw, n * U32 * dwm, d.sum(dim=(0, 2, 3)), n * U32 * d.abs().sum(dim=(0, 2, 3)))


def pool_fwd_emul(x, w, bias, H, W, lead, chan="div", origin=-1, swap=False):
    """The kernel's arithmetic: acc = bias, then fp32 FMAs over the taps ky, kx ascending, one bf16 rounding.  Wrong kernels for
    the host test: chan="mod" (channel map o % C), origin=0 (the window starts at 2 o instead of 2 o - 1), swap (ky / kx
    exchanged on the weights)."""
    C = x.shape[1]
    Ho, Wo = pool_out(H), pool_out(W)
    off = origin + 1
    xp = F.pad(_planes(x, H, W, lead, torch.float32), (1, 1 + off + 2, 1, 1 + off + 2))
    acc = bias.reshape(1, 2 * C, 1, 1).expand(POOL_B, 2 * C, Ho, Wo).contiguous()
    for ky in range(3):
        for kx in range(3):
            wt = w[:, kx * 3 + ky] if swap else w[:, ky * 3 + kx]
            acc = _fma32(wt.reshape(1, 2 * C, 1, 1), _windows(xp, ky + off, kx + off, Ho, Wo, chan), acc)
    return _rows(bf16(acc))


def pool_dx_emul(w, dout, H, W, lead, C):
    """fp32 FMAs in the kernel's order: ky, then kx, then o = 2c, 2c + 1; an input outside a window is not touched."""
    Ho, Wo = pool_out(H), pool_out(W)
    d = _planes(dout, Ho, Wo, 0, torch.float32)
    acc = torch.zeros(POOL_B, C, H + 3, W + 3)
    for ky in range(3):
        for kx in range(3):
            for j in range(2):
                prod = torch.zeros(POOL_B, C, H + 3, W + 3, dtype=torch.float64)
                prod[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] = w[j::2, ky * 3 + kx].double().reshape(1, C, 1, 1) * d[:, j::2].double()
                acc = (prod + acc.double()).float()
    return _rows(acc[:, :, 1:H + 1, 1:W + 1].double(), lead, 0.0)


def pool_dw_emul(x, dout, H, W, lead):
    """Per-sample partials over the output tokens in row-major order (fp32 FMAs; fp32 adds for the bias), then the samples in
    index order.  Returns (dw [2C, 9], dbias [2C])."""
    C = x.shape[1]
    Ho, Wo = pool_out(H), pool_out(W)
    xp = F.pad(_planes(x, H, W, lead, torch.float32), (1, 2, 1, 2))
    d = _planes(dout, Ho, Wo, 0, torch.float32)
    part = torch.zeros(POOL_B, 2 * C, 3, 3)
    pb = torch.zeros(POOL_B, 2 * C)
    for oy in range(Ho):
        for ox in range(Wo):
            win = xp[:, :, 2 * oy:2 * oy + 3, 2 * ox:2 * ox + 3].repeat_interleave(2, dim=1)
            part = _fma32(d[:, :, oy, ox].reshape(POOL_B, 2 * C, 1, 1), win, part)
            pb = pb + d[:, :, oy, ox]
    dw, db = torch.zeros(2 * C, 3, 3), torch.zeros(2 * C)
    for b in range(POOL_B):
        dw, db = dw + part[b], db + pb[b]
    return dw.reshape(2 * C, 9), db


# ---- overlapped patch unfold -------------------------------------------------------------------
# (ks, stride): PiT's patch 8 / 14 / 16 / 32 at stride p // 2, and non-overlapping 5 x 5
UNFOLD_CASES = ((8, 4), (14, 7), (16, 8), (32, 16), (5, 5))
UNFOLD_B, UNFOLD_C = 2, 3
# work items (8 features each) of one shape that the capped grid-stride loop (16384 workgroups of 256) walks in two full
# passes and a partial one: 3 * 171 * 171 * 96 = 8 421 408 > 2 * 16384 * 256 = 8 388 608
UNFOLD_BIG = (3, 3, 1376, 16, 8)                   # B, C, image side, ks, stride


def unfold_shape(ks, stride):
    """An image one pixel larger than a whole number of strides in both directions (the last partial window is dropped),
    not square."""
    return ks + 2 * stride + 1, ks + 3 * stride + 1


def unfold_input(ks, stride, dtype):
    H, W = unfold_shape(ks, stride)
    img = torch.randn(UNFOLD_B, UNFOLD_C, H, W, generator=_gen("unfold", ks, stride))
    return img.to(dtype)


def unfold_ref(img, ks, stride):
    """bf16 [B*Ho*Wo, pad8(ks*ks*C)]: F.unfold's columns as token rows, rounded to bf16, zero pad columns"""
    cols = F.unfold(img.float(), ks, stride=stride).transpose(1, 2)
    cols = bf16(cols.reshape(-1, cols.shape[-1]))
    return F.pad(cols, (0, -cols.shape[1] % 8))


def unfold_emul(img, ks, stride):
    """The kernel's addressing, element by element (slow: small shapes only): feature f = c ks^2 + ky ks + kx of token
    (b, oy, ox) is img[b, c, oy stride + ky, ox stride + kx], rounded to bf16 (nearest even) if fp32."""
    B, C, H, W = img.shape
    Ho, Wo = (H - ks) // stride + 1, (W - ks) // stride + 1
    Fn = C * ks * ks
    out = torch.zeros(B * Ho * Wo, (Fn + 7) // 8 * 8, dtype=torch.bfloat16)
    f = torch.arange(Fn)
    c, k = f // (ks * ks), f % (ks * ks)
    ky, kx = k // ks, k % ks
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                out[(b * Ho + oy) * Wo + ox, :Fn] = bf16(img[b, c, oy * stride + ky, ox * stride + kx])
    return out
