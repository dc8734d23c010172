"""Peaked attention inputs and a plain-torch reference of the attention definition (test infrastructure, no kernels).

`robust=True` exists for keys that almost no query attends to: the Sinkhorn column step rescales such a key's column back to
sum 1, so a key whose softmax weights are e^-12 .. e^-29 ends with O(1/N) weights and with dK / dV rows as large as any other
key's.  The builders here put chosen keys a chosen number of nats below the rest FOR EVERY QUERY; the reference evaluates

    P0 = softmax(scale q k^T + bias);  iters x { rows, columns };  rows;  (keep mask);  o = P v          (utils.py:1031-1037)

by autograd in float64 (or float32), optionally with the kernels' documented rounding points (P, dS and the outputs in bf16)
and nothing else.  `per_row_rel` is the metric: one relative L2 per (batch, head, token) row, so that a single wrong key is
not 1/N of a whole-tensor norm.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

Weak = Sequence[Tuple[int, float]]


def peaked_qkv(B: int, N: int, H: int, dh: int, weak: Weak, qc: float = 4.0, seed: int = 0) -> torch.Tensor:
    """bf16 [B*N, 3*H*dh] (the kernels' row-major layout).  randn; the component along u = ones(dh)/sqrt(dh) is removed from every
    q and k row; every query gets + qc u; key j gets - nats / (scale qc) u for each (j, nats) in `weak` (scale = dh^-0.5).  Every
    query then scores key j exactly `nats` below what it would otherwise, up to the bf16 rounding of the operands."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, 3, H, dh, generator=g, dtype=torch.float64)
    u = torch.full((dh,), dh ** -0.5, dtype=torch.float64)
    scale = dh ** -0.5
    for part in (0, 1):
        x[:, :, part] -= (x[:, :, part] @ u)[..., None] * u
    x[:, :, 0] += qc * u
    for j, nats in weak:
        assert 0 <= j < N, (j, N)
        x[:, j, 1] -= nats / (scale * qc) * u
    return x.reshape(B * N, 3 * H * dh).to(torch.bfloat16)


def peaked_scores(shape: Sequence[int], weak: Weak, std: float = 1.5, seed: int = 0) -> torch.Tensor:
    """fp32 scores [..., R, C] (any R, C): std * randn with `nats` subtracted from column j for each (j, nats) in `weak`."""
    g = torch.Generator().manual_seed(seed)
    S = std * torch.randn(*shape, generator=g, dtype=torch.float32)
    for j, nats in weak:
        assert 0 <= j < shape[-1], (j, shape)
        S[..., j] -= nats
    return S


def sinkhorn_definition(S: torch.Tensor, iters: int = 3) -> torch.Tensor:
    P = torch.softmax(S, dim=-1)
    for _ in range(iters):
        P = P / P.sum(dim=-1, keepdim=True)
        P = P / P.sum(dim=-2, keepdim=True)
    return P / P.sum(dim=-1, keepdim=True)


def sinkhorn_scalings(S: torch.Tensor, iters: int = 3):
    """The cumulative scalings the kernels save: a_1 b_1 .. a_iters b_iters a_{iters+1} with P = diag(a) softmax(S) diag(b) after each
    step -> (avec [..., iters + 1, R], bvec [..., iters, C])."""
    P0 = torch.softmax(S, dim=-1)
    a = torch.ones_like(P0[..., :, 0]); b = torch.ones_like(P0[..., 0, :])
    av, bv = [], []
    for _ in range(iters):
        a = 1.0 / (P0 * b[..., None, :]).sum(dim=-1); av.append(a)
        b = 1.0 / (P0 * a[..., :, None]).sum(dim=-2); bv.append(b)
    av.append(1.0 / (P0 * b[..., None, :]).sum(dim=-1))
    return torch.stack(av, dim=-2), (torch.stack(bv, dim=-2) if bv else None)


class _RoundGrad(torch.autograd.Function):
    """Identity whose gradient is rounded to bf16 (dS enters its two products in bf16)."""
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def _round_st(x: torch.Tensor) -> torch.Tensor:
    return x + (x.detach().to(torch.bfloat16).to(x.dtype) - x.detach())


def heads(t: torch.Tensor, B: int, N: int, H: int, dh: int) -> torch.Tensor:
    """[B*N, parts*H*dh] -> [parts, B, H, N, dh] (parts = 3 for qkv / dqkv, 1 for o / dout)."""
    parts = t.shape[1] // (H * dh)
    return t.reshape(B, N, parts, H, dh).permute(2, 0, 3, 1, 4)


def attention_reference(qkv: torch.Tensor, dout: Optional[torch.Tensor], B: int, N: int, H: int, dh: int, scale: float, *,
                        iters: int = 3, dtype: torch.dtype = torch.float64, emulate_bf16: bool = False,
                        bias: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None, pscale: float = 1.0,
                        drop_keys: Sequence[int] = (), device=None) -> dict:
    """o [B,H,N,dh], P [B,H,N,N] (before the keep mask), lse [B,H,N] and -- with `dout` [B*N, H*dh] -- dq, dk, dv [B,H,N,dh], all in
    `dtype`, by autograd through the definition.  `iters` = 0 is softmax attention.  `emulate_bf16`: P (after the keep mask), dS
    and o / dq / dk / dv are rounded to bf16 inside the evaluation (straight-through): the kernels' rounding points.
    `drop_keys`: the definition evaluated WITHOUT those keys (their score columns and value rows are removed; their dk / dv rows are
    zero) -- what a kernel must return for a key whose column underflows completely, where the definition itself is 0 / 0.
    `device`: where the evaluation runs and the results stay (default: the CPU) -- the same arithmetic in the same `dtype`."""
    device = torch.device("cpu") if device is None else device
    x = qkv.detach().to(device).to(dtype).requires_grad_(dout is not None)
    q, k, v = heads(x, B, N, H, dh)
    S = (q @ k.transpose(-1, -2)) * scale
    if bias is not None:
        S = S + bias.detach().to(device).to(dtype)
    if drop_keys:
        kept = [j for j in range(N) if j not in set(drop_keys)]
        S, v = S[..., kept], v[..., kept, :]
    if emulate_bf16:
        S = _RoundGrad.apply(S)
    P = sinkhorn_definition(S, iters)
    Pv = P if keep is None else P * (keep.detach().to(device) != 0).to(dtype) * pscale
    if emulate_bf16:
        Pv = _round_st(Pv)
    o = Pv @ v
    res = {"o": o.detach(), "P": P.detach(), "lse": torch.logsumexp(S.detach(), dim=-1)}
    if dout is not None:
        o.backward(heads(dout.detach().to(device).to(dtype), B, N, H, dh)[0])
        res["dq"], res["dk"], res["dv"] = heads(x.grad, B, N, H, dh)
    if emulate_bf16:
        for name in ("o", "dq", "dk", "dv"):
            if name in res:
                res[name] = res[name].to(torch.bfloat16).to(dtype)
    return res


def per_row_rel(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """Relative L2 of each row over the last (head) dimension, in float64.  A reference row of norm zero gives inf unless `got` is
    zero there too (then 0): callers assert that real tokens have none."""
    got = got.detach().cpu().double(); ref = ref.detach().cpu().double()
    num = (got - ref).norm(dim=-1); den = ref.norm(dim=-1)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num)))


def per_row_abs_vs_largest(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """|got - ref| per row relative to the LARGEST row norm of the reference tensor (softmax controls: a weak key's dk / dv rows
    are genuinely tiny there, so they are not compared relative to themselves)."""
    got = got.detach().cpu().double(); ref = ref.detach().cpu().double()
    return (got - ref).norm(dim=-1) / ref.norm(dim=-1).max().clamp_min(1e-300)


def std_weak(N: int) -> Weak:
    """Key 5 at -12 nats and key 77 (47 where N <= 77) at -20 nats."""
    return ((5, 12.0), (77 if N > 77 else 47, 20.0))


# (B, N, H, dh, weak): the shapes of the fused Sinkhorn kernels (N <= 256, dh 64) and of the composed path.  (2,196,1,64) has a
# weak key in the last, partial key tile (196 = 12 x 16 + 4); (1,65,1,64) has two weak keys in one 16-key tile and one in the
# one-key last tile.
FUSED_CASES = (
    (2, 197, 2, 64, std_weak(197)),
    (1, 256, 2, 64, std_weak(256)),
    (2, 49, 2, 64, std_weak(49)),
    (2, 196, 1, 64, ((5, 12.0), (195, 20.0))),
    (1, 65, 1, 64, ((34, 12.0), (40, 20.0), (64, 16.0))),
)
MANY_HEADS_CASE = (45, 197, 6, 64, std_weak(197))
COMPOSED_CASES = (
    (2, 257, 2, 80, ((5, 12.0), (77, 20.0), (256, 16.0))),
    (1, 577, 1, 64, std_weak(577)),
    (2, 100, 2, 96, std_weak(100)),
    (3, 17, 2, 32, ((5, 12.0), (16, 20.0))),
)
PER_ROW_BOUND = 3e-2          # dq / dk / dv rows of the Sinkhorn paths against fp64
EMULATION_BOUND = 1e-2        # what bf16 rounding at the documented points alone may cost (host test): a 3 x margin under the bound


def weak_key_vit_case(sd: dict, x: torch.Tensor, *, patch_size: int, num_heads: int, tokens=(5, 77), cosines=(1.0, 0.75),
                      qc: float = 8.0, nats: float = 24.0, beta: float = 8.0, seed: int = 0):
    """Turn a one-layer VisionTransformer state dict and an image batch (both modified in place, and returned) into a case in which
    the tokens `tokens` are weak keys in EVERY head of layer 0:
      * the patches behind those tokens are beta (cos p0 + sin p1) for two fixed random patches, so that after ln_1 the token lies
        along m = normalise(centre(W_conv p0)) with m . xn ~ cos sqrt(D), while every other token has m . xn ~ N(0, 1);
      * the KEY third of in_proj_weight gets the rank-one term - c u_h m^T in every head (u_h = ones(dh) / sqrt(dh)), and the query
        third of in_proj_bias + qc u_h, with c such that scale (qc) (c sqrt(D)) = nats.
    Returns (sd, x, logw): logw [B, H, S, len(tokens)] = log softmax of the layer's scores at those key columns, from the oracle's
    own arithmetic on the CPU (callers assert it is below -12 for every query)."""
    from oracle.simple_vit_oracle import layer_norm
    from oracle import vit_oracle as V
    g = torch.Generator().manual_seed(seed)
    pfx = "encoder.layers.encoder_layer_0."
    Wc = sd["conv_proj.weight"]
    D = Wc.shape[0]
    dh = D // num_heads
    p0, p1 = torch.randn(2, Wc[0].numel(), generator=g)
    t = Wc.reshape(D, -1) @ p0
    m = t - t.mean()
    m = m / m.norm()
    side = x.shape[-1] // patch_size
    for tok, c in zip(tokens, cosines):
        r, col = divmod(tok - 1, side)                      # token 0 is the class token
        patch = beta * (c * p0 + (1.0 - c * c) ** 0.5 * p1)
        x[:, :, r * patch_size:(r + 1) * patch_size, col * patch_size:(col + 1) * patch_size] = patch.reshape(Wc.shape[1:])
    coef = nats / (dh ** -0.5 * qc * D ** 0.5)
    sd[pfx + "self_attention.in_proj_weight"][D:2 * D] -= coef * dh ** -0.5 * m[None, :]
    sd[pfx + "self_attention.in_proj_bias"][:D] += qc * dh ** -0.5
    cap = {}
    with torch.no_grad():
        V.vit_forward(sd, x, patch_size=patch_size, num_heads=num_heads, robust=True, capture=cap)
        xn = layer_norm(cap["embed"], sd[pfx + "ln_1.weight"], sd[pfx + "ln_1.bias"], 1e-6)
        qkv = xn @ sd[pfx + "self_attention.in_proj_weight"].t() + sd[pfx + "self_attention.in_proj_bias"]
        B, S, _ = qkv.shape
        q, k, _ = (u.reshape(B, S, num_heads, dh).permute(0, 2, 1, 3) for u in qkv.chunk(3, dim=-1))
        logw = torch.log_softmax(q @ k.transpose(-1, -2) * dh ** -0.5, dim=-1)[..., list(tokens)]
    return sd, x, logw
