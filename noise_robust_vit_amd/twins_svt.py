"""Twins-SVT on the HIP path: drop-in for the reference's twins_svt.py.

    from noise_robust_vit_amd.twins_svt import TwinsSVT          # was: from vit_pytorch_robust.twins_svt import TwinsSVT
    model = TwinsSVT(num_classes=1000, s1_emb_dim=64, s2_emb_dim=128, s3_emb_dim=256, s4_emb_dim=512, robust=True).cuda()

Same keyword-only constructor and defaults, module tree, state_dict keys and shapes (`layers.s.0.proj.*`,
`layers.s.{1,3}.layers.i.{0,1,2,3}.fn.{norm.{g,b}, fn.{to_q.weight, to_kv.weight, to_out.0.*, net.{0,3}.*}}`, `layers.s.2.proj.fn.*`,
`layers.6.*`; the (1, C, 1, 1) `g` / `b` and the 4-D conv weights included) and parameter draw order as twins_svt.py:175-229, so
seeded models and reference checkpoints are interchangeable.  One added keyword on `TwinsSVT`, `Transformer`, `LocalAttention`
and `GlobalAttention`, `robust=False`, selects SinkhornAttention's normalisation (utils.py:1025-1037) instead of softmax.

The residual stream is fp32 token-major rows x [B*g*g, C] (the reference's NCHW map with the channels last); a stage is

    PatchEmbedFn  : nrv_soft_split_fwd with ks == stride == patch (the 'b c (h p1) (w p2) -> b (c p1 p2) h w' rearrange; the
                    NCHW image in stage 1, bf16 rows after that) -> NT GEMM with the bias into the new stream
    LocalAttnFn   : channel LayerNorm (the row LayerNorm on token-major rows) -> to_q and to_kv as two NT GEMMs into column
                    blocks of one packed [T, 3 * 512] buffer through ldc -> nrv_window_attn_fwd (shift 0, a zero table that is
                    not a parameter, softmax or Sinkhorn) -> to_out GEMM with the bias + residual epilogue
    GlobalAttnFn  : LayerNorm -> to_q GEMM; the k x k, stride-k to_kv convolution as nrv_soft_split_fwd + GEMM ([B*Nk, 2 * 512],
                    k | v) -> nrv_subattn_fwd (softmax, Nk <= 128: K and V of a head on chip, nothing [Nq, Nk]-sized in memory),
                    else the composed path nrv_bgemm -> nrv_sinkhorn_fwd (0 or 3 iterations) -> nrv_bgemm -> to_out GEMM
    FeedForwardFn : encoder.mlp_half_fwd (LayerNorm, fc1 + GELU, fc2 with the bias + residual epilogue)
    PegFn         : nrv_peg_fwd (x + depthwise conv(x) + bias on the fp32 stream), once per stage

and the backward mirrors it (weight gradients on the TN GEMM, nrv_soft_split_bwd for the unfolds, nrv_subattn_bwd,
nrv_window_attn_bwd whose table gradient is dropped, nrv_peg_bwd).  The final mean over the tokens and the Linear head are torch
(B * C elements).  The heads are always 8 x 64: TwinsSVT passes neither `heads` nor `dim_head` on, as in the reference.

Refused with NotImplementedError (nothing is approximated): dropout > 0 in training, non-square images, a map that
local_patch_size or global_k does not tile (the reference fails there too), global_k or patch sizes above 7, PEG kernels other
than 3 / 5 / 7, emb_dim not a multiple of 8 or above 4096, a window of more than 64 slots, head dims other than 32 / 64,
attention recording, and a direct call of the holder modules (Residual, PreNorm, LayerNorm, FeedForward, PatchEmbedding, PEG
and the two attention classes: a Transformer or TwinsSVT runs them).  CPU tensors raise NrvError.
"""
from __future__ import annotations

import torch
from torch import nn

from . import encoder as E
from . import kernels as K
from ._lib import EPI_BIAS, EPI_BIAS_RESIDUAL
from .encoder import WEIGHTS

Tensor = torch.Tensor

__all__ = ["TwinsSVT", "Transformer", "LocalAttention", "GlobalAttention", "FeedForward", "PatchEmbedding", "PEG", "PreNorm",
           "Residual", "LayerNorm", "group_dict_by_key", "group_by_key_prefix_and_remove_prefix"]

_KEEP_P_BYTES = 1 << 30          # the composed path keeps its probability matrix for the backward up to this size


# helper methods (twins_svt.py:10-21)

def group_dict_by_key(cond, d):
    return_val = [dict(), dict()]
    for key in d.keys():
        match = bool(cond(key))
        ind = int(not match)
        return_val[ind][key] = d[key]
    return (*return_val,)


def group_by_key_prefix_and_remove_prefix(prefix, d):
    kwargs_with_prefix, kwargs = group_dict_by_key(lambda x: x.startswith(prefix), d)
    kwargs_without_prefix = dict(map(lambda x: (x[0][len(prefix):], x[1]), tuple(kwargs_with_prefix.items())))
    return kwargs_without_prefix, kwargs


# ----------------------------------------------------------------------------------------------
# modules (parameter holders with the reference's names and construction order)
# ----------------------------------------------------------------------------------------------
Residual = E.Residual


class LayerNorm(E.Holder):
    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.g = nn.Parameter(torch.ones(1, dim, 1, 1))
        self.b = nn.Parameter(torch.zeros(1, dim, 1, 1))


class PreNorm(E.Holder):
    def __init__(self, dim, fn):
        super().__init__()
        self.norm = LayerNorm(dim)
        self.fn = fn


def _check_dim(dim: int, what: str) -> None:
    if dim % 8 or not 8 <= dim <= 4096:
        raise NotImplementedError(f"{what}: dim {dim} must be a multiple of 8 and at most 4096 (LayerNorm and the GEMMs)")


class FeedForward(E.Holder):
    def __init__(self, dim, mult=4, dropout=0.):
        super().__init__()
        _check_dim(dim, "FeedForward")
        self.net = nn.Sequential(nn.Conv2d(dim, dim * mult, 1), nn.GELU(), nn.Dropout(dropout), nn.Conv2d(dim * mult, dim, 1),
                                 nn.Dropout(dropout))


class PatchEmbedding(E.Holder):
    def __init__(self, *, dim, dim_out, patch_size):
        super().__init__()
        _check_dim(dim_out, "PatchEmbedding")
        if not 1 <= patch_size <= 7:
            raise NotImplementedError(f"patch_size {patch_size}: the unfold kernel takes 1 .. 7")
        self.dim = dim
        self.dim_out = dim_out
        self.patch_size = patch_size
        self.proj = nn.Conv2d(patch_size ** 2 * dim, dim_out, 1)


class PEG(E.Holder):
    def __init__(self, dim, kernel_size=3):
        super().__init__()
        if kernel_size not in (3, 5, 7):
            raise NotImplementedError(f"PEG kernel_size {kernel_size}: 3, 5 and 7 are implemented")
        self.proj = Residual(nn.Conv2d(dim, dim, kernel_size=kernel_size, padding=kernel_size // 2, groups=dim, stride=1))


def _check_heads(dim: int, heads: int, dim_head: int, what: str) -> None:
    _check_dim(dim, what)
    if dim_head not in (32, 64):
        raise NotImplementedError(f"{what}: dim_head {dim_head}: the attention kernels take 32 and 64")
    if heads < 1:
        raise NotImplementedError(f"{what}: heads {heads}")


class LocalAttention(E.Holder):
    def __init__(self, dim, heads=8, dim_head=64, dropout=0., patch_size=7, robust=False):
        super().__init__()
        _check_heads(dim, heads, dim_head, "LocalAttention")
        if patch_size < 1 or patch_size * patch_size > 64:
            raise NotImplementedError(f"local patch_size {patch_size}: a window of {patch_size * patch_size} slots, the kernel takes 64")
        inner_dim = dim_head * heads
        self.patch_size = patch_size
        self.heads = heads
        self.dim_head = dim_head
        self.scale = dim_head ** -0.5
        self.robust = bool(robust)
        self.to_q = nn.Conv2d(dim, inner_dim, 1, bias=False)
        self.to_kv = nn.Conv2d(dim, inner_dim * 2, 1, bias=False)
        self.to_out = nn.Sequential(nn.Conv2d(inner_dim, dim, 1), nn.Dropout(dropout))


class GlobalAttention(E.Holder):
    def __init__(self, dim, heads=8, dim_head=64, dropout=0., k=7, robust=False):
        super().__init__()
        _check_heads(dim, heads, dim_head, "GlobalAttention")
        if not 1 <= k <= 7:
            raise NotImplementedError(f"global k {k}: the unfold kernel takes 1 .. 7")
        inner_dim = dim_head * heads
        self.heads = heads
        self.dim_head = dim_head
        self.k = k
        self.scale = dim_head ** -0.5
        self.robust = bool(robust)
        self.to_q = nn.Conv2d(dim, inner_dim, 1, bias=False)
        self.to_kv = nn.Conv2d(dim, inner_dim * 2, k, stride=k, bias=False)
        self.dropout = nn.Dropout(dropout)
        self.to_out = nn.Sequential(nn.Conv2d(inner_dim, dim, 1), nn.Dropout(dropout))


# ----------------------------------------------------------------------------------------------
# autograd nodes on the fp32 stream x [B*g*g, C]
# ----------------------------------------------------------------------------------------------
def _flat(p: Tensor) -> Tensor:
    return p.detach().reshape(-1)


class PatchEmbedFn(torch.autograd.Function):
    """PatchEmbedding (twins_svt.py:68-79): src is the NCHW image (stage 1, no gradient) or the fp32 stream [B*G*G, C];
    -> fp32 [B*g*g, dim_out], g = G / p."""

    @staticmethod
    def forward(ctx, src, weight, bias, B: int, C: int, G: int, p: int, rows: bool):
        s = K.cast_bf16(src.detach().to(torch.float32).contiguous()) if rows else src.detach().contiguous()
        cols = K.soft_split_fwd(s, B, C, G, G, p, p, 0, rows)
        wb, _ = E.padded_images(weight, cols.shape[1], True)
        out = K.gemm_nt(cols, wb, out_dtype=torch.float32, epilogue=EPI_BIAS, bias=bias.detach())
        ctx.saved = cols
        ctx.cfg = (B, C, G, p, rows)
        ctx.params = (weight,)
        return out

    @staticmethod
    def backward(ctx, dy):
        cols = ctx.saved
        B, C, G, p, rows = ctx.cfg
        (weight,) = ctx.params
        ctx.saved = None
        F = weight[0].numel()
        d16 = K.cast_bf16(dy.to(torch.float32).contiguous())
        dw, db = K.gemm_tn(d16, cols, want_dbias=True)
        if cols.shape[1] != F:
            dw = dw[:, :F].contiguous()                                       # the zero-padded feature columns are dropped
        dx = None
        if rows:
            _, wt = E.padded_images(weight, cols.shape[1], True)
            dcols = K.gemm_nt(d16, wt, out_dtype=torch.bfloat16)
            dx = K.soft_split_bwd(dcols, B, C, G, G, p, p, 0, ld=C)
        return dx, dw.reshape(weight.shape), db, None, None, None, None, None


class PegFn(torch.autograd.Function):
    """PEG (twins_svt.py:81-87): x + Conv2d(C, C, ks, padding ks // 2, groups = C)(x) on the fp32 stream."""

    @staticmethod
    def forward(ctx, x, weight, bias, B: int, g: int):
        x = x.detach().contiguous()
        ctx.saved = x
        ctx.cfg = (B, g)
        ctx.params = (weight,)
        return K.peg_fwd(x, weight.detach(), bias.detach(), B, g, g)

    @staticmethod
    def backward(ctx, dy):
        B, g = ctx.cfg
        (weight,) = ctx.params
        x, ctx.saved = ctx.saved, None
        dx, dw, db = K.peg_bwd(x, weight.detach(), dy.to(torch.float32).contiguous(), B, g, g)
        return dx, dw, db, None, None


class FeedForwardFn(torch.autograd.Function):
    """Residual(PreNorm(FeedForward)) (twins_svt.py:55-66): x + fc2(gelu(fc1(LN x))), the 1 x 1 convolutions as GEMMs."""

    @staticmethod
    def forward(ctx, x, eps: float, g, b, w1, b1, w2, b2):
        meta = E.BlockMeta(heads=1, dim_head=x.shape[1], eps=eps)
        y, saved = E.mlp_half_fwd(x.detach().contiguous(), meta, _flat(g), _flat(b), w1, b1.detach(), w2, b2.detach(), residual=True)
        ctx.saved, ctx.meta = saved, meta
        ctx.params = (g, b, w1, b1, w2, b2)
        return y

    @staticmethod
    def backward(ctx, dy):
        g, b, w1, b1, w2, b2 = ctx.params
        saved, ctx.saved = ctx.saved, None
        dx, _, (dg, db, dw1, db1, dw2, db2) = E.mlp_half_bwd(dy.to(torch.float32).contiguous(), None, saved, ctx.meta, _flat(g), _flat(b),
                                                              w1, b1, w2, b2, residual=True, want_bf16=False)
        E.wgrad_flush(ctx.meta)
        return dx, None, dg.reshape(g.shape), db.reshape(b.shape), dw1.reshape(w1.shape), db1, dw2.reshape(w2.shape), db2


class LocalAttnFn(torch.autograd.Function):
    """Residual(PreNorm(LocalAttention)) (twins_svt.py:89-121): attention inside p x p windows of the map, no shift, no bias.
    cfg = (B, g, heads, dh, p, robust, eps)."""

    @staticmethod
    def forward(ctx, x, cfg, g_, b_, wq, wkv, wo, bo):
        B, g, H, dh, p, robust, eps = cfg
        x = x.detach().contiguous()
        inner = H * dh
        xn, mean, rstd = K.layernorm_fwd(x, _flat(g_), _flat(b_), eps)
        qkv = torch.empty(x.shape[0], 3 * inner, dtype=torch.bfloat16, device=x.device)
        K.gemm_nt(xn, WEIGHTS.get(wq, True)[0], out=qkv[:, :inner])
        K.gemm_nt(xn, WEIGHTS.get(wkv, True)[0], out=qkv[:, inner:])
        table = E.cached("twins.table", torch.zeros, (2 * p - 1) ** 2, H, device=x.device)
        o, stats = K.window_attn_fwd(qkv, table, B, g, g, inner, H, (p, p), (0, 0), robust)
        y = K.gemm_nt(o, WEIGHTS.get(wo, True)[0], out_dtype=torch.float32, epilogue=EPI_BIAS_RESIDUAL, bias=bo.detach(), aux=x)
        ctx.cfg = cfg
        ctx.saved = (x, xn, mean, rstd, qkv, o, stats, table)
        ctx.params = (g_, b_, wq, wkv, wo)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, g, H, dh, p, robust, eps = ctx.cfg
        x, xn, mean, rstd, qkv, o, stats, table = ctx.saved
        g_, b_, wq, wkv, wo = ctx.params
        ctx.saved = None
        inner = H * dh
        dy = dy.to(torch.float32).contiguous()
        d16 = K.cast_bf16(dy)
        dwo, dbo = K.gemm_tn(d16, o, want_dbias=True)
        do = K.gemm_nt(d16, WEIGHTS.get(wo, True)[1], out_dtype=torch.bfloat16)
        dqkv, _ = K.window_attn_bwd(qkv, table, do, stats, B, g, g, inner, H, (p, p), (0, 0), robust)    # the zero table takes no gradient
        dq, dkv = dqkv[:, :inner], dqkv[:, inner:]
        dwq = K.gemm_tn(dq, xn)
        dwkv = K.gemm_tn(dkv, xn)
        dxn = E.dx_sum([(dq, wq), (dkv, wkv)], torch.bfloat16)
        dx, _, dg, db = K.layernorm_bwd(dxn, x, _flat(g_), mean, rstd, dres=dy)
        return dx, None, dg.reshape(g_.shape), db.reshape(b_.shape), dwq.reshape(wq.shape), dwkv.reshape(wkv.shape), dwo.reshape(wo.shape), dbo


def _global_strides(Nq: int, Nk: int, H: int, dh: int):
    """(row, col, sample, head) element strides inside q / out [B*Nq, H*dh], kv [B*Nk, 2*H*dh] (k at column 0, v at H*dh) and a
    [B, H, Nq, Nk] matrix, each plain and transposed."""
    inner = H * dh
    q = (inner, 1, Nq * inner, dh)
    kv, kvT = (2 * inner, 1, Nk * 2 * inner, dh), (1, 2 * inner, Nk * 2 * inner, dh)
    mat, matT = (Nk, 1, H * Nq * Nk, Nq * Nk), (1, Nk, H * Nq * Nk, Nq * Nk)
    return q, kv, kvT, mat, matT


def _composed_probs(q: Tensor, kv: Tensor, B: int, H: int, Nq: int, Nk: int, dh: int, scale: float, iters: int):
    sq, _, kvT, mat, _ = _global_strides(Nq, Nk, H, dh)
    S = torch.empty(B, H, Nq, Nk, dtype=torch.float32, device=q.device)
    K.bgemm((q, 0), sq, (kv, 0), kvT, (S, 0), mat, B, H, Nq, Nk, dh, scale)
    P, lse, avec, bvec = K.sinkhorn_fwd(S, iters=iters)
    return S, P, lse, avec, bvec


class GlobalAttnFn(torch.autograd.Function):
    """Residual(PreNorm(GlobalAttention)) (twins_svt.py:123-154): every token against the Nk = (g / k)^2 keys of the k x k,
    stride-k to_kv convolution.  cfg = (B, g, heads, dh, k, robust, eps)."""

    @staticmethod
    def forward(ctx, x, cfg, g_, b_, wq, wkv, wo, bo):
        B, g, H, dh, k, robust, eps = cfg
        x = x.detach().contiguous()
        inner, D = H * dh, x.shape[1]
        Nq, gk = g * g, g // k
        Nk = gk * gk
        scale = dh ** -0.5
        xn, mean, rstd = K.layernorm_fwd(x, _flat(g_), _flat(b_), eps)
        q = K.gemm_nt(xn, WEIGHTS.get(wq, True)[0])
        cols = xn if k == 1 else K.soft_split_fwd(xn, B, D, g, g, k, k, 0, True)
        kv = K.gemm_nt(cols, WEIGHTS.get(wkv, True)[0])
        fused = not robust and Nk <= K.SUBATTN_MAX_NK
        if fused:
            o, lse = K.subattn_fwd(q, kv[:, :inner], kv[:, inner:], B, H, Nq, Nk, dh, scale)
            att = (lse,)
        else:
            sq, kvs, _, mat, _ = _global_strides(Nq, Nk, H, dh)
            iters = 3 if robust else 0
            _, P, lse, avec, bvec = _composed_probs(q, kv, B, H, Nq, Nk, dh, scale, iters)
            o = torch.empty(B * Nq, inner, dtype=torch.bfloat16, device=x.device)
            K.bgemm((P, 0), mat, (kv, inner), kvs, (o, 0), sq, B, H, Nq, dh, Nk, 1.0)
            att = (P if P.numel() * 4 <= _KEEP_P_BYTES else None, lse, avec, bvec, iters)
        y = K.gemm_nt(o, WEIGHTS.get(wo, True)[0], out_dtype=torch.float32, epilogue=EPI_BIAS_RESIDUAL, bias=bo.detach(), aux=x)
        ctx.cfg, ctx.fused = cfg, fused
        ctx.saved = (x, xn, mean, rstd, q, cols, kv, o, att)
        ctx.params = (g_, b_, wq, wkv, wo)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, g, H, dh, k, robust, eps = ctx.cfg
        x, xn, mean, rstd, q, cols, kv, o, att = ctx.saved
        g_, b_, wq, wkv, wo = ctx.params
        ctx.saved = None
        inner, D = H * dh, x.shape[1]
        Nq, gk = g * g, g // k
        Nk = gk * gk
        scale = dh ** -0.5
        dy = dy.to(torch.float32).contiguous()
        d16 = K.cast_bf16(dy)
        dwo, dbo = K.gemm_tn(d16, o, want_dbias=True)
        do = K.gemm_nt(d16, WEIGHTS.get(wo, True)[1], out_dtype=torch.bfloat16)
        dkv = torch.empty_like(kv)
        if ctx.fused:
            dq, _, _ = K.subattn_bwd(q, kv[:, :inner], kv[:, inner:], do, att[0], B, H, Nq, Nk, dh, scale, dk=dkv[:, :inner], dv=dkv[:, inner:])
        else:
            P, lse, avec, bvec, iters = att
            sq, kvs, kvT, mat, matT = _global_strides(Nq, Nk, H, dh)
            if P is None:                                        # not kept: recomputed with the scores the Sinkhorn backward needs
                S, P2 = _composed_probs(q, kv, B, H, Nq, Nk, dh, scale, iters)[:2]
            else:
                P2 = P
                S = torch.empty(B, H, Nq, Nk, dtype=torch.float32, device=x.device)
                K.bgemm((q, 0), sq, (kv, 0), kvT, (S, 0), mat, B, H, Nq, Nk, dh, scale)
            K.bgemm((P2, 0), matT, (do, 0), sq, (dkv, inner), kvs, B, H, Nk, dh, Nq, 1.0)               # dV = P^T dO
            dP = torch.empty_like(P2)
            K.bgemm((do, 0), sq, (kv, inner), kvT, (dP, 0), mat, B, H, Nq, Nk, dh, 1.0)                 # dP = dO V^T
            del P2, P
            dS = K.sinkhorn_bwd(S, dP, lse, avec, bvec, iters=iters)
            del dP, S
            dq = torch.empty_like(q)
            K.bgemm((dS, 0), mat, (kv, 0), kvs, (dq, 0), sq, B, H, Nq, dh, Nk, scale)                   # dQ = scale dS K
            K.bgemm((dS, 0), matT, (q, 0), sq, (dkv, 0), kvs, B, H, Nk, dh, Nq, scale)                  # dK = scale dS^T Q
        dwq = K.gemm_tn(dq, xn)
        dwkv = K.gemm_tn(dkv, cols)
        dcols = K.gemm_nt(dkv, WEIGHTS.get(wkv, True)[1], out_dtype=torch.float32 if k == 1 else torch.bfloat16)
        dxn_kv = dcols if k == 1 else K.soft_split_bwd(dcols, B, D, g, g, k, k, 0, ld=D)
        dxn = K.gemm_nt(dq, WEIGHTS.get(wq, True)[1], out_dtype=torch.bfloat16, epilogue=EPI_BIAS_RESIDUAL, aux=dxn_kv)
        dx, _, dg, db = K.layernorm_bwd(dxn, x, _flat(g_), mean, rstd, dres=dy)
        return dx, None, dg.reshape(g_.shape), db.reshape(b_.shape), dwq.reshape(wq.shape), dwkv.reshape(wkv.shape), dwo.reshape(wo.shape), dbo


# ----------------------------------------------------------------------------------------------
# the runnable modules
# ----------------------------------------------------------------------------------------------
class Transformer(nn.Module):
    """twins_svt.py:156-173.  forward(x [B, dim, g, g]) on the HIP device; `run` takes the fp32 token-major rows."""

    def __init__(self, dim, depth, heads=8, dim_head=64, mlp_mult=4, local_patch_size=7, global_k=7, dropout=0., has_local=True,
                 robust=False):
        super().__init__()
        self.layers = nn.ModuleList([])
        self.p = dropout
        self.robust = bool(robust)
        for _ in range(depth):
            self.layers.append(nn.ModuleList([
                Residual(PreNorm(dim, LocalAttention(dim, heads=heads, dim_head=dim_head, dropout=dropout, patch_size=local_patch_size,
                                                     robust=robust))) if has_local else nn.Identity(),
                Residual(PreNorm(dim, FeedForward(dim, mlp_mult, dropout=dropout))) if has_local else nn.Identity(),
                Residual(PreNorm(dim, GlobalAttention(dim, heads=heads, dim_head=dim_head, dropout=dropout, k=global_k, robust=robust))),
                Residual(PreNorm(dim, FeedForward(dim, mlp_mult, dropout=dropout)))]))

    def _check(self, x: Tensor, g: int) -> None:
        E.require_run(x, "Twins-SVT")
        if self.training and self.p > 0:
            raise NotImplementedError("dropout > 0 in training is not implemented for Twins-SVT (eval mode runs)")
        for la, _, ga, _ in self.layers:
            if isinstance(la, Residual) and g % la.fn.fn.patch_size:
                raise NotImplementedError(f"a {g} x {g} map is not tiled by local windows of {la.fn.fn.patch_size}")
            if g % ga.fn.fn.k:
                raise NotImplementedError(f"a {g} x {g} map is not tiled by the global k of {ga.fn.fn.k}")

    @staticmethod
    def _ff(x: Tensor, res: Residual) -> Tensor:
        pre = res.fn
        n0, n3 = pre.fn.net[0], pre.fn.net[3]
        return FeedForwardFn.apply(x, float(pre.norm.eps), pre.norm.g, pre.norm.b, n0.weight, n0.bias, n3.weight, n3.bias)

    def run(self, x: Tensor, B: int, g: int) -> Tensor:
        """fp32 stream [B*g*g, dim] -> the same shape."""
        self._check(x, g)
        for la, ff1, ga, ff2 in self.layers:
            if isinstance(la, Residual):
                pre, a = la.fn, la.fn.fn
                cfg = (B, g, a.heads, a.dim_head, a.patch_size, a.robust, float(pre.norm.eps))
                x = LocalAttnFn.apply(x, cfg, pre.norm.g, pre.norm.b, a.to_q.weight, a.to_kv.weight, a.to_out[0].weight, a.to_out[0].bias)
                x = self._ff(x, ff1)
            pre, a = ga.fn, ga.fn.fn
            cfg = (B, g, a.heads, a.dim_head, a.k, a.robust, float(pre.norm.eps))
            x = GlobalAttnFn.apply(x, cfg, pre.norm.g, pre.norm.b, a.to_q.weight, a.to_kv.weight, a.to_out[0].weight, a.to_out[0].bias)
            x = self._ff(x, ff2)
        return x

    def forward(self, x):
        if x.dim() != 4 or x.shape[2] != x.shape[3]:
            raise NotImplementedError(f"Transformer takes a square map [B, dim, g, g], got {tuple(x.shape)}")
        B, C, g, _ = x.shape
        rows = x.to(torch.float32).permute(0, 2, 3, 1).reshape(B * g * g, C)
        return self.run(rows, B, g).reshape(B, g, g, C).permute(0, 3, 1, 2)


class TwinsSVT(nn.Module):
    """twins_svt.py:175-232 with the reference's constructor arguments, plus `robust` (see the module docstring)."""

    def __init__(
        self,
        *,
        num_classes,
        s1_emb_dim=64,
        s1_patch_size=4,
        s1_local_patch_size=7,
        s1_global_k=7,
        s1_depth=1,
        s2_emb_dim=128,
        s2_patch_size=2,
        s2_local_patch_size=7,
        s2_global_k=7,
        s2_depth=1,
        s3_emb_dim=256,
        s3_patch_size=2,
        s3_local_patch_size=7,
        s3_global_k=7,
        s3_depth=5,
        s4_emb_dim=512,
        s4_patch_size=2,
        s4_local_patch_size=7,
        s4_global_k=7,
        s4_depth=4,
        peg_kernel_size=3,
        dropout=0.,
        robust=False
    ):
        super().__init__()
        kwargs = dict(locals())

        dim = 3
        layers = []

        for prefix in ('s1', 's2', 's3', 's4'):
            config, kwargs = group_by_key_prefix_and_remove_prefix(f'{prefix}_', kwargs)
            is_last = prefix == 's4'

            dim_next = config['emb_dim']

            layers.append(nn.Sequential(
                PatchEmbedding(dim=dim, dim_out=dim_next, patch_size=config['patch_size']),
                Transformer(dim=dim_next, depth=1, local_patch_size=config['local_patch_size'], global_k=config['global_k'],
                            dropout=dropout, has_local=not is_last, robust=robust),
                PEG(dim=dim_next, kernel_size=peg_kernel_size),
                Transformer(dim=dim_next, depth=config['depth'], local_patch_size=config['local_patch_size'],
                            global_k=config['global_k'], dropout=dropout, has_local=not is_last, robust=robust)
            ))

            dim = dim_next

        self.dropout_p = dropout
        self.layers = nn.Sequential(
            *layers,
            nn.AdaptiveAvgPool2d(1),
            E.Rearrange('... () () -> ...'),
            nn.Linear(dim, num_classes)
        )

    def grad_groups(self):
        return []

    def forward(self, x):
        E.require_run(x, "Twins-SVT")
        if self.training and self.dropout_p > 0:
            raise NotImplementedError("dropout > 0 in training is not implemented for Twins-SVT (eval mode runs)")
        if x.dim() != 4 or x.shape[2] != x.shape[3]:
            raise NotImplementedError(f"Twins-SVT takes square [B, C, S, S] images, got {tuple(x.shape)}")
        if x.requires_grad:
            raise E.NrvError("gradient w.r.t. the input image is not part of this hot path")
        B, C, G, _ = x.shape
        src, rows = x, False
        for stage in list(self.layers)[:4]:
            embed, t1, peg, t2 = stage
            p = embed.patch_size
            if G % p or C != embed.dim:
                raise NotImplementedError(f"a {G} x {G} map with {C} channels is not tiled by patches of {p} with {embed.dim} channels")
            g = G // p
            t1._check(x, g)
            t2._check(x, g)
            src = PatchEmbedFn.apply(src, embed.proj.weight, embed.proj.bias, B, C, G, p, rows)
            src = t1.run(src, B, g)
            conv = peg.proj.fn
            src = PegFn.apply(src, conv.weight, conv.bias, B, g)
            src = t2.run(src, B, g)
            rows, C, G = True, embed.dim_out, g
        pooled = src.reshape(B, G * G, C).mean(dim=1)                    # AdaptiveAvgPool2d(1) on token rows: B * C elements
        return self.layers[6](pooled)
