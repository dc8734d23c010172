"""Rotary Vision Transformer (`RvT`) on the HIP path: drop-in for the reference's rvt.py.

    from noise_robust_vit_amd.rvt import RvT          # was: from vit_pytorch_robust.rvt import RvT
    model = RvT(image_size=224, patch_size=16, num_classes=100, dim=384, depth=12, heads=6, mlp_dim=768, robust=True).cuda()

Same keyword-only constructor, module tree, state_dict keys (`to_patch_embedding.1.*`, `cls_token`, `transformer.pos_emb.scales`,
`transformer.layers.i.0.{norm.*, fn.{to_q.conv.net.{0,1}.weight, to_q.cls_proj.*, to_kv.weight, to_out.0.*}}`,
`transformer.layers.i.1.{norm.*, fn.net.{0,3}.*}`, `mlp_head.{0,1}.*`) and parameter draw order as rvt.py:178-211, so seeded
models and reference checkpoints are interchangeable.  One added keyword on `RvT` and `Transformer`, `robust=False`, selects
SinkhornAttention's normalisation (utils.py:1025-1037) instead of softmax, as in the CaiT and T2T-ViT ports.

One autograd node per layer (LayerFn) on the fp32 stream x [B*N, dim], N = 1 + g*g tokens with the class token in row 0:

    LN -> to_kv GEMM into columns [inner, 3*inner) of the packed qkv
       -> use_ds_conv: nrv_dwconv_fwd (5 x 5, lead = 1) on the normalised rows, the 1 x 1 conv as an NT GEMM into columns
          [0, inner); the class rows get cls_proj (a GEMM on a strided [B, dim] view) or, for Identity, a copy of the
          normalised class row;  else [to_q; to_kv] is one cached weight image and one GEMM (lucid_vit.Attention's)
       -> nrv_rotary_fwd in place (q and k, patch rows only) -> nrv_attn_fwd | nrv_attn_sinkhorn_fwd | the composed path
       -> to_out GEMM with the residual epilogue
    LN -> fc1 GEMM (bias) -> nrv_geglu_fwd -> fc2 GEMM with the residual epilogue        (use_glu=False: encoder.mlp_half_*)

The backward mirrors it: nrv_rotary_bwd on dqkv before any projection gradient, the depthwise taps' gradient from
nrv_dwconv_bwd, every Linear / 1 x 1 weight gradient on the TN GEMM.  The rotary tables are plumbing: torch computes them once
per (grid, dim_head, max_freq), exactly as AxialRotaryEmbedding.forward does.  q and k are rounded to bf16 by the GEMM and once
more after the rotation.

Refused with NotImplementedError (nothing is approximated): dropout / emb_dropout > 0 in training, attention recording,
non-square images or token grids, dim / heads * dim_head / mlp_dim / dim_head that are not multiples of 8, and a direct call of
Attention / FeedForward / GEGLU / SpatialConv / DepthWiseConv2d / PreNorm (they hold the parameters; a layer runs as a whole).
CPU tensors raise NrvError.
"""
from __future__ import annotations

from math import pi, sqrt

import torch
from torch import nn

from . import encoder as E
from . import kernels as K
from ._lib import EPI_BIAS_RESIDUAL, PATCH_P1P2C
from .encoder import WEIGHTS
from .lucid_vit import Attention as _LucidAttention
from .lucid_vit import _FusedRowsFn

Tensor = torch.Tensor

__all__ = ["RvT", "Transformer", "Attention", "FeedForward", "GEGLU", "SpatialConv", "DepthWiseConv2d", "PreNorm",
           "AxialRotaryEmbedding", "rotate_every_two"]

_LD_LIMIT = (1 << 31) // 1280            # the NT GEMM's epilogue addresses 320 fp32 rows of ldc with 32-bit byte offsets


# ----------------------------------------------------------------------------------------------
# rotary embeddings (rvt.py:12-44): torch, on whatever device the input lives
# ----------------------------------------------------------------------------------------------
def rotate_every_two(x):
    x1, x2 = x.reshape(*x.shape[:-1], -1, 2).unbind(dim=-1)
    return torch.stack((-x2, x1), dim=-1).reshape(x.shape)


def _axial_tables(n: int, dim: int, max_freq: float):
    """(sin, cos) fp32 [n*n, 2 * (dim // 4)]: entry (i*n + j, m) belongs to the feature pair (2m, 2m + 1); the row coordinate i
    drives the first dim // 4 frequencies, the column coordinate j the second dim // 4."""
    scales = torch.linspace(1., max_freq / 2, dim // 4)
    seq = torch.linspace(-1., 1., steps=n).unsqueeze(-1) * scales * pi
    x_sinu = seq.unsqueeze(1).expand(n, n, -1)
    y_sinu = seq.unsqueeze(0).expand(n, n, -1)
    sin = torch.cat((x_sinu.sin(), y_sinu.sin()), dim=-1).reshape(n * n, -1)
    cos = torch.cat((x_sinu.cos(), y_sinu.cos()), dim=-1).reshape(n * n, -1)
    return sin.contiguous(), cos.contiguous()


class AxialRotaryEmbedding(nn.Module):
    def __init__(self, dim, max_freq=10):
        super().__init__()
        self.dim = dim
        self.max_freq = max_freq
        self.register_buffer('scales', torch.linspace(1., max_freq / 2, self.dim // 4))

    def forward(self, x):
        """(sin, cos), each [1, n*n, 4 * (dim // 4)] with every table entry repeated for its pair, n = int(sqrt(tokens))."""
        n = int(sqrt(x.shape[-2]))
        seq = torch.linspace(-1., 1., steps=n, device=x.device).unsqueeze(-1) * self.scales.to(x) * pi
        x_sinu = seq.unsqueeze(1).expand(n, n, -1)
        y_sinu = seq.unsqueeze(0).expand(n, n, -1)
        sin = torch.cat((x_sinu.sin(), y_sinu.sin()), dim=-1).reshape(n * n, -1)
        cos = torch.cat((x_sinu.cos(), y_sinu.cos()), dim=-1).reshape(n * n, -1)
        return sin.repeat_interleave(2, dim=-1)[None], cos.repeat_interleave(2, dim=-1)[None]

    def tables(self, n: int, device):
        """The unrepeated fp32 tables [n*n, dr / 2] of nrv_rotary_*, built once per (grid, dim, max_freq, device)."""
        sin = E.cached("rvt.sin", lambda *a: _axial_tables(*a)[0], n, self.dim, float(self.max_freq), device=device)
        cos = E.cached("rvt.cos", lambda *a: _axial_tables(*a)[1], n, self.dim, float(self.max_freq), device=device)
        return sin, cos


# ----------------------------------------------------------------------------------------------
# modules (parameter holders with the reference's names and construction order)
# ----------------------------------------------------------------------------------------------
class DepthWiseConv2d(E.Holder):
    def __init__(self, dim_in, dim_out, kernel_size, padding, stride=1, bias=True):
        super().__init__()
        if stride != 1 or bias or padding != kernel_size // 2 or kernel_size not in (3, 5, 7):
            raise NotImplementedError("DepthWiseConv2d: kernel 3 / 5 / 7 with stride 1, padding kernel // 2 and no bias is implemented")
        self.net = nn.Sequential(
            nn.Conv2d(dim_in, dim_in, kernel_size=kernel_size, padding=padding, groups=dim_in, stride=stride, bias=bias),
            nn.Conv2d(dim_in, dim_out, kernel_size=1, bias=bias))


PreNorm = E.PreNorm


class SpatialConv(E.Holder):
    def __init__(self, dim_in, dim_out, kernel, bias=False):
        super().__init__()
        self.conv = DepthWiseConv2d(dim_in, dim_out, kernel, padding=kernel // 2, bias=False)
        self.cls_proj = nn.Linear(dim_in, dim_out) if dim_in != dim_out else nn.Identity()


class GEGLU(E.Holder):
    pass


class FeedForward(E.Holder):
    def __init__(self, dim, hidden_dim, dropout=0., use_glu=True):
        super().__init__()
        if dim % 8 or hidden_dim % 8:
            raise NotImplementedError(f"FeedForward {dim} -> {hidden_dim}: the kernels take multiples of 8")
        self.use_glu = bool(use_glu)
        self.net = nn.Sequential(nn.Linear(dim, hidden_dim * 2 if use_glu else hidden_dim), GEGLU() if use_glu else nn.GELU(),
                                 nn.Dropout(dropout), nn.Linear(hidden_dim, dim), nn.Dropout(dropout))


class Attention(E.Holder):
    def __init__(self, dim, heads=8, dim_head=64, dropout=0., use_rotary=True, use_ds_conv=True, conv_query_kernel=5):
        super().__init__()
        inner_dim = dim_head * heads
        if dim % 8 or inner_dim % 8 or dim_head % 8 or dim > 4096:
            raise NotImplementedError(f"Attention dim {dim}, heads * dim_head {inner_dim}, dim_head {dim_head}: the kernels take "
                                      "multiples of 8 and LayerNorm at most 4096 features")
        self.use_rotary = use_rotary
        self.heads = heads
        self.dim_head = dim_head
        self.scale = dim_head ** -0.5
        self.attend = nn.Softmax(dim=-1)
        self.dropout = nn.Dropout(dropout)
        self.use_ds_conv = use_ds_conv
        self.to_q = SpatialConv(dim, inner_dim, conv_query_kernel, bias=False) if use_ds_conv else nn.Linear(dim, inner_dim, bias=False)
        self.to_kv = nn.Linear(dim, inner_dim * 2, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner_dim, dim), nn.Dropout(dropout))
        self._fused = None               # use_ds_conv=False: the persistent [to_q.weight; to_kv.weight] of lucid_vit.Attention
        self._fused_key = None
        if not use_ds_conv:
            WEIGHTS.add_derived(self._refresh_fused)

    _refresh_fused = _LucidAttention._refresh_fused


# ----------------------------------------------------------------------------------------------
# the layer
# ----------------------------------------------------------------------------------------------
def _cls_rows(t: Tensor, B: int, N: int, cols: int) -> Tensor:
    """The class rows of t [B*N, ld] as a strided [B, cols] view of its first `cols` columns."""
    return t.view(B, N, t.shape[1])[:, 0, :cols]


def _attention_kind(dh: int, robust: bool) -> str:
    if robust:
        return "sinkhorn"
    return "softmax" if dh in K.ATTN_FUSED_DH else "composed"


class LayerFn(torch.autograd.Function):
    """One layer (rvt.py:168-174): x1 = x + attn(LN x), x2 = x1 + ff(LN x1), x fp32 [B*N, D].
    cfg = (B, g, H, dh, robust, use_rotary, use_glu, eps1, eps2); wq is the fused [to_q; to_kv] image when there is no conv
    (wkv is then None); sin / cos None without rotary."""

    @staticmethod
    def forward(ctx, x, cfg, sin, cos, n1w, n1b, wdw, wpw, wcls, bcls, wq, wkv, wo, bo, n2w, n2b, w1, b1, w2, b2):
        B, g, H, dh, robust, use_rotary, use_glu, eps1, eps2 = cfg
        x = x.detach().contiguous()
        N, inner, D = 1 + g * g, H * dh, x.shape[1]
        scale = dh ** -0.5
        xn, mean, rstd = K.layernorm_fwd(x, n1w.detach(), n1b.detach(), eps1)
        conv = None
        if wdw is not None:
            qkv = torch.empty(B * N, 3 * inner, dtype=torch.bfloat16, device=x.device)
            K.gemm_nt(xn, WEIGHTS.get(wkv, True)[0], out=qkv[:, inner:])
            conv = K.dwconv_fwd(xn, wdw.detach(), B, g, g, 1)
            K.gemm_nt(conv, WEIGHTS.get(wpw, True)[0], out=qkv[:, :inner])
            strided = N * max(3 * inner, D) < _LD_LIMIT
            q_cls, xn_cls = _cls_rows(qkv, B, N, inner), _cls_rows(xn, B, N, D)
            if wcls is None:
                q_cls.copy_(xn_cls)                                        # Identity: dim == inner, a copy of bf16 rows
            elif strided:
                K.gemm_nt(xn_cls, WEIGHTS.get(wcls, True)[0], out=q_cls, epilogue=E.EPI_BIAS, bias=bcls.detach())
            else:
                q_cls.copy_(E.linear(xn_cls.contiguous(), wcls, bcls))
        else:
            qkv = K.gemm_nt(xn, WEIGHTS.get(wq, True)[0], out_dtype=torch.bfloat16)
        if use_rotary:
            K.rotary_fwd(qkv, sin, cos, B, N, 1, H, dh)
        kind = _attention_kind(dh, robust)
        if kind == "sinkhorn":
            p7 = {}
            o, lse, scal = K.attn_sinkhorn_fwd(qkv, B, N, H, dh, scale, saved=p7)
            att = (lse, scal, p7)
        elif kind == "softmax":
            o, att = K.attn_fwd(qkv, B, N, H, dh, scale)
        else:
            o, att = K.attn_composed_fwd(qkv, B, N, H, dh, scale, 0)
        x1 = K.gemm_nt(o, WEIGHTS.get(wo, True)[0], out_dtype=torch.float32, epilogue=EPI_BIAS_RESIDUAL, bias=bo.detach(), aux=x)
        need = any(ctx.needs_input_grad)
        if use_glu:
            xn2, mean2, rstd2 = K.layernorm_fwd(x1, n2w.detach(), n2b.detach(), eps2)
            u = E.linear(xn2, w1, b1)
            h = K.geglu_fwd(u, w2.shape[1])
            x2 = K.gemm_nt(h, WEIGHTS.get(w2, True)[0], out_dtype=torch.float32, epilogue=EPI_BIAS_RESIDUAL, bias=b2.detach(), aux=x1)
            mlp = (x1, xn2, mean2, rstd2, u, h)
        else:
            meta = E.BlockMeta(heads=H, dim_head=dh, eps=eps2)
            x2, mlp = E.mlp_half_fwd(x1, meta, n2w.detach(), n2b.detach(), w1, b1.detach(), w2, b2.detach(), True, save=need)
        ctx.cfg, ctx.kind = cfg, kind
        ctx.saved = (x, xn, mean, rstd, conv, qkv, o, att, mlp, sin, cos)
        ctx.params = (n1w, wdw, wpw, wcls, bcls, wq, wkv, wo, n2w, n2b, w1, b1, w2, b2)
        return x2

    @staticmethod
    def backward(ctx, dx2):
        B, g, H, dh, robust, use_rotary, use_glu, eps1, eps2 = ctx.cfg
        x, xn, mean, rstd, conv, qkv, o, att, mlp, sin, cos = ctx.saved
        n1w, wdw, wpw, wcls, bcls, wq, wkv, wo, n2w, n2b, w1, b1, w2, b2 = ctx.params
        ctx.saved = None
        N, inner, D = 1 + g * g, H * dh, x.shape[1]
        scale = dh ** -0.5
        dx2 = dx2.to(torch.float32).contiguous()
        # feed-forward half
        if use_glu:
            x1, xn2, mean2, rstd2, u, h = mlp
            d16 = K.cast_bf16(dx2)
            dw2, db2 = K.gemm_tn(d16, h, want_dbias=True)
            dh16 = E.dx_sum([(d16, w2)], torch.bfloat16)
            du = K.geglu_bwd(u, dh16)
            dw1, db1 = K.gemm_tn(du, xn2, want_dbias=True)
            dxn2 = E.dx_sum([(du, w1)], torch.bfloat16)
            dx1, dx1_16, dn2w, dn2b = K.layernorm_bwd(dxn2, x1, n2w.detach(), mean2, rstd2, dres=dx2, want_bf16=True)
        else:
            meta = E.BlockMeta(heads=H, dim_head=dh, eps=eps2)
            dx1, dx1_16, (dn2w, dn2b, dw1, db1, dw2, db2) = E.mlp_half_bwd(dx2, None, mlp, meta, n2w.detach(), n2b.detach(), w1, b1, w2, b2,
                                                                            True, want_bf16=True)
        # attention half
        dwo, dbo = K.gemm_tn(dx1_16, o, want_dbias=True)
        do = E.dx_sum([(dx1_16, wo)], torch.bfloat16)
        if ctx.kind == "sinkhorn":
            lse, scal, p7 = att
            dqkv = K.attn_sinkhorn_bwd(qkv, do, lse, scal, B, N, H, dh, scale, saved=p7)
        elif ctx.kind == "softmax":
            dqkv = K.attn_bwd(qkv, o, do, att, B, N, H, dh, scale)
        else:
            dqkv = K.attn_composed_bwd(qkv, do, att, B, N, H, dh, scale)
        if use_rotary:
            K.rotary_bwd(dqkv, sin, cos, B, N, 1, H, dh)
        ddw = dpw = dcls = dbcls = dq_w = dkv_w = None
        if wdw is not None:
            dq, dkv = dqkv[:, :inner], dqkv[:, inner:]
            dkv_w = K.gemm_tn(dkv, xn)
            dpw = K.gemm_tn(dq, conv).reshape(wpw.shape)                   # the class rows of `conv` are zeros
            dconv = E.dx_sum([(dq, wpw)], torch.bfloat16)
            da, ddw = K.dwconv_bwd(xn, wdw.detach(), dconv, B, g, g, 1)    # the class rows of da come back as zeros
            dq_cls, xn_cls, da_cls = _cls_rows(dqkv, B, N, inner), _cls_rows(xn, B, N, D), _cls_rows(da, B, N, D)
            if wcls is None:
                da_cls.copy_(dq_cls)
            else:
                strided = N * max(3 * inner, D) < _LD_LIMIT
                dq_c = dq_cls if strided else dq_cls.contiguous()
                xn_c = xn_cls if strided else xn_cls.contiguous()
                dcls, dbcls = K.gemm_tn(dq_c, xn_c, want_dbias=True)
                if strided:
                    K.gemm_nt(dq_c, WEIGHTS.get(wcls, True)[1], out=da_cls)
                else:
                    da_cls.copy_(E.dx_sum([(dq_c, wcls)], torch.bfloat16))
            # dxn = dkv Wkv + (the conv's input gradient | the class projection's)
            dxn = K.gemm_nt(dkv, WEIGHTS.get(wkv, True)[1], out_dtype=torch.bfloat16, epilogue=EPI_BIAS_RESIDUAL, aux=da)
        else:
            dq_w = K.gemm_tn(dqkv, xn)
            dxn = E.dx_sum([(dqkv, wq)], torch.bfloat16)
        dx, _, dn1w, dn1b = K.layernorm_bwd(dxn, x, n1w.detach(), mean, rstd, dres=dx1)
        return (dx, None, None, None, dn1w, dn1b, ddw, dpw, dcls, dbcls, dq_w, dkv_w, dwo, dbo, dn2w, dn2b, dw1, db1, dw2, db2)


class Transformer(nn.Module):
    """rvt.py:158-174.  forward(x [B, 1 + g*g, dim], fmap_dims={'h': g, 'w': g}) on the HIP device."""

    def __init__(self, dim, depth, heads, dim_head, mlp_dim, image_size, dropout=0., use_rotary=True, use_ds_conv=True, use_glu=True,
                 robust=False):
        super().__init__()
        if mlp_dim % 8:
            raise NotImplementedError(f"mlp_dim {mlp_dim}: the kernels take multiples of 8")
        self.layers = nn.ModuleList([])
        self.pos_emb = AxialRotaryEmbedding(dim_head, max_freq=image_size)
        self.robust = bool(robust)
        self.p = dropout
        for _ in range(depth):
            self.layers.append(nn.ModuleList([
                PreNorm(dim, Attention(dim, heads=heads, dim_head=dim_head, dropout=dropout, use_rotary=use_rotary, use_ds_conv=use_ds_conv)),
                PreNorm(dim, FeedForward(dim, mlp_dim, dropout=dropout, use_glu=use_glu))]))

    def grad_groups(self):
        """Without the conv, to_q / to_kv are the row blocks of one fused projection (lucid_vit.Transformer.grad_groups)."""
        return [(a.fn.to_q.weight, a.fn.to_kv.weight) for a, _ in self.layers if not a.fn.use_ds_conv]

    def _check(self, x, g: int) -> None:
        E.require_run(x, "RvT")
        if self.training and self.p > 0:
            raise NotImplementedError("dropout > 0 in training is not implemented for RvT (eval mode runs)")
        if x.dim() != 3 or x.shape[1] != 1 + g * g:
            raise NotImplementedError(f"Transformer takes x [B, 1 + g*g, dim] on a square g x g token grid, got {tuple(x.shape)}")

    def run(self, x: Tensor, B: int, g: int) -> Tensor:
        """x fp32 [B*(1 + g*g), D] -> the same shape"""
        for attn, ff in self.layers:
            a, f = attn.fn, ff.fn
            sin = cos = None
            if a.use_rotary and self.pos_emb.dim // 4 > 0:
                sin, cos = self.pos_emb.tables(g, x.device)
            cfg = (B, g, a.heads, a.dim_head, self.robust, sin is not None, f.use_glu, float(attn.norm.eps), float(ff.norm.eps))
            if a.use_ds_conv:
                lin = a.to_q.cls_proj
                cls = (lin.weight, lin.bias) if isinstance(lin, nn.Linear) else (None, None)
                qp = (a.to_q.conv.net[0].weight, a.to_q.conv.net[1].weight, *cls, None, a.to_kv.weight)
            else:
                qp = (None, None, None, None, _FusedRowsFn.apply(a, a.to_q.weight, a.to_kv.weight), None)
            x = LayerFn.apply(x, cfg, sin, cos, attn.norm.weight, attn.norm.bias, *qp, a.to_out[0].weight, a.to_out[0].bias,
                              ff.norm.weight, ff.norm.bias, f.net[0].weight, f.net[0].bias, f.net[3].weight, f.net[3].bias)
        return x

    def forward(self, x, fmap_dims):
        if fmap_dims['h'] != fmap_dims['w']:
            raise NotImplementedError(f"RvT takes square token grids, got {fmap_dims}")
        g = int(fmap_dims['h'])
        self._check(x, g)
        B, N, D = x.shape
        return self.run(x.to(torch.float32).contiguous().reshape(B * N, D), B, g).reshape(B, N, D)


class RvT(nn.Module):
    """rvt.py:178-211 with the reference's constructor arguments, plus `robust` (see the module docstring)."""

    def __init__(self, *, image_size, patch_size, num_classes, dim, depth, heads, mlp_dim, channels=3, dim_head=64, dropout=0.,
                 emb_dropout=0., use_rotary=True, use_ds_conv=True, use_glu=True, robust=False):
        super().__init__()
        if isinstance(image_size, (tuple, list)):
            if len(image_size) != 2 or image_size[0] != image_size[1]:
                raise NotImplementedError("RvT takes square images only")
            image_size = image_size[0]
        assert image_size % patch_size == 0, 'Image dimensions must be divisible by the patch size.'
        patch_dim = channels * patch_size ** 2
        self.patch_size = patch_size
        self.emb_dropout = emb_dropout
        self.to_patch_embedding = nn.Sequential(E.Rearrange('b c (h p1) (w p2) -> b (h w) (p1 p2 c)', p1=patch_size, p2=patch_size),
                                                nn.Linear(patch_dim, dim))
        self.cls_token = nn.Parameter(torch.randn(1, 1, dim))
        self.transformer = Transformer(dim, depth, heads, dim_head, mlp_dim, image_size, dropout, use_rotary, use_ds_conv, use_glu,
                                       robust=robust)
        self.mlp_head = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, num_classes))

    def grad_groups(self):
        return self.transformer.grad_groups()

    def forward(self, img):
        E.require_cuda(img)
        if self.training and self.emb_dropout > 0:
            raise NotImplementedError("emb_dropout > 0 in training is not implemented for RvT (eval mode runs)")
        p = self.patch_size
        if img.dim() != 4 or img.shape[2] != img.shape[3] or img.shape[2] % p:
            raise NotImplementedError(f"RvT takes square [B, C, S, S] images with S a multiple of {p}, got {tuple(img.shape)}")
        g = img.shape[2] // p
        t = self.transformer
        t._check(img.new_empty(0, 1 + g * g, 0), g)
        B, D = img.shape[0], self.cls_token.shape[-1]
        lin = self.to_patch_embedding[1]
        # patch embedding and the class token as in lucid_vit.ViT; RvT has no positional table: the epilogue adds exact zeros
        nopos = E.cached("rvt.nopos", torch.zeros, 1, 1 + g * g, D, device=img.device)
        x = E.PatchEmbedFn.apply(img, lin.weight, lin.bias, nopos, self.cls_token, p, PATCH_P1P2C, None)
        x = t.run(x.reshape(B * (1 + g * g), D), B, g).reshape(B, 1 + g * g, D)
        return self.mlp_head(x[:, 0])
