"""Pooling-based Vision Transformer (`PiT`) on the HIP path: drop-in for the reference's pit.py.

    from noise_robust_vit_amd.pit import PiT          # was: from vit_pytorch_robust.pit import PiT
    model = PiT(image_size=224, patch_size=14, num_classes=1000, dim=64, depth=(2, 6, 4), heads=(2, 4, 8), mlp_dim=256, robust=True).cuda()

Same keyword-only constructor, module tree, state_dict keys (`to_patch_embedding.2.*`, `pos_embedding`, `cls_token`,
`layers.{2s}.layers.i.0.{norm.*, fn.{to_qkv.weight, to_out.0.*}}`, `layers.{2s}.layers.i.1.{norm.*, fn.net.{0,3}.*}`,
`layers.{2s+1}.{downsample.net.{0,1}.*, cls_ff.*}`, `mlp_head.{0,1}.*`) and parameter draw order as pit.py:121-173, so seeded
models and reference checkpoints are interchangeable.  One added keyword on `PiT` and `Transformer`, `robust=False`, selects
SinkhornAttention's normalisation (utils.py:1025-1037) instead of softmax in every stage, as in the CaiT, T2T-ViT and RvT ports.

The step on the fp32 stream x [B, 1 + g*g, dim], class token in row 0:

    PatchEmbedFn : nrv_unfold_patches (nn.Unfold(p, p // 2): overlapping patches, (c, ky, kx) features padded to 8) -> NT GEMM
                   with the bias + positional-table epilogue into rows 1.. of every sample; row 0 = cls_token + pos[0]
    per stage    : encoder.EncoderStackFn on the stage's twelve-parameter layers (packed to_qkv without bias); the token counts
                   shrink stage by stage, so one model crosses the streaming and the single-pass attention kernels
    PoolFn       : nrv_pool_dwconv_fwd (Conv2d(C, 2C, 3, stride 2, padding 1, groups = C) on the patch rows) -> the 1 x 1
                   convolution as an NT GEMM with bias into rows 1.. of the new [B, 1 + go*go, 2C] stream; cls_ff as a small
                   GEMM on the B class rows into row 0
    mlp_head     : LayerNorm + Linear on the B class rows (torch; B * dim elements)

The backward mirrors it: every Linear / 1 x 1 weight gradient on the TN GEMM, the taps' and the conv bias' gradients and the
input gradient from nrv_pool_dwconv_bwd, dpos / dcls / the embedding's dbias from one column sum.

Refused with NotImplementedError (nothing is approximated): dropout / emb_dropout > 0 in training, attention recording,
non-square images, an image whose token count differs from the positional table, a token grid that is not square at a stage,
heads == 1 with dim_head == dim (the reference's to_out = Identity branch), dim / heads * dim_head / mlp_dim that are not
multiples of 8, and a direct call of Attention / FeedForward / PreNorm / DepthWiseConv2d (they hold the parameters; a stage and
a Pool run as a whole).  CPU tensors raise NrvError.
"""
from __future__ import annotations

from math import isqrt

import torch
from torch import nn

from . import encoder as E
from . import kernels as K
from ._lib import EPI_BIAS_RESIDUAL
from .encoder import WEIGHTS

Tensor = torch.Tensor

__all__ = ["PiT", "Transformer", "Attention", "FeedForward", "PreNorm", "Pool", "DepthWiseConv2d", "cast_tuple", "conv_output_size"]


def cast_tuple(val, num):
    return val if isinstance(val, tuple) else (val,) * num


def conv_output_size(image_size, kernel_size, stride, padding=0):
    return int(((image_size - kernel_size + (2 * padding)) / stride) + 1)


# ----------------------------------------------------------------------------------------------
# modules (parameter holders with the reference's names and construction order)
# ----------------------------------------------------------------------------------------------
PreNorm, FeedForward = E.PreNorm, E.FeedForward


class Attention(E.Holder):
    def __init__(self, dim, heads=8, dim_head=64, dropout=0.):
        super().__init__()
        inner_dim = dim_head * heads
        if heads == 1 and dim_head == dim:
            raise NotImplementedError("heads == 1 with dim_head == dim (to_out = Identity in the reference) is not implemented")
        if dim % 8 or inner_dim % 8 or dim > 4096:
            raise NotImplementedError(f"Attention dim {dim}, heads * dim_head {inner_dim}: the kernels take multiples of 8 and LayerNorm "
                                      "at most 4096 features")
        self.heads = heads
        self.dim_head = dim_head
        self.scale = dim_head ** -0.5
        self.attend = nn.Softmax(dim=-1)
        self.dropout = nn.Dropout(dropout)
        self.to_qkv = nn.Linear(dim, inner_dim * 3, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner_dim, dim), nn.Dropout(dropout))


class DepthWiseConv2d(E.Holder):
    def __init__(self, dim_in, dim_out, kernel_size, padding, stride, bias=True):
        super().__init__()
        if kernel_size != 3 or stride != 2 or padding != 1 or not bias or dim_out != 2 * dim_in:
            raise NotImplementedError("DepthWiseConv2d: the Pool layer's 3 x 3, stride 2, padding 1, dim_out = 2 * dim_in with bias is implemented")
        self.net = nn.Sequential(
            nn.Conv2d(dim_in, dim_out, kernel_size=kernel_size, padding=padding, groups=dim_in, stride=stride, bias=bias),
            nn.Conv2d(dim_out, dim_out, kernel_size=1, bias=bias))


def _check_stream(x, what: str) -> int:
    """The side of the square token grid of x [B, 1 + g*g, dim]."""
    E.require_run(x, "PiT")
    g = isqrt(max(x.shape[1] - 1, 0)) if x.dim() == 3 else 0
    if x.dim() != 3 or g < 1 or x.shape[1] != 1 + g * g:
        raise NotImplementedError(f"{what} takes x [B, 1 + g*g, dim] on a square g x g token grid, got {tuple(x.shape)}")
    return g


class Transformer(nn.Module):
    """pit.py:73-86: depth pre-norm blocks, run as one encoder.EncoderStackFn.  forward(x [B, N, dim]) on the HIP device."""

    def __init__(self, dim, depth, heads, dim_head, mlp_dim, dropout=0., robust=False):
        super().__init__()
        self.layers = nn.ModuleList([])
        self.p = dropout
        for _ in range(depth):
            self.layers.append(nn.ModuleList([
                PreNorm(dim, Attention(dim, heads=heads, dim_head=dim_head, dropout=dropout)),
                PreNorm(dim, FeedForward(dim, mlp_dim, dropout=dropout))]))
        self._meta = E.BlockMeta(heads=heads, dim_head=dim_head, eps=1e-5, robust=bool(robust))

    def layer_params(self) -> list:
        flat = []
        for attn, ff in self.layers:
            a, f = attn.fn, ff.fn
            flat += [attn.norm.weight, attn.norm.bias, a.to_qkv.weight, None, a.to_out[0].weight, a.to_out[0].bias,
                     ff.norm.weight, ff.norm.bias, f.net[0].weight, f.net[0].bias, f.net[3].weight, f.net[3].bias]
        return flat

    def forward(self, x):
        _check_stream(x, "Transformer")
        if self.training and self.p > 0:
            raise NotImplementedError("dropout > 0 in training is not implemented for PiT (eval mode runs)")
        if not self.layers:
            return x
        self._meta.eps = float(self.layers[0][0].norm.eps)
        self._meta.dropout = self._meta.attn_dropout = 0.0
        return E.EncoderStackFn.apply(x, self._meta, *self.layer_params())


class PoolFn(torch.autograd.Function):
    """pit.py:102-117 on x fp32 [B, 1 + g*g, C] -> [B, 1 + go*go, 2C], go = (g - 1) // 2 + 1."""

    @staticmethod
    def forward(ctx, x, g: int, wdw, bdw, wpw, bpw, wcls, bcls):
        B, N, C = x.shape
        x2 = x.detach().to(torch.float32).contiguous().reshape(B * N, C)
        go = K.pool_out_size(g)
        S = 1 + go * go
        conv = K.pool_dwconv_fwd(x2, wdw.detach(), bdw.detach(), B, g, g, 1)
        out = torch.empty(B * S, 2 * C, dtype=torch.float32, device=x.device)
        # the output row remap rides on the bias + table epilogue of the patch embedding; a Pool has no table: it adds exact zeros
        nopos = E.cached("pit.nopos", torch.zeros, go * go, 2 * C, device=x.device)
        K.gemm_nt(conv, WEIGHTS.get(wpw, True)[0], epilogue=EPI_BIAS_RESIDUAL, bias=bpw.detach(), aux=nopos, aux_row_mod=go * go, out=out,
                  out_group=go * go, out_group_stride=S, out_row_offset=1)
        xc = K.cast_bf16(x2.view(B, N, C)[:, 0].contiguous())             # the B class rows: not the hot path
        out.view(B, S, 2 * C)[:, 0] = E.linear(xc, wcls, bcls, torch.float32)
        ctx.saved = (x2, conv, xc)
        ctx.cfg = (B, g, go, C)
        ctx.params = (wdw, wpw, wcls)
        return out.reshape(B, S, 2 * C)

    @staticmethod
    def backward(ctx, dy):
        x2, conv, xc = ctx.saved
        B, g, go, C = ctx.cfg
        wdw, wpw, wcls = ctx.params
        ctx.saved = None
        S = 1 + go * go
        d16 = K.cast_bf16(dy.to(torch.float32).contiguous().reshape(B * S, 2 * C)).view(B, S, 2 * C)
        dp = d16[:, 1:].reshape(B * go * go, 2 * C)                        # dense patch rows (one bf16 copy)
        dc = d16[:, 0].contiguous()
        dpw, dbpw = K.gemm_tn(dp, conv, want_dbias=True)
        dconv = K.gemm_nt(dp, WEIGHTS.get(wpw, True)[1], out_dtype=torch.bfloat16)
        dx, ddw, dbdw = K.pool_dwconv_bwd(x2, wdw.detach(), dconv, B, g, g, 1)     # the class rows of dx come back as zeros
        dcls, dbcls = K.gemm_tn(dc, xc, want_dbias=True)
        dx.view(B, 1 + g * g, C)[:, 0] = K.gemm_nt(dc, WEIGHTS.get(wcls, True)[1], out_dtype=torch.float32)
        return dx.reshape(B, 1 + g * g, C), None, ddw, dbdw, dpw.reshape(wpw.shape), dbpw, dcls, dbcls


class Pool(nn.Module):
    """pit.py:102-117.  forward(x [B, 1 + g*g, dim]) -> [B, 1 + go*go, 2 * dim] on the HIP device."""

    def __init__(self, dim):
        super().__init__()
        if dim % 8:
            raise NotImplementedError(f"Pool dim {dim}: the kernels take multiples of 8")
        self.downsample = DepthWiseConv2d(dim, dim * 2, kernel_size=3, stride=2, padding=1)
        self.cls_ff = nn.Linear(dim, dim * 2)

    def forward(self, x):
        g = _check_stream(x, "Pool")
        dw, pw = self.downsample.net
        return PoolFn.apply(x, g, dw.weight, dw.bias, pw.weight, pw.bias, self.cls_ff.weight, self.cls_ff.bias)


# ----------------------------------------------------------------------------------------------
# patch embedding
# ----------------------------------------------------------------------------------------------
class PatchEmbedFn(torch.autograd.Function):
    """nn.Unfold(ks, stride) + Linear + class token + positional table (pit.py:144-148, 176-181), written straight into the
    fp32 stream [B, 1 + n, D].  The image takes no gradient."""

    @staticmethod
    def forward(ctx, img, weight, bias, pos, cls_token, ks: int, stride: int):
        if img.requires_grad:
            raise E.NrvError("gradient w.r.t. the input image is not part of this hot path")
        Bn = img.shape[0]
        D, F = weight.shape
        cols = K.unfold_patches(img.detach().contiguous(), ks, stride)
        n, FP = cols.shape[0] // Bn, cols.shape[1]
        wb, _ = E.padded_images(weight, FP, False)                         # 3 * 14 * 14 = 588 features ride as 592
        S = n + 1
        pos2 = pos.detach().reshape(-1, D).to(torch.float32)
        out = torch.empty(Bn * S, D, dtype=torch.float32, device=img.device)
        K.gemm_nt(cols, wb, epilogue=EPI_BIAS_RESIDUAL, bias=bias.detach(), aux=pos2[1:], aux_row_mod=n, out=out, out_group=n,
                  out_group_stride=S, out_row_offset=1)
        out.view(Bn, S, D)[:, 0] = cls_token.detach().reshape(D) + pos2[0]          # B * D elements: not the hot path
        ctx.saved = cols
        ctx.cfg = (Bn, n, S, D, F, pos.shape, weight.shape)
        return out.reshape(Bn, S, D)

    @staticmethod
    def backward(ctx, dy):
        cols = ctx.saved
        Bn, n, S, D, F, pos_shape, wshape = ctx.cfg
        ctx.saved = None
        d16 = K.cast_bf16(dy.to(torch.float32).contiguous().reshape(Bn * S, D))
        dw = K.gemm_tn(d16, cols, a_group=n, a_group_stride=S, a_row_offset=1, T=Bn * n)
        if cols.shape[1] != F:
            dw = dw[:, :F].contiguous()                                        # the zero-padded feature columns are dropped
        dsum = K.colsum(d16.reshape(Bn, S * D)).reshape(S, D)                 # dy summed over the batch
        return None, dw.reshape(wshape), dsum[1:].sum(0), dsum.reshape(pos_shape), dsum[0].reshape(1, 1, D), None, None


class PiT(nn.Module):
    """pit.py:121-186 with the reference's constructor arguments, plus `robust` (see the module docstring)."""

    def __init__(self, *, image_size, patch_size, num_classes, dim, depth, heads, mlp_dim, dim_head=64, dropout=0., emb_dropout=0.,
                 channels=3, robust=False):
        super().__init__()
        if isinstance(image_size, (tuple, list)):
            if len(image_size) != 2 or image_size[0] != image_size[1]:
                raise NotImplementedError("PiT takes square images only")
            image_size = image_size[0]
        assert image_size % patch_size == 0, 'Image dimensions must be divisible by the patch size.'
        assert isinstance(depth, tuple), 'depth must be a tuple of integers, specifying the number of blocks before each downsizing'
        heads = cast_tuple(heads, len(depth))
        if mlp_dim % 8 or not 2 <= patch_size <= 32:
            raise NotImplementedError(f"mlp_dim {mlp_dim} / patch_size {patch_size}: the kernels take mlp_dim % 8 == 0 and patches of 2 .. 32")
        patch_dim = channels * patch_size ** 2
        self.image_size = image_size
        self.patch_size = patch_size
        self.emb_dropout = emb_dropout
        self.to_patch_embedding = nn.Sequential(nn.Unfold(kernel_size=patch_size, stride=patch_size // 2), E.Rearrange('b c n -> b n c'),
                                                nn.Linear(patch_dim, dim))
        output_size = conv_output_size(image_size, patch_size, patch_size // 2)
        num_patches = output_size ** 2
        self.pos_embedding = nn.Parameter(torch.randn(1, num_patches + 1, dim))
        self.cls_token = nn.Parameter(torch.randn(1, 1, dim))
        self.dropout = nn.Dropout(emb_dropout)
        layers = []
        for ind, (layer_depth, layer_heads) in enumerate(zip(depth, heads)):
            not_last = ind < (len(depth) - 1)
            layers.append(Transformer(dim, layer_depth, layer_heads, dim_head, mlp_dim, dropout, robust=robust))
            if not_last:
                layers.append(Pool(dim))
                dim *= 2
        self.layers = nn.Sequential(*layers)
        self.mlp_head = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, num_classes))

    def grad_groups(self):
        return []

    def forward(self, img):
        E.require_cuda(img)
        if self.training and (self.emb_dropout > 0 or any(getattr(m, "p", 0.) > 0 for m in self.layers)):
            raise NotImplementedError("dropout / emb_dropout > 0 in training is not implemented for PiT (eval mode runs)")
        E.refuse_recording("PiT")
        p = self.patch_size
        if img.dim() != 4 or img.shape[2] != img.shape[3] or img.shape[2] < p:
            raise NotImplementedError(f"PiT takes square [B, C, S, S] images, got {tuple(img.shape)}")
        g = (img.shape[2] - p) // (p // 2) + 1
        if 1 + g * g != self.pos_embedding.shape[1]:
            raise NotImplementedError(f"a {img.shape[2]} px image gives {g * g} patches + class token, the positional table has "
                                      f"{self.pos_embedding.shape[1]} rows")
        lin = self.to_patch_embedding[2]
        if img.shape[1] * p * p != lin.in_features:
            raise NotImplementedError(f"{img.shape[1]} channels: the projection takes {lin.in_features} features")
        x = PatchEmbedFn.apply(img, lin.weight, lin.bias, self.pos_embedding, self.cls_token, p, p // 2)
        x = self.layers(x)
        return self.mlp_head(x[:, 0])
