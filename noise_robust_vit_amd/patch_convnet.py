"""PatchConvNet on the HIP hot path: drop-in for the reference's patch_convnet.S60 / S120 / B60 / B120 / L60 / L120.

    from noise_robust_vit_amd import patch_convnet    # was: from vit_pytorch_robust import patch_convnet
    model = patch_convnet.S60(num_classes=100).cuda()

The modules take the reference's constructor arguments and hold the same parameters under the same names (patch_embed.proj.*,
blocks.i.{norm1, attn.qkv_pos.*, gamma_1}, blocks_token_only.0.*, cls_token, norm, head), drawn from the RNG in the same
order, so seeded models and reference checkpoints are interchangeable.  The arithmetic runs through libnrv_hip.so on
token-major rows [B*H*W, C] (the reference's NCHW view of them, patch_convnet.py:239-243, needs no copy):

    ConvStem        4 x (nrv_conv_unfold + NT GEMM), GELU between them in the GEMM epilogue (zero bias, bf16 gelu' stream);
                    backward: TN GEMM (dW), NT GEMM + nrv_conv_fold + nrv_dgelu_rows (dX)          (patch_convnet.py:268-305)
    conv block      LN -> 1x1 conv GEMM + bias + GELU (8-bit gelu' stream) -> nrv_dwconv3x3_fwd (+ GELU, + the SE squeeze)
                    -> nrv_se_fwd -> nrv_se_apply -> 1x1 conv GEMM + bias (fp32) -> nrv_ls_add_f32 (gamma_1, drop path)
                                                                                                   (patch_convnet.py:221-265)
    token block     LN of the class rows and of the patch rows -> q (class rows only), k, v GEMMs -> nrv_cls_attn_* with the
                    class and patch keys as two sources (the cat of :215 is never formed) -> proj -> nrv_ls_add_f32 -> LN ->
                    fc1 + GELU -> fc2 -> nrv_ls_add_f32, all on B rows                              (patch_convnet.py:154-218)
    norm, head      the final LayerNorm on the class rows only (x[:, 0] is all the reference reads, :465-470); the head in
                    PyTorch, like the ViT, Swin and LeViT heads

LayerScale and the SE gate are passes of their own, not GEMM epilogues: the shared GEMM kernel stays as it is, at the cost of
one extra fp32 read and write of the branch output per block.

Refused with NotImplementedError (nothing is approximated): robust=True at forward (see Learned_Aggregation_Layer), multiclass
(S60_multi), drop_rate / attn_drop_rate > 0 in training, act_layer other than nn.GELU, norm_layer other than an affine
LayerNorm, block / attention / patch layers other than the defaults, stem or embedding channels that are not multiples of 8,
non-square images or sides that are not multiples of 16, class-attention shapes outside the kernel's range (head dim % 8,
<= 1024, <= 4096 keys), and attention-map recording.
"""
from __future__ import annotations

from functools import partial
from typing import Callable, Optional

import torch
from torch import nn

from . import encoder as E
from . import kernels as K
from ._lib import EPI_BIAS_GELU
from .encoder import WEIGHTS

Tensor = torch.Tensor

__all__ = ["S60", "S120", "B60", "B120", "L60", "L120", "S60_multi", "PatchConvnet", "Mlp", "Learned_Aggregation_Layer",
           "Layer_scale_init_Block_only_token", "Conv_blocks_se", "Layer_scale_init_Block", "SqueezeExcite", "ConvStem",
           "conv3x3", "DropPath"]

_ROBUST_MSG = ("robust=True is not implemented for PatchConvNet's class attention.  The reference raises TypeError there "
               "(its normalisation call at patch_convnet.py:93 passes no dim), and the evident intent has no meaningful form: with one "
               "query per sample the column normalisation divides every entry by itself, so the attention becomes uniform 1/Nk.")


# ----------------------------------------------------------------------------------------------
# modules (parameter holders with the reference's names and construction order)
# ----------------------------------------------------------------------------------------------
class DropPath(nn.Module):
    """Per-sample stochastic depth (utils.py:1100-1112); applied inside the fused LayerScale residual."""

    def __init__(self, drop_prob: float = 0.0, scale_by_keep: bool = True):
        super().__init__()
        self.drop_prob = drop_prob
        self.scale_by_keep = scale_by_keep

    def extra_repr(self):
        return f"drop_prob={round(self.drop_prob, 3):0.3f}"


class SqueezeExcite(nn.Module):
    """Squeeze-and-excitation (utils.py:1148-1184) with its defaults: ReLU, Sigmoid gate, rd = round(C * rd_ratio)."""

    def __init__(self, in_chs, rd_ratio=0.25, rd_channels=None, act_layer=nn.ReLU, gate_layer=nn.Sigmoid, force_act_layer=None,
                 rd_round_fn=None):
        super().__init__()
        if rd_channels is None:
            rd_channels = (rd_round_fn or round)(in_chs * rd_ratio)
        if (force_act_layer or act_layer) is not nn.ReLU or gate_layer is not nn.Sigmoid:
            raise NotImplementedError("SqueezeExcite: only the ReLU / Sigmoid defaults are implemented")
        self.conv_reduce = nn.Conv2d(in_chs, rd_channels, 1, bias=True)
        self.act1 = nn.ReLU(inplace=True)
        self.conv_expand = nn.Conv2d(rd_channels, in_chs, 1, bias=True)
        self.gate = nn.Sigmoid()


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)


class Learned_Aggregation_Layer(nn.Module):
    """Class attention (patch_convnet.py:41-105): one query (the class token) against the class and patch tokens.

    robust=True constructs (the state_dict is the same) but its forward raises NotImplementedError: the reference raises
    TypeError there, and with a single query the Sinkhorn column step would make the attention uniform."""

    def __init__(self, dim, num_heads=1, qkv_bias=False, qk_scale=None, attn_drop=0.0, proj_drop=0.0, robust=False):
        super().__init__()
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.q = nn.Linear(dim, dim, bias=qkv_bias)
        self.k = nn.Linear(dim, dim, bias=qkv_bias)
        self.v = nn.Linear(dim, dim, bias=qkv_bias)
        self.id = nn.Identity()
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.robust = robust
        if dim % num_heads or head_dim % 8 or head_dim > 1024:
            raise NotImplementedError(f"class attention with dim {dim} / {num_heads} heads: the kernel takes head dims that are "
                                      "multiples of 8 and at most 1024")


class Layer_scale_init_Block_only_token(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=False, qk_scale=None, drop=0.0, attn_drop=0.0, drop_path=0.0,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, Attention_block=Learned_Aggregation_Layer, Mlp_block=Mlp,
                 init_values=1e-4, robust=False):
        super().__init__()
        if Attention_block is not Learned_Aggregation_Layer or Mlp_block is not Mlp:
            raise NotImplementedError("only Learned_Aggregation_Layer and Mlp are implemented in the class-token block")
        self.norm1 = norm_layer(dim)
        self.attn = Attention_block(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop,
                                    proj_drop=drop, robust=robust)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp_block(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.gamma_1 = nn.Parameter(init_values * torch.ones((dim)), requires_grad=True)
        self.gamma_2 = nn.Parameter(init_values * torch.ones((dim)), requires_grad=True)


class Conv_blocks_se(nn.Module):
    """1x1 conv -> GELU -> depthwise 3x3 -> GELU -> SE -> 1x1 conv (patch_convnet.py:221-244); `robust` is ignored, as there."""

    def __init__(self, dim, robust=False):
        super().__init__()
        self.robust = robust
        self.qkv_pos = nn.Sequential(
            nn.Conv2d(dim, dim, kernel_size=1),
            nn.GELU(),
            nn.Conv2d(dim, dim, groups=dim, kernel_size=3, padding=1, stride=1, bias=True),
            nn.GELU(),
            SqueezeExcite(dim, rd_ratio=0.25),
            nn.Conv2d(dim, dim, kernel_size=1),
        )


class Layer_scale_init_Block(nn.Module):
    """x + drop_path(gamma_1 * attn(norm1(x))) (patch_convnet.py:247-265).  The keep values are drawn on the input's device,
    torch.rand(B) >= drop, or taken from `keep_source(batch, device)` (tests)."""

    def __init__(self, dim, drop_path=0.0, act_layer=nn.GELU, norm_layer=nn.LayerNorm, Attention_block=None, init_values=1e-4,
                 robust=False):
        super().__init__()
        if Attention_block is not Conv_blocks_se:
            raise NotImplementedError("only Conv_blocks_se is implemented as the PatchConvNet block")
        self.norm1 = norm_layer(dim)
        self.attn = Attention_block(dim, robust=robust)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.gamma_1 = nn.Parameter(init_values * torch.ones((dim)), requires_grad=True)
        self.keep_source: Optional[Callable[[int, torch.device], Tensor]] = None

    def draw(self, batch: int, device):
        """(keep fp32 [batch] or None, survival)."""
        drop = self.drop_path.drop_prob if isinstance(self.drop_path, DropPath) else 0.0
        if not (self.training and drop > 0):
            return None, 1.0
        if self.keep_source is not None:
            keep = self.keep_source(batch, device).to(device=device, dtype=torch.float32).contiguous()
        else:
            keep = torch.rand(batch, device=device).ge_(drop).to(torch.float32)
        return keep, 1.0 - drop


def conv3x3(in_planes, out_planes, stride=1):
    return nn.Sequential(nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=1, bias=False))


class ConvStem(nn.Module):
    """4 x Conv2d(3x3, stride 2, pad 1, no bias) with GELU between them (patch_convnet.py:268-305)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768):
        super().__init__()
        img_size = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)
        patch_size = (patch_size, patch_size) if isinstance(patch_size, int) else tuple(patch_size)
        self.img_size, self.patch_size = img_size, patch_size
        self.num_patches = (img_size[1] // patch_size[1]) * (img_size[0] // patch_size[0])
        self.proj = nn.Sequential(
            conv3x3(in_chans, embed_dim // 8, 2), nn.GELU(),
            conv3x3(embed_dim // 8, embed_dim // 4, 2), nn.GELU(),
            conv3x3(embed_dim // 4, embed_dim // 2, 2), nn.GELU(),
            conv3x3(embed_dim // 2, embed_dim, 2),
        )


# ----------------------------------------------------------------------------------------------
# autograd nodes
# ----------------------------------------------------------------------------------------------
_ZEROS = {}


def _zeros(n: int, device) -> Tensor:
    key = (n, str(device))
    t = _ZEROS.get(key)
    if t is None:
        t = _ZEROS[key] = torch.zeros(n, dtype=torch.float32, device=device)
    return t


class StemFn(torch.autograd.Function):
    """ConvStem on NHWC rows: returns the fp32 token stream [B*N, C] (= flatten(2).transpose(1, 2)).  The weight images are
    re-staged every forward (four small casts), so a captured graph re-reads them."""

    @staticmethod
    def forward(ctx, img, *weights):
        B, Cin, H, W = img.shape
        src, layers = img.detach().contiguous(), []
        for li, w in enumerate(weights):
            Co = w.shape[0]
            cols, wb, wt = E.conv_cols(src, w, B, Cin, H, W, 3, 2, 1, li > 0)
            if li < len(weights) - 1:
                gd = torch.empty(cols.shape[0], Co, dtype=torch.bfloat16, device=img.device)
                src = K.gemm_nt(cols, wb, out_dtype=torch.bfloat16, epilogue=EPI_BIAS_GELU, bias=_zeros(Co, img.device), aux_out=gd)
            else:
                gd = None
                x32 = K.gemm_nt(cols, wb, out_dtype=torch.float32)
            layers.append((cols, wt, gd, (Cin, H, W)))
            Cin, H, W = Co, K.conv_out_size(H, 3, 2, 1), K.conv_out_size(W, 3, 2, 1)
        ctx.layers, ctx.B = layers, B
        return x32

    @staticmethod
    def backward(ctx, dx):
        layers, B = ctx.layers, ctx.B
        grads = [None] * len(layers)
        dy = K.cast_bf16(dx.to(torch.float32).contiguous())
        for li in range(len(layers) - 1, -1, -1):
            cols, wt, _, (Cin, H, W) = layers[li]
            grads[li] = E.conv_wgrad(dy, cols, Cin, 3)
            if li > 0:
                dz = E.conv_dx(dy, wt, B, Cin, H, W, 3, 2, 1)
                dy = K.dgelu_rows(dz, layers[li - 1][2])              # the GELU that produced this conv's input
        return (None, *grads)


class _BlockMeta:
    __slots__ = ("B", "H", "W", "eps", "keep", "survival")

    def __init__(self, B, H, W, eps, keep, survival):
        self.B, self.H, self.W, self.eps, self.keep, self.survival = B, H, W, eps, keep, survival


class ConvBlockFn(torch.autograd.Function):
    """Layer_scale_init_Block(Conv_blocks_se) on the fp32 stream x [B*H*W, C] (patch_convnet.py:221-265)."""

    @staticmethod
    def forward(ctx, x, meta: _BlockMeta, ln_w, ln_b, w1, b1, wdw, bdw, wr, br, we, be, w2, b2, gamma):
        x = x.detach()
        B, H, W = meta.B, meta.H, meta.W
        HW, C = H * W, x.shape[1]
        xn, mean, rstd = K.layernorm_fwd(x, ln_w, ln_b, meta.eps)
        w1b, _ = WEIGHTS.get(w1, True)
        a, u = E.fc1_gelu(xn, w1b, b1.detach(), q8=C % 64 == 0)
        d, sq = K.dwconv3x3_fwd(a, wdw.detach(), bdw.detach(), B, H, W)
        s, hid = K.se_fwd(sq, HW, wr.detach(), br.detach(), we.detach(), be.detach())
        g = K.se_apply(d, s, HW)
        y = E.linear(g, w2, b2, torch.float32)
        out = K.ls_add(x, y, gamma.detach(), meta.keep, meta.survival)
        ctx.meta = meta
        ctx.saved = (x, xn, mean, rstd, u, a, d, sq, s, hid, g, y)
        ctx.params = (ln_w, w1, wdw, bdw, wr, we, w2, gamma)
        return out

    @staticmethod
    def backward(ctx, dout):
        meta = ctx.meta
        B, H, W = meta.B, meta.H, meta.W
        x, xn, mean, rstd, u, a, d, sq, s, hid, g, y = ctx.saved
        ln_w, w1, wdw, bdw, wr, we, w2, gamma = ctx.params
        dout = dout.to(torch.float32).contiguous()
        dz, dgamma = K.ls_bwd(dout, y, gamma.detach(), meta.keep, meta.survival)
        dw2, db2 = K.gemm_tn(dz, g, want_dbias=True)
        _, w2t = WEIGHTS.get(w2, True)
        dg = K.gemm_nt(dz, w2t, out_dtype=torch.bfloat16)
        dmean, dwr, dbr, dwe, dbe = K.se_bwd(dg, d, sq, H * W, s, hid, wr.detach(), we.detach())
        da, dwdw, dbdw = K.dwconv3x3_bwd(a, wdw.detach(), bdw.detach(), dg, s, dmean, B, H, W, gelu_stream=u)
        dw1, db1 = K.gemm_tn(da, xn, want_dbias=True)
        _, w1t = WEIGHTS.get(w1, True)
        dxn = K.gemm_nt(da, w1t, out_dtype=torch.bfloat16)
        dx, _, dlnw, dlnb = K.layernorm_bwd(dxn, x, ln_w.detach(), mean, rstd, dres=dout)
        return (dx, None, dlnw, dlnb, dw1.reshape(w1.shape), db1, dwdw, dbdw, dwr, dbr, dwe, dbe, dw2.reshape(w2.shape), db2,
                dgamma)


class TokenBlockFn(torch.autograd.Function):
    """Layer_scale_init_Block_only_token (patch_convnet.py:154-218) on the class rows cls [B, C] and the patch stream x [B*N, C]:
        c1 = cls + gamma_1 proj(cls_attn(q(LN1 cls), k / v(LN1 [cls; x])));   c2 = c1 + gamma_2 fc2(gelu(fc1(LN2 c1)))"""

    @staticmethod
    def forward(ctx, x, cls, meta, n1w, n1b, wq, bq, wk, bk, wv, bv, wp, bp, g1, n2w, n2b, wf1, bf1, wf2, bf2, g2):
        x, cls = x.detach(), cls.detach().contiguous()
        B, N, H, dh, scale, eps1, eps2 = meta
        xc, mc, rc = K.layernorm_fwd(cls, n1w, n1b, eps1)
        xp, mp, rp = K.layernorm_fwd(x, n1w, n1b, eps1)
        q = E.linear(xc, wq, bq)
        kc, kp = E.linear(xc, wk, bk), E.linear(xp, wk, bk)
        vc, vp = E.linear(xc, wv, bv), E.linear(xp, wv, bv)
        o, lse = K.cls_attn_fwd(q, kc, kp, vc, vp, B, H, N, dh, scale)
        y1 = E.linear(o, wp, bp, torch.float32)
        c1 = K.ls_add(cls, y1, g1.detach())
        # the stream has B rows, B may be odd: bf16, never the byte stream in row pairs
        c2, mlp = E.ls_mlp_half_fwd(c1, eps2, n2w, n2b, wf1, bf1, wf2, bf2, g2.detach(), q8=False)
        ctx.meta = meta
        ctx.saved = (x, cls, xc, mc, rc, xp, mp, rp, q, kc, kp, vc, vp, o, lse, y1, mlp)
        ctx.params = (n1w, wq, bq, wk, bk, wv, bv, wp, g1, n2w, wf1, wf2, g2)
        return c2

    @staticmethod
    def backward(ctx, dc2):
        B, N, H, dh, scale, _, _ = ctx.meta
        x, cls, xc, mc, rc, xp, mp, rp, q, kc, kp, vc, vp, o, lse, y1, mlp = ctx.saved
        n1w, wq, bq, wk, bk, wv, bv, wp, g1, n2w, wf1, wf2, g2 = ctx.params
        dc2 = dc2.to(torch.float32).contiguous()
        dc1, (dg2, dn2w, dn2b, dwf1, dbf1, dwf2, dbf2) = E.ls_mlp_half_bwd(dc2, mlp, n2w, wf1, wf2, g2.detach())
        dz1, dg1 = K.ls_bwd(dc1, y1, g1.detach())
        dwp, dbp = K.gemm_tn(dz1, o, want_dbias=True)
        do = E.dx_sum([(dz1, wp)], torch.bfloat16)
        dq, dkc, dkp, dvc, dvp = K.cls_attn_bwd(q, kc, kp, vc, vp, do, lse, B, H, N, dh, scale)
        dwq, dbq = E.wgrad([dq], [xc], bq is not None)
        dwk, dbk = E.wgrad([dkc, dkp], [xc, xp], bk is not None)
        dwv, dbv = E.wgrad([dvc, dvp], [xc, xp], bv is not None)
        dxc = E.dx_sum([(dq, wq), (dkc, wk), (dvc, wv)], torch.bfloat16)
        dxp = E.dx_sum([(dkp, wk), (dvp, wv)], torch.bfloat16)
        dcls, _, dn1w, dn1b = K.layernorm_bwd(dxc, cls, n1w.detach(), mc, rc, dres=dc1)
        dx, _, dn1w, dn1b = K.layernorm_bwd(dxp, x, n1w.detach(), mp, rp, dgamma=dn1w, dbeta=dn1b, accumulate=True)
        return (dx, dcls, None, dn1w, dn1b, dwq, dbq, dwk, dbk, dwv, dbv, dwp, dbp, dg1, dn2w, dn2b, dwf1, dbf1, dwf2, dbf2, dg2)


# ----------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------
def _ln_eps(norm: nn.Module) -> float:
    if type(norm) is not nn.LayerNorm or not norm.elementwise_affine or norm.bias is None or len(norm.normalized_shape) != 1:
        raise NotImplementedError("only an affine nn.LayerNorm is implemented as PatchConvNet's norm_layer")
    return float(norm.eps)


class PatchConvnet(nn.Module):
    """PatchConvnet (patch_convnet.py:308-471) with the reference's constructor arguments, `robust` included."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12, num_heads=1,
                 qkv_bias=False, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0, hybrid_backbone=None,
                 norm_layer=nn.LayerNorm, global_pool=None, block_layers=Layer_scale_init_Block,
                 block_layers_token=Layer_scale_init_Block_only_token, Patch_layer=ConvStem, act_layer=nn.GELU,
                 Attention_block=Conv_blocks_se, dpr_constant=True, init_scale=1e-4,
                 Attention_block_token_only=Learned_Aggregation_Layer, Mlp_block_token_only=Mlp, depth_token_only=1,
                 mlp_ratio_clstk=3.0, multiclass=False, robust=False):
        super().__init__()
        if multiclass:
            raise NotImplementedError("multiclass PatchConvNet (S60_multi, Learned_Aggregation_Layer_multi) is not implemented")
        if act_layer is not nn.GELU:
            raise NotImplementedError(f"act_layer {act_layer!r}: only nn.GELU is implemented (it is fused into the kernels)")
        if block_layers is not Layer_scale_init_Block or block_layers_token is not Layer_scale_init_Block_only_token:
            raise NotImplementedError("only the default block_layers / block_layers_token are implemented")
        if Patch_layer is not ConvStem or Attention_block is not Conv_blocks_se:
            raise NotImplementedError("only the default Patch_layer (ConvStem) and Attention_block (Conv_blocks_se) are implemented")
        if Attention_block_token_only is not Learned_Aggregation_Layer or Mlp_block_token_only is not Mlp:
            raise NotImplementedError("only the default Attention_block_token_only / Mlp_block_token_only are implemented")
        if embed_dim % 64:
            raise NotImplementedError(f"embed_dim {embed_dim}: the stem's channels embed_dim / 8 .. embed_dim must be multiples of 8")
        self.multiclass = multiclass
        self.patch_size = patch_size
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        self.drop_rate, self.attn_drop_rate = drop_rate, attn_drop_rate
        self.patch_embed = Patch_layer(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, int(embed_dim)))
        if not dpr_constant:
            dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
        else:
            dpr = [drop_path_rate for _ in range(depth)]
        self.blocks = nn.ModuleList([
            block_layers(dim=embed_dim, drop_path=dpr[i], norm_layer=norm_layer, act_layer=act_layer, Attention_block=Attention_block,
                         init_values=init_scale, robust=robust)
            for i in range(depth)])
        self.blocks_token_only = nn.ModuleList([
            block_layers_token(dim=int(embed_dim), num_heads=num_heads, mlp_ratio=mlp_ratio_clstk, qkv_bias=qkv_bias,
                               qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate, drop_path=0.0, norm_layer=norm_layer,
                               act_layer=act_layer, Attention_block=Attention_block_token_only, Mlp_block=Mlp_block_token_only,
                               init_values=init_scale, robust=robust)
            for _ in range(depth_token_only)])
        self.norm = norm_layer(int(embed_dim))
        self.total_len = depth_token_only + depth
        self.feature_info = [dict(num_chs=int(embed_dim), reduction=0, module="head")]
        self.head = nn.Linear(int(embed_dim), num_classes) if num_classes > 0 else nn.Identity()
        self.rescale = 0.02
        nn.init.trunc_normal_(self.cls_token, std=self.rescale)
        self.apply(self._init_weights)
        for m in [self.norm] + [b.norm1 for b in self.blocks] + [m for b in self.blocks_token_only for m in (b.norm1, b.norm2)]:
            _ln_eps(m)
        rd = self.blocks[0].attn.qkv_pos[4].conv_reduce.out_channels if depth else 1
        if embed_dim > 4096 or rd > 1024:
            raise NotImplementedError("squeeze-and-excitation takes at most 4096 channels and 1024 hidden units")

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=self.rescale)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {"cls_token"}

    def get_classifier(self):
        return self.head

    def get_num_layers(self):
        return len(self.blocks)

    def reset_classifier(self, num_classes: int, global_pool: str = ""):
        self.num_classes = num_classes
        self.head = nn.Linear(self.embed_dim, num_classes) if num_classes > 0 else nn.Identity()

    def _check_forward(self, x: Tensor) -> None:
        E.require_run(x, "PatchConvNet")
        if any(b.attn.robust for b in self.blocks_token_only):
            raise NotImplementedError(_ROBUST_MSG)
        if self.training and (self.drop_rate > 0 or self.attn_drop_rate > 0):
            raise NotImplementedError("dropout (drop_rate / attn_drop_rate > 0) in training is not implemented for PatchConvNet")
        if x.dim() != 4 or x.shape[2] != x.shape[3] or x.shape[2] % 16:
            raise NotImplementedError(f"image {tuple(x.shape[2:])}: PatchConvNet runs square images with sides that are multiples "
                                      "of 16 (the reference's int(N ** 0.5) grid, patch_convnet.py:238)")

    def forward_features(self, x: Tensor) -> Tensor:
        self._check_forward(x)
        B, C = x.shape[0], self.embed_dim
        r = x.shape[2] // 16
        N = r * r
        if N + 1 > 4096:
            raise NotImplementedError(f"{N + 1} keys: the class-attention kernel takes at most 4096")
        convs = [self.patch_embed.proj[i][0] for i in range(0, 7, 2)]
        x32 = StemFn.apply(x.to(torch.float32), *[c.weight for c in convs])
        for blk in self.blocks:
            keep, survival = blk.draw(B, x.device)
            qp = blk.attn.qkv_pos
            se = qp[4]
            meta = _BlockMeta(B, r, r, float(blk.norm1.eps), keep, survival)
            x32 = ConvBlockFn.apply(x32, meta, blk.norm1.weight, blk.norm1.bias, qp[0].weight, qp[0].bias, qp[2].weight, qp[2].bias,
                                    se.conv_reduce.weight, se.conv_reduce.bias, se.conv_expand.weight, se.conv_expand.bias,
                                    qp[5].weight, qp[5].bias, blk.gamma_1)
        cls = self.cls_token.expand(B, 1, C).reshape(B, C)
        for blk in self.blocks_token_only:
            a, m = blk.attn, blk.mlp
            H = a.num_heads
            meta = (B, N, H, C // H, float(a.scale), float(blk.norm1.eps), float(blk.norm2.eps))
            cls = TokenBlockFn.apply(x32, cls.contiguous(), meta, blk.norm1.weight, blk.norm1.bias, a.q.weight, a.q.bias, a.k.weight,
                                     a.k.bias, a.v.weight, a.v.bias, a.proj.weight, a.proj.bias, blk.gamma_1, blk.norm2.weight,
                                     blk.norm2.bias, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, blk.gamma_2)
        return E.LayerNormFn.apply(cls.contiguous(), self.norm.weight, self.norm.bias, float(self.norm.eps))

    def forward(self, x: Tensor) -> Tensor:
        return self.head(self.forward_features(x))


def _builder(embed_dim, depth, init_scale=None, mlp_ratio_clstk=3.0):
    def make(pretrained: bool = False, **kwargs):
        extra = {} if init_scale is None else {"init_scale": init_scale}
        return PatchConvnet(patch_size=16, embed_dim=embed_dim, depth=depth, num_heads=1, qkv_bias=True,
                            norm_layer=partial(nn.LayerNorm, eps=1e-6), Patch_layer=ConvStem, Attention_block=Conv_blocks_se,
                            mlp_ratio_clstk=mlp_ratio_clstk, **extra, **kwargs)
    return make


S60 = _builder(384, 60)
S120 = _builder(384, 120, 1e-6)
B60 = _builder(768, 60, 1e-6)
B120 = _builder(768, 120, 1e-6)
L60 = _builder(1024, 60, 1e-6)
L120 = _builder(1024, 120, 1e-6)
for _n, _f in (("S60", S60), ("S120", S120), ("B60", B60), ("B120", B120), ("L60", L60), ("L120", L120)):
    _f.__name__ = _f.__qualname__ = _n


def S60_multi(pretrained: bool = False, **kwargs):
    raise NotImplementedError("S60_multi (Learned_Aggregation_Layer_multi) is not implemented")
