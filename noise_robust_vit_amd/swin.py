"""Swin Transformer (V1) on the HIP hot path: drop-in for the reference's swin_t / swin_s / swin_b (swin.py:604-800).

    from noise_robust_vit_amd import swin_t          # was: from vit_pytorch_robust import swin_t
    model = swin_t(num_classes=100, robust=True).cuda()

The modules take the reference's constructor arguments and hold the same parameters and buffers under the same names
(nn.Linear / nn.LayerNorm / nn.Conv2d children only hold them), drawn from the RNG in the same order, so seeded models and
reference checkpoints are interchangeable.  The arithmetic of a forward / backward runs through libnrv_hip.so:

    patch embedding  nrv_patch_unfold (c, p1, p2) + NT GEMM + bias, LayerNorm                         (swin.py:660-670)
    block            LN -> [gather into the zero-padded grid] -> QKV GEMM -> nrv_window_attn -> [gather the real rows]
                     -> proj GEMM + residual (or row-mode stochastic depth), then the encoder's MLP half     (swin.py:525-535)
    patch merging    nrv_gather_rows (the x0 x1 x2 x3 concatenation and the odd-size pad) -> LN(4C) -> GEMM  (swin.py:30-83)
    head             final LN on every token (HIP); mean pool and the classifier in PyTorch, like the ViT head

Refused with NotImplementedError (nothing is approximated): dropout > 0 and attention_dropout > 0 -- the reference applies
F.dropout at swin.py:248 and :251 with its default training=True, i.e. even in eval mode --, Swin V2 (cosine attention and the
continuous position-bias MLP), other block / norm / downsample classes, and attention-map recording.
"""
from __future__ import annotations

from functools import partial
from typing import Any, Callable, List, Optional

import torch
from torch import nn

from . import encoder as E
from . import kernels as K
from ._lib import EPI_BIAS, EPI_BIAS_RESIDUAL, EPI_NONE, PATCH_CP1P2
from .encoder import WEIGHTS, BlockMeta, PatchEmbedFn

Tensor = torch.Tensor

__all__ = ["SwinTransformer", "SwinTransformerBlock", "ShiftedWindowAttention", "PatchMerging", "swin_t", "swin_s", "swin_b",
           "swin_v2_t", "swin_v2_s", "swin_v2_b"]


# ----------------------------------------------------------------------------------------------
# index builders (host arithmetic, cached per geometry on the device)
# ----------------------------------------------------------------------------------------------
def window_geometry(H: int, W: int, window: List[int], shift: List[int]):
    """(pH, pW, sh, sw): the padded map and the shift after the reference's rule (swin.py:146-161)."""
    Wh, Ww = window
    pH = H + (Wh - H % Wh) % Wh
    pW = W + (Ww - W % Ww) % Ww
    sh = 0 if Wh >= pH else shift[0]
    sw = 0 if Ww >= pW else shift[1]
    return pH, pW, sh, sw


def pad_index(B: int, H: int, W: int, pH: int, pW: int) -> Tensor:
    """Row of the real map for every row of the padded map (b, y, x), -1 (= zero row) for the pad (F.pad, swin.py:150-154)."""
    y = torch.arange(pH)[:, None].expand(pH, pW)
    x = torch.arange(pW)[None, :].expand(pH, pW)
    real = (y < H) & (x < W)
    idx = torch.where(real, y * W + x, torch.full_like(y, -1))
    b = torch.arange(B)[:, None, None] * (H * W)
    return torch.where(idx[None] >= 0, idx[None] + b, torch.full_like(b, -1).expand(B, pH, pW)).reshape(-1).to(torch.int64)


def real_index(B: int, H: int, W: int, pH: int, pW: int) -> Tensor:
    """Row of the padded map for every row of the real map (the unpad slice x[:, :H, :W], swin.py:266)."""
    y = torch.arange(H)[:, None] * pW + torch.arange(W)[None, :]
    return (torch.arange(B)[:, None, None] * (pH * pW) + y[None]).reshape(-1).to(torch.int64)


def merge_index(B: int, H: int, W: int) -> Tensor:
    """Source row for every C-wide slice of the merged rows [B, H2, W2, 4 C] (x0 x1 x2 x3 of swin.py:30-38, x1 = odd row /
    even column, x2 = even row / odd column); -1 where the odd-size zero pad is read."""
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    y2 = torch.arange(H2)[:, None, None]
    x2 = torch.arange(W2)[None, :, None]
    dy = torch.tensor([0, 1, 0, 1])[None, None, :]
    dx = torch.tensor([0, 0, 1, 1])[None, None, :]
    y, x = 2 * y2 + dy, 2 * x2 + dx
    idx = torch.where((y < H) & (x < W), y * W + x, torch.full_like(y * x, -1))            # [H2, W2, 4]
    b = torch.arange(B)[:, None, None, None] * (H * W)
    return torch.where(idx[None] >= 0, idx[None] + b, torch.full_like(idx[None] + b, -1)).reshape(-1).to(torch.int64)


# ----------------------------------------------------------------------------------------------
# autograd boundary
# ----------------------------------------------------------------------------------------------
class SwinGeom:
    """Geometry of one block call: the real map H x W of B samples, the padded map, window and effective shift."""

    def __init__(self, B: int, H: int, W: int, C: int, heads: int, window: List[int], shift: List[int], robust: bool, device):
        self.B, self.H, self.W, self.C, self.heads, self.robust = B, H, W, C, heads, robust
        self.window = tuple(window)
        self.pH, self.pW, sh, sw = window_geometry(H, W, list(window), list(shift))
        self.shift = (sh, sw)
        self.padded = (self.pH, self.pW) != (H, W)
        if self.padded:
            self.pad_idx = E.cached("pad", pad_index, B, H, W, self.pH, self.pW, device=device)
            self.real_idx = E.cached("real", real_index, B, H, W, self.pH, self.pW, device=device)

    def attn_args(self):
        return (self.B, self.pH, self.pW, self.C, self.heads, self.window, self.shift, self.robust)


class SwinBlockFn(torch.autograd.Function):
    """One SwinTransformerBlock (swin.py:525-535) on the fp32 stream x [B*H*W, C]:
        x1 = x + sd(proj(window_attn(qkv(LN1(x)))));   x2 = x1 + sd(mlp(LN2(x1)))
    keep1 / keep2: per-sample stochastic-depth keep values (fp32 [B]) or None (no stochastic depth); survival = 1 - p."""

    @staticmethod
    def forward(ctx, x, geom: SwinGeom, meta: BlockMeta, keep1, keep2, survival: float,
                ln1_w, ln1_b, wqkv, bqkv, table, wo, bo, ln2_w, ln2_b, w1, b1, w2, b2):
        x = x.detach()
        xn, mean1, rstd1 = K.layernorm_fwd(x, ln1_w, ln1_b, meta.eps)
        xp = E.rows_bf16(xn, geom.pad_idx) if geom.padded else xn
        wqkv_b, _ = WEIGHTS.get(wqkv, True)
        wo_b, _ = WEIGHTS.get(wo, True)
        qkv = K.gemm_nt(xp, wqkv_b, out_dtype=torch.bfloat16, epilogue=EPI_BIAS if bqkv is not None else EPI_NONE,
                        bias=None if bqkv is None else bqkv.detach())
        o, stats = K.window_attn_fwd(qkv, table.detach(), *geom.attn_args())
        o_real = E.rows_bf16(o, geom.real_idx) if geom.padded else o
        bo_d = None if bo is None else bo.detach()
        if keep1 is not None:
            yb = K.gemm_nt(o_real, wo_b, out_dtype=torch.float32, epilogue=EPI_BIAS if bo is not None else EPI_NONE, bias=bo_d)
            x1 = K.sd_add(x, yb, keep1, survival, out=yb)
        else:
            x1 = K.gemm_nt(o_real, wo_b, out_dtype=torch.float32, epilogue=EPI_BIAS_RESIDUAL, bias=bo_d, aux=x)
        if keep2 is not None:
            y, saved2 = E.mlp_half_fwd(x1, meta, ln2_w, ln2_b, w1, b1, w2, b2, residual=False)
            x2 = K.sd_add(x1, y, keep2, survival, out=y)
        else:
            x2, saved2 = E.mlp_half_fwd(x1, meta, ln2_w, ln2_b, w1, b1, w2, b2, residual=True)
        ctx.geom, ctx.meta, ctx.keeps, ctx.survival = geom, meta, (keep1, keep2), survival
        ctx.params = (ln1_w, ln1_b, wqkv, bqkv, table, wo, bo, ln2_w, ln2_b, w1, b1, w2, b2)
        ctx.saved1 = (x, xp, mean1, rstd1, qkv, o_real, stats)
        ctx.saved2 = saved2
        return x2

    @staticmethod
    def backward(ctx, dy):
        geom, meta = ctx.geom, ctx.meta
        keep1, keep2 = ctx.keeps
        ln1_w, ln1_b, wqkv, bqkv, table, wo, bo, ln2_w, ln2_b, w1, b1, w2, b2 = ctx.params
        x, xp, mean1, rstd1, qkv, o_real, stats = ctx.saved1
        d2 = dy.to(torch.float32).contiguous()
        d16 = K.sd_scale_bf16(d2, keep2, ctx.survival) if keep2 is not None else None
        d1, _, g_mlp = E.mlp_half_bwd(d2, d16, ctx.saved2, meta, ln2_w, ln2_b, w1, b1, w2, b2, residual=True, want_bf16=False)
        d16 = K.sd_scale_bf16(d1, keep1, ctx.survival) if keep1 is not None else K.cast_bf16(d1)
        dwo, dbo = E._dw_db(meta, d16, o_real, wo, bo)
        _, wo_t = WEIGHTS.get(wo, True)
        _, wqkv_t = WEIGHTS.get(wqkv, True)
        do = K.gemm_nt(d16, wo_t, out_dtype=torch.bfloat16)
        if geom.padded:
            do = E.scatter_bf16(do, geom.real_idx, geom.B * geom.pH * geom.pW)
        dqkv, dtable = K.window_attn_bwd(qkv, table.detach(), do, stats, *geom.attn_args())
        dwqkv, dbqkv = E._dw_db(meta, dqkv, xp, wqkv, bqkv)
        dxp = K.gemm_nt(dqkv, wqkv_t, out_dtype=torch.bfloat16)
        dxn = E.rows_bf16(dxp, geom.real_idx) if geom.padded else dxp
        dx, _, dg1, db1 = K.layernorm_bwd(dxn, x, ln1_w, mean1, rstd1, dres=d1, want_f32=True)
        grads = E._mask_sink_grads(meta, [dg1, db1, dwqkv, dbqkv, dtable, dwo, dbo] + g_mlp)
        return (dx, None, None, None, None, None, *grads)


class MergeFn(torch.autograd.Function):
    """PatchMerging (swin.py:60-83) on the fp32 stream [B*H*W, C] -> [B*H2*W2, 2C]: row gather into the 4C rows, LN(4C), GEMM."""

    @staticmethod
    def forward(ctx, x, index, eps: float, ln_w, ln_b, w):
        C = x.shape[1]
        g = K.gather_rows(x.detach().contiguous(), index).reshape(-1, 4 * C)
        gn, mean, rstd = K.layernorm_fwd(g, ln_w, ln_b, eps)
        wb, _ = WEIGHTS.get(w, True)
        y = K.gemm_nt(gn, wb, out_dtype=torch.float32, epilogue=EPI_NONE)
        ctx.saved = (g, gn, mean, rstd, index, x.shape[0])
        ctx.params = (ln_w, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        g, gn, mean, rstd, index, rows = ctx.saved
        ln_w, w = ctx.params
        d16 = K.cast_bf16(dy.to(torch.float32).contiguous())
        dw = K.gemm_tn(d16, gn)
        _, wt = WEIGHTS.get(w, True)
        dgn = K.gemm_nt(d16, wt, out_dtype=torch.bfloat16)
        dg, _, dlw, dlb = K.layernorm_bwd(dgn, g, ln_w, mean, rstd, want_f32=True)
        dx = K.scatter_rows(dg.reshape(-1, dg.shape[1] // 4), index, rows)
        return dx, None, None, dlw, dlb, dw


# ----------------------------------------------------------------------------------------------
# modules (parameter holders with the reference's names)
# ----------------------------------------------------------------------------------------------
def _ln_eps(norm: nn.Module) -> float:
    if not isinstance(norm, nn.LayerNorm) or not norm.elementwise_affine:
        raise NotImplementedError("only nn.LayerNorm with affine parameters is implemented as the Swin norm_layer")
    return float(norm.eps)


class Permute(nn.Module):
    """torchvision.ops.misc.Permute (no parameters; kept for the reference's module tree)."""

    def __init__(self, dims: List[int]):
        super().__init__()
        self.dims = dims

    def forward(self, x: Tensor) -> Tensor:
        return torch.permute(x, self.dims)


class StochasticDepth(nn.Module):
    """torchvision StochasticDepth(p, "row"): in training each sample's branch is kept with probability 1 - p and scaled by
    1 / (1 - p).  The keep values are drawn here (or taken from `keep_source(batch, device)`, for tests); the add runs in
    the HIP kernels of SwinBlockFn."""

    def __init__(self, p: float, mode: str) -> None:
        super().__init__()
        if mode != "row":
            raise NotImplementedError(f"stochastic depth mode {mode!r}: only 'row' is used by the Swin blocks")
        if p < 0.0 or p > 1.0:
            raise ValueError(f"drop probability has to be between 0 and 1, but got {p}")
        self.p, self.mode = p, mode
        self.keep_source: Optional[Callable[[int, torch.device], Tensor]] = None

    def draw(self, batch: int, device):
        """(keep fp32 [batch], survival) for the next forward, or None when the branch passes unchanged."""
        if not self.training or self.p == 0.0:
            return None
        survival = 1.0 - self.p
        if self.keep_source is not None:
            keep = self.keep_source(batch, device).to(device=device, dtype=torch.float32).contiguous()
        else:
            keep = torch.empty(batch, dtype=torch.float32, device=device).bernoulli_(survival)
        if survival == 0.0:                       # p = 1: the reference multiplies by the undivided (all-zero) noise
            return torch.zeros_like(keep), 1.0
        return keep, survival

    def extra_repr(self) -> str:
        return f"p={self.p}, mode={self.mode}"


class MLP(nn.Sequential):
    """torchvision.ops.misc.MLP(dim, [hidden, dim], activation_layer=nn.GELU, dropout): Linear, GELU, Dropout, Linear, Dropout."""

    def __init__(self, in_channels: int, hidden_channels: List[int], dropout: float = 0.0):
        hidden, out = hidden_channels
        super().__init__(nn.Linear(in_channels, hidden, bias=True), nn.GELU(), nn.Dropout(dropout),
                         nn.Linear(hidden, out, bias=True), nn.Dropout(dropout))


class PatchMerging(nn.Module):
    """Patch Merging Layer (swin.py:60-83): [..., H, W, C] -> [..., H/2, W/2, 2C]."""

    def __init__(self, dim: int, norm_layer: Callable[..., nn.Module] = nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = norm_layer(4 * dim)

    def run(self, x: Tensor, B: int, H: int, W: int):
        """fp32 stream [B*H*W, C] -> ([B*H2*W2, 2C], H2, W2)."""
        idx = E.cached("merge", merge_index, B, H, W, device=x.device)
        y = MergeFn.apply(x, idx, _ln_eps(self.norm), self.norm.weight, self.norm.bias, self.reduction.weight)
        return y, (H + 1) // 2, (W + 1) // 2

    def forward(self, x: Tensor) -> Tensor:
        E.require_cuda(x)
        B, H, W, C = x.shape
        y, H2, W2 = self.run(x.to(torch.float32).contiguous().reshape(B * H * W, C), B, H, W)
        return y.reshape(B, H2, W2, 2 * C)


class ShiftedWindowAttention(nn.Module):
    """Window multi-head self-attention with relative position bias (swin.py:270-366).  Holds the parameters; the attention
    runs inside SwinTransformerBlock (its residual and MLP are fused around the kernel)."""

    def __init__(self, dim: int, window_size: List[int], shift_size: List[int], num_heads: int, qkv_bias: bool = True,
                 proj_bias: bool = True, attention_dropout: float = 0.0, dropout: float = 0.0, robust: bool = False):
        super().__init__()
        if len(window_size) != 2 or len(shift_size) != 2:
            raise ValueError("window_size and shift_size must be of length 2")
        self.window_size = window_size
        self.shift_size = shift_size
        self.num_heads = num_heads
        self.attention_dropout = attention_dropout
        self.dropout = dropout
        self.robust = robust
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim, bias=proj_bias)
        self.define_relative_position_bias_table()
        self.define_relative_position_index()

    def define_relative_position_bias_table(self):
        self.relative_position_bias_table = nn.Parameter(
            torch.zeros((2 * self.window_size[0] - 1) * (2 * self.window_size[1] - 1), self.num_heads))
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)

    def define_relative_position_index(self):
        Wh, Ww = self.window_size
        yy, xx = torch.meshgrid(torch.arange(Wh), torch.arange(Ww), indexing="ij")
        y, x = yy.flatten(), xx.flatten()
        dy = y[:, None] - y[None, :] + Wh - 1          # query - key
        dx = x[:, None] - x[None, :] + Ww - 1
        self.register_buffer("relative_position_index", (dy * (2 * Ww - 1) + dx).flatten())

    def forward(self, x: Tensor):
        raise NotImplementedError("ShiftedWindowAttention runs inside SwinTransformerBlock (its residual and MLP are fused "
                                  "around the window-attention kernel); call the block")


class SwinTransformerBlock(nn.Module):
    """Swin Transformer Block (swin.py:469-535): x + sd(attn(norm1(x))), then x + sd(mlp(norm2(x)))."""

    def __init__(self, dim: int, num_heads: int, window_size: List[int], shift_size: List[int], mlp_ratio: float = 4.0,
                 dropout: float = 0.0, attention_dropout: float = 0.0, stochastic_depth_prob: float = 0.0,
                 norm_layer: Callable[..., nn.Module] = nn.LayerNorm, attn_layer: Callable[..., nn.Module] = ShiftedWindowAttention,
                 robust: bool = False):
        super().__init__()
        if attn_layer is not ShiftedWindowAttention:
            raise NotImplementedError("only ShiftedWindowAttention (Swin V1) is implemented; Swin V2 is not")
        self.norm1 = norm_layer(dim)
        self.attn = attn_layer(dim, window_size, shift_size, num_heads, attention_dropout=attention_dropout, dropout=dropout,
                               robust=robust)
        self.stochastic_depth = StochasticDepth(stochastic_depth_prob, "row")
        self.norm2 = norm_layer(dim)
        self.mlp = MLP(dim, [int(dim * mlp_ratio), dim], dropout=dropout)
        for m in self.mlp.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.normal_(m.bias, std=1e-6)

    def _check(self) -> None:
        a = self.attn
        if a.dropout > 0.0 or a.attention_dropout > 0.0:
            raise NotImplementedError("dropout > 0 / attention_dropout > 0 are not implemented: the reference applies them with "
                                      "F.dropout(..., training=True) (swin.py:248,251), i.e. even in eval mode")
        E.refuse_recording("the Swin window attention")

    def run(self, x: Tensor, B: int, H: int, W: int) -> Tensor:
        """fp32 stream [B*H*W, C] -> the same shape."""
        self._check()
        a = self.attn
        C = x.shape[1]
        heads = a.num_heads
        geom = SwinGeom(B, H, W, C, heads, list(a.window_size), list(a.shift_size), bool(a.robust), x.device)
        meta = BlockMeta(heads=heads, dim_head=C // heads, eps=_ln_eps(self.norm1), robust=bool(a.robust))
        if _ln_eps(self.norm2) != meta.eps:
            raise NotImplementedError("norm1 and norm2 with different eps")
        d1 = self.stochastic_depth.draw(B, x.device)
        d2 = self.stochastic_depth.draw(B, x.device)
        survival = 1.0 if d1 is None else d1[1]
        l0, l3 = self.mlp[0], self.mlp[3]
        return SwinBlockFn.apply(x, geom, meta, None if d1 is None else d1[0], None if d2 is None else d2[0], survival,
                                 self.norm1.weight, self.norm1.bias, a.qkv.weight, a.qkv.bias, a.relative_position_bias_table,
                                 a.proj.weight, a.proj.bias, self.norm2.weight, self.norm2.bias,
                                 l0.weight, l0.bias, l3.weight, l3.bias)

    def forward(self, x: Tensor) -> Tensor:
        E.require_cuda(x)
        B, H, W, C = x.shape
        return self.run(x.to(torch.float32).contiguous().reshape(B * H * W, C), B, H, W).reshape(B, H, W, C)


class SwinTransformer(nn.Module):
    """Swin Transformer (swin.py:580-700) with the reference's constructor arguments, `robust` included."""

    def __init__(self, patch_size: List[int], embed_dim: int, depths: List[int], num_heads: List[int], window_size: List[int],
                 mlp_ratio: float = 4.0, dropout: float = 0.0, attention_dropout: float = 0.0, stochastic_depth_prob: float = 0.1,
                 num_classes: int = 1000, norm_layer: Optional[Callable[..., nn.Module]] = None,
                 block: Optional[Callable[..., nn.Module]] = None, downsample_layer: Callable[..., nn.Module] = PatchMerging,
                 robust: bool = False):
        super().__init__()
        self.num_classes = num_classes
        if block is None:
            block = SwinTransformerBlock
        if block is not SwinTransformerBlock or downsample_layer is not PatchMerging:
            raise NotImplementedError("only the Swin V1 block and PatchMerging are implemented (Swin V2 is not)")
        if norm_layer is None:
            norm_layer = partial(nn.LayerNorm, eps=1e-5)
        if patch_size[0] != patch_size[1]:
            raise NotImplementedError("square patches only")
        self.patch_size = patch_size[0]
        layers: List[nn.Module] = [nn.Sequential(
            nn.Conv2d(3, embed_dim, kernel_size=(patch_size[0], patch_size[1]), stride=(patch_size[0], patch_size[1])),
            Permute([0, 2, 3, 1]),
            norm_layer(embed_dim))]
        total_stage_blocks = sum(depths)
        stage_block_id = 0
        for i_stage in range(len(depths)):
            stage: List[nn.Module] = []
            dim = embed_dim * 2 ** i_stage
            for i_layer in range(depths[i_stage]):
                sd_prob = stochastic_depth_prob * float(stage_block_id) / (total_stage_blocks - 1)
                stage.append(block(dim, num_heads[i_stage], window_size=window_size,
                                   shift_size=[0 if i_layer % 2 == 0 else w // 2 for w in window_size], mlp_ratio=mlp_ratio,
                                   dropout=dropout, attention_dropout=attention_dropout, stochastic_depth_prob=sd_prob,
                                   norm_layer=norm_layer, robust=robust))
                stage_block_id += 1
            layers.append(nn.Sequential(*stage))
            if i_stage < (len(depths) - 1):
                layers.append(downsample_layer(dim, norm_layer))
        self.features = nn.Sequential(*layers)
        num_features = embed_dim * 2 ** (len(depths) - 1)
        self.norm = norm_layer(num_features)
        self.permute = Permute([0, 3, 1, 2])
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.flatten = nn.Flatten(1)
        self.head = nn.Linear(num_features, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward(self, x: Tensor) -> Tensor:
        E.require_cuda(x)
        B, _, Hi, Wi = x.shape
        p = self.patch_size
        if Hi % p or Wi % p:
            raise NotImplementedError(f"image {Hi}x{Wi} is not a multiple of the patch size {p}")
        H, W = Hi // p, Wi // p
        embed = self.features[0]
        conv, norm0 = embed[0], embed[2]
        zeros = torch.zeros(H * W, conv.out_channels, device=x.device)
        t = PatchEmbedFn.apply(x, conv.weight, conv.bias, zeros, None, p, PATCH_CP1P2, None)     # [B, H*W, D] fp32
        t = E.LayerNormFn.apply(t.reshape(B * H * W, -1), norm0.weight, norm0.bias, _ln_eps(norm0))
        for m in list(self.features)[1:]:
            if isinstance(m, PatchMerging):
                t, H, W = m.run(t, B, H, W)
            else:
                for blk in m:
                    t = blk.run(t, B, H, W)
        t = E.LayerNormFn.apply(t, self.norm.weight, self.norm.bias, _ln_eps(self.norm))
        pooled = t.reshape(B, H * W, -1).mean(dim=1)                 # permute + AdaptiveAvgPool2d(1) + flatten (swin.py:694-697)
        return self.head(pooled)


def _swin_transformer(patch_size, embed_dim, depths, num_heads, window_size, stochastic_depth_prob, **kwargs: Any):
    if kwargs.pop("weights", None) is not None:
        raise NotImplementedError("pretrained weights are not bundled; load a state_dict instead")
    kwargs.pop("progress", None)
    return SwinTransformer(patch_size=patch_size, embed_dim=embed_dim, depths=depths, num_heads=num_heads,
                           window_size=window_size, stochastic_depth_prob=stochastic_depth_prob, **kwargs)


def swin_t(*args, **kwargs: Any) -> SwinTransformer:
    """swin_tiny (swin.py:727-756): patch 4, embed 96, depths [2, 2, 6, 2], heads [3, 6, 12, 24], window 7, sd 0.2."""
    return _swin_transformer([4, 4], 96, [2, 2, 6, 2], [3, 6, 12, 24], [7, 7], 0.2, **kwargs)


def swin_s(*args, **kwargs: Any) -> SwinTransformer:
    """swin_small: depths [2, 2, 18, 2], sd 0.3."""
    return _swin_transformer([4, 4], 96, [2, 2, 18, 2], [3, 6, 12, 24], [7, 7], 0.3, **kwargs)


def swin_b(*args, **kwargs: Any) -> SwinTransformer:
    """swin_base: embed 128, depths [2, 2, 18, 2], heads [4, 8, 16, 32], sd 0.5."""
    return _swin_transformer([4, 4], 128, [2, 2, 18, 2], [4, 8, 16, 32], [7, 7], 0.5, **kwargs)


def _v2(*args, **kwargs):
    raise NotImplementedError("Swin V2 (cosine attention, continuous position-bias MLP) is not implemented")


swin_v2_t = swin_v2_s = swin_v2_b = _v2
