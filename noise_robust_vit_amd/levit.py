"""LeViT on the HIP hot path: drop-in for the reference's levit.LeViT_128S / 128 / 192 / 256 / 384 (levit.py:531-587).

    from noise_robust_vit_amd import levit           # was: from vit_pytorch_robust import levit
    model = levit.LeViT_128S(num_classes=100, robust=True).cuda()

The modules take the reference's constructor arguments and hold the same parameters and buffers under the same names
(Conv2d / Linear / BatchNorm children, attention_biases, the persistent int64 attention_bias_idxs), drawn from the RNG in the
same order, so seeded models and reference checkpoints are interchangeable.  The arithmetic runs through libnrv_hip.so:

    stem (b16)         nrv_conv_unfold (NCHW image, then NHWC rows) + NT GEMM -> nrv_bn_stats / nrv_bn_apply (+ Hardswish);
                       backward: nrv_bn_bwd, TN GEMM (dW), NT GEMM + nrv_conv_fold (dX)                     (levit.py:166-175)
    Linear_BN          NT GEMM (fp32 out) -> BN over all B*N rows, applied with the consumer's epilogue  (levit.py:103-134)
    Attention          qkv Linear_BN -> nrv_bias_attn (bias table, softmax or Sinkhorn, Hardswish) -> proj Linear_BN
                       + residual (and row-mode drop-path) in the BN apply                                 (levit.py:198-281)
    AttentionSubsample kv Linear_BN; row gather (Subsample) -> q Linear_BN; nrv_bias_attn with Nq < Nk; proj Linear_BN
                                                                                                           (levit.py:284-403)
    MLP                Linear_BN -> Hardswish (fused in the BN apply) -> Linear_BN + residual                 (levit.py:467-480)
    head               mean over tokens and BN_Linear in PyTorch, like the ViT and Swin heads

Train and eval follow each BatchNorm's `training` flag: training normalises with the batch statistics and updates the running
mean / (unbiased) variance and num_batches_tracked; eval normalises with the running statistics and updates nothing.
The attention reads the live attention_biases table in both modes (the reference caches `ab` at .eval(), levit.py:249-254:
the values differ only if the table is edited between .eval() and a forward).

Refused with NotImplementedError (nothing is approximated): activations other than nn.Hardswish, a hybrid_backbone that is not
the b16 structure, down_ops other than "Subsample", shapes outside the kernels' range (more than 256 keys, key_dim not 16 / 32,
value dim not 32 / 64 / 128, channels not a multiple of 8), BatchNorm with momentum=None or without running statistics, and
attention-map recording.
"""
from __future__ import annotations

import itertools
from typing import Callable, List, Optional

import numpy as np
import torch
from torch import nn

from . import encoder as E
from . import kernels as K
from ._lib import EPI_BIAS_RESIDUAL, NrvError
from .encoder import WEIGHTS

Tensor = torch.Tensor

__all__ = ["specification", "LeViT", "LeViT_128S", "LeViT_128", "LeViT_192", "LeViT_256", "LeViT_384", "Conv2d_BN", "Linear_BN",
           "BN_Linear", "Residual", "Attention", "Subsample", "AttentionSubsample", "b16", "model_factory"]

specification = {
    "LeViT_128S": {"C": "128_256_384", "D": 16, "N": "4_6_8", "X": "2_3_4", "drop_path": 0},
    "LeViT_128": {"C": "128_256_384", "D": 16, "N": "4_8_12", "X": "4_4_4", "drop_path": 0},
    "LeViT_192": {"C": "192_288_384", "D": 32, "N": "3_5_6", "X": "4_4_4", "drop_path": 0},
    "LeViT_256": {"C": "256_384_512", "D": 32, "N": "4_6_8", "X": "4_4_4", "drop_path": 0},
    "LeViT_384": {"C": "384_512_768", "D": 32, "N": "6_9_12", "X": "4_4_4", "drop_path": 0.1},
}

_KD = (16, 32)
_DV = (32, 64, 128)
_NMAX = 256


def _check_act(act) -> None:
    if act is not nn.Hardswish:
        raise NotImplementedError(f"activation {act!r}: only torch.nn.Hardswish is implemented (its forward and derivative are "
                                  "fused into the batch-norm and attention kernels)")


# ----------------------------------------------------------------------------------------------
# batch norm over token rows
# ----------------------------------------------------------------------------------------------
def _bn_check(bn: nn.Module) -> None:
    if bn.momentum is None:
        raise NotImplementedError("BatchNorm with momentum=None (cumulative moving average) is not implemented")
    if not bn.track_running_stats or bn.running_mean is None or not bn.affine:
        raise NotImplementedError("only affine BatchNorm with running statistics is implemented")


class _BnState:
    """What the backward of one BN needs: the fp32 GEMM output y and the statistics it was normalised with."""
    __slots__ = ("y", "mean", "scale", "is_var", "eps", "training")

    def __init__(self, bn: nn.Module, y: Tensor):
        self.y, self.eps, self.training = y, float(bn.eps), bool(bn.training)
        if self.training:
            self.mean, self.scale, _ = K.bn_stats(y, bn.eps, bn.momentum, bn.running_mean, bn.running_var)
            bn.num_batches_tracked.add_(1)
            self.is_var = False
        else:
            self.mean, self.scale, self.is_var = bn.running_mean, bn.running_var, True

    def apply(self, g: Tensor, b: Tensor, **kw):
        return K.bn_apply(self.y, self.mean, self.scale, g.detach(), b.detach(), eps=self.eps, scale_is_var=self.is_var, **kw)

    def backward(self, dz: Tensor, g: Tensor, b: Tensor, **kw):
        return K.bn_bwd(dz, self.y, self.mean, self.scale, g.detach(), b.detach(), eps=self.eps, scale_is_var=self.is_var,
                        training=self.training, **kw)


def _linear_bn(x16: Tensor, lbn: "Linear_BN") -> _BnState:
    wb, _ = WEIGHTS.get(lbn.c.weight, True)
    return _BnState(lbn.bn, K.gemm_nt(x16, wb, out_dtype=torch.float32))


def _dx(d16: Tensor, w: Tensor, dres: Optional[Tensor]) -> Tensor:
    """fp32 input gradient d16 . W (+ dres) of a Linear."""
    _, wt = WEIGHTS.get(w, True)
    if dres is None:
        return K.gemm_nt(d16, wt, out_dtype=torch.float32)
    return K.gemm_nt(d16, wt, out_dtype=torch.float32, epilogue=EPI_BIAS_RESIDUAL, aux=dres)


# ----------------------------------------------------------------------------------------------
# autograd nodes: the stem, and one per block
# ----------------------------------------------------------------------------------------------
class StemFn(torch.autograd.Function):
    """b16 (levit.py:166-175): 4 x (Conv2d 3x3 / stride 2 / pad 1 -> BatchNorm2d), Hardswish between them, on NHWC rows.
    Returns the fp32 token stream [B*N, C] (= flatten(2).transpose(1, 2), levit.py:524) and its bf16 image.  The weight images
    are re-staged every forward (four small casts, < 0.1 M elements for every builder), so a captured graph re-reads them."""

    @staticmethod
    def forward(ctx, img, convs, *params):
        B, _, H, W = img.shape
        src, layers = img.detach().contiguous(), []
        for li, cbn in enumerate(convs):
            c = cbn.c
            Cin, Co = c.in_channels, c.out_channels
            cols, wb, wt = E.conv_cols(src, c.weight, B, Cin, H, W, 3, 2, 1, li > 0)
            st = _BnState(cbn.bn, K.gemm_nt(cols, wb, out_dtype=torch.float32))
            Ho, Wo = K.conv_out_size(H, 3, 2, 1), K.conv_out_size(W, 3, 2, 1)
            layers.append((cols, wt, st, (Cin, H, W)))
            if li < len(convs) - 1:
                _, src = st.apply(cbn.bn.weight, cbn.bn.bias, act=True)
            else:
                x32, x16 = st.apply(cbn.bn.weight, cbn.bn.bias, want_f32=True)
            H, W = Ho, Wo
        ctx.convs, ctx.layers, ctx.B = convs, layers, B
        ctx.mark_non_differentiable(x16)
        return x32, x16

    @staticmethod
    def backward(ctx, dx, _d16):
        convs, layers, B = ctx.convs, ctx.layers, ctx.B
        grads = [None] * (3 * len(convs))
        dz, act = dx.to(torch.float32).contiguous(), False
        for li in range(len(convs) - 1, -1, -1):
            cols, wt, st, (Cin, H, W) = layers[li]
            bn = convs[li].bn
            dy, dg, db = st.backward(dz, bn.weight, bn.bias, act=act)
            grads[3 * li:3 * li + 3] = [E.conv_wgrad(dy, cols, Cin, 3), dg, db]
            if li > 0:
                dz, act = E.conv_dx(dy, wt, B, Cin, H, W, 3, 2, 1), True
        return (None, None, *grads)


class AttnFn(torch.autograd.Function):
    """Residual(Attention) (levit.py:178-195, 240-258): x + sd(proj_bn(hardswish(attn(qkv_bn(x)))))."""

    @staticmethod
    def forward(ctx, x32, x16, meta, keep, survival, wqkv, gqkv, bqkv, table, wproj, gproj, bproj):
        a = meta.mod
        B, N, H, kd, d = meta.B, meta.N, a.num_heads, a.key_dim, a.d
        s1 = _linear_bn(x16, a.qkv)
        _, qkv = s1.apply(gqkv, bqkv)
        hs = 2 * kd + d
        o, ao, stats = K.bias_attn_fwd(qkv, qkv[:, kd:], qkv[:, 2 * kd:], hs, hs, hs, table.detach(), meta.index,
                                       B, H, N, N, kd, d, a.robust)
        s2 = _linear_bn(ao, a.proj[1])
        y32, y16 = s2.apply(gproj, bproj, residual=x32.detach(), keep=keep, survival=survival, want_f32=True)
        ctx.meta, ctx.keep, ctx.survival = meta, keep, survival
        ctx.saved = (x16, s1, qkv, o, ao, stats, s2)
        ctx.params = (wqkv, gqkv, bqkv, table, wproj, gproj, bproj)
        ctx.mark_non_differentiable(y16)
        return y32, y16

    @staticmethod
    def backward(ctx, dy, _d16):
        meta = ctx.meta
        a = meta.mod
        B, N, H, kd, d = meta.B, meta.N, a.num_heads, a.key_dim, a.d
        x16, s1, qkv, o, ao, stats, s2 = ctx.saved
        wqkv, gqkv, bqkv, table, wproj, gproj, bproj = ctx.params
        dy = dy.to(torch.float32).contiguous()
        d2, dg2, db2 = s2.backward(dy, gproj, bproj, keep=ctx.keep, survival=ctx.survival)
        dwproj = K.gemm_tn(d2, ao)
        _, wpt = WEIGHTS.get(wproj, True)
        dact = K.gemm_nt(d2, wpt, out_dtype=torch.bfloat16)
        dqkv = torch.empty_like(qkv)
        hs = 2 * kd + d
        dtable = K.bias_attn_bwd(qkv, qkv[:, kd:], qkv[:, 2 * kd:], hs, hs, hs, table.detach(), meta.index, o, dact, stats,
                                 dqkv, dqkv[:, kd:], dqkv[:, 2 * kd:], B, H, N, N, kd, d, a.robust)
        d1, dg1, db1 = s1.backward(dqkv, gqkv, bqkv)
        dwqkv = K.gemm_tn(d1, x16)
        dx = _dx(d1, wqkv, dy)
        return dx, None, None, None, None, dwqkv, dg1, db1, dtable, dwproj, dg2, db2


class MlpFn(torch.autograd.Function):
    """Residual(Linear_BN -> Hardswish -> Linear_BN) (levit.py:467-480)."""

    @staticmethod
    def forward(ctx, x32, x16, mlp, keep, survival, w1, g1, b1, w2, g2, b2):
        s1 = _linear_bn(x16, mlp[0])
        _, h16 = s1.apply(g1, b1, act=True)
        s2 = _linear_bn(h16, mlp[2])
        y32, y16 = s2.apply(g2, b2, residual=x32.detach(), keep=keep, survival=survival, want_f32=True)
        ctx.keep, ctx.survival = keep, survival
        ctx.saved = (x16, s1, h16, s2)
        ctx.params = (w1, g1, b1, w2, g2, b2)
        ctx.mark_non_differentiable(y16)
        return y32, y16

    @staticmethod
    def backward(ctx, dy, _d16):
        x16, s1, h16, s2 = ctx.saved
        w1, g1, b1, w2, g2, b2 = ctx.params
        dy = dy.to(torch.float32).contiguous()
        d2, dg2, db2 = s2.backward(dy, g2, b2, keep=ctx.keep, survival=ctx.survival)
        dw2 = K.gemm_tn(d2, h16)
        dh = _dx(d2, w2, None)
        d1, dg1, db1 = s1.backward(dh, g1, b1, act=True)
        dw1 = K.gemm_tn(d1, x16)
        dx = _dx(d1, w1, dy)
        return dx, None, None, None, None, dw1, dg1, db1, dw2, dg2, db2


class SubsampleFn(torch.autograd.Function):
    """AttentionSubsample (levit.py:380-403): kv_bn(x), q_bn(Subsample(x)), attention with Nq < Nk, proj_bn(hardswish(.))."""

    @staticmethod
    def forward(ctx, x32, x16, meta, wkv, gkv, bkv, wq, gq, bq, table, wproj, gproj, bproj):
        a = meta.mod
        B, Nq, Nk, H, kd, d = meta.B, meta.Nq, meta.N, a.num_heads, a.key_dim, a.d
        skv = _linear_bn(x16, a.kv)
        _, kv = skv.apply(gkv, bkv)
        xs16 = E.rows_bf16(x16, meta.sub_index)
        sq = _linear_bn(xs16, a.q[1])
        _, q = sq.apply(gq, bq)
        o, ao, stats = K.bias_attn_fwd(q, kv, kv[:, kd:], kd, kd + d, kd + d, table.detach(), meta.index, B, H, Nq, Nk, kd, d,
                                       a.robust)
        sp = _linear_bn(ao, a.proj[1])
        y32, y16 = sp.apply(gproj, bproj, want_f32=True)
        ctx.meta = meta
        ctx.saved = (x16, skv, kv, xs16, sq, q, o, ao, stats, sp)
        ctx.params = (wkv, gkv, bkv, wq, gq, bq, table, wproj, gproj, bproj)
        ctx.mark_non_differentiable(y16)
        return y32, y16

    @staticmethod
    def backward(ctx, dy, _d16):
        meta = ctx.meta
        a = meta.mod
        B, Nq, Nk, H, kd, d = meta.B, meta.Nq, meta.N, a.num_heads, a.key_dim, a.d
        x16, skv, kv, xs16, sq, q, o, ao, stats, sp = ctx.saved
        wkv, gkv, bkv, wq, gq, bq, table, wproj, gproj, bproj = ctx.params
        dp, dgp, dbp = sp.backward(dy.to(torch.float32).contiguous(), gproj, bproj)
        dwproj = K.gemm_tn(dp, ao)
        _, wpt = WEIGHTS.get(wproj, True)
        dact = K.gemm_nt(dp, wpt, out_dtype=torch.bfloat16)
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)
        dtable = K.bias_attn_bwd(q, kv, kv[:, kd:], kd, kd + d, kd + d, table.detach(), meta.index, o, dact, stats,
                                 dq, dkv, dkv[:, kd:], B, H, Nq, Nk, kd, d, a.robust)
        d1q, dgq, dbq = sq.backward(dq, gq, bq)
        dwq = K.gemm_tn(d1q, xs16)
        dxs = _dx(d1q, wq, None)
        d1kv, dgkv, dbkv = skv.backward(dkv, gkv, bkv)
        dwkv = K.gemm_tn(d1kv, x16)
        # x feeds both branches: the kv branch's dX plus the q branch's dX scattered back to the subsampled rows
        dx = _dx(d1kv, wkv, K.scatter_rows(dxs, meta.sub_index, B * Nk))
        return dx, None, None, dwkv, dgkv, dbkv, dwq, dgq, dbq, dtable, dwproj, dgp, dbp


class _Meta:
    __slots__ = ("mod", "B", "N", "Nq", "index", "sub_index")

    def __init__(self, mod, B, N, Nq, index, sub_index=None):
        self.mod, self.B, self.N, self.Nq, self.index, self.sub_index = mod, B, N, Nq, index, sub_index


# ----------------------------------------------------------------------------------------------
# index builders (host arithmetic, cached per geometry)
# ----------------------------------------------------------------------------------------------
def attention_offsets(points_q, points_k, stride: int):
    """(idxs, n_offsets): the reference's first-appearance numbering of (|p1 s - p2|) offsets (levit.py:235-244, 338-353)."""
    offsets, idxs = {}, []
    for p1 in points_q:
        for p2 in points_k:
            off = (abs(p1[0] * stride - p2[0]), abs(p1[1] * stride - p2[1]))
            if off not in offsets:
                offsets[off] = len(offsets)
            idxs.append(offsets[off])
    return idxs, len(offsets)


def subsample_index(B: int, r: int, s: int) -> Tensor:
    """Rows of x.view(B, r, r, C)[:, ::s, ::s] (levit.py:290-295) in the [B*r*r, C] stream."""
    ys = torch.arange(0, r, s)
    grid = (ys[:, None] * r + ys[None, :]).reshape(-1)
    return (torch.arange(B)[:, None] * (r * r) + grid[None, :]).reshape(-1).to(torch.int64)


def _bias_index(mod: nn.Module) -> K.BiasIndex:
    """Device copies of the module's attention_bias_idxs (int32) and its inverse, built on the host once per geometry and kept on
    the module for its lifetime: a captured graph reads them by address.  Rebuilt only when the buffer moves or its values
    change; a superseded copy stays alive with the module too."""
    buf, n = mod.attention_bias_idxs, mod.attention_biases.shape[1]
    st = mod.__dict__.setdefault("_bias_index_state", {"key": None, "index": None, "host": None, "kept": []})
    key = (buf.data_ptr(), buf._version, str(buf.device), n)
    if st["key"] != key:
        host = buf.detach().cpu().numpy()
        cur = st["index"]
        if cur is None or cur.idx.device != buf.device or cur.n_offsets != n or not np.array_equal(host, st["host"]):
            if cur is not None:
                st["kept"].append(cur)
            st["index"], st["host"] = K.bias_index(buf, n, buf.device), host
        st["key"] = key
    return st["index"]


# ----------------------------------------------------------------------------------------------
# modules (parameter holders with the reference's names)
# ----------------------------------------------------------------------------------------------
class Conv2d_BN(nn.Sequential):
    """Conv2d (no bias) + BatchNorm2d (levit.py:57-100).  forward(x NCHW) runs the stem's unfold + GEMM + BN kernels (3x3,
    stride 2, pad 1 only) and returns NCHW fp32."""

    def __init__(self, a, b, ks=1, stride=1, pad=0, dilation=1, groups=1, bn_weight_init=1, resolution=-10000):
        super().__init__()
        self.add_module("c", nn.Conv2d(a, b, ks, stride, pad, dilation, groups, bias=False))
        bn = nn.BatchNorm2d(b)
        nn.init.constant_(bn.weight, bn_weight_init)
        nn.init.constant_(bn.bias, 0)
        self.add_module("bn", bn)

    def _check(self) -> None:
        c = self.c
        if c.kernel_size != (3, 3) or c.stride != (2, 2) or c.padding != (1, 1) or c.dilation != (1, 1) or c.groups != 1:
            raise NotImplementedError("only Conv2d(3x3, stride 2, pad 1) (the b16 stem) is implemented")
        if c.out_channels % 8 or (c.in_channels % 8 and c.in_channels != 3):
            raise NotImplementedError("stem channels must be multiples of 8 (the image may have 3)")
        _bn_check(self.bn)

    def forward(self, x: Tensor) -> Tensor:
        E.require_cuda(x)
        self._check()
        B, _, H, W = x.shape
        y32, _ = StemFn.apply(x.to(torch.float32), [self], self.c.weight, self.bn.weight, self.bn.bias)
        Ho, Wo = K.conv_out_size(H, 3, 2, 1), K.conv_out_size(W, 3, 2, 1)
        return y32.reshape(B, Ho, Wo, -1).permute(0, 3, 1, 2)


class Linear_BN(nn.Sequential):
    """Linear (no bias) + BatchNorm1d over all B*N rows (levit.py:103-134).  Runs inside the blocks."""

    def __init__(self, a, b, bn_weight_init=1, resolution=-100000):
        super().__init__()
        self.add_module("c", nn.Linear(a, b, bias=False))
        bn = nn.BatchNorm1d(b)
        nn.init.constant_(bn.weight, bn_weight_init)
        nn.init.constant_(bn.bias, 0)
        self.add_module("bn", bn)

    def forward(self, x: Tensor) -> Tensor:
        raise NotImplementedError("Linear_BN runs inside the LeViT blocks (its BN is fused with the consumer's epilogue)")


class BN_Linear(nn.Sequential):
    """BatchNorm1d + Linear: the classifier head (levit.py:137-163); runs in PyTorch like the ViT / Swin heads."""

    def __init__(self, a, b, bias=True, std=0.02):
        super().__init__()
        self.add_module("bn", nn.BatchNorm1d(a))
        lin = nn.Linear(a, b, bias=bias)
        nn.init.trunc_normal_(lin.weight, std=std)
        if bias:
            nn.init.constant_(lin.bias, 0)
        self.add_module("l", lin)


def b16(n, activation, resolution=224):
    """The convolutional stem (levit.py:166-175): 224 -> 14, channels n/8, n/4, n/2, n."""
    return nn.Sequential(
        Conv2d_BN(3, n // 8, 3, 2, 1, resolution=resolution), activation(),
        Conv2d_BN(n // 8, n // 4, 3, 2, 1, resolution=resolution // 2), activation(),
        Conv2d_BN(n // 4, n // 2, 3, 2, 1, resolution=resolution // 4), activation(),
        Conv2d_BN(n // 2, n, 3, 2, 1, resolution=resolution // 8))


class Residual(nn.Module):
    """x + m(x), with per-sample drop-path in training (levit.py:178-195).  The keep values are drawn as the reference draws
    them, torch.rand(B) >= drop on the input's device, or taken from `keep_source(batch, device)` (tests)."""

    def __init__(self, m, drop):
        super().__init__()
        self.m = m
        self.drop = drop
        self.keep_source: Optional[Callable[[int, torch.device], Tensor]] = None

    def draw(self, batch: int, device):
        """(keep fp32 [batch] or None, survival)."""
        if not (self.training and self.drop > 0):
            return None, 1.0
        if self.keep_source is not None:
            keep = self.keep_source(batch, device).to(device=device, dtype=torch.float32).contiguous()
        else:
            keep = torch.rand(batch, device=device).ge_(self.drop).to(torch.float32)
        return keep, 1.0 - self.drop

    def forward(self, x: Tensor) -> Tensor:
        raise NotImplementedError("Residual runs inside LeViT (its add is fused into the branch's batch-norm apply)")


class Attention(nn.Module):
    """Multi-head attention with a learned offset bias (levit.py:198-281).  Holds the parameters; runs inside LeViT."""

    def __init__(self, dim, key_dim, num_heads=8, attn_ratio=4, activation=None, resolution=14, robust=False):
        super().__init__()
        _check_act(activation)
        self.num_heads = num_heads
        self.robust = robust
        self.scale = key_dim ** -0.5
        self.key_dim = key_dim
        self.nh_kd = nh_kd = key_dim * num_heads
        self.d = int(attn_ratio * key_dim)
        self.dh = int(attn_ratio * key_dim) * num_heads
        self.attn_ratio = attn_ratio
        h = self.dh + nh_kd * 2
        self.qkv = Linear_BN(dim, h, resolution=resolution)
        self.proj = nn.Sequential(activation(), Linear_BN(self.dh, dim, bn_weight_init=0, resolution=resolution))
        points = list(itertools.product(range(resolution), range(resolution)))
        idxs, n = attention_offsets(points, points, 1)
        self.attention_biases = nn.Parameter(torch.zeros(num_heads, n))
        self.register_buffer("attention_bias_idxs", torch.LongTensor(idxs).view(len(points), len(points)))
        self.resolution = resolution
        _check_shapes(key_dim, self.d, len(points), len(points), dim)

    def forward(self, x: Tensor) -> Tensor:
        raise NotImplementedError("Attention runs inside LeViT (its residual is fused into the proj batch norm); call the model")


class Subsample(nn.Module):
    """x.view(B, r, r, C)[:, ::s, ::s] (levit.py:284-295): a row gather inside AttentionSubsample."""

    def __init__(self, stride, resolution):
        super().__init__()
        self.stride = stride
        self.resolution = resolution

    def forward(self, x: Tensor) -> Tensor:
        raise NotImplementedError("Subsample runs inside AttentionSubsample (a row gather of the token stream)")


class AttentionSubsample(nn.Module):
    """Attention whose queries are a strided subset of the tokens (levit.py:298-403).  Runs inside LeViT."""

    def __init__(self, in_dim, out_dim, key_dim, num_heads=8, attn_ratio=2, activation=None, stride=2, resolution=14,
                 resolution_=7, robust=False):
        super().__init__()
        _check_act(activation)
        self.robust = robust
        self.num_heads = num_heads
        self.scale = key_dim ** -0.5
        self.key_dim = key_dim
        self.nh_kd = nh_kd = key_dim * num_heads
        self.d = int(attn_ratio * key_dim)
        self.dh = int(attn_ratio * key_dim) * self.num_heads
        self.attn_ratio = attn_ratio
        self.resolution_ = resolution_
        self.resolution_2 = resolution_ ** 2
        h = self.dh + nh_kd
        self.kv = Linear_BN(in_dim, h, resolution=resolution)
        self.q = nn.Sequential(Subsample(stride, resolution), Linear_BN(in_dim, nh_kd, resolution=resolution_))
        self.proj = nn.Sequential(activation(), Linear_BN(self.dh, out_dim, resolution=resolution_))
        self.stride = stride
        self.resolution = resolution
        points = list(itertools.product(range(resolution), range(resolution)))
        points_ = list(itertools.product(range(resolution_), range(resolution_)))
        idxs, n = attention_offsets(points_, points, stride)
        self.attention_biases = nn.Parameter(torch.zeros(num_heads, n))
        self.register_buffer("attention_bias_idxs", torch.LongTensor(idxs).view(len(points_), len(points)))
        if (resolution - 1) // stride + 1 != resolution_:
            raise NotImplementedError(f"resolution_ {resolution_} is not the strided grid of {resolution} (stride {stride})")
        _check_shapes(key_dim, self.d, len(points_), len(points), in_dim, out_dim)

    def forward(self, x: Tensor) -> Tensor:
        raise NotImplementedError("AttentionSubsample runs inside LeViT; call the model")


def _check_shapes(kd: int, d: int, Nq: int, Nk: int, *dims: int) -> None:
    if kd not in _KD or d not in _DV:
        raise NotImplementedError(f"key_dim {kd} / value dim {d}: the attention kernels take key_dim in {_KD}, value dim in {_DV}")
    if Nk > _NMAX or Nq > Nk:
        raise NotImplementedError(f"{Nq} queries x {Nk} keys: the attention kernels take Nq <= Nk <= {_NMAX} tokens")
    _check_channels(*dims)


def _check_channels(*dims: int) -> None:
    if any(c % 8 for c in dims):
        raise NotImplementedError(f"channel counts {dims} must be multiples of 8")


def _check_backbone(pe) -> List[Conv2d_BN]:
    ok = isinstance(pe, nn.Sequential) and len(pe) == 7
    if ok:
        for i, m in enumerate(pe):
            ok = ok and (isinstance(m, Conv2d_BN) if i % 2 == 0 else isinstance(m, nn.Hardswish))
    if not ok:
        raise NotImplementedError("only the b16 hybrid_backbone (4 x Conv2d_BN with Hardswish between them) is implemented")
    convs = [pe[i] for i in range(0, 7, 2)]
    for c in convs:
        c._check()
    return convs


class LeViT(nn.Module):
    """LeViT (levit.py:406-528) with the reference's constructor arguments, `robust` included."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=[192], key_dim=[64], depth=[12],
                 num_heads=[3], attn_ratio=[2], mlp_ratio=[2], hybrid_backbone=None, down_ops=[],
                 attention_activation=nn.Hardswish, mlp_activation=nn.Hardswish, drop_path=0, robust=False):
        super().__init__()
        _check_act(attention_activation)
        _check_act(mlp_activation)
        self.num_classes = num_classes
        self.num_features = embed_dim[-1]
        self.embed_dim = embed_dim
        self.patch_embed = hybrid_backbone
        self._convs = _check_backbone(hybrid_backbone)
        if self._convs[-1].c.out_channels != embed_dim[0]:
            raise NotImplementedError("the stem must end at embed_dim[0] channels")
        blocks = []
        down_ops = list(down_ops) + [[""]]          # the reference appends to the caller's list (levit.py:445); a copy here
        resolution = img_size // patch_size
        for i, (ed, kd, dpth, nh, ar, mr, do) in enumerate(zip(embed_dim, key_dim, depth, num_heads, attn_ratio, mlp_ratio, down_ops)):
            for _ in range(dpth):
                blocks.append(Residual(Attention(ed, kd, nh, attn_ratio=ar, activation=attention_activation,
                                                 resolution=resolution, robust=robust), drop_path))
                if mr > 0:
                    h = int(ed * mr)
                    blocks.append(Residual(nn.Sequential(
                        Linear_BN(ed, h, resolution=resolution), mlp_activation(),
                        Linear_BN(h, ed, bn_weight_init=0, resolution=resolution)), drop_path))
                    _check_channels(ed, h)
            if do[0] == "Subsample":
                resolution_ = (resolution - 1) // do[5] + 1
                blocks.append(AttentionSubsample(*embed_dim[i:i + 2], key_dim=do[1], num_heads=do[2], attn_ratio=do[3],
                                                 activation=attention_activation, stride=do[5], resolution=resolution,
                                                 resolution_=resolution_, robust=robust))
                resolution = resolution_
                if do[4] > 0:
                    h = int(embed_dim[i + 1] * do[4])
                    blocks.append(Residual(nn.Sequential(
                        Linear_BN(embed_dim[i + 1], h, resolution=resolution), mlp_activation(),
                        Linear_BN(h, embed_dim[i + 1], bn_weight_init=0, resolution=resolution)), drop_path))
            elif do[0] != "":
                raise NotImplementedError(f"down_ops {do[0]!r}: only 'Subsample' is implemented")
        self.blocks = nn.Sequential(*blocks)
        self.head = BN_Linear(embed_dim[-1], num_classes) if num_classes > 0 else nn.Identity()
        self.img_size, self.patch_size = img_size, patch_size

    @torch.jit.ignore
    def no_weight_decay(self):
        return {x for x in self.state_dict().keys() if "attention_biases" in x}

    def forward(self, x: Tensor) -> Tensor:
        E.require_run(x, "LeViT")
        B, _, Hi, Wi = x.shape
        r = Hi
        for _ in self._convs:
            r = K.conv_out_size(r, 3, 2, 1)
        if Hi != Wi or r != self.img_size // self.patch_size:
            raise NrvError(f"image {Hi}x{Wi} gives a {r}-token grid; the model was built for {self.img_size // self.patch_size}")
        for c in self._convs:
            c._check()
        params = []
        for c in self._convs:
            params += [c.c.weight, c.bn.weight, c.bn.bias]
        x32, x16 = StemFn.apply(x.to(torch.float32), self._convs, *params)
        for blk in self.blocks:
            if isinstance(blk, AttentionSubsample):
                a = blk
                for lbn in (a.kv, a.q[1], a.proj[1]):
                    _bn_check(lbn.bn)
                Nq = a.resolution_2
                meta = _Meta(a, B, r * r, Nq, _bias_index(a),
                             E.cached("levit_sub", subsample_index, B, r, a.stride, device=x.device))
                x32, x16 = SubsampleFn.apply(x32, x16, meta, a.kv.c.weight, a.kv.bn.weight, a.kv.bn.bias,
                                             a.q[1].c.weight, a.q[1].bn.weight, a.q[1].bn.bias, a.attention_biases,
                                             a.proj[1].c.weight, a.proj[1].bn.weight, a.proj[1].bn.bias)
                r = a.resolution_
                continue
            keep, survival = blk.draw(B, x.device)
            m = blk.m
            if isinstance(m, Attention):
                for lbn in (m.qkv, m.proj[1]):
                    _bn_check(lbn.bn)
                meta = _Meta(m, B, r * r, r * r, _bias_index(m))
                x32, x16 = AttnFn.apply(x32, x16, meta, keep, survival, m.qkv.c.weight, m.qkv.bn.weight, m.qkv.bn.bias,
                                        m.attention_biases, m.proj[1].c.weight, m.proj[1].bn.weight, m.proj[1].bn.bias)
            else:
                l1, l2 = m[0], m[2]
                _bn_check(l1.bn)
                _bn_check(l2.bn)
                x32, x16 = MlpFn.apply(x32, x16, m, keep, survival, l1.c.weight, l1.bn.weight, l1.bn.bias,
                                       l2.c.weight, l2.bn.weight, l2.bn.bias)
        pooled = x32.reshape(B, r * r, -1).mean(1)
        return self.head(pooled)


def model_factory(C, D, X, N, drop_path, num_classes, fuse, robust):
    embed_dim = [int(x) for x in C.split("_")]
    num_heads = [int(x) for x in N.split("_")]
    depth = [int(x) for x in X.split("_")]
    act = nn.Hardswish
    return LeViT(patch_size=16, embed_dim=embed_dim, num_heads=num_heads, key_dim=[D] * 3, depth=depth, attn_ratio=[2, 2, 2],
                 mlp_ratio=[2, 2, 2],
                 down_ops=[["Subsample", D, embed_dim[0] // D, 4, 2, 2], ["Subsample", D, embed_dim[1] // D, 4, 2, 2]],
                 attention_activation=act, mlp_activation=act, hybrid_backbone=b16(embed_dim[0], activation=act),
                 num_classes=num_classes, drop_path=drop_path, robust=robust)


def LeViT_128S(num_classes=1000, fuse=False, robust=False):
    return model_factory(**specification["LeViT_128S"], num_classes=num_classes, fuse=fuse, robust=robust)


def LeViT_128(num_classes=1000, fuse=False, robust=False):
    return model_factory(**specification["LeViT_128"], num_classes=num_classes, fuse=fuse, robust=robust)


def LeViT_192(num_classes=1000, fuse=False, robust=False):
    return model_factory(**specification["LeViT_192"], num_classes=num_classes, fuse=fuse, robust=robust)


def LeViT_256(num_classes=1000, fuse=False, robust=False):
    return model_factory(**specification["LeViT_256"], num_classes=num_classes, fuse=fuse, robust=robust)


def LeViT_384(num_classes=1000, fuse=False, robust=False):
    return model_factory(**specification["LeViT_384"], num_classes=num_classes, fuse=fuse, robust=robust)
