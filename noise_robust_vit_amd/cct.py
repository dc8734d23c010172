"""Compact Convolutional Transformer (`CCT`) on the HIP path: drop-in for the reference's cct.py.

    from noise_robust_vit_amd.cct import cct_7          # was: from vit_pytorch_robust.cct import cct_7
    model = cct_7(img_size=32, n_conv_layers=1, kernel_size=3, num_classes=100, robust=True).cuda()

Same builders (`cct_2` .. `cct_16`), classes, signatures (the `*args / **kwargs` pass-through included), module tree, state_dict
keys (`tokenizer.conv_layers.i.0.weight`, `classifier.{positional_emb, attention_pool.*, blocks.i.{pre_norm, self_attn.qkv,
self_attn.proj, linear1, norm1, linear2}.*, norm.*, fc.*}`, `class_emb` with seq_pool=False) and construction / init order as
cct.py, so seeded models and reference checkpoints are interchangeable.  `sinusoidal_embedding` is the reference's expression.

Added keywords, all defaulting to the reference's behaviour: `robust=False` on CCT, TransformerClassifier,
TransformerEncoderLayer and Attention selects SinkhornAttention's normalisation (utils.py:1025-1037) instead of softmax;
`attention_dropout=0.1` on CCT; `fused_attention_dropout=False` on the same four classes runs the dropout on the attention
weights inside the fused softmax kernels (kernels.attn_drop_fwd: the mask is a function of a 64-bit seed, regenerated in the
backward, nothing of size n^2 is written) instead of on the composed path's materialised matrix -- robust=True stays
composed.  The reference's CCT hard-wires attention_dropout=0.1, seq_pool=True and dropout_rate=0. in its
call of TransformerClassifier, so passing seq_pool or dropout_rate to CCT raises TypeError (here too), and it passes a
`stochastic_depth=0.1` that the classifier's **kwargs swallows: the knob that works is `stochastic_depth_rate` (default 0.1).
That quirk is kept.

The step on the fp32 stream x [B*n, D]:

    TokenizerFn  per conv layer: nrv_conv_unfold (NCHW image, then bf16 NHWC rows) -> NT GEMM on the tap-major weight image ->
                 nrv_relu_maxpool_fwd (fp32 token stream from the last layer, bf16 rows for the next conv, uint8 argmax kept)
    + positional table, class token (torch: B*n*D elements of plumbing)
    BlockFn      x1 = x + dp(attn(LN_pre x))     encoder.attn_half_fwd (fused softmax / Sinkhorn; weight dropout in training:
                                                 the composed path, or the fused kernels with fused_attention_dropout), per-sample drop path through nrv_sd_add_f32
                 y  = LN_1(x1)                   nrv_layernorm_f32_fwd: the LayerNorm's OUTPUT is the fp32 stream (post-norm)
                 out = y + dp(linear2(gelu(linear1 y)))
    head         nrv_layernorm_f32_fwd -> nrv_seqpool_fwd (or row 0 with seq_pool=False) -> fc (torch, B rows)

The backward mirrors it; the gradient at y is the fp32 stream gradient plus linear1's input gradient, summed by that GEMM's
residual epilogue, and enters nrv_layernorm_f32_bwd as fp32.

Refused with NotImplementedError (nothing is approximated): dropout_rate > 0 in training, a Tokenizer activation other than None
/ nn.ReLU, max_pool=False, conv_bias=True, a conv kernel > 7 or a pooling geometry outside the kernel's (kernel 2 or 3, 1 <= stride
<= kernel, padding <= kernel // 2), an image size other than the constructed one, embedding_dim / dim_feedforward / channel
counts that are not multiples of 8, embedding_dim > 4096, head dims other than 32 / 64 / 80 / 96 / 128, more than 4096 tokens,
attention-map recording, and a direct call of Attention.  CPU tensors raise NrvError.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import encoder as E
from . import kernels as K
from ._lib import EPI_BIAS, EPI_BIAS_RESIDUAL

Tensor = torch.Tensor

__all__ = ["cct_2", "cct_4", "cct_6", "cct_7", "cct_8", "cct_14", "cct_16", "CCT", "Tokenizer", "TransformerClassifier",
           "TransformerEncoderLayer", "Attention", "DropPath", "sinusoidal_embedding"]

MAX_TOKENS = 4096                         # nrv_seqpool_*'s tokens per sample
CONV_OUT_F32 = False                      # the conv GEMM writes bf16 rows; nrv_relu_maxpool_fwd takes both


def exists(val):
    return val is not None


def default(val, d):
    return val if exists(val) else d


def pair(t):
    return t if isinstance(t, tuple) else (t, t)


def cct_2(*args, **kwargs):
    return _cct(num_layers=2, num_heads=2, mlp_ratio=1, embedding_dim=128, *args, **kwargs)


def cct_4(*args, **kwargs):
    return _cct(num_layers=4, num_heads=2, mlp_ratio=1, embedding_dim=128, *args, **kwargs)


def cct_6(*args, **kwargs):
    return _cct(num_layers=6, num_heads=4, mlp_ratio=2, embedding_dim=256, *args, **kwargs)


def cct_7(*args, **kwargs):
    return _cct(num_layers=7, num_heads=4, mlp_ratio=2, embedding_dim=256, *args, **kwargs)


def cct_8(*args, **kwargs):
    return _cct(num_layers=8, num_heads=4, mlp_ratio=2, embedding_dim=256, *args, **kwargs)


def cct_14(*args, **kwargs):
    return _cct(num_layers=14, num_heads=6, mlp_ratio=3, embedding_dim=384, *args, **kwargs)


def cct_16(*args, **kwargs):
    return _cct(num_layers=16, num_heads=6, mlp_ratio=3, embedding_dim=384, *args, **kwargs)


def _cct(num_layers, num_heads, mlp_ratio, embedding_dim, kernel_size=3, stride=None, padding=None, *args, **kwargs):
    stride = default(stride, max(1, (kernel_size // 2) - 1))
    padding = default(padding, max(1, (kernel_size // 2)))
    return CCT(num_layers=num_layers, num_heads=num_heads, mlp_ratio=mlp_ratio, embedding_dim=embedding_dim,
               kernel_size=kernel_size, stride=stride, padding=padding, *args, **kwargs)


def sinusoidal_embedding(n_channels, dim):
    """cct.py:75-80, the same expression (the table is bit-equal to the reference's)."""
    pe = torch.FloatTensor([[p / (10000 ** (2 * (i // 2) / dim)) for i in range(dim)]
                            for p in range(n_channels)])
    pe[:, 0::2] = torch.sin(pe[:, 0::2])
    pe[:, 1::2] = torch.cos(pe[:, 1::2])
    return pe.unsqueeze(0)


# ----------------------------------------------------------------------------------------------
# modules (the reference's names and construction order)
# ----------------------------------------------------------------------------------------------
class Attention(nn.Module):
    """cct.py:84-111.  Holds the parameters; the attention runs inside its TransformerEncoderLayer's schedule."""

    def __init__(self, dim, num_heads=8, attention_dropout=0.1, projection_dropout=0.1, robust=False, fused_attention_dropout=False):
        super().__init__()
        self.heads = num_heads
        head_dim = dim // self.heads
        if dim % 8 or dim > 4096 or head_dim * num_heads != dim or head_dim not in K.ATTN_FUSED_DH:
            raise NotImplementedError(f"Attention dim {dim} / {num_heads} heads: dim % 8 == 0, dim <= 4096 and a head dim of "
                                      f"{K.ATTN_FUSED_DH} (the attention kernels)")
        self.scale = head_dim ** -0.5
        self.robust = bool(robust)
        # dropout on the attention weights inside the fused softmax kernels (kernels.attn_drop_fwd) instead of on a materialised
        # [B, H, n, n] matrix; robust=True keeps the composed path
        self.fused_attention_dropout = bool(fused_attention_dropout)
        self.qkv = nn.Linear(dim, dim * 3, bias=False)
        self.attn_drop = nn.Dropout(attention_dropout)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(projection_dropout)

    def forward(self, x):
        raise NotImplementedError("Attention holds parameters only: a CCT block runs as one fused HIP schedule, call the "
                                  "TransformerEncoderLayer (or TransformerClassifier / CCT) that owns it")


class DropPath(nn.Module):
    """cct.py:144-160: per-sample drop path.  The keep values are drawn on the device (or taken from
    `keep_source(batch, device)`, for tests); inside a block the add runs in nrv_sd_add_f32."""

    def __init__(self, drop_prob=None):
        super().__init__()
        self.drop_prob = float(drop_prob)
        self.keep_source: Optional[Callable[[int, torch.device], Tensor]] = None

    def draw(self, batch: int, device):
        """(keep fp32 [batch], survival) for one call, or None when the branch passes unchanged."""
        if self.drop_prob <= 0. or not self.training:
            return None
        survival = 1.0 - self.drop_prob
        if not survival > 0.0:
            raise NotImplementedError("DropPath with drop_prob >= 1 divides by zero in the reference")
        if self.keep_source is not None:
            keep = self.keep_source(batch, device).to(device=device, dtype=torch.float32).contiguous()
        else:
            keep = torch.empty(batch, dtype=torch.float32, device=device).bernoulli_(survival)
        return keep, survival

    def forward(self, x):
        E.require_cuda(x)
        kd = self.draw(x.shape[0], x.device)
        return x if kd is None else _DropPathFn.apply(x, kd[0], kd[1])


class _DropPathFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, keep, survival: float):
        x2 = x.detach().to(torch.float32).contiguous().reshape(x.shape[0], -1)
        ctx.keep, ctx.survival = keep, survival
        return K.sd_add(torch.zeros_like(x2), x2, keep, survival).reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        d2 = dy.to(torch.float32).contiguous().reshape(dy.shape[0], -1)
        return K.sd_add(torch.zeros_like(d2), d2, ctx.keep, ctx.survival).reshape(dy.shape), None, None


def _sd_add(x: Tensor, branch: Tensor, kd) -> Tensor:
    return K.sd_add(x, branch, kd[0], kd[1], out=branch)


class BlockFn(torch.autograd.Function):
    """One post-norm block on the fp32 stream (cct.py:137-142).  params: pre_norm.{weight, bias}, qkv.weight, proj.{weight,
    bias}, linear1.{weight, bias}, norm1.{weight, bias}, linear2.{weight, bias}.  kd1 / kd2: the drop-path draws (or None)."""

    @staticmethod
    def forward(ctx, x, meta: E.BlockMeta, adrop, kd1, kd2, *params):
        pre_w, pre_b, wqkv, wo, bo, w1, b1, n1w, n1b, w2, b2 = params
        x2, B, N, D = E._as_stream(x)
        E._PENDING.clear()
        train = any(ctx.needs_input_grad)
        if kd1 is None:
            x1, sa = E.attn_half_fwd(x2, B, N, meta, pre_w, pre_b, wqkv, None, wo, bo, residual=True, adrop=adrop)
        else:
            ya, sa = E.attn_half_fwd(x2, B, N, meta, pre_w, pre_b, wqkv, None, wo, bo, residual=False, adrop=adrop)
            x1 = _sd_add(x2, ya, kd1)
        y32, y16, mean, rstd = K.layernorm_f32_fwd(x1, n1w.detach(), n1b.detach(), meta.eps, want_bf16=True)
        w1_b, _ = E.WEIGHTS.get(w1, True)
        w2_b, _ = E.WEIGHTS.get(w2, True)
        h, u = E.fc1_gelu(y16, w1_b, b1.detach(), E.GELU_STREAM_U8 and w1.shape[0] % 64 == 0, save=train)
        if kd2 is None:
            out = K.gemm_nt(h, w2_b, out_dtype=torch.float32, epilogue=EPI_BIAS_RESIDUAL, bias=b2.detach(), aux=y32)
        else:
            out = _sd_add(y32, K.gemm_nt(h, w2_b, out_dtype=torch.float32, epilogue=EPI_BIAS, bias=b2.detach()), kd2)
        ctx.meta, ctx.params, ctx.shape, ctx.kd = meta, params, (B, N, D), (kd1, kd2)
        ctx.saved = (sa, x1, mean, rstd, y16, u, h) if train else None
        return out.reshape(B, N, D)

    @staticmethod
    def backward(ctx, dy):
        pre_w, pre_b, wqkv, wo, bo, w1, b1, n1w, n1b, w2, b2 = ctx.params
        sa, x1, mean, rstd, y16, u, h = ctx.saved
        ctx.saved = None
        meta, (B, N, D), (kd1, kd2) = ctx.meta, ctx.shape, ctx.kd
        d32 = dy.to(torch.float32).contiguous().reshape(B * N, D)
        d16 = K.cast_bf16(d32) if kd2 is None else K.sd_scale_bf16(d32, kd2[0], kd2[1])
        _, w2_t = E.WEIGHTS.get(w2, True)
        _, w1_t = E.WEIGHTS.get(w1, True)
        dw2, db2 = E._dw_db(meta, d16, h, w2, b2)
        du = E.dgelu_bwd(d16, w2_t, u)
        dw1, db1 = E._dw_db(meta, du, y16, w1, b1)
        # the gradient at y: the stream's (fp32) plus linear1's input gradient, summed in the GEMM's residual epilogue
        dyn = K.gemm_nt(du, w1_t, out_dtype=torch.float32, epilogue=EPI_BIAS_RESIDUAL, aux=d32)
        dx1, dx1_16, dg1, dbn1 = K.layernorm_f32_bwd(dyn, x1, n1w.detach(), mean, rstd, want_bf16=kd1 is None)
        if kd1 is not None:
            dx1_16 = K.sd_scale_bf16(dx1, kd1[0], kd1[1])          # the branch sees the kept share, the residual path all of it
        dx, _, ga = E.attn_half_bwd(dx1, dx1_16, sa, B, N, meta, pre_w, pre_b, wqkv, None, wo, bo, residual=True, want_bf16=False)
        E.wgrad_flush(meta)
        dgp, dbp, dwqkv, _, dwo, dbo = ga
        return (dx.reshape(B, N, D), None, None, None, None, dgp, dbp, dwqkv, dwo, dbo, dw1, db1, dg1, dbn1, dw2, db2)


class TransformerEncoderLayer(nn.Module):
    """cct.py:114-142.  forward(src [B, n, d_model]) on the HIP device."""

    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, attention_dropout=0.1, drop_path_rate=0.1, robust=False,
                 fused_attention_dropout=False):
        super().__init__()
        if dim_feedforward % 8 or dim_feedforward < 8:
            raise NotImplementedError(f"dim_feedforward {dim_feedforward}: the kernels take multiples of 8")
        self.pre_norm = nn.LayerNorm(d_model)
        self.self_attn = Attention(dim=d_model, num_heads=nhead, attention_dropout=attention_dropout, projection_dropout=dropout,
                                   robust=robust, fused_attention_dropout=fused_attention_dropout)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout1 = nn.Dropout(dropout)
        self.norm1 = nn.LayerNorm(d_model)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.dropout2 = nn.Dropout(dropout)
        self.drop_path = DropPath(drop_path_rate)
        self.activation = F.gelu
        self._meta = E.BlockMeta(heads=nhead, dim_head=d_model // nhead, eps=1e-5, robust=bool(robust))
        self._site = -2              # the attention-dropout site handed to BlockMeta.mask_source: -(2 + layer index)

    def block_params(self) -> list:
        a = self.self_attn
        return [self.pre_norm.weight, self.pre_norm.bias, a.qkv.weight, a.proj.weight, a.proj.bias, self.linear1.weight,
                self.linear1.bias, self.norm1.weight, self.norm1.bias, self.linear2.weight, self.linear2.bias]

    def forward(self, src, *args, **kwargs):
        E.require_run(src, "CCT")
        if src.dim() != 3 or src.shape[2] != self.pre_norm.normalized_shape[0] or not 1 <= src.shape[1] <= MAX_TOKENS:
            raise NotImplementedError(f"TransformerEncoderLayer takes [B, n <= {MAX_TOKENS}, {self.pre_norm.normalized_shape[0]}], "
                                      f"got {tuple(src.shape)}")
        if self.training and (self.dropout1.p > 0 or self.dropout2.p > 0 or self.self_attn.proj_drop.p > 0):
            raise NotImplementedError("dropout_rate > 0 in training is not implemented for CCT (eval mode runs)")
        if self.pre_norm.eps != self.norm1.eps:
            raise NotImplementedError("pre_norm and norm1 with different eps")
        meta = self._meta
        meta.eps = float(self.pre_norm.eps)
        meta.robust = self.self_attn.robust
        meta.attn_dropout_fused = self.self_attn.fused_attention_dropout
        pa = float(self.self_attn.attn_drop.p) if self.training else 0.0
        if not 0.0 <= pa < 1.0:
            raise NotImplementedError(f"attention dropout probability {pa} outside [0, 1)")
        adrop = (1.0 / (1.0 - pa), self._site, pa) if pa > 0.0 else None
        B = src.shape[0]
        kd1, kd2 = self.drop_path.draw(B, src.device), self.drop_path.draw(B, src.device)
        return BlockFn.apply(src, meta, adrop, kd1, kd2, *self.block_params())


class TokenizerFn(torch.autograd.Function):
    """The conv layers on NHWC rows: returns the fp32 token stream [B, n, C_out] (= 'b c h w -> b (h w) c').  geom: per layer
    (ks, stride, pad, relu, pk, ps, pp).  The weight images are re-staged every forward, so a captured graph re-reads them."""

    @staticmethod
    def forward(ctx, img, geom, *weights):
        if img.requires_grad:
            raise E.NrvError("gradient w.r.t. the input image is not part of this hot path")
        B, Cin, H, W = img.shape
        src, layers, x32 = img.detach().contiguous(), [], None
        for li, (w, (ks, st, pad, relu, pk, ps, pp)) in enumerate(zip(weights, geom)):
            Co = w.shape[0]
            last = li == len(weights) - 1
            cols, wb, wt = E.conv_cols(src, w, B, Cin, H, W, ks, st, pad, li > 0)
            Hc, Wc = K.conv_out_size(H, ks, st, pad), K.conv_out_size(W, ks, st, pad)
            y = K.gemm_nt(cols, wb, out_dtype=torch.float32 if CONV_OUT_F32 else torch.bfloat16)
            x32, src, idx = K.relu_maxpool_fwd(y, B, Hc, Wc, pk, ps, pp, relu=relu, want_f32=last, want_bf16=not last)
            layers.append((cols, wt, idx, (Cin, H, W, Hc, Wc)))
            Cin, H, W = Co, K.maxpool_out_size(Hc, pk, ps, pp), K.maxpool_out_size(Wc, pk, ps, pp)
        ctx.layers, ctx.B, ctx.geom = layers, B, geom
        return x32.reshape(B, H * W, Cin)

    @staticmethod
    def backward(ctx, dx):
        layers, B = ctx.layers, ctx.B
        ctx.layers = None
        grads = [None] * len(layers)
        dout = dx.to(torch.float32).contiguous().reshape(-1, dx.shape[-1])
        for li in range(len(layers) - 1, -1, -1):
            cols, wt, idx, (Cin, H, W, Hc, Wc) = layers[li]
            ks, st, pad, _, pk, ps, pp = ctx.geom[li]
            dy = K.relu_maxpool_bwd(dout, idx, B, Hc, Wc, pk, ps, pp)
            grads[li] = E.conv_wgrad(dy, cols, Cin, ks)
            if li > 0:
                dout = E.conv_dx(dy, wt, B, Cin, H, W, ks, st, pad)    # the previous pool's dout, fp32 NHWC rows
        return (None, None, *grads)


class Tokenizer(nn.Module):
    """cct.py:162-206.  forward(x [B, C, H, W]) -> [B, n, n_output_channels] on the HIP device."""

    def __init__(self,
                 kernel_size, stride, padding,
                 pooling_kernel_size=3, pooling_stride=2, pooling_padding=1,
                 n_conv_layers=1,
                 n_input_channels=3,
                 n_output_channels=64,
                 in_planes=64,
                 activation=None,
                 max_pool=True,
                 conv_bias=False):
        super().__init__()
        if exists(activation) and activation is not nn.ReLU:
            raise NotImplementedError("Tokenizer: the fused pool takes activation=None or nn.ReLU")
        if not max_pool:
            raise NotImplementedError("Tokenizer(max_pool=False) is not implemented")
        if conv_bias:
            raise NotImplementedError("Tokenizer(conv_bias=True) is not implemented (CCT builds its tokenizer without)")
        pk, ps, pp = pooling_kernel_size, pooling_stride, pooling_padding
        if not all(isinstance(v, int) for v in (kernel_size, stride, padding, pk, ps, pp)):
            raise NotImplementedError("Tokenizer: square integer kernel / stride / padding only")
        if not 1 <= kernel_size <= 7 or stride < 1 or not 0 <= padding < kernel_size:
            raise NotImplementedError(f"Tokenizer: conv kernel {kernel_size} stride {stride} padding {padding}: kernels of 1 .. 7 with "
                                      "padding < kernel (nrv_conv_unfold)")
        if pk not in (2, 3) or not 1 <= ps <= pk or not 0 <= pp <= pk // 2:
            raise NotImplementedError(f"Tokenizer: pooling ({pk}, {ps}, {pp}): kernel 2 or 3, 1 <= stride <= kernel, padding <= kernel // 2")
        n_filter_list = [n_input_channels] + \
                        [in_planes for _ in range(n_conv_layers - 1)] + \
                        [n_output_channels]
        if any(c % 8 or c < 8 for c in n_filter_list[1:]):
            raise NotImplementedError(f"Tokenizer channels {n_filter_list[1:]}: the kernels take multiples of 8")
        n_filter_list_pairs = zip(n_filter_list[:-1], n_filter_list[1:])
        self.conv_layers = nn.Sequential(
            *[nn.Sequential(
                nn.Conv2d(chan_in, chan_out,
                          kernel_size=(kernel_size, kernel_size),
                          stride=(stride, stride),
                          padding=(padding, padding), bias=conv_bias),
                nn.Identity() if not exists(activation) else activation(),
                nn.MaxPool2d(kernel_size=pooling_kernel_size,
                             stride=pooling_stride,
                             padding=pooling_padding) if max_pool else nn.Identity()
            )
                for chan_in, chan_out in n_filter_list_pairs
            ])
        self._geom = tuple((kernel_size, stride, padding, exists(activation), pk, ps, pp) for _ in range(n_conv_layers))
        self.apply(self.init_weight)

    def plane(self, height: int, width: int):
        """(rows, columns) of the token grid of a height x width image, or None when a layer's plane runs out."""
        for ks, st, pad, _, pk, ps, pp in self._geom:
            if height + 2 * pad < ks or width + 2 * pad < ks:
                return None
            height, width = K.conv_out_size(height, ks, st, pad), K.conv_out_size(width, ks, st, pad)
            if height + 2 * pp < pk or width + 2 * pp < pk:
                return None
            height, width = K.maxpool_out_size(height, pk, ps, pp), K.maxpool_out_size(width, pk, ps, pp)
        return height, width

    def sequence_length(self, n_channels=3, height=224, width=224):
        """Computed arithmetically (the reference runs a CPU forward on zeros)."""
        hw = self.plane(height, width)
        if hw is None:
            raise NotImplementedError(f"a {height} x {width} image is smaller than the tokenizer's kernels")
        return hw[0] * hw[1]

    def forward(self, x):
        E.require_cuda(x)
        if x.dim() != 4 or x.shape[1] != self.conv_layers[0][0].in_channels or self.plane(x.shape[2], x.shape[3]) is None:
            raise NotImplementedError(f"Tokenizer takes [B, {self.conv_layers[0][0].in_channels}, H, W] images that cover its kernels, "
                                      f"got {tuple(x.shape)}")
        return TokenizerFn.apply(x, self._geom, *[seq[0].weight for seq in self.conv_layers])

    @staticmethod
    def init_weight(m):
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight)


class LayerNormF32Fn(torch.autograd.Function):
    """nn.LayerNorm on the fp32 stream x [B, n, D] -> fp32 (nrv_layernorm_f32_*)."""

    @staticmethod
    def forward(ctx, x, w, b, eps: float):
        x2, B, N, D = E._as_stream(x)
        y, _, mean, rstd = K.layernorm_f32_fwd(x2, w.detach(), b.detach(), eps)
        ctx.saved, ctx.w, ctx.shape = (x2, mean, rstd), w, (B, N, D)
        return y.reshape(B, N, D)

    @staticmethod
    def backward(ctx, dy):
        x2, mean, rstd = ctx.saved
        B, N, D = ctx.shape
        dx, _, dg, db = K.layernorm_f32_bwd(dy.to(torch.float32).contiguous().reshape(B * N, D), x2, ctx.w.detach(), mean, rstd)
        return dx.reshape(B, N, D), dg, db, None


class SeqPoolFn(torch.autograd.Function):
    """softmax_n(Linear(D, 1)(y)) . y (cct.py:286-288): y fp32 [B, n, D] -> [B, D] (nrv_seqpool_*)."""

    @staticmethod
    def forward(ctx, y, weight, bias):
        y2, B, N, D = E._as_stream(y)
        a = weight.detach().reshape(D).contiguous()
        w, out = K.seqpool_fwd(y2, a, bias.detach(), B, N)
        ctx.saved, ctx.shape, ctx.wshape = (y2, a, w), (B, N, D), weight.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        y2, a, w = ctx.saved
        B, N, D = ctx.shape
        dy, da, db = K.seqpool_bwd(dout.to(torch.float32).contiguous(), y2, a, w, B, N)
        return dy.reshape(B, N, D), da.reshape(ctx.wshape), db


class TransformerClassifier(nn.Module):
    """cct.py:209-302 with the reference's constructor arguments, plus `robust` (see the module docstring).
    forward(x [B, n, embedding_dim]) on the HIP device."""

    def __init__(self,
                 seq_pool=True,
                 embedding_dim=768,
                 num_layers=12,
                 num_heads=12,
                 mlp_ratio=4.0,
                 num_classes=1000,
                 dropout_rate=0.1,
                 attention_dropout=0.1,
                 stochastic_depth_rate=0.1,
                 positional_embedding='sine',
                 sequence_length=None,
                 *args, robust=False, fused_attention_dropout=False, **kwargs):
        super().__init__()
        assert positional_embedding in {'sine', 'learnable', 'none'}

        dim_feedforward = int(embedding_dim * mlp_ratio)
        self.embedding_dim = embedding_dim
        self.sequence_length = sequence_length
        self.seq_pool = seq_pool

        assert exists(sequence_length) or positional_embedding == 'none', \
            f"Positional embedding is set to {positional_embedding} and" \
            f" the sequence length was not specified."
        if embedding_dim % 8 or embedding_dim > 4096:
            raise NotImplementedError(f"embedding_dim {embedding_dim}: the kernels take multiples of 8 up to 4096")
        if exists(sequence_length) and sequence_length + (0 if seq_pool else 1) > MAX_TOKENS:
            raise NotImplementedError(f"{sequence_length} tokens: at most {MAX_TOKENS} (class token included)")

        if not seq_pool:
            sequence_length += 1
            self.class_emb = nn.Parameter(torch.zeros(1, 1, self.embedding_dim), requires_grad=True)
        else:
            self.attention_pool = nn.Linear(self.embedding_dim, 1)

        if positional_embedding == 'none':
            self.positional_emb = None
        elif positional_embedding == 'learnable':
            self.positional_emb = nn.Parameter(torch.zeros(1, sequence_length, embedding_dim),
                                               requires_grad=True)
            nn.init.trunc_normal_(self.positional_emb, std=0.2)
        else:
            self.positional_emb = nn.Parameter(sinusoidal_embedding(sequence_length, embedding_dim),
                                               requires_grad=False)

        self.dropout = nn.Dropout(p=dropout_rate)

        dpr = [x.item() for x in torch.linspace(0, stochastic_depth_rate, num_layers)]

        self.blocks = nn.ModuleList([
            TransformerEncoderLayer(d_model=embedding_dim, nhead=num_heads,
                                    dim_feedforward=dim_feedforward, dropout=dropout_rate,
                                    attention_dropout=attention_dropout, drop_path_rate=layer_dpr, robust=robust,
                                    fused_attention_dropout=fused_attention_dropout)
            for layer_dpr in dpr])
        for i, blk in enumerate(self.blocks):
            blk._site = -(2 + i)

        self.norm = nn.LayerNorm(embedding_dim)

        self.fc = nn.Linear(embedding_dim, num_classes)
        self.apply(self.init_weight)

    def grad_groups(self):
        return []

    def forward(self, x):
        E.require_run(x, "CCT")
        if self.training and self.dropout.p > 0:
            raise NotImplementedError("dropout_rate > 0 in training is not implemented for CCT (eval mode runs)")
        if x.dim() != 3 or x.shape[2] != self.embedding_dim:
            raise NotImplementedError(f"TransformerClassifier takes [B, n, {self.embedding_dim}] tokens, got {tuple(x.shape)}")
        if exists(self.sequence_length) and x.shape[1] != self.sequence_length:
            # the reference's padding branch reads a non-existent self.n_channels; a positional table of another length does not add
            raise NotImplementedError(f"{x.shape[1]} tokens, the classifier was built for {self.sequence_length}")
        if x.shape[1] + (0 if self.seq_pool else 1) > MAX_TOKENS:
            raise NotImplementedError(f"{x.shape[1]} tokens: at most {MAX_TOKENS} (class token included)")
        b = x.shape[0]
        x = x.to(torch.float32)
        if not self.seq_pool:
            x = torch.cat((self.class_emb.expand(b, -1, -1), x), dim=1)
        if exists(self.positional_emb):
            x = x + self.positional_emb
        for blk in self.blocks:
            x = blk(x)
        x = LayerNormF32Fn.apply(x, self.norm.weight, self.norm.bias, float(self.norm.eps))
        if self.seq_pool:
            x = SeqPoolFn.apply(x, self.attention_pool.weight, self.attention_pool.bias)
        else:
            x = x[:, 0]
        return self.fc(x)

    @staticmethod
    def init_weight(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=.02)
            if isinstance(m, nn.Linear) and exists(m.bias):
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)


class CCT(nn.Module):
    """cct.py:306-350 with the reference's constructor arguments, plus `robust` and `attention_dropout` (see the module
    docstring; `stochastic_depth_rate`, not `stochastic_depth`, sets the drop-path rate, as in the reference)."""

    def __init__(
        self,
        img_size=224,
        embedding_dim=768,
        n_input_channels=3,
        n_conv_layers=1,
        kernel_size=7,
        stride=2,
        padding=3,
        pooling_kernel_size=3,
        pooling_stride=2,
        pooling_padding=1,
        *args, robust=False, attention_dropout=0.1, fused_attention_dropout=False, **kwargs
    ):
        super().__init__()
        img_height, img_width = pair(img_size)
        self.img_size = (img_height, img_width)

        self.tokenizer = Tokenizer(n_input_channels=n_input_channels,
                                   n_output_channels=embedding_dim,
                                   kernel_size=kernel_size,
                                   stride=stride,
                                   padding=padding,
                                   pooling_kernel_size=pooling_kernel_size,
                                   pooling_stride=pooling_stride,
                                   pooling_padding=pooling_padding,
                                   max_pool=True,
                                   activation=nn.ReLU,
                                   n_conv_layers=n_conv_layers,
                                   conv_bias=False)

        self.classifier = TransformerClassifier(
            sequence_length=self.tokenizer.sequence_length(n_channels=n_input_channels,
                                                           height=img_height,
                                                           width=img_width),
            embedding_dim=embedding_dim,
            seq_pool=True,
            dropout_rate=0.,
            attention_dropout=attention_dropout,
            stochastic_depth=0.1,
            robust=robust,
            fused_attention_dropout=fused_attention_dropout,
            *args, **kwargs)

    def grad_groups(self):
        return []

    def forward(self, x):
        E.require_run(x, "CCT")
        if x.dim() != 4 or tuple(x.shape[2:]) != self.img_size:
            raise NotImplementedError(f"CCT was built for {self.img_size[0]} x {self.img_size[1]} images, got {tuple(x.shape)}")
        x = self.tokenizer(x)
        return self.classifier(x)
