"""Tokens-to-token ViT (`T2TViT`) on the HIP path.

Drop-in for the reference's `t2t.py` (`vit_pytorch_robust/t2t.py:32-136`): same keyword-only constructor, same
module tree and state_dict keys (`to_patch_embedding.{3,7}.layers.0.{0,1}...`, `to_patch_embedding.12.{weight,bias}`,
`pos_embedding`, `cls_token`, `transformer.layers...`, `mlp_head.{0,1}...`) and the same parameter draw order.  The stage
transformers and the backbone are `lucid_vit.Transformer`, the module the reference's `from vit_pytorch_robust.vit import
Transformer` intends (its Attention always has `to_out.0`, scale `dim_head ** -0.5`).  One added keyword, `robust=False`, sets
`BlockMeta.robust` on the backbone only; the stage transformers stay softmax.

What runs where (csrc/nrv_t2t.hip, nrv_attn_gen.hip):
  soft split   nn.Unfold(k, stride, stride // 2) as nrv_soft_split_fwd / _bwd on token-major rows; RearrangeImage is addressing
  odd widths   a stage's C = 147, 1323, 11907 features are stored in rows of pad8(C) columns whose pad columns are exact zeros
               everywhere in the residual stream; weights are staged as zero-padded bf16 images, so the padded GEMM K and N are
               exact; nrv_layernorm_pad_* normalises over the true C
  attention    one head of dim C: 128 < pad8(C) <= 192 runs the streaming nrv_attn_wide_* (no [N, N] matrix); the fused head
               dims of nrv_attn_fwd run there; everything else is the composed path (nrv_bgemm + softmax on the matrix)
The last split feeds `Linear(C, dim)` on the NT / TN GEMMs; class token, positions, pooling and the head are PyTorch plumbing
as in lucid_vit.ViT.

Refused with NotImplementedError: dropout / emb_dropout > 0 in training, attention recording, non-square images (every split
uses one kernel, stride and padding for both axes, so a square image gives a square token grid at every stage; the stage
function checks its token count against that grid), a t2t kernel above 7, a per-stage width above 4096 (the last stage may be
wider).
"""
from __future__ import annotations

import math

import torch
from torch import nn

from . import encoder as E
from . import kernels as K
from ._lib import EPI_BIAS, EPI_BIAS_RESIDUAL, NrvError
from .lucid_vit import Transformer

MAX_KERNEL = 7
MAX_STAGE_DIM = 4096


def exists(val):
    return val is not None


def conv_output_size(image_size, kernel_size, stride, padding):
    return int(((image_size - kernel_size + (2 * padding)) / stride) + 1)


class RearrangeImage(nn.Module):
    """'b (h w) c -> b c h w' (t2t.py:25-27).  Inside T2TViT the soft split reads the token rows directly."""

    def forward(self, x):
        h = int(math.sqrt(x.shape[1]))
        return x.reshape(x.shape[0], h, x.shape[1] // h, x.shape[2]).permute(0, 3, 1, 2)


class TokensLast(nn.Module):
    """'b c n -> b n c' (t2t.py:74): the soft-split kernel writes token-major rows, so inside T2TViT this is the identity."""

    def forward(self, x):
        return x.transpose(1, 2)


def _padded(w: torch.Tensor, rows: int, cols: int, blocks: int = 1) -> torch.Tensor:
    """fp32 [blocks * rows, cols] with block i of w's rows at row i * rows, zeros elsewhere (weight staging, once per forward)."""
    w = w.detach()
    r = w.shape[0] // blocks
    out = torch.zeros(blocks * rows, cols, dtype=torch.float32, device=w.device)
    out.view(blocks, rows, cols)[:, :r, :w.shape[1]].copy_(w.reshape(blocks, r, w.shape[1]))
    return out


def _padded_vec(b: torch.Tensor, n: int) -> torch.Tensor:
    out = torch.zeros(n, dtype=torch.float32, device=b.device)
    out[:b.numel()].copy_(b.detach())
    return out


def _attention_kind(cp: int) -> str:
    if K.attn_wide_shape(cp):
        return "wide"
    return "fused" if cp in K.ATTN_FUSED_DH else "composed"


class _SplitFn(torch.autograd.Function):
    """One soft split.  x: the NCHW image (first stage, no gradient) or the residual stream [B*h*w, pad8(C)] of the stage
    before; returns bf16 token rows [B*h'*w', pad8(k*k*C)]."""

    @staticmethod
    def forward(ctx, x, geom):
        B, C, H, W, ks, stride = geom
        if not x.is_cuda:
            raise NrvError("noise_robust_vit_amd runs on the MI355X (HIP) device only; there is no CPU fallback")
        rows = x.dim() == 2
        if rows:
            src = x.detach() if x.dtype == torch.bfloat16 else K.cast_bf16(x.detach().contiguous())
        else:
            src = x.detach().contiguous()
            if src.dtype not in (torch.float32, torch.bfloat16):
                src = src.float()
        ctx.geom, ctx.rows, ctx.ld = geom, rows, (x.shape[1] if rows else 0)
        ctx.in_dtype = x.dtype
        return K.soft_split_fwd(src, B, C, H, W, ks, stride, stride // 2, rows)

    @staticmethod
    def backward(ctx, dcols):
        if not ctx.rows:
            return None, None
        B, C, H, W, ks, stride = ctx.geom
        d16 = dcols if dcols.dtype == torch.bfloat16 else K.cast_bf16(dcols.contiguous())
        dx = K.soft_split_bwd(d16.contiguous(), B, C, H, W, ks, stride, stride // 2, ld=ctx.ld)
        return dx, None


class _StageFn(torch.autograd.Function):
    """One stage transformer layer (t2t.py:76-83: heads = 1, dim_head = mlp_dim = C) on rows of pad8(C) columns.
    x [B*N, Cp] bf16 (the soft split's rows) or fp32 -> fp32 [B*N, Cp]; the pad columns stay zero."""

    @staticmethod
    def forward(ctx, x, meta, ln1_w, ln1_b, wq, wkv, wo, bo, ln2_w, ln2_b, w1, b1, w2, b2):
        B, N, C, eps = meta
        Cp = K.pad8(C)
        x = x.detach().contiguous()
        if tuple(x.shape) != (B * N, Cp):
            raise NrvError(f"stage input is {tuple(x.shape)}, expected [{B * N}, {Cp}]")
        scale = C ** -0.5
        kind = _attention_kind(Cp)
        P = [t.detach() for t in (ln1_w, ln1_b, ln2_w, ln2_b)]
        # zero-padded bf16 images: [q; k; v] blocks of Cp rows each, so that the pad columns of q, k, v are exact zeros
        wqkv_b, wqkv_t = K.cast_transpose(_padded(torch.cat((wq.detach(), wkv.detach()), 0), Cp, Cp, blocks=3))
        wo_b, wo_t = K.cast_transpose(_padded(wo, Cp, Cp))
        w1_b, w1_t = K.cast_transpose(_padded(w1, Cp, Cp))
        w2_b, w2_t = K.cast_transpose(_padded(w2, Cp, Cp))
        bo_p, b1_p, b2_p = _padded_vec(bo, Cp), _padded_vec(b1, Cp), _padded_vec(b2, Cp)

        xn, mean1, rstd1 = K.layernorm_pad_fwd(x, C, P[0], P[1], eps)
        qkv = K.gemm_nt(xn, wqkv_b, out_dtype=torch.bfloat16)
        if kind == "wide":
            o, att = K.attn_wide_fwd(qkv, B, N, 1, Cp, scale)
        elif kind == "fused":
            o, att = K.attn_fwd(qkv, B, N, 1, Cp, scale)
        else:
            o, att = K.attn_composed_fwd(qkv, B, N, 1, Cp, scale, 0)
        x1 = K.gemm_nt(o, wo_b, out_dtype=torch.float32, epilogue=EPI_BIAS_RESIDUAL, bias=bo_p, aux=x)
        xn2, mean2, rstd2 = K.layernorm_pad_fwd(x1, C, P[2], P[3], eps)
        need = any(ctx.needs_input_grad)                    # grad mode is off inside forward: ask what the backward will want
        h, u = E.fc1_gelu(xn2, w1_b, b1_p, q8=False, save=need)
        y = K.gemm_nt(h, w2_b, out_dtype=torch.float32, epilogue=EPI_BIAS_RESIDUAL, bias=b2_p, aux=x1)
        ctx.meta, ctx.kind = meta, kind
        ctx.saved = (x, xn, mean1, rstd1, qkv, o, att, x1, xn2, mean2, rstd2, u, h, P, wqkv_t, wo_t, w1_t, w2_t)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, N, C, _ = ctx.meta
        Cp = K.pad8(C)
        scale = C ** -0.5
        x, xn, mean1, rstd1, qkv, o, att, x1, xn2, mean2, rstd2, u, h, P, wqkv_t, wo_t, w1_t, w2_t = ctx.saved
        ctx.saved = None
        dy = dy.to(torch.float32).contiguous()
        dy16 = K.cast_bf16(dy)
        # MLP half: y = x1 + W2 gelu(W1 LN(x1) + b1) + b2
        dw2, db2 = K.gemm_tn(dy16, h, want_dbias=True)
        du = E.dgelu_bwd(dy16, w2_t, u)
        dw1, db1 = K.gemm_tn(du, xn2, want_dbias=True)
        dxn2 = K.gemm_nt(du, w1_t, out_dtype=torch.bfloat16)
        dx1, dx1_16, dg2, dbt2 = K.layernorm_pad_bwd(dxn2, x1, C, P[2], mean2, rstd2, dres=dy, want_f32=True, want_bf16=True)
        # attention half: x1 = x + Wo attn(Wqkv LN(x)) + bo
        dwo, dbo = K.gemm_tn(dx1_16, o, want_dbias=True)
        do = K.gemm_nt(dx1_16, wo_t, out_dtype=torch.bfloat16)
        if ctx.kind == "wide":
            dqkv = K.attn_wide_bwd(qkv, o, do, att, B, N, 1, Cp, scale)
        elif ctx.kind == "fused":
            dqkv = K.attn_bwd(qkv, o, do, att, B, N, 1, Cp, scale)
        else:
            dqkv = K.attn_composed_bwd(qkv, do, att, B, N, 1, Cp, scale)
        dwqkv = K.gemm_tn(dqkv, xn)
        dxn = K.gemm_nt(dqkv, wqkv_t, out_dtype=torch.bfloat16)
        # the soft split in front takes its gradient in bf16, an fp32 stream in fp32
        to16 = x.dtype == torch.bfloat16
        dx32, dx16, dg1, dbt1 = K.layernorm_pad_bwd(dxn, x, C, P[0], mean1, rstd1, dres=dx1, want_f32=not to16, want_bf16=to16)
        sq = lambda w: w[:C, :C].contiguous()                                  # noqa: E731
        dq = dwqkv[:C, :C].contiguous()
        dkv = torch.cat((dwqkv[Cp:Cp + C, :C], dwqkv[2 * Cp:2 * Cp + C, :C]), 0)
        return (dx16 if to16 else dx32, None, dg1, dbt1, dq, dkv, sq(dwo), dbo[:C].contiguous(), dg2, dbt2,
                sq(dw1), db1[:C].contiguous(), sq(dw2), db2[:C].contiguous())


class _ProjectFn(torch.autograd.Function):
    """The Linear behind the last split (t2t.py:90): cols bf16 [T, pad8(C)] . W^T + b -> fp32 [T, dim], W [dim, C] staged
    zero-padded to pad8(C) columns."""

    @staticmethod
    def forward(ctx, cols, weight, bias):
        C, Cp = weight.shape[1], cols.shape[1]
        wb, wt = K.cast_transpose(_padded(weight, weight.shape[0], Cp))
        y = K.gemm_nt(cols, wb, out_dtype=torch.float32, epilogue=EPI_BIAS, bias=bias.detach())
        ctx.saved = (cols, wt, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        cols, wt, C = ctx.saved
        ctx.saved = None
        d16 = K.cast_bf16(dy.to(torch.float32).contiguous())
        dw, db = K.gemm_tn(d16, cols, want_dbias=True)
        dcols = K.gemm_nt(d16, wt, out_dtype=torch.bfloat16)
        return dcols, dw[:, :C].contiguous(), db


class PatchEmbedding(nn.Sequential):
    """The reference's `to_patch_embedding` Sequential (t2t.py:58-91), run through the soft-split and stage kernels."""

    def forward(self, img):
        E.refuse_recording("T2TViT")
        if img.dim() != 4 or img.shape[2] != img.shape[3]:
            raise NotImplementedError(f"T2TViT takes square [B, C, S, S] images, got {tuple(img.shape)}")
        mods = list(self)
        B, C, size = img.shape[0], img.shape[1], img.shape[2]
        x = img
        if len(mods) % 4 != 1 or not isinstance(mods[-1], nn.Linear):
            raise NrvError("to_patch_embedding must hold (rearrange, nn.Unfold, tokens-last, Transformer | Identity) per stage and a final nn.Linear")
        for i in range(0, len(mods) - 1, 4):
            unfold, stage = mods[i + 1], mods[i + 3]
            if not isinstance(unfold, nn.Unfold) or not isinstance(stage, (Transformer, nn.Identity)):
                raise NrvError(f"to_patch_embedding[{i + 1}] / [{i + 3}] must be nn.Unfold and a Transformer or nn.Identity")
            ks, stride = _one(unfold.kernel_size), _one(unfold.stride)
            if _one(unfold.padding) != stride // 2 or _one(unfold.dilation) != 1:
                raise NotImplementedError("soft splits with padding != stride // 2 or a dilation are not implemented")
            if isinstance(stage, Transformer) and (len(stage.layers) != 1 or stage.layers[0][0].heads != 1
                                                   or stage.layers[0][0].to_q.in_features != C * ks * ks):
                raise NotImplementedError("a stage transformer is one single-head layer of the split's full width")
            x = _SplitFn.apply(x, (B, C, size, size, ks, stride))
            size = K.conv_out_size(size, ks, stride, stride // 2)
            C = C * ks * ks
            if isinstance(stage, Transformer):
                attn, ff = stage.layers[0]
                if self.training and stage.p > 0.0:
                    raise NotImplementedError("dropout > 0 in training is not implemented for T2TViT's stage transformers")
                x = _StageFn.apply(x, (B, size * size, C, attn.norm.eps), attn.norm.weight, attn.norm.bias, attn.to_q.weight,
                                   attn.to_kv.weight, attn.to_out[0].weight, attn.to_out[0].bias, *ff.layer_params())
        lin = mods[-1]
        return _ProjectFn.apply(x, lin.weight, lin.bias).reshape(B, size * size, lin.out_features)


def _one(v) -> int:
    return int(v[0]) if isinstance(v, (tuple, list)) else int(v)


class T2TViT(nn.Module):
    def __init__(self, *, image_size, num_classes, dim, depth=None, heads=None, mlp_dim=None, pool='cls', channels=3,
                 dim_head=64, dropout=0., emb_dropout=0., transformer=None, t2t_layers=((7, 4), (3, 2), (3, 2)), robust=False):
        super().__init__()
        assert pool in {'cls', 'mean'}, 'pool type must be either cls (cls token) or mean (mean pooling)'
        if isinstance(image_size, (tuple, list)):
            if len(image_size) != 2 or image_size[0] != image_size[1]:
                raise NotImplementedError("T2TViT takes square images only")
            image_size = image_size[0]
        if robust and exists(transformer):
            raise ValueError("robust=True configures the built-in backbone; a user-supplied transformer= is used as given")
        layers = []
        layer_dim = channels
        output_image_size = image_size
        for i, (kernel_size, stride) in enumerate(t2t_layers):
            layer_dim *= kernel_size ** 2
            is_first = i == 0
            is_last = i == (len(t2t_layers) - 1)
            if kernel_size > MAX_KERNEL:
                raise NotImplementedError(f"t2t_layers: kernel {kernel_size} > {MAX_KERNEL} is not implemented")
            if not is_last and layer_dim > MAX_STAGE_DIM:
                raise NotImplementedError(f"t2t_layers: stage {i} has {layer_dim} features, more than {MAX_STAGE_DIM}")
            output_image_size = conv_output_size(output_image_size, kernel_size, stride, stride // 2)
            if output_image_size <= 0:
                raise NotImplementedError(f"t2t_layers: stage {i} leaves no tokens at image size {image_size}")
            layers.extend([
                RearrangeImage() if not is_first else nn.Identity(),
                nn.Unfold(kernel_size=kernel_size, stride=stride, padding=stride // 2),
                TokensLast(),
                Transformer(dim=layer_dim, heads=1, depth=1, dim_head=layer_dim, mlp_dim=layer_dim, dropout=dropout)
                if not is_last else nn.Identity(),
            ])
        layers.append(nn.Linear(layer_dim, dim))
        self.to_patch_embedding = PatchEmbedding(*layers)

        self.pos_embedding = nn.Parameter(torch.randn(1, output_image_size ** 2 + 1, dim))
        self.cls_token = nn.Parameter(torch.randn(1, 1, dim))
        self.dropout = nn.Dropout(emb_dropout)

        if not exists(transformer):
            assert all([exists(depth), exists(heads), exists(mlp_dim)]), 'depth, heads, and mlp_dim must be supplied'
            self.transformer = Transformer(dim, depth, heads, dim_head, mlp_dim, dropout)
            self.transformer._meta.robust = bool(robust)
        else:
            self.transformer = transformer
        self.robust = bool(robust)
        self.image_size = image_size
        self.pool = pool
        self.to_latent = nn.Identity()
        self.mlp_head = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, num_classes))

    def grad_groups(self):
        return self.transformer.grad_groups() if hasattr(self.transformer, "grad_groups") else []

    def attach_grad_sink(self, sink) -> None:
        """As lucid_vit.ViT: the backbone's weight gradients go straight into the sink's flat buffer; the odd-width stage
        layers and the projection hand theirs to autograd."""
        if hasattr(self.transformer, "attach_grad_sink"):
            self.transformer.attach_grad_sink(sink)

    def forward(self, img):
        if self.training and (self.dropout.p > 0.0 or getattr(self.transformer, "p", 0.0) > 0.0):
            raise NotImplementedError("dropout / emb_dropout > 0 in training is not implemented for T2TViT")
        E.refuse_recording("T2TViT")
        if img.dim() != 4 or img.shape[2] != img.shape[3]:
            raise NotImplementedError(f"T2TViT takes square [B, C, S, S] images, got {tuple(img.shape)}")
        x = self.to_patch_embedding(img)
        b, n, _ = x.shape
        if n + 1 > self.pos_embedding.shape[1]:
            raise NrvError(f"{n} tokens, but pos_embedding holds {self.pos_embedding.shape[1] - 1}")
        # class token and positions (t2t.py:117-120): plumbing on [B, n + 1, dim], as in lucid_vit.ViT
        x = torch.cat((self.cls_token.expand(b, -1, -1), x), dim=1) + self.pos_embedding[:, :n + 1]
        x = self.transformer(x)
        x = x.mean(dim=1) if self.pool == 'mean' else x[:, 0]
        return self.mlp_head(self.to_latent(x))
