"""CaiT (class-attention image transformer with talking-heads attention) on the HIP hot path: drop-in for the reference's cait.py.

    from noise_robust_vit_amd.cait import CaiT        # was: from vit_pytorch_robust.cait import CaiT
    model = CaiT(image_size=224, patch_size=16, num_classes=100, dim=192, depth=24, cls_depth=2, heads=4, mlp_dim=768,
                 dim_head=48, robust=True).cuda()

The modules take the reference's constructor arguments and hold the same parameters under the same names (pos_embedding,
cls_token, to_patch_embedding.1.*, patch_transformer.layers.i.0.{scale, fn.norm.*, fn.fn.{mix_heads_pre_attn,
mix_heads_post_attn, to_q, to_kv, to_out.0}.*}, ...layers.i.1.{scale, fn.norm.*, fn.fn.net.{0,3}.*}, cls_transformer...,
mlp_head.{0,1}.*), drawn from the RNG in the same order, so seeded models and reference checkpoints are interchangeable.
`CaiT(robust=...)` is an addition: the reference's CaiT builds both transformers with softmax and only its Transformer /
Attention take `robust` (cait.py:80-92, 131); the keyword (default False = the reference) passes it to both transformers.

One autograd node per layer (LayerFn), on the fp32 stream x [B*n, dim]; with a context the keys / values are cat(LN(x), context)
with the context rows NOT normalised (PreNorm normalises x only, cait.py:60-61, 100-103):

    LN -> to_q, to_kv GEMMs (no bias) -> nrv_bgemm q k^T * scale -> talking heads: nrv_th_softmax_fwd, or with robust=True
    nrv_head_mix_fwd(pre) -> nrv_sinkhorn_fwd (3 iterations) -> nrv_head_mix_fwd(post) -> nrv_bgemm attn v -> to_out GEMM + bias ->
    nrv_ls_add_f32 (LayerScale) -> LN -> fc1 + GELU (8-bit gelu' stream) -> fc2 -> nrv_ls_add_f32             (cait.py:95-165)

Class stage: to_kv runs on the B class rows and on the B*N patch rows separately (the fp32 cat of the inputs is never built);
the two bf16 results are copied into one [B, 1 + N, 2 * inner] buffer, which both nrv_bgemm products read through strides.  The
patch rows' gradient is the sum over the class layers.  With robust=True and one query the Sinkhorn weights are uniform, so the
gradients of to_q and mix_heads_pre_attn vanish there; the path runs as everywhere else.

Refused with NotImplementedError (nothing is approximated): dropout / emb_dropout > 0 in training, more than 16 heads or more
than 1025 keys (the talking-heads kernels' range), dim / heads * dim_head / mlp_dim that are not multiples of 8 or dim > 4096,
attention-map recording, and a direct call of Attention / FeedForward / PreNorm / LayerScale (they hold the parameters; a layer
runs as a whole).  CPU tensors raise NrvError.
"""
from __future__ import annotations

from random import randrange
from typing import Optional

import torch
from torch import nn

from . import encoder as E
from . import kernels as K
from ._lib import EPI_NONE, PATCH_P1P2C
from .encoder import WEIGHTS

Tensor = torch.Tensor

__all__ = ["CaiT", "Transformer", "Attention", "FeedForward", "LayerScale", "PreNorm", "dropout_layers"]

def exists(val):
    return val is not None


def dropout_layers(layers, dropout):
    """The layers that survive layer dropout (cait.py:16-30): one host draw from torch's CPU generator per call, and
    random.randrange when every layer was dropped."""
    if dropout == 0:
        return layers
    num_layers = len(layers)
    to_drop = torch.zeros(num_layers).uniform_(0.0, 1.0) < dropout
    if all(to_drop):
        to_drop[randrange(num_layers)] = False
    return [layer for (layer, drop) in zip(layers, to_drop) if not drop]


# ----------------------------------------------------------------------------------------------
# modules (parameter holders with the reference's names and construction order)
# ----------------------------------------------------------------------------------------------
class LayerScale(E.Holder):
    def __init__(self, dim, fn, depth):
        super().__init__()
        if depth <= 18:                  # epsilon detailed in section 2 of the paper (cait.py:39-44)
            init_eps = 0.1
        elif depth > 18 and depth <= 24:
            init_eps = 1e-5
        else:
            init_eps = 1e-6
        self.scale = nn.Parameter(torch.zeros(1, 1, dim).fill_(init_eps))
        self.fn = fn


PreNorm, FeedForward = E.PreNorm, E.FeedForward


class Attention(E.Holder):
    """Talking-heads attention (cait.py:76-120); robust=True normalises with SinkhornAttention instead of softmax."""

    def __init__(self, dim, heads=8, dim_head=64, dropout=0.0, robust=False):
        super().__init__()
        inner_dim = dim_head * heads
        if heads > K.TH_MAX_HEADS:
            raise NotImplementedError(f"{heads} heads: the talking-heads kernels take at most {K.TH_MAX_HEADS}")
        if dim % 8 or inner_dim % 8 or dim > 4096:
            raise NotImplementedError(f"Attention dim {dim}, heads * dim_head {inner_dim}: the GEMMs take multiples of 8 and "
                                      "LayerNorm at most 4096 features")
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.robust = bool(robust)
        self.to_q = nn.Linear(dim, inner_dim, bias=False)
        self.to_kv = nn.Linear(dim, inner_dim * 2, bias=False)
        self.attend = nn.Identity()      # no parameters in either form; the normalisation runs in the layer's schedule
        self.dropout = nn.Dropout(dropout)
        self.mix_heads_pre_attn = nn.Parameter(torch.randn(heads, heads))
        self.mix_heads_post_attn = nn.Parameter(torch.randn(heads, heads))
        self.to_out = nn.Sequential(nn.Linear(inner_dim, dim), nn.Dropout(dropout))


# ----------------------------------------------------------------------------------------------
# the layer
# ----------------------------------------------------------------------------------------------
def _strides(n: int, Nk: int, H: int, dh: int):
    """(row, col, batch, head) element strides of a head's slice of q / out [B*n, H*dh], of k or v inside kv [B, Nk, 2*H*dh] and
    of the same read transposed, and of a head's [n, Nk] block of a [B,H,n,Nk] matrix and of that read transposed."""
    inner = H * dh
    return ((inner, 1, n * inner, dh), (2 * inner, 1, Nk * 2 * inner, dh), (1, 2 * inner, Nk * 2 * inner, dh),
            (Nk, 1, H * n * Nk, n * Nk), (1, Nk, H * n * Nk, n * Nk))


class LayerFn(torch.autograd.Function):
    """One Transformer layer (cait.py:157-165): x1 = x + scale_a * attn(LN x, context);  x2 = x1 + scale_f * ff(LN x1).
    x fp32 [B*n, D]; context fp32 [B*N, D] with its bf16 image c16, or None."""

    @staticmethod
    def forward(ctx, x, context, c16, meta, n1w, n1b, wq, wkv, w1, w2, wo, bo, sa, n2w, n2b, wf1, bf1, wf2, bf2, sf):
        B, n, N, H, dh, scale, robust, eps1, eps2 = meta
        x = x.detach().contiguous()
        inner, Nk, D = H * dh, n + N, x.shape[1]
        dev = x.device
        xn, mean, rstd = K.layernorm_fwd(x, n1w, n1b, eps1)
        wqb, _ = WEIGHTS.get(wq, True)
        wkvb, _ = WEIGHTS.get(wkv, True)
        q = K.gemm_nt(xn, wqb, out_dtype=torch.bfloat16, epilogue=EPI_NONE)
        kv = K.gemm_nt(xn, wkvb, out_dtype=torch.bfloat16, epilogue=EPI_NONE)
        if N:
            kvc = K.gemm_nt(c16, wkvb, out_dtype=torch.bfloat16, epilogue=EPI_NONE)
            both = torch.empty(B, Nk, 2 * inner, dtype=torch.bfloat16, device=dev)
            both[:, :n] = kv.view(B, n, 2 * inner)                 # a copy of bf16 rows, no arithmetic
            both[:, n:] = kvc.view(B, N, 2 * inner)
            kv = both
            del kvc, both
        sq, skv, skvT, mat, _ = _strides(n, Nk, H, dh)
        S = torch.empty(B, H, n, Nk, dtype=torch.float32, device=dev)
        K.bgemm((q, 0), sq, (kv, 0), skvT, (S, 0), mat, B, H, n, Nk, dh, scale)
        w1d, w2d = w1.detach(), w2.detach()
        if robust:
            T = K.head_mix_fwd(S, w1d)
            P, lse, avec, bvec = K.sinkhorn_fwd(T, iters=K.SINKHORN_ITERS)
            del T
            A = K.head_mix_fwd(P, w2d, out_dtype=torch.bfloat16)
            stats = (lse, avec, bvec)
        else:
            P, A = K.th_softmax_fwd(S, w1d, w2d, a_dtype=torch.bfloat16)
            stats = None
        o = torch.empty(B * n, inner, dtype=torch.bfloat16, device=dev)
        K.bgemm((A, 0), mat, (kv, inner), skv, (o, 0), sq, B, H, n, dh, Nk, 1.0)
        y1 = E.linear(o, wo, bo, torch.float32)
        x1 = K.ls_add(x, y1, sa.detach().reshape(D))
        q8 = wf1.shape[0] % 64 == 0                  # mlp_dim: the byte stream needs whole 64-column tiles
        x2, mlp = E.ls_mlp_half_fwd(x1, eps2, n2w, n2b, wf1, bf1, wf2, bf2, sf.detach().reshape(D), q8)
        ctx.meta = meta
        ctx.saved = (x, c16, xn, mean, rstd, q, kv, S, P, A, stats, o, y1, mlp)
        ctx.params = (n1w, wq, wkv, w1, w2, wo, sa, n2w, wf1, wf2, sf)
        return x2

    @staticmethod
    def backward(ctx, dx2):
        B, n, N, H, dh, scale, robust, _, _ = ctx.meta
        x, c16, xn, mean, rstd, q, kv, S, P, A, stats, o, y1, mlp = ctx.saved
        n1w, wq, wkv, w1, w2, wo, sa, n2w, wf1, wf2, sf = ctx.params
        ctx.saved = None
        inner, Nk, D = H * dh, n + N, x.shape[1]
        dev = x.device
        dx2 = dx2.to(torch.float32).contiguous()
        # feed-forward half
        dx1, (dsf, dn2w, dn2b, dwf1, dbf1, dwf2, dbf2) = E.ls_mlp_half_bwd(dx2, mlp, n2w, wf1, wf2, sf.detach().reshape(D))
        # attention half
        dz1, dsa = K.ls_bwd(dx1, y1, sa.detach().reshape(D))
        dwo, dbo = K.gemm_tn(dz1, o, want_dbias=True)
        do = E.dx_sum([(dz1, wo)], torch.bfloat16)
        sq, skv, skvT, mat, matT = _strides(n, Nk, H, dh)
        dq = torch.empty(B * n, inner, dtype=torch.bfloat16, device=dev)
        dkv = torch.empty(B, Nk, 2 * inner, dtype=torch.bfloat16, device=dev)
        K.bgemm((A, 0), matT, (do, 0), sq, (dkv, inner), skv, B, H, Nk, dh, n, 1.0)                 # dV = A^T dO
        dA = torch.empty(B, H, n, Nk, dtype=torch.float32, device=dev)
        K.bgemm((do, 0), sq, (kv, inner), skvT, (dA, 0), mat, B, H, n, Nk, dh, 1.0)                 # dA = dO v^T
        del A
        w1d, w2d = w1.detach(), w2.detach()
        if robust:
            dP, dw2 = K.head_mix_bwd(dA, P, w2d)
            del dA, P
            T = K.head_mix_fwd(S, w1d)
            dT = K.sinkhorn_bwd(T, dP, *stats, iters=K.SINKHORN_ITERS)
            del T, dP
            dS, dw1 = K.head_mix_bwd(dT, S, w1d)
            del dT
        else:
            dS, dw1, dw2 = K.th_softmax_bwd(dA, P, S, w1d, w2d)
            del dA, P
        del S
        K.bgemm((dS, 0), mat, (kv, 0), skv, (dq, 0), sq, B, H, n, dh, Nk, scale)                    # dQ = scale dS k
        K.bgemm((dS, 0), matT, (q, 0), sq, (dkv, 0), skv, B, H, Nk, dh, n, scale)                   # dK = scale dS^T q
        del dS
        dwq = K.gemm_tn(dq, xn)
        dctx = None
        if N:
            dkx = dkv[:, :n].reshape(B * n, 2 * inner).contiguous()
            dkc = dkv[:, n:].reshape(B * N, 2 * inner).contiguous()
            dwkv, _ = E.wgrad([dkx, dkc], [xn, c16], False)
            _, wkvt = WEIGHTS.get(wkv, True)
            dctx = K.gemm_nt(dkc, wkvt, out_dtype=torch.float32)
        else:
            dkx = dkv.view(B * n, 2 * inner)
            dwkv = K.gemm_tn(dkx, xn)
        dxn = E.dx_sum([(dq, wq), (dkx, wkv)], torch.bfloat16)
        dx, _, dn1w, dn1b = K.layernorm_bwd(dxn, x, n1w.detach(), mean, rstd, dres=dx1)
        return (dx, dctx, None, None, dn1w, dn1b, dwq.reshape(wq.shape), dwkv.reshape(wkv.shape), dw1, dw2, dwo.reshape(wo.shape),
                dbo, dsa.reshape(sa.shape), dn2w, dn2b, dwf1, dbf1, dwf2, dbf2,
                dsf.reshape(sf.shape))


class Transformer(nn.Module):
    """cait.py:123-165.  forward(x [B, n, dim], context [B, N, dim] or None) on the HIP device; layer dropout draws on the host
    whenever it is called, in eval mode too, as the reference does."""

    def __init__(self, dim, depth, heads, dim_head, mlp_dim, dropout=0.0, layer_dropout=0.0, robust=False):
        super().__init__()
        self.layers = nn.ModuleList([])
        self.layer_dropout = layer_dropout
        self.dropout = dropout
        for ind in range(depth):
            self.layers.append(nn.ModuleList([
                LayerScale(dim, PreNorm(dim, Attention(dim, heads=heads, dim_head=dim_head, dropout=dropout, robust=robust)),
                           depth=ind + 1),
                LayerScale(dim, PreNorm(dim, FeedForward(dim, mlp_dim, dropout=dropout)), depth=ind + 1),
            ]))

    def _check_forward(self, x, context=None) -> None:
        if context is not None:
            E.require_cuda(context)                  # ahead of the recording refusal, as a CPU x is
        E.require_run(x, "CaiT")
        if self.training and self.dropout > 0:
            raise NotImplementedError("dropout > 0 in training is not implemented for CaiT (eval mode runs)")
        if x.dim() != 3 or (context is not None and (context.dim() != 3 or context.shape[0] != x.shape[0] or
                                                     context.shape[2] != x.shape[2])):
            raise NotImplementedError("Transformer takes x [B, n, dim] and a context [B, N, dim]")
        n, N = x.shape[1], (context.shape[1] if context is not None else 0)
        for attn, _ in self.layers:
            if not K.th_shape_ok(attn.fn.fn.heads, n, n + N):
                raise NotImplementedError(f"{n} queries x {n + N} keys with {attn.fn.fn.heads} heads: the talking-heads kernels "
                                          f"take at most {K.TH_MAX_KEYS} keys and {K.TH_MAX_HEADS} heads")

    def run(self, x: Tensor, B: int, n: int, context: Optional[Tensor] = None, N: int = 0) -> Tensor:
        """x fp32 [B*n, D] (and context fp32 [B*N, D]) -> [B*n, D]"""
        layers = dropout_layers(self.layers, dropout=self.layer_dropout)
        c16 = K.cast_bf16(context.detach()) if context is not None else None
        for attn, ff in layers:
            a, f = attn.fn.fn, ff.fn.fn
            meta = (B, n, N, a.heads, a.to_q.out_features // a.heads, float(a.scale), a.robust, float(attn.fn.norm.eps),
                    float(ff.fn.norm.eps))
            x = LayerFn.apply(x, context, c16, meta, attn.fn.norm.weight, attn.fn.norm.bias, a.to_q.weight, a.to_kv.weight,
                              a.mix_heads_pre_attn, a.mix_heads_post_attn, a.to_out[0].weight, a.to_out[0].bias, attn.scale,
                              ff.fn.norm.weight, ff.fn.norm.bias, f.net[0].weight, f.net[0].bias, f.net[3].weight, f.net[3].bias,
                              ff.scale)
        return x

    def forward(self, x, context=None):
        self._check_forward(x, context)
        B, n, D = x.shape
        c, N = None, 0
        if context is not None:
            N = context.shape[1]
            c = context.to(torch.float32).contiguous().reshape(B * N, D)
        return self.run(x.to(torch.float32).contiguous().reshape(B * n, D), B, n, c, N).reshape(B, n, D)


class CaiT(nn.Module):
    """cait.py:168-232 with the reference's constructor arguments, plus `robust` (see the module docstring)."""

    def __init__(self, *, image_size, patch_size, num_classes, dim, depth, cls_depth, heads, mlp_dim, dim_head=64, dropout=0.0,
                 emb_dropout=0.0, layer_dropout=0.0, robust=False):
        super().__init__()
        assert image_size % patch_size == 0, "Image dimensions must be divisible by the patch size."
        num_patches = (image_size // patch_size) ** 2
        patch_dim = 3 * patch_size ** 2
        self.patch_size = patch_size
        self.to_patch_embedding = nn.Sequential(E.Rearrange('b c (h p1) (w p2) -> b (h w) (p1 p2 c)', p1=patch_size, p2=patch_size),
                                                nn.Linear(patch_dim, dim))
        self.pos_embedding = nn.Parameter(torch.randn(1, num_patches, dim))
        self.cls_token = nn.Parameter(torch.randn(1, 1, dim))
        self.dropout = nn.Dropout(emb_dropout)
        self.patch_transformer = Transformer(dim, depth, heads, dim_head, mlp_dim, dropout, layer_dropout, robust=robust)
        self.cls_transformer = Transformer(dim, cls_depth, heads, dim_head, mlp_dim, dropout, layer_dropout, robust=robust)
        self.mlp_head = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, num_classes))

    @property
    def layer_dropout(self) -> float:
        return max(self.patch_transformer.layer_dropout, self.cls_transformer.layer_dropout)

    def _check_forward(self, img) -> None:
        E.require_run(img, "CaiT")
        if self.training and (self.dropout.p > 0 or self.patch_transformer.dropout > 0 or self.cls_transformer.dropout > 0):
            raise NotImplementedError("dropout / emb_dropout > 0 in training is not implemented for CaiT (eval mode runs)")
        p = self.patch_size
        if img.dim() != 4 or img.shape[1] != 3 or img.shape[2] % p or img.shape[3] % p:
            raise NotImplementedError(f"image {tuple(img.shape)}: CaiT takes [B, 3, H, W] with sides that are multiples of {p}")
        n = (img.shape[2] // p) * (img.shape[3] // p)
        if n > self.pos_embedding.shape[1]:
            raise NotImplementedError(f"{n} patches but the positional table has {self.pos_embedding.shape[1]} rows")
        heads = [a.fn.fn.heads for t in (self.patch_transformer, self.cls_transformer) for a, _ in t.layers]
        if n + 1 > K.TH_MAX_KEYS or any(h > K.TH_MAX_HEADS for h in heads):
            raise NotImplementedError(f"{n} patches + the class key: the talking-heads kernels take at most {K.TH_MAX_KEYS} keys and "
                                      f"{K.TH_MAX_HEADS} heads")

    def forward(self, img: Tensor) -> Tensor:
        self._check_forward(img)
        B, D = img.shape[0], self.cls_token.shape[-1]
        lin = self.to_patch_embedding[1]
        p = self.patch_size
        n = (img.shape[2] // p) * (img.shape[3] // p)
        x = E.PatchEmbedFn.apply(img, lin.weight, lin.bias, self.pos_embedding[:, :n], None, p, PATCH_P1P2C, None)
        x = self.patch_transformer.run(x.reshape(B * n, D), B, n)
        cls = self.cls_token.expand(B, 1, D).reshape(B, D).contiguous()
        cls = self.cls_transformer.run(cls, B, 1, x, n)
        norm, head = self.mlp_head[0], self.mlp_head[1]
        return head(E.LayerNormFn.apply(cls, norm.weight, norm.bias, float(norm.eps)))
