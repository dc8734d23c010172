"""DeepViT (ViT with re-attention) on the HIP hot path: drop-in for the reference's deepvit.py.

    from noise_robust_vit_amd.deepvit import DeepViT        # was: from vit_pytorch_robust.deepvit import DeepViT
    model = DeepViT(image_size=224, patch_size=16, num_classes=100, dim=384, depth=16, heads=12, mlp_dim=1152, dim_head=32,
                    robust=True).cuda()

The modules take the reference's constructor arguments and hold the same parameters under the same names (pos_embedding,
cls_token, to_patch_embedding.1.*, transformer.layers.i.0.fn.norm.*, ...0.fn.fn.{reattn_weights, to_qkv.weight,
reattn_norm.1.{weight, bias}, to_out.0.{weight, bias}}, ...1.fn.norm.*, ...1.fn.fn.net.{0,3}.*, mlp_head.{0,1}.*), drawn from the
RNG in the same order, so seeded models and reference checkpoints are interchangeable.  `robust=...` on DeepViT, Transformer and
Attention is an addition: the reference's DeepViT calls `dots.softmax` directly (deepvit.py:68) and has no robust form; the
keyword (default False = the reference) normalises with SinkhornAttention's three iterations (utils.py:1025-1037) instead.

One autograd node per layer (LayerFn), on the fp32 stream x [B*n, dim]:

    LN -> to_qkv GEMM (no bias; one packed bf16 [B*n, 3*inner] buffer read through strides) -> nrv_bgemm q k^T * scale ->
    re-attention: nrv_reattn_softmax_fwd, or with robust=True nrv_sinkhorn_fwd (3 iterations) -> nrv_reattn_norm_fwd ->
    nrv_bgemm attn v -> to_out GEMM + bias + residual -> LN -> fc1 + GELU (8-bit gelu' stream) -> fc2 + residual  (deepvit.py:60-96)

Re-attention mixes the softmax weights of all heads with reattn_weights and then applies a LayerNorm over the H heads at every
(query, key) position (deepvit.py:47-53, 73-74), so it runs on the materialised [B, H, n, n] matrix.  Kept per layer for the
backward: P in fp32 and the normalised A in bf16 (6 bytes per element); robust=True also keeps the scores S (10 bytes).

Refused with NotImplementedError (nothing is approximated): dropout / emb_dropout > 0 in training, more than 16 heads or more
than 1025 tokens (the re-attention kernels' range), dim / heads * dim_head / mlp_dim that are not multiples of 8 or dim > 4096,
attention-map recording, and a direct call of Attention / FeedForward / PreNorm / Residual (they hold the parameters; a layer
runs as a whole).  CPU tensors raise NrvError.
"""
from __future__ import annotations

import torch
from torch import nn

from . import encoder as E
from . import kernels as K
from ._lib import EPI_BIAS_RESIDUAL, PATCH_P1P2C
from .encoder import WEIGHTS

Tensor = torch.Tensor

__all__ = ["DeepViT", "Transformer", "Attention", "FeedForward", "PreNorm", "Residual"]

# ----------------------------------------------------------------------------------------------
# modules (parameter holders with the reference's names and construction order)
# ----------------------------------------------------------------------------------------------
PreNorm, FeedForward, Residual = E.PreNorm, E.FeedForward, E.Residual


class Attention(E.Holder):
    """Attention with re-attention (deepvit.py:36-81); robust=True normalises with SinkhornAttention instead of softmax."""

    def __init__(self, dim, heads=8, dim_head=64, dropout=0.0, robust=False):
        super().__init__()
        inner_dim = dim_head * heads
        if heads > K.TH_MAX_HEADS:
            raise NotImplementedError(f"{heads} heads: the re-attention kernels take at most {K.TH_MAX_HEADS}")
        if dim % 8 or inner_dim % 8 or dim > 4096:
            raise NotImplementedError(f"Attention dim {dim}, heads * dim_head {inner_dim}: the GEMMs take multiples of 8 and "
                                      "LayerNorm at most 4096 features")
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.robust = bool(robust)
        self.to_qkv = nn.Linear(dim, inner_dim * 3, bias=False)
        self.dropout = nn.Dropout(dropout)
        self.reattn_weights = nn.Parameter(torch.randn(heads, heads))
        # the two permutes around the LayerNorm over heads are the re-attention kernels' indexing
        self.reattn_norm = nn.Sequential(E.Rearrange('b h i j -> b i j h'), nn.LayerNorm(heads), E.Rearrange('b i j h -> b h i j'))
        self.to_out = nn.Sequential(nn.Linear(inner_dim, dim), nn.Dropout(dropout))


# ----------------------------------------------------------------------------------------------
# the layer
# ----------------------------------------------------------------------------------------------
def _strides(n: int, H: int, dh: int):
    """(row, col, batch, head) element strides of a head's slice of out [B*n, H*dh], of q / k / v inside qkv [B*n, 3*H*dh] and of
    the same read transposed, and of a head's [n, n] block of a [B,H,n,n] matrix and of that read transposed."""
    inner = H * dh
    return ((inner, 1, n * inner, dh), (3 * inner, 1, n * 3 * inner, dh), (1, 3 * inner, n * 3 * inner, dh),
            (n, 1, H * n * n, n * n), (1, n, H * n * n, n * n))


class LayerFn(torch.autograd.Function):
    """One Transformer layer (deepvit.py:92-96): x1 = x + attn(LN x);  x2 = x1 + ff(LN x1).  x fp32 [B*n, D]."""

    @staticmethod
    def forward(ctx, x, meta, n1w, n1b, wqkv, wr, rg, rb, wo, bo, n2w, n2b, wf1, bf1, wf2, bf2):
        B, n, H, dh, scale, robust, eps1, epsr, eps2 = meta
        x = x.detach().contiguous()
        inner = H * dh
        dev = x.device
        xn, mean, rstd = K.layernorm_fwd(x, n1w.detach(), n1b.detach(), eps1)
        qkv = K.gemm_nt(xn, WEIGHTS.get(wqkv, True)[0], out_dtype=torch.bfloat16)
        so, sp, spT, mat, _ = _strides(n, H, dh)
        S = torch.empty(B, H, n, n, dtype=torch.float32, device=dev)
        K.bgemm((qkv, 0), sp, (qkv, inner), spT, (S, 0), mat, B, H, n, n, dh, scale)
        wrd, rgd, rbd = wr.detach(), rg.detach(), rb.detach()
        if robust:
            P, lse, avec, bvec = K.sinkhorn_fwd(S, iters=K.SINKHORN_ITERS)
            A = K.reattn_norm_fwd(P, wrd, rgd, rbd, epsr, a_dtype=torch.bfloat16)
            stats = (S, lse, avec, bvec)
        else:
            P, A = K.reattn_softmax_fwd(S, wrd, rgd, rbd, epsr, a_dtype=torch.bfloat16)
            stats = None
        del S
        o = torch.empty(B * n, inner, dtype=torch.bfloat16, device=dev)
        K.bgemm((A, 0), mat, (qkv, 2 * inner), sp, (o, 0), so, B, H, n, dh, n, 1.0)
        x1 = K.gemm_nt(o, WEIGHTS.get(wo, True)[0], out_dtype=torch.float32, epilogue=EPI_BIAS_RESIDUAL, bias=bo.detach(), aux=x)
        need = any(ctx.needs_input_grad)
        mmeta = E.BlockMeta(heads=H, dim_head=dh, eps=eps2)
        x2, mlp = E.mlp_half_fwd(x1, mmeta, n2w.detach(), n2b.detach(), wf1, bf1.detach(), wf2, bf2.detach(), True, save=need)
        ctx.meta = meta
        ctx.saved = (x, xn, mean, rstd, qkv, P, A, stats, o, mlp) if need else None
        ctx.params = (n1w, wqkv, wr, rg, wo, n2w, n2b, wf1, bf1, wf2, bf2)
        return x2

    @staticmethod
    def backward(ctx, dx2):
        B, n, H, dh, scale, robust, _, epsr, eps2 = ctx.meta
        x, xn, mean, rstd, qkv, P, A, stats, o, mlp = ctx.saved
        n1w, wqkv, wr, rg, wo, n2w, n2b, wf1, bf1, wf2, bf2 = ctx.params
        ctx.saved = None
        inner = H * dh
        dev = x.device
        dx2 = dx2.to(torch.float32).contiguous()
        # feed-forward half
        mmeta = E.BlockMeta(heads=H, dim_head=dh, eps=eps2)
        dx1, dx1_16, (dn2w, dn2b, dwf1, dbf1, dwf2, dbf2) = E.mlp_half_bwd(dx2, None, mlp, mmeta, n2w.detach(), n2b.detach(), wf1, bf1,
                                                                            wf2, bf2, True, want_bf16=True)
        # attention half
        dwo, dbo = K.gemm_tn(dx1_16, o, want_dbias=True)
        do = E.dx_sum([(dx1_16, wo)], torch.bfloat16)
        so, sp, spT, mat, matT = _strides(n, H, dh)
        dqkv = torch.empty(B * n, 3 * inner, dtype=torch.bfloat16, device=dev)
        K.bgemm((A, 0), matT, (do, 0), so, (dqkv, 2 * inner), sp, B, H, n, dh, n, 1.0)              # dV = A^T dO
        dA = torch.empty(B, H, n, n, dtype=torch.float32, device=dev)
        K.bgemm((do, 0), so, (qkv, 2 * inner), spT, (dA, 0), mat, B, H, n, n, dh, 1.0)              # dA = dO v^T
        del A
        wrd, rgd = wr.detach(), rg.detach()
        if robust:
            S, lse, avec, bvec = stats
            dP, dwr, drg, drb = K.reattn_norm_bwd(dA, P, wrd, rgd, epsr)
            del dA, P
            dS = K.sinkhorn_bwd(S, dP, lse, avec, bvec, iters=K.SINKHORN_ITERS)
            del dP, S
        else:
            dS, dwr, drg, drb = K.reattn_softmax_bwd(dA, P, wrd, rgd, epsr)
            del dA, P
        K.bgemm((dS, 0), mat, (qkv, inner), sp, (dqkv, 0), sp, B, H, n, dh, n, scale)               # dQ = scale dS k
        K.bgemm((dS, 0), matT, (qkv, 0), sp, (dqkv, inner), sp, B, H, n, dh, n, scale)              # dK = scale dS^T q
        del dS
        dwqkv = K.gemm_tn(dqkv, xn)
        dxn = E.dx_sum([(dqkv, wqkv)], torch.bfloat16)
        dx, _, dn1w, dn1b = K.layernorm_bwd(dxn, x, n1w.detach(), mean, rstd, dres=dx1)
        return (dx, None, dn1w, dn1b, dwqkv.reshape(wqkv.shape), dwr, drg, drb, dwo.reshape(wo.shape), dbo, dn2w, dn2b,
                dwf1, dbf1, dwf2, dbf2)


class Transformer(nn.Module):
    """deepvit.py:83-96.  forward(x [B, n, dim]) on the HIP device."""

    def __init__(self, dim, depth, heads, dim_head, mlp_dim, dropout=0.0, robust=False):
        super().__init__()
        self.layers = nn.ModuleList([])
        self.dropout = dropout
        for _ in range(depth):
            self.layers.append(nn.ModuleList([
                Residual(PreNorm(dim, Attention(dim, heads=heads, dim_head=dim_head, dropout=dropout, robust=robust))),
                Residual(PreNorm(dim, FeedForward(dim, mlp_dim, dropout=dropout))),
            ]))

    def _check_forward(self, x) -> None:
        E.require_run(x, "DeepViT")
        if self.training and self.dropout > 0:
            raise NotImplementedError("dropout > 0 in training is not implemented for DeepViT (eval mode runs)")
        if x.dim() != 3:
            raise NotImplementedError("Transformer takes x [B, n, dim]")
        n = x.shape[1]
        for attn, _ in self.layers:
            if not K.th_shape_ok(attn.fn.fn.heads, n, n):
                raise NotImplementedError(f"{n} tokens with {attn.fn.fn.heads} heads: the re-attention kernels take at most "
                                          f"{K.TH_MAX_KEYS} tokens and {K.TH_MAX_HEADS} heads")

    def run(self, x: Tensor, B: int, n: int) -> Tensor:
        """x fp32 [B*n, D] -> [B*n, D]"""
        for attn, ff in self.layers:
            a, f, ln = attn.fn.fn, ff.fn.fn, attn.fn.fn.reattn_norm[1]
            meta = (B, n, a.heads, a.to_qkv.out_features // (3 * a.heads), float(a.scale), a.robust, float(attn.fn.norm.eps),
                    float(ln.eps), float(ff.fn.norm.eps))
            x = LayerFn.apply(x, meta, attn.fn.norm.weight, attn.fn.norm.bias, a.to_qkv.weight, a.reattn_weights, ln.weight, ln.bias,
                              a.to_out[0].weight, a.to_out[0].bias, ff.fn.norm.weight, ff.fn.norm.bias, f.net[0].weight,
                              f.net[0].bias, f.net[3].weight, f.net[3].bias)
        return x

    def forward(self, x):
        self._check_forward(x)
        B, n, D = x.shape
        return self.run(x.to(torch.float32).contiguous().reshape(B * n, D), B, n).reshape(B, n, D)


class DeepViT(nn.Module):
    """deepvit.py:98-139 with the reference's constructor arguments, plus `robust` (see the module docstring)."""

    def __init__(self, *, image_size, patch_size, num_classes, dim, depth, heads, mlp_dim, pool='cls', channels=3, dim_head=64,
                 dropout=0.0, emb_dropout=0.0, robust=False):
        super().__init__()
        assert image_size % patch_size == 0, 'Image dimensions must be divisible by the patch size.'
        num_patches = (image_size // patch_size) ** 2
        patch_dim = channels * patch_size ** 2
        assert pool in {'cls', 'mean'}, 'pool type must be either cls (cls token) or mean (mean pooling)'
        self.patch_size, self.channels = patch_size, channels
        self.to_patch_embedding = nn.Sequential(
            E.Rearrange('b c (h p1) (w p2) -> b (h w) (p1 p2 c)', p1=patch_size, p2=patch_size), nn.Linear(patch_dim, dim))
        self.pos_embedding = nn.Parameter(torch.randn(1, num_patches + 1, dim))
        self.cls_token = nn.Parameter(torch.randn(1, 1, dim))
        self.dropout = nn.Dropout(emb_dropout)
        self.transformer = Transformer(dim, depth, heads, dim_head, mlp_dim, dropout, robust=robust)
        self.pool = pool
        self.to_latent = nn.Identity()
        self.mlp_head = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, num_classes))

    def _check_forward(self, img) -> None:
        E.require_run(img, "DeepViT")
        if self.training and (self.dropout.p > 0 or self.transformer.dropout > 0):
            raise NotImplementedError("dropout / emb_dropout > 0 in training is not implemented for DeepViT (eval mode runs)")
        p, c = self.patch_size, self.channels
        if img.dim() != 4 or img.shape[1] != c or img.shape[2] % p or img.shape[3] % p:
            raise NotImplementedError(f"image {tuple(img.shape)}: DeepViT takes [B, {c}, H, W] with sides that are multiples of {p}")
        n = (img.shape[2] // p) * (img.shape[3] // p)
        if n + 1 > self.pos_embedding.shape[1]:
            raise NotImplementedError(f"{n} patches but the positional table has {self.pos_embedding.shape[1]} rows")
        heads = [a.fn.fn.heads for a, _ in self.transformer.layers]
        if n + 1 > K.TH_MAX_KEYS or any(h > K.TH_MAX_HEADS for h in heads):
            raise NotImplementedError(f"{n} patches + the class token: the re-attention kernels take at most {K.TH_MAX_KEYS} tokens "
                                      f"and {K.TH_MAX_HEADS} heads")

    def forward(self, img: Tensor) -> Tensor:
        self._check_forward(img)
        B, D = img.shape[0], self.cls_token.shape[-1]
        lin = self.to_patch_embedding[1]
        p = self.patch_size
        n = (img.shape[2] // p) * (img.shape[3] // p) + 1
        x = E.PatchEmbedFn.apply(img, lin.weight, lin.bias, self.pos_embedding[:, :n], self.cls_token, p, PATCH_P1P2C, None)
        x = self.transformer.run(x.reshape(B * n, D), B, n).reshape(B, n, D)
        x = x.mean(dim=1) if self.pool == 'mean' else x[:, 0]      # pooling and the head's Linear are PyTorch plumbing
        norm, head = self.mlp_head[0], self.mlp_head[1]
        return head(E.LayerNormFn.apply(self.to_latent(x), norm.weight, norm.bias, float(norm.eps)))
