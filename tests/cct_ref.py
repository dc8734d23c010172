"""References for CCT.

(a) The fp32 PyTorch restatement of CCT's forward (cct.py:84-350), the oracle of the GPU model tests.  Written from the
    reference's equations: it walks a noise_robust_vit_amd.cct model for the structure and takes fp32 copies of its weights.

        logits, loss, grads = cct_loss_and_grads(model, x, y, autocast=False, masks=None)

    Runs on the device of `x`.  autocast=True evaluates the same code under torch.autocast(bfloat16): the bf16 leg the GPU tests
    size their bounds with.  `masks` (cct_fixture.unpack_masks) injects the keep masks of the attention dropout and the drop path;
    a training-mode model that drops needs them.

(b) fp64 per-element references of the three kernel families of csrc/nrv_cct.hip, the bound of each, an fp32 emulation of each
    kernel's arithmetic (tests/test_cct_ref_host.py shows the bounds hold for it and that wrong kernels break them) and the seeded
    inputs the GPU kernel test and the host test share.  The bounds are derived, not tuned (method of pit_ref.py): one bf16
    rounding costs 2^-8 |ref| (BF16), n fp32 operations on a sum lose at most n 2^-23 sum |terms| (U32).

    ReLU + max pool.  The forward copies values: out and idx are exact equalities with max_pool2d(relu(y)) in fp64 and the tap
      of its first maximum (idx 255 where relu leaves nothing).  The backward sums at most ceil(pk / ps)^2 fp32 terms and rounds
      once: BF16 |ref| + ceil(pk / ps)^2 U32 sum |terms|; an element nobody selected has bound 0 (an exact zero).
    LayerNorm (fp32 in, fp32 out).  The derivation of tests/norm_ref.py (its docstring: mean, x^, rstd, y, dx, dgamma, dbeta) with
      this kernel's path lengths: n_sum = 4 J + 6 (J 4-element chunks per lane, then a 6-step shuffle tree), n_col = R rows per
      wave (R = max(8, ceil(rows / 4096))) + 4 waves of a workgroup + ceil(P / 64) + 64 for the P partial rows, one per
      workgroup; the bf16 store term ub |.| only on the bf16 copies.
    Sequence pooling, forward.  Logit: (D + 2) U32 (sum_d |y a| + |bias|) = el.  Weight: exp of l - max carries 2 max el +
      U32 |l - max| absolutely, i.e. relatively on w, plus expf, the n-term sum and the division: (n + 8) U32, and 2^-126
      absolutely (fp32 underflows where fp64 does not).  out: sum_n bound(w_n) |y_n| + n U32 sum_n |w_n y_n|.
    Sequence pooling, backward (w is an input).  t_n: et = (D + 2) U32 sum_d |dout y|.  s = sum w t: es = sum w et + n' U32 sum
      |w t|, n' = ceil(n / 256) + 10 (per-thread strides, then the 8-step tree).  dl_n: w_n (et_n + es + U32 (|t_n| + |s|)) + 2 U32
      |dl_n| = edl.  dy: edl |a| + 3 U32 (|w dout| + |dl a|).  da: sum edl |y| + (n + B + 2) U32 sum |dl y|.  dbias: sum edl +
      (n' + B) U32 sum |dl|.
"""
from __future__ import annotations

import contextlib
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import norm_ref as NR
from rvt_ref import BF16, U32, _gen, bf16, ratio, sinkhorn  # noqa: F401


# ----------------------------------------------------------------------------------------------
# (a) the model
# ----------------------------------------------------------------------------------------------
def _block(P, p, x, blk, masks, li):
    D = x.shape[-1]
    heads = blk.self_attn.heads
    pa = float(blk.self_attn.attn_drop.p) if blk.training else 0.0
    pd = float(blk.drop_path.drop_prob) if blk.training else 0.0
    if (pa > 0 or pd > 0) and masks is None:
        raise ValueError("a training-mode block that drops needs the recorded masks")
    xn = F.layer_norm(x, (D,), P[p + "pre_norm.weight"], P[p + "pre_norm.bias"], 1e-5)
    B, n, _ = xn.shape
    q, k, v = (t.reshape(B, n, heads, -1).permute(0, 2, 1, 3) for t in F.linear(xn, P[p + "self_attn.qkv.weight"]).chunk(3, dim=-1))
    dots = torch.matmul(q * q.shape[-1] ** -0.5, k.transpose(-1, -2))
    w = torch.softmax(dots.float(), dim=-1)
    if blk.self_attn.robust:
        w = sinkhorn(w)
    if pa > 0:
        w = w * masks["attn"][li].to(w.device, w.dtype) / (1.0 - pa)
    o = torch.matmul(w.to(v.dtype), v).permute(0, 2, 1, 3).reshape(B, n, -1)
    a = F.linear(o, P[p + "self_attn.proj.weight"], P[p + "self_attn.proj.bias"])
    keeps = [None, None]
    if pd > 0:
        keeps = [masks["path"][li][c].to(x.device, torch.float32).reshape(B, 1, 1) / (1.0 - pd) for c in range(2)]
    x = x + (a if keeps[0] is None else a * keeps[0])
    x = F.layer_norm(x, (D,), P[p + "norm1.weight"], P[p + "norm1.bias"], 1e-5)
    u = F.gelu(F.linear(x, P[p + "linear1.weight"], P[p + "linear1.bias"]))
    m = F.linear(u, P[p + "linear2.weight"], P[p + "linear2.bias"])
    return x + (m if keeps[1] is None else m * keeps[1])


def classifier_forward(cls, P, p, x, masks=None):
    B, D = x.shape[0], x.shape[-1]
    if not cls.seq_pool:
        x = torch.cat((P[p + "class_emb"].expand(B, -1, -1), x.to(P[p + "class_emb"].dtype)), dim=1)
    if cls.positional_emb is not None:
        x = x + P[p + "positional_emb"]
    for li, blk in enumerate(cls.blocks):
        x = _block(P, f"{p}blocks.{li}.", x, blk, masks, li)
    x = F.layer_norm(x, (D,), P[p + "norm.weight"], P[p + "norm.bias"], 1e-5)
    if cls.seq_pool:
        l = F.linear(x, P[p + "attention_pool.weight"], P[p + "attention_pool.bias"]).squeeze(-1)
        x = torch.einsum("bn,bnd->bd", torch.softmax(l.float(), dim=1).to(x.dtype), x)
    else:
        x = x[:, 0]
    return F.linear(x, P[p + "fc.weight"], P[p + "fc.bias"])


def forward(model, P, x, masks=None):
    if not hasattr(model, "tokenizer"):
        return classifier_forward(model, P, "", x, masks)
    for li, (seq, (ks, st, pad, relu, pk, ps, pp)) in enumerate(zip(model.tokenizer.conv_layers, model.tokenizer._geom)):
        x = F.conv2d(x, P[f"tokenizer.conv_layers.{li}.0.weight"], stride=st, padding=pad)
        if relu:
            x = F.relu(x)
        x = F.max_pool2d(x, pk, ps, pp)
    return classifier_forward(model.classifier, P, "classifier.", x.flatten(2).transpose(1, 2), masks)


def cct_loss_and_grads(model, x, y, autocast=False, masks=None):
    P = {k: v.detach().to(x.device, torch.float32).clone().requires_grad_(model.training and v.requires_grad)
         for k, v in model.named_parameters()}
    ctx = torch.autocast(x.device.type, dtype=torch.bfloat16) if autocast else contextlib.nullcontext()
    with ctx:
        logits = forward(model, P, x.float(), masks)
    logits = logits.float()
    loss = F.cross_entropy(logits, y)
    grads = {}
    if model.training:
        loss.backward()
        grads = {k: v.grad for k, v in P.items()}
    return logits.detach(), loss.detach(), grads


# ----------------------------------------------------------------------------------------------
# (b) kernel references
# ----------------------------------------------------------------------------------------------
# ---- ReLU + max pool ---------------------------------------------------------------------------
# the kernels have no spatial tile (one thread per token and 8 channels, exact grids); (33, 20) at C = 72 runs 18 workgroups
POOL_PLANES = ((1, 1), (2, 3), (3, 5), (4, 4), (7, 7), (9, 6), (33, 20))
POOL_B = 3
POOL_C = (8, 72)
POOL_GEOMS = ((3, 2, 1), (2, 2, 0), (3, 1, 1))
POOL_KINDS = ("random", "grid", "negative", "onehot")


def pool_valid(H, W, geom) -> bool:
    pk, _, pp = geom
    return H + 2 * pp >= pk and W + 2 * pp >= pk                      # (2, 2, 0) does not fit the 1 x 1 plane: NRV_ERR_SHAPE


def pool_out(n, geom):
    pk, ps, pp = geom
    return (n + 2 * pp - pk) // ps + 1


def pool_inputs(H, W, C, geom, kind="random", dtype=torch.float32):
    """(y rows [B*H*W, C] of `dtype`, dout fp32 rows [B*Ho*Wo, C]).  "grid": half-integers in [-2, 2], so most windows tie;
    "negative": every value < 0 (relu leaves nothing); "onehot": random y, dout one at one token per sample."""
    gen = _gen("cctpool", H, W, C, geom)
    Ho, Wo = pool_out(H, geom), pool_out(W, geom)
    y = torch.randn(POOL_B * H * W, C, generator=gen)
    dout = torch.randn(POOL_B * Ho * Wo, C, generator=gen)
    if kind == "grid":
        y = torch.randint(-4, 5, y.shape, generator=gen).float() / 2
    elif kind == "negative":
        y = -y.abs() - 0.125
    elif kind == "onehot":
        d3 = torch.zeros(POOL_B, Ho * Wo, C)
        for b in range(POOL_B):
            d3[b, (b * 7 + (Ho * Wo) // 2) % (Ho * Wo)] = 1.0
        dout = d3.reshape(-1, C)
    return y.to(dtype).contiguous(), dout.contiguous()


def _to_planes(rows, H, W, dtype=torch.float64):
    return rows.to(dtype).reshape(POOL_B, H, W, rows.shape[1]).permute(0, 3, 1, 2)


def _to_rows(planes):
    B, C, H, W = planes.shape
    return planes.permute(0, 2, 3, 1).reshape(B * H * W, C)


def pool_ref(y, dout, H, W, geom, relu):
    """(out fp64 rows, idx uint8 rows, dy fp64 rows, bound of dy): autograd's max_pool2d(relu(y)) in fp64."""
    pk, ps, pp = geom
    p = _to_planes(y, H, W).clone().requires_grad_(True)
    z = F.relu(p) if relu else p
    out, ind = F.max_pool2d(z, pk, ps, pp, return_indices=True)
    Ho, Wo = out.shape[2:]
    oy = torch.arange(Ho).reshape(1, 1, Ho, 1)
    ox = torch.arange(Wo).reshape(1, 1, 1, Wo)
    tap = (ind // W - (oy * ps - pp)) * pk + (ind % W - (ox * ps - pp))
    if relu:
        tap = torch.where(out > 0, tap, torch.full_like(tap, 255))
    d = _to_planes(dout, Ho, Wo)
    out.backward(d)
    dy = p.grad.clone()
    p.grad = None
    q = _to_planes(y, H, W).clone().requires_grad_(True)
    F.max_pool2d(F.relu(q) if relu else q, pk, ps, pp).backward(d.abs())
    n = math.ceil(pk / ps) ** 2
    return _to_rows(out.detach()), _to_rows(tap).to(torch.uint8), _to_rows(dy), _to_rows(BF16 * dy.abs() + n * U32 * q.grad)


def pool_fwd_emul(y, H, W, geom, relu, tie="first", mark=True):
    """The kernel's walk: ky then kx ascending over the in-bounds taps, a later tap wins when strictly larger.  Wrong kernels
    for the host test: tie="last" (a later tap wins when equal), mark=False (no 255 where relu leaves nothing).
    Returns (out fp32 rows, idx uint8 rows)."""
    pk, ps, pp = geom
    Ho, Wo = pool_out(H, geom), pool_out(W, geom)
    p = F.pad(_to_planes(y, H, W, torch.float32), (pp, pk, pp, pk), value=float("nan"))     # out of bounds: NaN compares false
    best = torch.full((POOL_B, y.shape[1], Ho, Wo), float("nan"))
    tap = torch.zeros(best.shape, dtype=torch.int64)
    for ky in range(pk):
        for kx in range(pk):
            v = p[:, :, ky:ky + ps * Ho:ps, kx:kx + ps * Wo:ps][:, :, :Ho, :Wo]
            upd = (~torch.isnan(v)) & (torch.isnan(best) | ((v >= best) if tie == "last" else (v > best)))
            best = torch.where(upd, v, best)
            tap = torch.where(upd, torch.full_like(tap, ky * pk + kx), tap)
    if relu:
        dead = ~(best > 0)
        best = torch.where(dead, torch.zeros_like(best), best)
        if mark:
            tap = torch.where(dead, torch.full_like(tap, 255), tap)
    return _to_rows(best), _to_rows(tap).to(torch.uint8)


def pool_bwd_emul(dout, idx, H, W, geom):
    """Gather form in fp32: for an input element the windows oy, then ox, ascending are the taps ky, then kx, DESCENDING; one
    bf16 rounding.  Returns bf16 rows."""
    pk, ps, pp = geom
    Ho, Wo = pool_out(H, geom), pool_out(W, geom)
    C = dout.shape[1]
    d, ix = _to_planes(dout, Ho, Wo, torch.float32), _to_planes(idx, Ho, Wo, torch.int64)
    acc = torch.zeros(POOL_B, C, H + 2 * pk, W + 2 * pk)
    for ky in reversed(range(pk)):
        for kx in reversed(range(pk)):
            term = torch.zeros_like(acc)
            term[:, :, ky:ky + ps * Ho:ps, kx:kx + ps * Wo:ps][:, :, :Ho, :Wo] = torch.where(ix == ky * pk + kx, d, torch.zeros_like(d))
            acc = acc + term
    return bf16(_to_rows(acc[:, :, pp:pp + H, pp:pp + W]))


# ---- LayerNorm on the fp32 stream ----------------------------------------------------------------
LN_DIMS = (8, 136, 384, 520, 4096)
LN_ROWS = (1, 3, 37)                       # 37 rows: ten forward workgroups of 4 rows; five backward waves of 8 (the last with 5) in two workgroups
LN_BIG = (32781, 8)                        # more than 8 * 4096 rows: a backward wave walks 9 rows (the other value of the loop bound)
LN_EPS = 1e-5
LN_ROWS_PER_WAVE, LN_MAX_WAVES = 8, 4096


def ln_rpw(rows):
    """rows a backward wave walks, and the number of workgroups (partial rows)"""
    rpw = max(LN_ROWS_PER_WAVE, -(-rows // LN_MAX_WAVES))
    return rpw, -(-(-(-rows // rpw)) // 4)


def ln_inputs(rows, dim, kind="random"):
    """dict of fp32 numpy arrays x, dy [rows, dim], gamma, beta [dim].  kind="constant": every row of x is one value (variance
    0: y = beta)."""
    gen = _gen("cctln", rows, dim)
    x = torch.randn(rows, dim, generator=gen) * 1.5 + torch.randn(rows, 1, generator=gen)
    if kind == "constant":
        x = (torch.randn(rows, 1, generator=gen) * 3).expand(rows, dim).contiguous()
    dy = torch.randn(rows, dim, generator=gen)
    gamma = 1.0 + 0.2 * torch.randn(dim, generator=gen)
    beta = 0.1 * torch.randn(dim, generator=gen)
    return {"n": dim, "x": x.numpy(), "dy": dy.numpy(), "gamma": gamma.numpy(), "beta": beta.numpy(), "dres": None}


def ln_ref(i) -> dict:
    """norm_ref.ln_ref (the definitions in fp64) on these inputs"""
    return NR.ln_ref(SimpleNamespace(eps=LN_EPS, acc=False), i)


def ln_maxj(dim):
    chunks = (dim // 4 + 63) // 64
    return next(s for s in (1, 2, 4, 8, 16) if chunks <= s)


def ln_bounds(i, ref) -> dict:
    """norm_ref.ln_bounds' formulas with this kernel's path lengths; `y16` / `dx16` add the bf16 store term"""
    rows, n = i["x"].shape
    U = NR.U
    n_sum = 4 * ln_maxj(n) + 6
    rpw, P = ln_rpw(rows)
    n_col = rpw + 4 + -(-P // 64) + 64
    x, dy = np.abs(i["x"].astype(np.float64)), np.abs(i["dy"].astype(np.float64))
    g = np.abs(i["gamma"].astype(np.float64))
    xmax = x.max(1)
    K = (xmax + np.abs(ref["mean"])) * ref["rstd"]
    E = 2 * (n_sum + 8) * U * K
    rel_rs = (n_sum + 8) * U + (n_sum * U * K) ** 2
    ymax = np.abs(ref["y"]).max(1)
    G = (dy * g).max(1)
    X = np.maximum(1.0, np.abs(ref["xh"]).max(1))
    core = ref["rstd"] * G * (2 + X) * (2 * (n_sum + 8) * U + E + (n_sum * U * K) ** 2)
    dxmax = np.abs(ref["dx"]).max(1)
    axh = np.abs(ref["xh"])
    y32 = (g.max() * E + 4 * U * ymax)[:, None] + np.zeros_like(x)
    dx32 = (core + np.where(G > 0, 2 * U * dxmax, 0.0))[:, None] + np.zeros_like(x)
    return {"mean": (n_sum + 2) * U * xmax, "rstd": ref["rstd"] * rel_rs, "y": y32, "y16": y32 + NR.UB * np.abs(ref["y"]),
            "dx": dx32, "dx16": dx32 + NR.UB * np.abs(ref["dx"]),
            "dgamma": (dy * (E[:, None] + 4 * U * axh)).sum(0) + n_col * U * (dy * axh).sum(0) + 2 * U * np.abs(ref["dgamma"]),
            "dbeta": n_col * U * dy.sum(0) + 2 * U * np.abs(ref["dbeta"])}


def _wave_sum(v):
    """v fp32 [rows, 64]: the xor-shuffle tree, offsets 32 .. 1; every lane ends with the same value"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lanes ^ o]).astype(np.float32)
    return v[:, 0]


def _lanes(a, J):
    """[rows, dim] -> [rows, J, 64, 4]: chunk j of lane l is elements 4 (l + 64 j) .., zero beyond dim"""
    rows, dim = a.shape
    out = np.zeros((rows, J * 256), dtype=np.float32)
    out[:, :dim] = a
    return out.reshape(rows, J, 64, 4)


def _row_sum(v4):
    """sum of a [rows, J, 64, 4] value: per chunk (a + b) + (c + d), chunks in order per lane, then the tree"""
    f = np.float32
    s = np.zeros(v4.shape[:1] + (64,), dtype=f)
    for j in range(v4.shape[1]):
        c = v4[:, j]
        s = (s + ((c[..., 0] + c[..., 1]).astype(f) + (c[..., 2] + c[..., 3]).astype(f)).astype(f)).astype(f)
    return _wave_sum(s)


def ln_emul(i, wrong=None) -> dict:
    """The kernels' arithmetic in fp32 (numpy): two-pass statistics per wave, R rows per backward wave, the four waves of a
    workgroup added in order, the workgroups' partial rows summed by 64 lanes with stride 64 and then in order.
    wrong="no_c2": a backward that drops the mean of dy gamma."""
    f = np.float32
    x, dy, g, b = i["x"].astype(f), i["dy"].astype(f), i["gamma"].astype(f), i["beta"].astype(f)
    rows, dim = x.shape
    J = ln_maxj(dim)
    inv = f(1.0) / f(dim)
    mu = (_row_sum(_lanes(x, J)) * inv).astype(f)
    d = (x - mu[:, None]).astype(f)
    var = (_row_sum(_lanes((d * d).astype(f), J)) * inv).astype(f)
    rs = (f(1.0) / np.sqrt((var + f(LN_EPS)).astype(f))).astype(f)
    y = (((d * rs[:, None]).astype(f) * g).astype(f) + b).astype(f)
    xh = (d * rs[:, None]).astype(f)
    gg = (dy * g).astype(f)
    c1 = (_row_sum(_lanes((gg * xh).astype(f), J)) * inv).astype(f)
    c2 = (_row_sum(_lanes(gg, J)) * inv).astype(f)
    if wrong == "no_c2":
        c2 = np.zeros_like(c2)
    dx = (((gg - c2[:, None]).astype(f) - (xh * c1[:, None]).astype(f)).astype(f) * rs[:, None]).astype(f)
    rpw, P = ln_rpw(rows)
    waves = np.zeros((P * 4, 2, dim), dtype=f)
    dyx = (dy * xh).astype(f)
    for r in range(rows):
        w = r // rpw
        waves[w, 0] = (waves[w, 0] + dyx[r]).astype(f)
        waves[w, 1] = (waves[w, 1] + dy[r]).astype(f)
    w4 = waves.reshape(P, 4, 2, dim)
    part = (((w4[:, 0] + w4[:, 1]).astype(f) + w4[:, 2]).astype(f) + w4[:, 3]).astype(f)
    lane = np.zeros((64, 2, dim), dtype=f)
    for p in range(P):
        lane[p % 64] = (lane[p % 64] + part[p]).astype(f)
    tot = np.zeros((2, dim), dtype=f)
    for k in range(64):
        tot = (tot + lane[k]).astype(f)
    return {"mean": mu, "rstd": rs, "y": y, "y16": bf16(torch.from_numpy(y)).float().numpy(), "dx": dx,
            "dx16": bf16(torch.from_numpy(dx)).float().numpy(), "dgamma": tot[0], "dbeta": tot[1]}


def ln_ratios(got: dict, ref: dict, bounds: dict) -> dict:
    """name -> max error / bound over the elements, for the names present in `got`"""
    key = {"y16": "y", "dx16": "dx"}
    return {k: ratio(torch.as_tensor(np.asarray(v, dtype=np.float64)), torch.as_tensor(ref[key.get(k, k)]),
                     torch.as_tensor(np.broadcast_to(bounds[k], np.shape(ref[key.get(k, k)])).copy())) for k, v in got.items()}


# ---- sequence pooling ------------------------------------------------------------------------------
SP_NS = (1, 2, 16, 257, 3136, 4096)
SP_DS = (8, 72, 384)
SP_B = 3
SP_KINDS = ("random", "equal", "peaked")
SP_HIGH, SP_LOW = 60.0, -120.0             # nats relative to the other logits ("peaked")


def seqpool_inputs(n, D, kind="random"):
    """(y fp32 [B*n, D], a fp32 [D], bias fp32 [1], dout fp32 [B, D]).  "equal": a = 0, every logit is the bias (uniform w);
    "peaked": a = e_0 and column 0 of y holds the logits: zero but for one token 60 nats above and (n >= 3) one 120 nats below."""
    gen = _gen("cctsp", n, D)
    y = torch.randn(SP_B * n, D, generator=gen)
    a = torch.randn(D, generator=gen) / D ** 0.5
    bias = torch.randn(1, generator=gen)
    dout = torch.randn(SP_B, D, generator=gen)
    if kind == "equal":
        a = torch.zeros(D)
    elif kind == "peaked":
        a = torch.zeros(D)
        a[0] = 1.0
        y3 = y.reshape(SP_B, n, D)
        y3[:, :, 0] = 0.0
        for b in range(SP_B):
            y3[b, (b * 5 + n // 2) % n, 0] = SP_HIGH
            if n >= 3:
                y3[b, (b * 5 + n // 2 + 1) % n, 0] = SP_LOW
    return y.contiguous(), a, bias, dout


def sp_low_rows(n):
    """flat [B, n] positions of the underflowing weight of the "peaked" kind (n >= 3)"""
    return [(b, (b * 5 + n // 2 + 1) % n) for b in range(SP_B)] if n >= 3 else []


def seqpool_fwd_ref(y, a, bias, n):
    """(w fp64 [B, n], its bound, out fp64 [B, D], its bound)"""
    D = y.shape[1]
    y3, a64 = y.double().reshape(SP_B, n, D), a.double()
    l = y3 @ a64 + bias.double()
    el = (D + 2) * U32 * ((y3.abs() @ a64.abs()) + bias.double().abs())
    m = l.max(1, keepdim=True).values
    w = torch.softmax(l, dim=1)
    bw = w * (2 * el.max(1, keepdim=True).values + U32 * (l - m).abs() + (n + 8) * U32) + 2.0 ** -126
    out = torch.einsum("bn,bnd->bd", w, y3)
    bo = torch.einsum("bn,bnd->bd", bw, y3.abs()) + n * U32 * torch.einsum("bn,bnd->bd", w, y3.abs())
    return w, bw, out, bo


def seqpool_bwd_ref(dout, y, a, w, n):
    """From the inputs as stored (w fp32 [B, n] is one): dict name -> (ref fp64, bound) for dy, da, dbias"""
    D = y.shape[1]
    y3, a64, w64, d64 = y.double().reshape(SP_B, n, D), a.double(), w.double(), dout.double()
    t = torch.einsum("bd,bnd->bn", d64, y3)
    et = (D + 2) * U32 * torch.einsum("bd,bnd->bn", d64.abs(), y3.abs())
    np_ = -(-n // 256) + 10
    s = (w64 * t).sum(1, keepdim=True)
    es = (w64 * et).sum(1, keepdim=True) + np_ * U32 * (w64 * t).abs().sum(1, keepdim=True)
    dl = w64 * (t - s)
    edl = w64 * (et + es + U32 * (t.abs() + s.abs())) + 2 * U32 * dl.abs()
    dy = w64[..., None] * d64[:, None, :] + dl[..., None] * a64
    bdy = edl[..., None] * a64.abs() + 3 * U32 * ((w64[..., None] * d64[:, None, :]).abs() + (dl[..., None] * a64).abs())
    da = torch.einsum("bn,bnd->d", dl, y3)
    bda = torch.einsum("bn,bnd->d", edl, y3.abs()) + (n + SP_B + 2) * U32 * torch.einsum("bn,bnd->d", dl.abs(), y3.abs())
    db = dl.sum().reshape(1)
    bdb = (edl.sum() + (np_ + SP_B) * U32 * dl.abs().sum()).reshape(1)
    return {"dy": (dy.reshape(SP_B * n, D), bdy.reshape(SP_B * n, D)), "da": (da, bda), "dbias": (db, bdb)}


def _tree256(v):
    """v fp32 [B, 256]: the LDS tree of block_sum_256 (offsets 128 .. 1)"""
    v = v.clone()
    o = 128
    while o:
        v[:, :o] = v[:, :o] + v[:, o:2 * o]
        o //= 2
    return v[:, 0]


def _strided256(v, n):
    """per-thread partial sums of v [B, n]: thread k adds elements k, k + 256, ... in order -> [B, 256]"""
    acc = torch.zeros(v.shape[0], 256)
    for s in range(0, n, 256):
        c = v[:, s:s + 256]
        acc[:, :c.shape[1]] = acc[:, :c.shape[1]] + c
    return acc


def seqpool_fwd_emul(y, a, bias, n):
    """fp32 in the kernel's order (torch fp32 on the CPU; a dot product's lane order is not followed, its fp32 rounding is)."""
    D = y.shape[1]
    y3 = y.reshape(SP_B, n, D)
    l = (y3 @ a) + bias
    m = l.max(1, keepdim=True).values
    e = torch.exp(l - m)
    w = e / _tree256(_strided256(e, n))[:, None]
    out = torch.zeros(SP_B, D)
    for t in range(n):
        out = torch.addcmul(out, w[:, t:t + 1], y3[:, t])
    return w, out


def seqpool_bwd_emul(dout, y, a, w, n, wrong=None):
    """wrong="no_s": a backward without the sum_m w_m t_m term"""
    D = y.shape[1]
    y3 = y.reshape(SP_B, n, D)
    t = torch.einsum("bd,bnd->bn", dout, y3)
    s = _tree256(_strided256(w * t, n))[:, None]
    if wrong == "no_s":
        s = torch.zeros_like(s)
    dl = w * (t - s)
    db = _tree256(_strided256(dl, n)).sum().reshape(1)
    dy = dl[..., None] * a + w[..., None] * dout[:, None, :]
    part = torch.zeros(SP_B, D)
    for k in range(n):
        part = torch.addcmul(part, dl[:, k:k + 1], y3[:, k])
    da = torch.zeros(D)
    for b in range(SP_B):                     # 64 lanes of stride 64, then in order: index order for the B = 3 samples here
        da = da + part[b]
    return {"dy": dy.reshape(SP_B * n, D), "da": da, "dbias": db}
