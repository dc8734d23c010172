"""fp64 restatement of the two attention families that add a learned, index-addressed bias to the scores -- Swin's shifted-window
attention (csrc/nrv_window_attn.hip) and LeViT's offset-biased attention (csrc/nrv_bias_attn.hip) -- their per-element error bounds,
an fp32 emulation of the kernels' arithmetic, and the seeded inputs of tests/test_biased_attn_edges_gpu.py (test infrastructure,
plain torch, no kernels).

One dense core serves both: dense_core takes fp64 q (already scaled), k, v and an additive bias matrix and returns P0, lse, the
Sinkhorn scalings (peaked_ref.sinkhorn_scalings), o and a hand-written backward (dq, dk, dv, dS).  window_ref builds each window's
bias from table[rel] plus the -100 region mask (the mask by the slice-filling rule of the model, the slots by torch.roll) and
bias_ref takes table[h, idx] and the strided operand views; the table gradients are dS folded through the index.  The operands are
the kernels' own (bf16 q / k / v / dout, fp32 table) upcast to fp64; LeViT's Hardswish' is taken on the kernel's saved bf16 o.

Bounds.  EPS, BF, acc(n, sum|terms|), EXP_REL and excess() are those of pcn_ref.py.  Everything below is first order; HIGHER = 1.01
covers the higher orders.
  * score: S = q . k + bias is kd products, one scale rounding and one or two adds: e_S = acc(kd + 2, sum|q k| + |bias|) (the -100
    of the mask is one of the terms).
  * lse = m + log(sum exp(S - m)): a score error moves lse by at most the row's largest e_S; the sum of Nk positive terms through
    __expf and the __logf add 2 EXP_REL + (Nk + 8) EPS; the final add 4 EPS |lse|.
  * P0: relative error rP = e_S + (row's largest e_S + 3 EXP_REL + (Nk + 16) EPS + 4 EPS |lse|), whether formed as exp(S - m) / l
    (forward) or as exp(S - lse) from the saved fp32 lse (backward).
  * scalings: a_t = 1 / sum_j P0 b_{t-1} is a sum of positive terms, so its relative error is the weighted mean of the terms'
    relative errors (rP + the error of b_{t-1}) plus (Nk + 10) EPS for the sum and the reciprocal; b_t likewise from a_t.  The
    chain is carried per element and so grows with the step: a1 < b1 < a2 < ... < a4.
  * o = sum_j P_ij v_j: sum_j P_ij |v_j| (relative error of P_ij) + acc(Nk, sum P |v|), with P = a4 P0 b3 carrying the errors of
    a4 and b3; a bf16 output gets BF |ref| on top.  ao = hardswish(o) is taken on the fp32 o: slope at most 1.5, then 4 EPS |ao|.
  * softmax-path gradients: dP = do . v (e_dP = acc(dv + 2, .)); r = sum_j P0 dP carries rP and e_dP; dS = P0 (dP - r) carries all
    three (e_dS); dq, dk, dv and the table gradient carry e_dS (or rP, for dv) through their sums plus acc(terms, sum|terms|).
  * Sinkhorn-path gradients: the chain through seven normalisations is not carried.  Every element of a gradient block -- the
    (window, head) or (sample, head) slice of dq, dk, dv or dS -- is held to BF |ref| + C_SINK (largest |ref| of that block); the
    table gradient folds the dS bound through the index.  C_SINK is measured, not tuned: the worst error of the fp32 emulation
    below (same sums as the kernel, P0 recomputed from the saved lse, exact exp and reciprocal), before its bf16 output rounding,
    against this fp64 restatement over every case of WINDOW_CASES and BIAS_CASES is 9.9e-7 (SINK_MEASURED = 1e-6) of the block's largest
    element (tests/test_biased_attn_ref_host.py prints and re-checks it).  C_SINK = 2^-17 = 7.6e-6 is the next power of two at
    or above 4 x that; the 4 covers __expf and v_rcp being 1-2 ulp approximations and another summation order.  It is far below
    ROW_REL = 2e-2.  One exception, derived in dense_core: with a single query the Sinkhorn result does not depend on the scores,
    dS = 0 exactly, and a bound relative to the block's largest element is undefined; those blocks get an absolute bound.
  * underflow: every bound carries a floor of (number of terms) x 2^-126 x (largest factor).  With window (7, 8) and shift (3, 4)
    on a 7-row map some table entries collect only masked pairs; their fp64 gradient is ~1e-46 and a kernel that flushes them to 0
    is correct.
"""
from __future__ import annotations

import torch

from pcn_ref import BF, D, EPS, EXP_REL, ROW_REL, _gen, _randn, acc, bf16_tol, excess, up
from peaked_ref import sinkhorn_scalings

TINY = 2.0 ** -126
HIGHER = 1.01
SINK_MEASURED = 1.0e-6          # worst fp32-emulation error of a Sinkhorn-path gradient block, relative to the block's largest element
C_SINK = 2.0 ** -17             # next power of two >= 4 SINK_MEASURED
assert 4 * SINK_MEASURED <= C_SINK < 8 * SINK_MEASURED and C_SINK <= ROW_REL
bf = torch.bfloat16


def hardswish(x):
    return x * (x + 3.0).clamp(0.0, 6.0) / 6.0


def hardswish_grad(x):
    return torch.where(x < -3, torch.zeros_like(x), torch.where(x <= 3, x / 3 + 0.5, torch.ones_like(x)))


def f32_scale(width: int) -> float:
    """1 / sqrt(width) as the kernels hold it: rounded to fp32."""
    return float(torch.tensor(width ** -0.5, dtype=torch.float32))


def _bmax(t):
    return t.abs().amax((-2, -1), keepdim=True)


# ---- the dense core -------------------------------------------------------------------------------------------------------------
def dense_core(qs, k, v, bias, robust: bool, do=None, bias_abs=None) -> dict:
    """qs [..., Nq, kd] (the scale folded in), k [..., Nk, kd], v [..., Nk, dv], bias [..., Nq, Nk], do [..., Nq, dv] (optional), all
    fp64.  S = qs k^T + bias, P0 = softmax(S); robust: P = diag(a4) P0 diag(b3).  Returns P0, lse, a [..., 4, Nq], b [..., 3, Nk], o
    and (with do) dq (with respect to qs), dk, dv, dS, each with the bound of the module docstring under `<name>_A` (absolute part;
    bf16 outputs add BF |ref|) or `<name>_tol`."""
    Nq, Nk, kd, dv_ = qs.shape[-2], k.shape[-2], qs.shape[-1], v.shape[-1]
    S = qs @ k.mT + bias
    lse = torch.logsumexp(S, -1)
    P0 = torch.exp(S - lse[..., None])
    e_S = acc(kd + 2, qs.abs() @ k.abs().mT + (bias.abs() if bias_abs is None else bias_abs))
    e_row = e_S.amax(-1)
    lse_tol = e_row + 2 * EXP_REL + (Nk + 8) * EPS + 4 * EPS * lse.abs()
    rP = e_S + (e_row + 3 * EXP_REL + (Nk + 16) * EPS + 4 * EPS * lse.abs())[..., None]
    r = {"P0": P0, "lse": lse, "lse_tol": HIGHER * lse_tol, "S": S}
    a = b = None
    if robust:
        av, bv = sinkhorn_scalings(S)
        a = [torch.ones_like(av[..., 0, :])] + list(av.unbind(-2))          # a_0 (= 1) .. a_4
        b = [torch.ones_like(bv[..., 0, :])] + list(bv.unbind(-2))          # b_0 (= 1) .. b_3
        ea, eb = [torch.zeros_like(a[0])], [torch.zeros_like(b[0])]
        for t in range(1, 5):
            ea.append(a[t] * (P0 * b[t - 1][..., None, :] * (rP + eb[t - 1][..., None, :])).sum(-1) + (Nk + 10) * EPS)
            if t < 4:
                eb.append(b[t] * (a[t][..., :, None] * P0 * (rP + ea[t][..., :, None])).sum(-2) + (Nq + 10) * EPS)
        r.update({"a": av, "b": bv, "a_tol": HIGHER * torch.stack(ea[1:], -2) * av, "b_tol": HIGHER * torch.stack(eb[1:], -2) * bv})
        P = a[4][..., :, None] * P0 * b[3][..., None, :]
        eP = rP + ea[4][..., :, None] + eb[3][..., None, :]
    else:
        P, eP = P0, rP
    va = v.abs()
    r["P"], r["o"] = P, P @ v
    r["o_A"] = HIGHER * ((P * eP) @ va) + acc(Nk, P @ va) + Nk * TINY * va.amax()
    if do is None:
        return r
    dP = do @ v.mT
    r["dv"] = P.mT @ do
    G = dP
    if robust:
        # the seven normalisations walked back; each is X -> X / (its row or column sums), whose sums are a ratio of saved scalings
        G = (G - (G * P).sum(-1, keepdim=True)) * (a[4] / a[3])[..., :, None]
        for t in (3, 2, 1):
            Y = a[t][..., :, None] * P0 * b[t][..., None, :]
            G = (G - (G * Y).sum(-2, keepdim=True)) * (b[t] / b[t - 1])[..., None, :]
            Y = a[t][..., :, None] * P0 * b[t - 1][..., None, :]
            G = (G - (G * Y).sum(-1, keepdim=True)) * (a[t] / a[t - 1])[..., :, None]
    rr = (G * P0).sum(-1, keepdim=True)
    dS = P0 * (G - rr)
    r.update({"dS": dS, "dq": dS @ k, "dk": dS.mT @ qs})
    ka, qa, doa = k.abs(), qs.abs(), do.abs()
    if robust and Nq > 1:
        e_dS = C_SINK * _bmax(dS).expand_as(dS)
        A = {n: C_SINK * _bmax(r[n]).expand_as(r[n]) for n in ("dq", "dk", "dv")}
    else:
        if robust:
            # One query: every column holds one entry, each column step makes it 1 and the last row step 1 / Nk whatever the scores
            # are, so dS = 0 exactly and "relative to the block's largest element" means nothing.  What a kernel leaves is the
            # residue of the first column step walked back, G - G (a3 P0 b3) with |a3 P0 b3 - 1| <= th = 2 max rP + 8 EPS (P0 is
            # recomputed from lse); the later steps multiply by further such residues and by scaling ratios whose product is 1.
            # |dS| <= 8 th P0 max|dP|, the 8 for the three row-step subtractions; dv = do / Nk keeps the block rule.
            e_dS = 8.0 * (2.0 * rP.amax() + 8 * EPS) * P0 * dP.abs().amax()
            dvA = C_SINK * _bmax(r["dv"]).expand_as(r["dv"])
        else:
            e_dP = acc(dv_ + 2, doa @ va.mT)
            e_r = (P0 * (e_dP + rP * dP.abs())).sum(-1, keepdim=True) + acc(Nk, (P0 * dP.abs()).sum(-1, keepdim=True))
            e_dS = HIGHER * (P0 * (e_dP + e_r + 4 * EPS * (dP.abs() + rr.abs())) + rP * dS.abs())
            dvA = HIGHER * ((P0 * rP).mT @ doa) + acc(Nq, P0.mT @ doa)
        A = {"dq": e_dS @ ka + acc(Nk, dS.abs() @ ka), "dk": e_dS.mT @ qa + acc(Nq, dS.abs().mT @ qa), "dv": dvA}
    r["dS_tol"] = e_dS + TINY * (1.0 + 2.0 * dP.abs().amax())
    r["dq_A"] = A["dq"] + Nk * TINY * ka.amax()
    r["dk_A"] = A["dk"] + Nq * TINY * qa.amax()
    r["dv_A"] = A["dv"] + Nq * TINY * doa.amax()
    return r


# ---- shifted-window attention ---------------------------------------------------------------------------------------------------
def window_index(pH: int, pW: int, window, shift):
    """rel [N, N]: the table row of the pair (i, j), (cy_i - cy_j + Wh - 1)(2 Ww - 1) + cx_i - cx_j + Ww - 1.  mask [windows per
    sample, N, N] bool: the pairs whose slots lie in different shift regions, the regions filled slice by slice into a map of the
    rolled grid -- (0, -W), (-W, -s), (-s, None) along each axis, later slices overwriting earlier ones -- as the model does."""
    Wh, Ww = window
    sh, sw = shift
    n = torch.arange(Wh * Ww)
    cy, cx = n // Ww, n % Ww
    rel = (cy[:, None] - cy[None, :] + Wh - 1) * (2 * Ww - 1) + (cx[:, None] - cx[None, :] + Ww - 1)
    img = torch.zeros(pH, pW, dtype=torch.int64)
    count = 0
    for hs in ((0, -Wh), (-Wh, -sh), (-sh, None)):
        for ws in ((0, -Ww), (-Ww, -sw), (-sw, None)):
            img[hs[0]:hs[1], ws[0]:ws[1]] = count
            count += 1
    reg = _partition(img[None, :, :, None], Wh, Ww)[..., 0]                       # [windows, N]
    mask = reg[:, :, None] != reg[:, None, :]
    if sh + sw == 0:
        mask = torch.zeros_like(mask)
    return rel, mask


def _partition(x, Wh: int, Ww: int):
    """[B, pH, pW, F] -> [B * windows, Wh * Ww, F], windows of a sample row-major."""
    B, pH, pW, F = x.shape
    return x.reshape(B, pH // Wh, Wh, pW // Ww, Ww, F).permute(0, 1, 3, 2, 4, 5).reshape(-1, Wh * Ww, F)


def _unpartition(w, B: int, pH: int, pW: int, Wh: int, Ww: int):
    return w.reshape(B, pH // Wh, pW // Ww, Wh, Ww, -1).permute(0, 1, 3, 2, 4, 5).reshape(B, pH, pW, -1)


def window_ref(qkv, table, dout, B, pH, pW, C, heads, window, shift, robust) -> dict:
    """qkv [B pH pW, 3C], table [T, heads], dout [B pH pW, C] (None: forward only).  In the kernels' layouts: o [tokens, C]; stats
    [tokens, heads, S] = lse (a1 b1 a2 b2 a3 b3 a4: a_t of the token as a query, b_t as a key); dq / dk / dv [tokens, C] (the three
    column thirds of dqkv); dtable [T, heads]; `<name>_tol` beside each.  `blocks`: dq / dk / dv / dS per (window, head)."""
    Wh, Ww = window
    sh, sw = shift
    N, dh, T = Wh * Ww, C // heads, (2 * Wh - 1) * (2 * Ww - 1)
    scale = f32_scale(dh)

    def gather(t, parts):            # token rows -> [parts, windows, heads, N, dh] by the roll and the partition
        x = torch.roll(up(t).reshape(B, pH, pW, -1), (-sh, -sw), (1, 2))
        return _partition(x, Wh, Ww).reshape(-1, N, parts, heads, dh).permute(2, 0, 3, 1, 4)

    def scatter(t):                  # [windows, heads, N, w] -> token rows [tokens, heads * w]
        x = _unpartition(t.permute(0, 2, 1, 3).reshape(t.shape[0], N, -1), B, pH, pW, Wh, Ww)
        return torch.roll(x, (sh, sw), (1, 2)).reshape(B * pH * pW, -1)

    q, k, v = gather(qkv, 3)
    rel, mask = window_index(pH, pW, window, shift)
    tb = up(table)[rel].permute(2, 0, 1)[None]                                   # [1, heads, N, N]
    m = -100.0 * mask.to(D).repeat(B, 1, 1)[:, None]                             # [windows, 1, N, N]
    do = None if dout is None else gather(dout, 1)[0]
    c = dense_core(q * scale, k, v, tb + m, robust, do, bias_abs=tb.abs() + m.abs())
    o = scatter(c["o"])
    st, st_tol = [c["lse"]], [c["lse_tol"]]
    if robust:
        for t in range(4):
            st.append(c["a"][..., t, :]); st_tol.append(c["a_tol"][..., t, :])
            if t < 3:
                st.append(c["b"][..., t, :]); st_tol.append(c["b_tol"][..., t, :])
    r = {"o": o, "o_tol": bf16_tol(o, scatter(c["o_A"])), "stats": scatter(torch.stack(st, -1)).reshape(B * pH * pW, heads, -1),
         "stats_tol": scatter(torch.stack(st_tol, -1)).reshape(B * pH * pW, heads, -1)}
    if dout is None:
        return r
    for n, f in (("dq", scale), ("dk", 1.0), ("dv", 1.0)):
        r[n] = scatter(c[n]) * f
        r[n + "_tol"] = bf16_tol(r[n], scatter(c[n + "_A"]) * f + 2 * EPS * r[n].abs())
    fold = lambda x: torch.zeros(heads, T, dtype=D).index_add_(1, rel.reshape(-1), x.sum(0).reshape(heads, N * N)).t()
    terms = torch.bincount(rel.reshape(-1), minlength=T).to(D)[:, None] * c["dS"].shape[0]
    r["dtable"] = fold(c["dS"])
    r["dtable_tol"] = fold(c["dS_tol"]) + acc(terms, fold(c["dS"].abs()))
    r["blocks"] = {n: c[n] * (scale if n == "dq" else 1.0) for n in ("dq", "dk", "dv", "dS")}
    return r


def check_window(ref: dict, o=None, stats=None, dqkv=None, dtable=None) -> dict:
    """Worst |error| / bound per output (<= 1 passes); the statistics one by one."""
    r = {}
    if o is not None:
        r["o"] = excess(o, ref["o"], ref["o_tol"])
    if stats is not None:
        names = ("lse", "a1", "b1", "a2", "b2", "a3", "b3", "a4")
        for s in range(ref["stats"].shape[-1]):
            r[names[s]] = excess(stats.reshape(ref["stats"].shape)[..., s], ref["stats"][..., s], ref["stats_tol"][..., s])
    if dqkv is not None:
        C = ref["dq"].shape[1]
        for t, n in enumerate(("dq", "dk", "dv")):
            r[n] = excess(dqkv[:, t * C:(t + 1) * C], ref[n], ref[n + "_tol"])
    if dtable is not None:
        r["dtable"] = excess(dtable, ref["dtable"], ref["dtable_tol"])
    return r


# ---- LeViT's offset-biased attention --------------------------------------------------------------------------------------------
def bias_heads(t, B: int, rows: int, H: int, hs: int, w: int):
    """A row-major [B rows, >= (H - 1) hs + w] view whose head h starts at column h hs -> [B, H, rows, w]."""
    return torch.stack([t[:, h * hs:h * hs + w] for h in range(H)], 1).reshape(B, rows, H, w).permute(0, 2, 1, 3)


def _rows(t):
    """[B, H, rows, w] -> [B rows, H w]."""
    B, H, n, w = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * n, H * w)


def bias_ref(q, k, v, hs, table, idx, dact, o_saved, B, H, Nq, Nk, kd, d, robust) -> dict:
    """q / k / v: the views the ABI takes (head h at column h hs[0 | 1 | 2]); table [H, T]; idx [Nq, Nk]; dact [B Nq, H d] and o_saved
    (the kernel's bf16 o, where Hardswish' is taken) or None for the forward alone.  o / ao [B Nq, H d]; stats [B H, SZ] = lse [Nq],
    a1..a4 [4][Nq], b1..b3 [3][Nk]; dq [B, H, Nq, kd], dk [B, H, Nk, kd], dv [B, H, Nk, d]; dtable [H, T]; `_tol` beside each."""
    T = table.shape[1]
    scale = f32_scale(kd)
    qh, kh, vh = (up(bias_heads(t, B, n, H, s, w)) for t, n, s, w in ((q, Nq, hs[0], kd), (k, Nk, hs[1], kd), (v, Nk, hs[2], d)))
    do = None
    if dact is not None:
        do = bias_heads(up(dact) * hardswish_grad(up(o_saved)), B, Nq, H, d, d)
    c = dense_core(qh * scale, kh, vh, up(table)[:, idx][None], robust, do)
    o = _rows(c["o"])
    ao = hardswish(o)
    st, st_tol = [c["lse"]], [c["lse_tol"]]
    if robust:
        st += [c["a"].reshape(B, H, -1), c["b"].reshape(B, H, -1)]
        st_tol += [c["a_tol"].reshape(B, H, -1), c["b_tol"].reshape(B, H, -1)]
    oA = _rows(c["o_A"])
    r = {"o": o, "o_tol": bf16_tol(o, oA), "ao": ao, "ao_tol": bf16_tol(ao, 1.5 * oA + 4 * EPS * ao.abs()),
         "stats": torch.cat(st, -1).reshape(B * H, -1), "stats_tol": torch.cat(st_tol, -1).reshape(B * H, -1)}
    if dact is None:
        return r
    for n, f in (("dq", scale), ("dk", 1.0), ("dv", 1.0)):
        r[n] = c[n] * f
        r[n + "_tol"] = bf16_tol(r[n], c[n + "_A"] * f + 2 * EPS * r[n].abs())
    fold = lambda x: torch.zeros(H, T, dtype=D).index_add_(1, idx.reshape(-1), x.sum(0).reshape(H, Nq * Nk))
    terms = torch.bincount(idx.reshape(-1), minlength=T).to(D)[None, :] * B
    r["dtable"] = fold(c["dS"])
    r["dtable_tol"] = fold(c["dS_tol"]) + acc(terms, fold(c["dS"].abs()))
    r["dtable_tol"] = torch.where(terms > 0, r["dtable_tol"], torch.zeros_like(terms))          # an entry no pair uses: exactly 0
    r["blocks"] = {"dv": r["dv"]} if Nq == 1 else {"dq": r["dq"], "dk": r["dk"], "dv": r["dv"], "dS": c["dS"]}          # Nq = 1: dS = 0 exactly
    return r


def check_bias(ref: dict, Nq: int, Nk: int, o=None, ao=None, stats=None, dq=None, dk=None, dv=None, dtable=None) -> dict:
    r = {}
    for n, g in (("o", o), ("ao", ao), ("dq", dq), ("dk", dk), ("dv", dv), ("dtable", dtable)):
        if g is not None:
            r[n] = excess(g, ref[n], ref[n + "_tol"])
    if stats is not None:
        cuts = [("lse", 0, Nq)]
        if ref["stats"].shape[1] > Nq:
            cuts += [(f"a{t}", t * Nq, (t + 1) * Nq) for t in range(1, 5)] + [(f"b{t}", 5 * Nq + (t - 1) * Nk, 5 * Nq + t * Nk) for t in range(1, 4)]
        for n, lo, hi in cuts:
            r[n] = excess(stats[:, lo:hi], ref["stats"][:, lo:hi], ref["stats_tol"][:, lo:hi])
    return r


# ---- fp32 emulation of the kernels' arithmetic (same sums, P0 recomputed from the saved lse, bf16 only at the outputs) ----------
# `bug` names one deliberate mistake (tests/test_biased_attn_ref_host.py requires the bounds to catch each); None is the kernel.
def emu_core_fwd(qs, k, v, bias, robust: bool):
    S = qs @ k.mT + bias
    m = S.amax(-1, keepdim=True)
    e = torch.exp(S - m)
    l = e.sum(-1, keepdim=True)
    P0 = e * (1.0 / l)
    st = {"lse": (m + torch.log(l))[..., 0], "a": [], "b": []}
    if not robust:
        return P0 @ v, st
    b = torch.ones_like(P0[..., 0, :])
    for t in range(3):
        a = 1.0 / (P0 * b[..., None, :]).sum(-1)
        b = 1.0 / (a[..., :, None] * P0).sum(-2)
        st["a"].append(a); st["b"].append(b)
    a = 1.0 / (P0 * b[..., None, :]).sum(-1)
    st["a"].append(a)
    return ((P0 * b[..., None, :]) @ v) * a[..., :, None], st


def emu_core_bwd(qs, k, v, bias, robust: bool, do, st, bug=None):
    """-> dq (with respect to qs), dk, dv, dS in fp32."""
    P0 = torch.exp(qs @ k.mT + bias - st["lse"][..., None])
    G = do @ v.mT
    P = P0
    if robust:
        one = torch.ones_like
        a = [one(st["a"][0])] + st["a"]
        b = [one(st["b"][0])] + st["b"]
        G = (G - ((G * P0 * b[3][..., None, :]).sum(-1) * a[4])[..., None]) * (a[4] / a[3])[..., :, None]
        for t in (3, 2, 1):
            hs = (G * (a[t][..., :, None] * P0)).sum(-2) * b[t]
            G = (G - hs[..., None, :]) * (b[t] / b[t - 1])[..., None, :]
            r = (G * P0 * b[t - 1][..., None, :]).sum(-1) * a[t]
            G = (G - r[..., None]) * (a[t] / a[t - 1])[..., :, None]
        P = a[4][..., :, None] * P0 * b[2 if bug == "b2_for_b3" else 3][..., None, :]
    GP = G * P0
    r = (GP[..., :-1] if bug == "drop_last_key" else GP).sum(-1, keepdim=True)
    dS = P0 * (G - r)
    return dS @ k, dS.mT @ qs, P.mT @ do, dS


def emu_window(qkv, table, dout, B, pH, pW, C, heads, window, shift, robust, bug=None) -> dict:
    """The window kernels' index arithmetic (slot_row, region_1d, base - (yj tw + xj), the (dy, dx) decode of the table gradient, the
    partials of WA_CHUNK = 8 windows) restated on integer tensors, around emu_core_*.  Outputs as the kernels store them; `blocks`
    holds the fp32 gradients before the bf16 rounding."""
    Wh, Ww = window
    sh, sw = shift
    N, dh, T = Wh * Ww, C // heads, (2 * Wh - 1) * (2 * Ww - 1)
    nWx, nW1 = pW // Ww, (pH // Wh) * (pW // Ww)
    nwin, tok = B * nW1, B * pH * pW
    w, i = torch.arange(nW1), torch.arange(N)
    wy, wx, yi, xi = w // nWx, w % nWx, i // Ww, i % Ww
    sg = -1 if bug == "roll_neg" else 1
    y, x = (wy[:, None] * Wh + yi[None] + sg * sh) % pH, (wx[:, None] * Ww + xi[None] + sg * sw) % pW
    rows = ((torch.arange(B)[:, None, None] * pH + y[None]) * pW + x[None]).reshape(nwin, N)              # slot_row

    def region(pos, extent, ws, s):
        if s == 0:
            return torch.full_like(pos, 2)
        return torch.where(pos < extent - ws, 0, torch.where(pos < extent - s + (bug == "region_off_by_one"), 1, 2))

    reg = region(wy[:, None] * Wh + yi[None], pH, Wh, sh) * 3 + region(wx[:, None] * Ww + xi[None], pW, Ww, sw)
    tw = 2 * Wh - 1 if bug == "tw_from_wh" else 2 * Ww - 1
    ridx = (((yi + Wh - 1) * tw + xi + Ww - 1)[:, None] - (yi * tw + xi)[None, :]).clamp(0, T - 1)        # base - (yj tw + xj)
    flat = table.float().reshape(-1)
    t_ = torch.arange(T)
    stab = torch.stack([flat[(t_ + h).clamp(max=T * heads - 1) if bug == "table_stride_1" else t_ * heads + h] for h in range(heads)])
    bias = stab[:, ridx][None]
    if sh + sw > 0:
        bias = bias + torch.where(reg[:, :, None] != reg[:, None, :], -100.0, 0.0).repeat(B, 1, 1)[:, None]
    g = qkv.float()[rows].reshape(nwin, N, 3, heads, dh).permute(2, 0, 3, 1, 4)
    scale = torch.tensor(dh ** -0.5, dtype=torch.float32)
    qs, k, v = g[0] * scale, g[1], g[2]
    o32, st = emu_core_fwd(qs, k, v, bias, robust)

    def put(t, width):               # [windows, heads, N, w] -> the token rows
        out = torch.zeros(tok, heads * width)
        out[rows.reshape(-1)] = t.permute(0, 2, 1, 3).reshape(nwin * N, heads * width)
        return out

    cols = [st["lse"]] + ([st["a"][0], st["b"][0], st["a"][1], st["b"][1], st["a"][2], st["b"][2], st["a"][3]] if robust else [])
    r = {"o": put(o32, dh).to(bf), "stats": put(torch.stack(cols, -1), len(cols)).reshape(tok, heads, -1)}
    if dout is None:
        return r
    do = dout.float()[rows].reshape(nwin, N, heads, dh).permute(0, 2, 1, 3)
    dq, dk, dv, dS = emu_core_bwd(qs, k, v, bias, robust, do, st, bug)
    dq = dq * scale
    r["dqkv"] = torch.cat((put(dq, dh), put(dk, dh), put(dv, dh)), 1).to(bf)
    # entry t = (dy, dx) collects dS[i][j] over the pairs with coord_i - coord_j = (dy, dx)
    if bug == "decode_swapped":
        dy, dx = t_ % tw - (Wh - 1), t_ // tw - (Ww - 1)
    else:
        dy, dx = t_ // tw - (Wh - 1), t_ % tw - (Ww - 1)
    yj, xj = yi[None] - dy[:, None], xi[None] - dx[:, None]                                                  # [T, N]
    ok = (yj >= 0) & (yj < Wh) & (xj >= 0) & (xj < Ww)
    j = (yj * Ww + xj).clamp(0, N - 1)
    per = (dS[:, :, i[None].expand(T, N), j] * ok).sum(-1)                                                   # [windows, heads, T]
    if bug == "skip_tail_window":
        per = per[:-1]
    chunks = -(-nwin // 8)
    per = torch.cat((per, per.new_zeros(chunks * 8 - per.shape[0], heads, T)))
    r["part"] = per.reshape(chunks, 8, heads, T).sum(1)
    r["dtable"] = r["part"].sum(0).t().contiguous()
    r["blocks"] = {"dq": dq, "dk": dk, "dv": dv, "dS": dS}
    return r


def bias_csr(idx, T: int):
    """The inverse index the host builds once per geometry: entry t's pairs are pos[ptr[t] : ptr[t + 1]] (flat i Nk + j)."""
    flat = idx.reshape(-1)
    ptr = torch.zeros(T + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.bincount(flat, minlength=T), 0)
    return ptr, torch.sort(flat, stable=True).indices


def emu_bias(q, k, v, hs, table, idx, dact, B, H, Nq, Nk, kd, d, robust, bug=None) -> dict:
    """Forward, then the backward from the forward's own bf16 o and fp32 statistics, as the kernels chain."""
    T = table.shape[1]
    scale = torch.tensor(kd ** -0.5, dtype=torch.float32)
    qh, kh, vh = (bias_heads(t, B, n, H, s, w).float() for t, n, s, w in ((q, Nq, hs[0], kd), (k, Nk, hs[1], kd), (v, Nk, hs[2], d)))
    bias = table.float()[:, idx][None]
    o32, st = emu_core_fwd(qh * scale, kh, vh, bias, robust)
    o32 = _rows(o32)
    cols = [st["lse"]] + ([torch.stack(st["a"], -2).reshape(B, H, -1), torch.stack(st["b"], -2).reshape(B, H, -1)] if robust else [])
    r = {"o": o32.to(bf), "ao": hardswish(o32).to(bf), "stats": torch.cat(cols, -1).reshape(B * H, -1)}
    if dact is None:
        return r
    do = bias_heads(dact.float() * hardswish_grad(r["o"].float()), B, Nq, H, d, d)
    dq, dk, dv, dS = emu_core_bwd(qh * scale, kh, vh, bias, robust, do, st, bug)
    dq = dq * scale
    ptr, pos = bias_csr(idx, T)
    flat = dS.reshape(B, H, Nq * Nk)
    part = torch.zeros(B, H, T)
    for t in range(T):
        e0, e1 = int(ptr[t]), int(ptr[t + 1])
        if bug == "unused_entry_kept" and e1 == e0:
            e1 = min(e0 + 1, Nq * Nk)
        part[:, :, t] = flat[:, :, pos[e0:e1]].sum(-1)
    r.update({"dq": dq.to(bf), "dk": dk.to(bf), "dv": dv.to(bf), "dtable": part.sum(0), "blocks": {"dq": dq, "dk": dk, "dv": dv, "dS": dS}})
    return r


def block_error(ref_blocks: dict, emu_blocks: dict) -> float:
    """Worst |emulation - restatement| over a gradient block's largest |restatement|, over dq / dk / dv / dS: what C_SINK rests on."""
    worst = 0.0
    for n, ref in ref_blocks.items():
        big = _bmax(ref)
        assert bool((big > 0).all()), n
        worst = max(worst, float(((up(emu_blocks[n]) - ref).abs() / big).max()))
    return worst


# ---- the cases and their seeded inputs ------------------------------------------------------------------------------------------
# (B, pH, pW, C, heads, window, shift)
WINDOW_CASES = (
    (1, 2, 2, 32, 1, (2, 2), (0, 0)),         # N = 4 (60 idle lanes), T = 9 (one tacc slot), one window: a single, partial chunk
    (3, 2, 9, 96, 3, (2, 3), (0, 2)),         # non-square N = 6, T = 15; heads 3 (table column stride 3); 9 windows = chunks of 8 + 1,
                                              # 3 windows per sample so the first chunk straddles samples; shift Ww - 1
    (2, 7, 16, 64, 1, (7, 8), (3, 4)),        # N = 56, T = 195 (fourth tacc slot partly used), dh 64; a shift on the single-window row
                                              # axis (pH == Wh); table entries that collect only masked pairs (gradient ~1e-46)
    (2, 16, 7, 128, 2, (8, 7), (4, 3)),       # the transpose of the previous case: shifted single-window column axis
    (1, 2, 128, 64, 2, (1, 64), (0, 63)),     # Wh = 1, N = 64 (no idle lane), T = 127 (two tacc slots), shift Ww - 1
    (2, 16, 24, 64, 2, (8, 8), (7, 1)),       # T = 225 (all four tacc slots); shifts W - 1 and 1; 12 windows = 8 + 4
    (5, 14, 21, 32, 1, (7, 7), (3, 0)),       # row-axis shift only; 6 windows per sample; 30 windows = 8, 8, 8, 6, chunks straddle samples
)

# (B, H, Nq, Nk, kd, d, T, layout, (q pad, kv pad) columns, idx).  layout "sep": q in one buffer [B Nq, H kd + pad], k | v per head in
# another [B Nk, H (kd + d) + pad]; "int": q | k | v per head in one buffer [B Nk, H (2 kd + d) + pad], q in its first B Nq rows.
BIAS_CASES = (
    (1, 1, 1, 1, 16, 32, 1, "sep", (0, 0), "rand"),            # the smallest sizes, T = 1
    (2, 3, 1, 256, 16, 32, 256, "sep", (0, 0), "perm"),        # Nq = 1, Nk = 256 (every thread a column thread), T = 256; idx a permutation:
                                                               # every entry used exactly once
    (1, 2, 153, 256, 32, 64, 200, "sep", (0, 0), "rand"),      # the LDS limit at Nk = 256
    (2, 1, 198, 198, 16, 128, 256, "int", (0, 0), "rand"),     # the LDS limit of a square matrix
    (2, 2, 63, 65, 32, 32, 7, "int", (8, 8), "holes"),         # odd sizes across a wave; padded stride; entry 3 used by no pair, entry 5 by one
    (3, 2, 129, 255, 16, 64, 256, "sep", (8, 24), "rand"),     # odd sizes; both strides padded: gap columns
)
BIAS_REFUSED = ((1, 1, 154, 256, 16, 32, 8), (1, 1, 199, 199, 16, 32, 8))          # (B, H, Nq, Nk, kd, d, T): one row past the LDS limit
HOLE_UNUSED, HOLE_ONCE = 3, 5


def window_inputs(case, seed: int = 0) -> dict:
    B, pH, pW, C, heads, (Wh, Ww), _ = case
    tok = B * pH * pW
    return {"qkv": _randn((tok, 3 * C), seed + 1, dtype=bf), "table": _randn(((2 * Wh - 1) * (2 * Ww - 1), heads), seed + 2, 0.5),
            "dout": _randn((tok, C), seed + 3, dtype=bf)}


def bias_layout(case) -> dict:
    """Buffer shapes, head strides and the column offsets of k and v in their buffer."""
    B, H, Nq, Nk, kd, d, T, layout, (pq, pkv), _ = case
    if layout == "sep":
        return {"qshape": (B * Nq, H * kd + pq), "kvshape": (B * Nk, H * (kd + d) + pkv), "hs": (kd, kd + d, kd + d), "koff": 0, "voff": kd,
                "qcols": H * kd, "kvcols": H * (kd + d)}
    return {"qshape": None, "kvshape": (B * Nk, H * (2 * kd + d) + pkv), "hs": (2 * kd + d,) * 3, "koff": kd, "voff": 2 * kd,
            "qcols": None, "kvcols": H * (2 * kd + d)}


def bias_views(case, qbuf, kvbuf):
    """(q, k, v) as the ABI takes them, from buffers of bias_layout's shapes (qbuf is ignored for "int")."""
    B, _, Nq = case[:3]
    L = bias_layout(case)
    q = qbuf if L["qshape"] is not None else kvbuf[:B * Nq]
    return q, kvbuf[:, L["koff"]:], kvbuf[:, L["voff"]:]


def bias_written(case):
    """bool masks (q buffer or None, kv buffer): the elements a backward writes; every other element must keep what it held."""
    B, H, Nq, Nk, kd, d = case[:6]
    L = bias_layout(case)
    mq = None if L["qshape"] is None else torch.zeros(L["qshape"], dtype=torch.bool)
    mkv = torch.zeros(L["kvshape"], dtype=torch.bool)
    for h in range(H):
        (mkv[:B * Nq] if mq is None else mq)[:, h * L["hs"][0]:h * L["hs"][0] + kd] = True
        mkv[:, L["koff"] + h * L["hs"][1]:L["koff"] + h * L["hs"][1] + kd] = True
        mkv[:, L["voff"] + h * L["hs"][2]:L["voff"] + h * L["hs"][2] + d] = True
    return mq, mkv


def bias_inputs(case, seed: int = 0) -> dict:
    B, H, Nq, Nk, kd, d, T, layout, _, kind = case
    L = bias_layout(case)
    g = _gen(seed + 5)
    if kind == "perm":
        assert T == Nq * Nk
        idx = torch.randperm(T, generator=g).reshape(Nq, Nk)
    elif kind == "holes":
        used = torch.tensor([t for t in range(T) if t not in (HOLE_UNUSED, HOLE_ONCE)])
        idx = used[torch.randint(0, len(used), (Nq, Nk), generator=g)]
        idx[Nq // 2, Nk - 1] = HOLE_ONCE
    else:
        idx = torch.randint(0, T, (Nq, Nk), generator=g)
    return {"qbuf": None if L["qshape"] is None else _randn(L["qshape"], seed + 1, dtype=bf), "kvbuf": _randn(L["kvshape"], seed + 2, dtype=bf),
            "table": _randn((H, T), seed + 3, 0.5), "dact": _randn((B * Nq, H * d), seed + 4, dtype=bf), "idx": idx, "hs": L["hs"]}
