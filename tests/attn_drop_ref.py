"""Attention-weight dropout inside the fused softmax attention kernels (nrv_attn_drop_*): the keep decisions restated in numpy, an fp64
reference for a given mask, a plain restatement of the three kernels' use of the mask, the case list and the probe inputs (test
infrastructure, no kernels).  Builds on attn_edges_ref.py.

The decisions (include/nrv.h, "Attention-weight dropout"): keep(seed, g, q, k) is a stateless function of the 64-bit seed, g = b H + h,
the query and the key.  Three kernels regenerate it: the forward and the query-owner backward (dQ), whose lanes hold four keys of one
query, and the key-owner backward (dK / dV), whose lanes hold four queries of one key.  `restated` therefore carries three masks --
forward, query-owner, key-owner -- which are the same mask unless one of MISTAKES is switched on.

Random inputs move a row by ~ 1 / N per wrong decision, under any bound.  The probe inputs make a wrong decision exact: with q = 0 every
row is P = 1 / N exactly, and
  forward probe   v one-hot over a block of dh keys (key j dh + d has v = e_d): o[q, d] = keep(q, j dh + d) rs / N, so the zero pattern of
                  o is the forward kernel's mask of that block
  dV probe        dO one-hot over a block of dh queries: dv[k, d] = keep(j dh + d, k) rs / N, the key-owner kernel's mask
  dQ probe        v_k = dO_q = e_0 for every key and query and k one-hot over a block: N dq[q, d] / scale = keep(q, j dh + d) rs - delta_q
                  with delta_q = o[q, 0], so N dq / scale + o[q, 0] is rs (kept) or 0 (dropped): the query-owner kernel's mask.  (The
                  bare sign of dq does not decide a row in which every key is kept: there rs - delta is a cancellation.)
The forward and the dV probe share a call; ceil(N / dh) blocks cover the mask.
"""
from __future__ import annotations

import functools
from collections import namedtuple
from typing import Callable, Optional

import numpy as np
import torch

import attn_edges_ref as AE
from attn_edges_ref import KERNEL_ROUNDING_BOUND, LSE_TOL, PER_ROW_BOUND, heads, per_row_rel  # noqa: F401  (re-exported)

GT = 64
U32 = np.uint32
GOLD, M1, M2 = U32(0x9E3779B9), U32(0x85EBCA6B), U32(0xC2B2AE35)
C0, C1 = U32(0x9E3779B9), U32(0x7F4A7C15)
BASE_SEED = 0x5DEECE66D1234567                 # the GPU tests' seeds are BASE_SEED + a small case number: both words are in use

Case = namedtuple("Case", "family B N H dh p seed")


# ---- the decisions ----------------------------------------------------------------------------------------------------------------
def threshold(p: float) -> int:
    """nrv_attn_drop_threshold: T = floor(p 2^16 + 1/2) of the float32 p; -2 (NRV_ERR_SHAPE) for p < 0, p >= 1, NaN or T = 65536."""
    p = float(np.float32(p))
    if not (p >= 0.0) or not (p < 1.0):
        return -2
    T = int(p * 65536.0 + 0.5)
    return -2 if T > 65535 else T


def p_eff(p: float) -> float:
    return threshold(p) / 65536.0


def _fmix(h: np.ndarray) -> np.ndarray:
    h = np.asarray(h, dtype=U32).copy()
    h ^= h >> U32(16)
    h *= M1
    h ^= h >> U32(13)
    h *= M2
    return h ^ (h >> U32(16))


def words(seed: int, g: np.ndarray, q: np.ndarray, kp: np.ndarray) -> np.ndarray:
    """the 32-bit word of (seed, g, query, key pair kp = key >> 1), broadcast over the three index arrays (uint32, wrapping)"""
    lo, hi = np.asarray([seed & 0xFFFFFFFF], dtype=U32), np.asarray([(seed >> 32) & 0xFFFFFFFF], dtype=U32)
    g, q, kp = (np.asarray(a, dtype=U32) for a in (g, q, kp))

    def head(c):
        return _fmix(_fmix(_fmix(lo + c) ^ hi) + g)

    a0, a1 = _fmix(head(C0) ^ q), _fmix(head(C1) ^ q)
    t = a0 + kp * GOLD
    t = t ^ (t >> U32(16))
    t = t * M1
    t = t ^ a1
    t = t ^ (t >> U32(13))
    t = t * M2
    return t ^ (t >> U32(16))


def keep_mask(seed: int, p: float, B: int, H: int, N: int, g_of: Optional[Callable] = None, key_of: Optional[Callable] = None,
              Nk: Optional[int] = None) -> np.ndarray:
    """bool [B, H, N, Nk]: keep <=> the key's 16-bit half of the word >= T.  `g_of(b, h)` and `key_of(k)` restate mistakes."""
    T = threshold(p)
    assert T >= 0
    Nk = N if Nk is None else Nk
    b, h = np.meshgrid(np.arange(B), np.arange(H), indexing="ij")
    g = (b * H + h) if g_of is None else g_of(b, h)
    key = np.arange(Nk) if key_of is None else key_of(np.arange(Nk))
    w = words(seed, g[:, :, None, None], np.arange(N)[None, None, :, None], (key >> 1)[None, None, None, :])
    r = (w >> ((key & 1) * 16).astype(U32)[None, None, None, :]) & U32(0xFFFF)
    return r >= U32(T)


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def _cases():
    shapes = [("single", N, 64) for N in AE.SINGLE_PASS_NS]
    for dh in AE.STREAM_DH:
        for N in (1, 63, 64, 65, 129, 257) + ((300,) if dh == 64 else ()):
            if dh != 64 or N > 256:                                   # dh 64 streams only where N > 256
                shapes.append(("stream", N, dh))
    # p alternates 0.5 / 0.1 in list order.  Every N = 1 case sits at an even index and so carries p = 0.5: there 1 / (1 - p_eff) = 2 and
    # o = 2 v is exact in bf16, which is what the one-key cancellation bound of `check` rests on (delta = dO . o against dO . v).  At
    # p = 0.1 the forward's rounding of o = 1.11 v to bf16 alone leaves dq and dk of a one-key row at ~ 2^-9 |dO| |v|, 15 to 150 times
    # that bound in `restated(kernel_rounding=True)`: the documented rounding point of o, not a cancellation of two fp32 sums.
    cases = tuple(Case(f, 2, N, 2, dh, (0.5, 0.1)[i % 2], BASE_SEED + i) for i, (f, N, dh) in enumerate(shapes))
    assert all(c.p == 0.5 for c in cases if c.N == 1)
    return cases


CASES = _cases()

# the shapes whose first draw left a row outside KERNEL_ROUNDING_BOUND on the CPU, and the number of the draw that stays inside
# (tests/test_attn_drop_ref_host.py asserts the bound for every case as drawn here): other inputs, not another bound
RESEEDED: dict = {}


def case_id(c: Case) -> str:
    return f"{c.family}-N{c.N}-dh{c.dh}-p{c.p}"


@functools.lru_cache(maxsize=None)
def _inputs(c: Case) -> dict:
    g = torch.Generator().manual_seed(5000 + 7 * c.N + c.dh + 100003 * RESEEDED.get((c.N, c.dh, c.p), 0))
    qkv = torch.randn(c.B * c.N, 3 * c.H * c.dh, generator=g).to(torch.bfloat16)
    dout = torch.randn(c.B * c.N, c.H * c.dh, generator=g).to(torch.bfloat16)
    return {"qkv": qkv, "dout": dout, "scale": c.dh ** -0.5}


def inputs(c: Case) -> dict:
    """qkv bf16 [B*N, 3*H*dh] and dout bf16 [B*N, H*dh], N(0, 1); shared by every test of the case: do not modify."""
    return _inputs(c)


@functools.lru_cache(maxsize=None)
def case_mask(c: Case) -> torch.Tensor:
    return torch.from_numpy(keep_mask(c.seed, c.p, c.B, c.H, c.N))


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def drop_reference(qkv, dout, keep: torch.Tensor, pe: float, B: int, N: int, H: int, dh: int, scale: float) -> dict:
    """F.dropout(softmax(scale q k^T), p) v with the given keep mask, by autograd in fp64: o, dq, dk, dv [B,H,N,dh], lse [B,H,N] of
    the undropped rows, `none` [B,H,N] (no key kept)."""
    x = qkv.detach().cpu().double().requires_grad_(True)
    q, k, v = heads(x, B, N, H, dh)
    S = (q @ k.transpose(-1, -2)) * scale
    P = torch.softmax(S, dim=-1)
    o = (P * keep.double() / (1.0 - pe)) @ v
    o.backward(heads(dout.detach().cpu().double(), B, N, H, dh)[0])
    res = {"o": o.detach(), "lse": torch.logsumexp(S.detach(), dim=-1), "none": ~keep.any(dim=-1)}
    res["dq"], res["dk"], res["dv"] = heads(x.grad, B, N, H, dh)
    return res


@functools.lru_cache(maxsize=None)
def reference(c: Case) -> dict:
    """The fp64 reference of a case with the restated mask, computed once and shared: do not modify."""
    i = inputs(c)
    return drop_reference(i["qkv"], i["dout"], case_mask(c), p_eff(c.p), c.B, c.N, c.H, c.dh, i["scale"])


# ---- the kernels' use of the mask, restated ---------------------------------------------------------------------------------------
MISTAKES = ("mask_transposed", "bwd_unmasked", "head_index", "dv_unscaled", "rowsum_after_drop", "tile_local_k", "seed_low_only")


def kernel_masks(c: Case, mistake: Optional[str] = None):
    """(forward, query-owner, key-owner) keep masks [B,H,N,N] as the three kernels draw them, with at most one mistake"""
    seed, kw = c.seed, {}
    if mistake == "seed_low_only":
        seed &= 0xFFFFFFFF
    if mistake == "head_index":
        kw["g_of"] = lambda b, h: h + 0 * b
    if mistake == "tile_local_k":
        kw["key_of"] = lambda k: k % GT
    m = torch.from_numpy(keep_mask(seed, c.p, c.B, c.H, c.N, **kw))
    mk = m.transpose(-1, -2).contiguous() if mistake == "mask_transposed" else m
    return m, m, mk


def restated_run(c: Case, qkv, dout, mistake: Optional[str] = None, kernel_rounding: bool = False) -> dict:
    """The three kernels on the given inputs, written out in fp64: the forward (row statistics of the undropped row, P o keep into
    P.V, 1 / (l (1 - p_eff)) at the end), the query-owner backward (dS = P (M dP - delta) -> dq) and the key-owner backward (the same dS
    -> dk, (P o keep)^T dO / (1 - p_eff) -> dv), each with its own copy of the mask.  `kernel_rounding`: P o keep, dS and the bf16 outputs
    are rounded to bf16 and delta is formed from the bf16 o, as the kernels do."""
    assert mistake is None or mistake in MISTAKES, mistake
    B, N, H, dh, scale = c.B, c.N, c.H, c.dh, c.dh ** -0.5
    rs = 1.0 / (1.0 - p_eff(c.p))
    mf, mq, mk = (m.double() for m in kernel_masks(c, mistake))
    q, k, v = heads(qkv.double(), B, N, H, dh)
    dO = heads(dout.double(), B, N, H, dh)[0]
    rnd = (lambda t: t.to(torch.bfloat16).double()) if kernel_rounding else (lambda t: t)
    s = (q @ k.transpose(-1, -2)) * scale
    m = s.amax(dim=-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(dim=-1, keepdim=True)
    lse = (m + torch.log(l))[..., 0]
    lf = (e * mf).sum(dim=-1, keepdim=True).clamp_min(1e-300) * rs if mistake == "rowsum_after_drop" else l   # rows renormalised
    o = rnd((rnd(e * mf) @ v) * (rs / lf))
    P = torch.exp(s - lse[..., None])
    delta = (dO * o).sum(dim=-1, keepdim=True)
    dP = dO @ v.transpose(-1, -2)
    if mistake == "bwd_unmasked":
        Mq, Mk = torch.full_like(mq, rs), torch.full_like(mk, rs)
    else:
        Mq, Mk = mq * rs, mk * rs
    dq = rnd(scale * rnd(P * (Mq * dP - delta)) @ k)
    dk = rnd(scale * rnd(P * (Mk * dP - delta)).transpose(-1, -2) @ q)
    dv = rnd((rnd(P * mk).transpose(-1, -2) @ dO) * (1.0 if mistake == "dv_unscaled" else rs))
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def restated(c: Case, mistake: Optional[str] = None, kernel_rounding: bool = False) -> dict:
    i = inputs(c)
    return restated_run(c, i["qkv"], i["dout"], mistake, kernel_rounding)


# ---- the check --------------------------------------------------------------------------------------------------------------------
def check(c: Case, got: dict, ref: Optional[dict] = None, bound: float = PER_ROW_BOUND) -> dict:
    """error / bound of o, dq, dk, dv (per-row relative L2 over `bound`; every row; a reference row that is exactly zero -- a query with
    no kept key has o = dq = 0, a key no query keeps has dv = 0 -- must be exactly zero, else inf) and of lse (LSE_TOL max(1, |lse|)).
    N = 1: dq and dk are the one-key cancellation of attn_edges_ref.check, bounded absolutely, times 1 / (1 - p_eff)."""
    ref = reference(c) if ref is None else ref
    i = inputs(c)
    out = {}
    for name in ("o", "dq", "dk", "dv"):
        g, r = got[name].detach().cpu().double(), ref[name]
        assert g.shape == r.shape, (name, g.shape, r.shape)
        if not bool(torch.isfinite(g).all()):
            out[name] = float("inf")
            continue
        if c.N == 1 and name in ("dq", "dk"):
            q, k, v = heads(i["qkv"].double(), c.B, c.N, c.H, c.dh)
            dO = heads(i["dout"].double(), c.B, c.N, c.H, c.dh)[0]
            assert bool((r.abs() < 1e-12).all())
            cancel = (2 * c.dh * 2.0 ** -24 * dO.norm(dim=-1) * v.norm(dim=-1) * i["scale"] * (k if name == "dq" else q).norm(dim=-1)
                      / (1.0 - p_eff(c.p)))
            out[name] = (g.norm(dim=-1) / cancel).max().item()
            if name == "dq" and bool((g[ref["none"]] != 0).any()):
                out[name] = float("inf")
            continue
        out[name] = per_row_rel(g, r).max().item() / bound
    g, r = got["lse"].detach().cpu().double(), ref["lse"]
    out["lse"] = ((g - r).abs().max() / (LSE_TOL * max(1.0, r.abs().max().item()))).item()
    return out


# ---- probes -----------------------------------------------------------------------------------------------------------------------
def probe_blocks(c: Case) -> int:
    return (c.N + c.dh - 1) // c.dh


def probe_inputs(c: Case, kind: str, j: int):
    """(qkv, dout) bf16 of probe call `kind` ("fwd_dv" | "dq") for block j; q = 0 everywhere."""
    B, N, H, dh = c.B, c.N, c.H, c.dh
    x = torch.zeros(B, N, 3, H, dh)
    d = torch.zeros(B, N, H, dh)
    rows = torch.arange(j * dh, min(N, (j + 1) * dh))
    if kind == "fwd_dv":
        x[:, rows, 2, :, rows - j * dh] = 1.0            # v one-hot over the key block
        d[:, rows, :, rows - j * dh] = 1.0               # dO one-hot over the query block
    else:
        x[:, :, 2, :, 0] = 1.0                           # v_k = e_0
        d[:, :, :, 0] = 1.0                              # dO_q = e_0
        x[:, rows, 1, :, rows - j * dh] = 1.0            # k one-hot over the key block
    return x.reshape(B * N, 3 * H * dh).to(torch.bfloat16), d.reshape(B * N, H * dh).to(torch.bfloat16)


def probe_decode(c: Case, run: Callable) -> dict:
    """`run(qkv, dout) -> {"o", "dq", "dv"} [B,H,N,dh]`: the masks the forward ("fwd"), the key-owner ("dv") and the query-owner ("dq")
    kernel used, bool [B,H,N,N], decoded from ceil(N / dh) pairs of probe calls."""
    B, N, H, dh = c.B, c.N, c.H, c.dh
    rs = 1.0 / (1.0 - p_eff(c.p))
    out = {n: torch.zeros(B, H, N, N, dtype=torch.bool) for n in ("fwd", "dv", "dq")}
    for j in range(probe_blocks(c)):
        w = min(N, (j + 1) * dh) - j * dh
        sl = slice(j * dh, j * dh + w)
        a = run(*probe_inputs(c, "fwd_dv", j))
        out["fwd"][:, :, :, sl] = a["o"].double()[..., :w] != 0                               # o[q, d]: key j dh + d
        out["dv"][:, :, sl, :] = (a["dv"].double()[..., :w] != 0).transpose(-1, -2)           # dv[k, d]: query j dh + d
        b = run(*probe_inputs(c, "dq", j))
        val = b["dq"].double()[..., :w] * (N / dh ** -0.5) + b["o"].double()[..., :1]
        out["dq"][:, :, :, sl] = val > rs / 2
    return out
