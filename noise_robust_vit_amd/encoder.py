"""Encoder-block hot path: forward/backward schedules over the HIP kernels, exposed as autograd Functions.

One transformer block = two "halves", both pre-LayerNorm with a residual add:

    attention half :  x -> LN -> QKV GEMM -> fused attention -> out-proj GEMM (+bias) (+x)
    MLP half       :  x -> LN -> fc1 GEMM +bias +GELU -> fc2 GEMM +bias (+x)

which is `Transformer.forward` of the reference (simple_vit.py:93-97: x = attn(x) + x; x = ff(x) + x) and
`EncoderBlock.forward` (vit.py:118-130).  The residual stream is fp32 in HBM; every GEMM operand is bf16;
LayerNorm statistics, softmax and all accumulation are fp32 (DESIGN.md "Numerics").

Backward is hand-scheduled (no autograd graph inside the stack): per half,
    dW2 = dY^T H (TN GEMM), dH = dY W2 (NT GEMM on the staged W2^T) with the GELU' epilogue, ...
and the LayerNorm backward kernel adds the residual-stream gradient and emits both the fp32 stream
gradient and the bf16 copy the next GEMMs consume.

Nothing here computes with torch ops: torch supplies memory, streams and the autograd boundary.
"""
from __future__ import annotations

import functools
import weakref
from dataclasses import dataclass
from typing import Callable, List, NamedTuple, Optional, Sequence

import torch
from torch import nn

from . import kernels as K
from ._lib import (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_Q8, EPI_BIAS_RESIDUAL, EPI_DGELU, EPI_DGELU_Q8, EPI_NONE, NrvError)

Tensor = torch.Tensor

PARAMS_PER_LAYER = 12   # ln1_w ln1_b wqkv bqkv wo bo ln2_w ln2_b w1 b1 w2 b2


# ----------------------------------------------------------------------------------------------
# bf16 weight staging: W (fp32 master, nn.Parameter) -> bf16 W and bf16 W^T, refreshed when the
# parameter's version counter changes (i.e. once per optimizer step).
# ----------------------------------------------------------------------------------------------
class WeightCache:
    """(id(owner), data_ptr, shape) -> (weakref(owner), version, bf16 W, bf16 W^T); owner = the tensor, or its base when
    it is a view of a persistent buffer (lucid_vit.Attention's fused [to_q; to_kv] projection).  Dead entries are purged.

    `derived` sources: fp32 buffers that are COPIES of parameters (the fused projection above) register a refresher; it
    runs before `refresh_all()` re-stages the images and whenever `epoch` moved, so a copy never outlives an update of
    its parameters through raw pointers (which leaves version counters untouched)."""

    def __init__(self) -> None:
        self._d = {}
        self._jobs = None
        self._derived = []           # weak references to bound methods
        self.epoch = 0

    @staticmethod
    def _owner(w: Tensor) -> Tensor:
        return w._base if w._base is not None else w

    def get(self, w: Tensor, need_t: bool):
        owner = self._owner(w)
        key = (id(owner), w.data_ptr(), tuple(w.shape))
        ent = self._d.get(key)
        ver = w._version
        if ent is not None and ent[0]() is owner and ent[1] == ver:
            return ent[2], ent[3]
        w2 = w.detach()
        if w2.dim() != 2:                       # Conv2d patch-embed weight [D, C, p, p] viewed as [D, C*p*p]
            w2 = w2.reshape(w2.shape[0], -1)
        wb, wt = K.cast_transpose(w2, need_t=True)
        if len(self._d) > 2048:
            self._d = {k: v for k, v in self._d.items() if v[0]() is not None}
        self._d[key] = (weakref.ref(owner), ver, wb, wt)
        self._jobs = None
        return wb, wt

    def add_derived(self, bound_method) -> None:
        self._derived.append(weakref.WeakMethod(bound_method))

    def _run_derived(self) -> None:
        alive = []
        for r in self._derived:
            fn = r()
            if fn is not None:
                fn()
                alive.append(r)
        self._derived = alive

    def clear(self) -> None:
        self._d.clear()
        self._jobs = None
        self.epoch += 1

    def refresh_all(self) -> None:
        """Re-stage every live entry IN PLACE with one batched launch (after an optimizer step that updated the fp32 masters
        through raw pointers: version counters and addresses are unchanged, so the entries stay valid afterwards)."""
        self.epoch += 1
        self._run_derived()                    # fp32 copies of parameters first: their images are re-staged below
        live = [(k, v) for k, v in self._d.items() if v[0]() is not None]
        if len(live) != len(self._d):
            self._d = dict(live)
            self._jobs = None
        key = tuple(k for k, _ in live)
        jobs = self._jobs
        if jobs is None or jobs[0] != key:
            srcs = []
            for k, (ref, ver, wb, wt) in live:
                w = ref().detach()
                if w.data_ptr() != k[1] or w.numel() != wb.numel() or not w.is_contiguous():
                    self.clear()                 # something else changed (or a partial view): fall back to lazy re-staging
                    return
                srcs.append((w.reshape(wb.shape), wb, wt))
            jobs = (key, K.build_cast_jobs(srcs), srcs)
            self._jobs = jobs
        K.run_cast_jobs(jobs[1])
        # the images are current again: entries whose source bumped its version meanwhile (derived copies) stay valid
        for k, v in list(self._d.items()):
            o = v[0]()
            if o is not None:
                self._d[k] = (v[0], o._version, v[2], v[3])


WEIGHTS = WeightCache()


# ----------------------------------------------------------------------------------------------
# host helpers shared by the model ports (Swin, LeViT, PatchConvNet, CaiT, T2T-ViT, RvT, PiT, DeepViT, CCT, Twins-SVT): a port
# imports them from here, never from another port
# ----------------------------------------------------------------------------------------------
def require_cuda(x: Tensor) -> None:
    if not x.is_cuda:
        raise NrvError("noise_robust_vit_amd runs on the MI355X (HIP) device only: move the module and its input to 'cuda'.  "
                       "There is deliberately no CPU fallback on this path.")


def refuse_recording(what: str) -> None:
    if _RECORDING is not None:
        raise NotImplementedError(f"attention-map recording is not implemented for {what}")


def require_run(x: Tensor, what: str) -> None:
    """The guard in front of a port's schedule: a device tensor, and no record_attention around the call."""
    require_cuda(x)
    refuse_recording(what)


class Holder(nn.Module):
    """A module that only carries the reference's parameter names; the layer it belongs to runs as one fused schedule."""

    def forward(self, *args, **kwargs):
        raise NotImplementedError(f"{type(self).__name__} holds parameters only: its layer runs as one fused HIP schedule, call the "
                                  "Transformer (or the model) that owns it")


class Residual(Holder):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn


class PreNorm(Holder):
    def __init__(self, dim, fn):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.fn = fn


class FeedForward(Holder):
    def __init__(self, dim, hidden_dim, dropout=0.):
        super().__init__()
        if dim % 8 or hidden_dim % 8:
            raise NotImplementedError(f"FeedForward {dim} -> {hidden_dim}: the kernels take multiples of 8")
        self.net = nn.Sequential(nn.Linear(dim, hidden_dim), nn.GELU(), nn.Dropout(dropout), nn.Linear(hidden_dim, dim), nn.Dropout(dropout))


class Rearrange(nn.Module):
    """Placeholder for an einops Rearrange (no parameters): what the pattern names is the kernels' addressing."""

    def __init__(self, pattern: str, **axes):
        super().__init__()
        self.pattern, self.axes = pattern, axes

    def extra_repr(self):
        return ", ".join([repr(self.pattern)] + [f"{k}={v}" for k, v in self.axes.items()])


_INDEX_CACHE = {}


def cached(kind: str, fn, *args, device) -> Tensor:
    """fn(*args) (an index tensor built by host arithmetic) on `device`, built once per (kind, args, device)."""
    key = (kind, args, str(device))
    t = _INDEX_CACHE.get(key)
    if t is None:
        if len(_INDEX_CACHE) > 256:
            _INDEX_CACHE.clear()
        t = fn(*args).to(device)
        _INDEX_CACHE[key] = t
    return t


def rows_bf16(src: Tensor, index: Tensor) -> Tensor:
    """bf16 row gather through the fp32 row kernel: a row of C bf16 is C / 2 fp32 words (C % 8 == 0)."""
    return K.gather_rows(src.view(torch.float32), index).view(torch.bfloat16)


def scatter_bf16(src: Tensor, index: Tensor, rows: int) -> Tensor:
    return K.scatter_rows(src.view(torch.float32), index, rows).view(torch.bfloat16)


def conv_to_columns(w: Tensor, KP: int) -> Tensor:
    """A Conv2d weight [Co, C, ks, ks] as [Co, KP] in the unfold's (ky, kx, c) feature order, zero columns behind ks * ks * C."""
    w2 = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    if w2.shape[1] != KP:
        w2 = torch.nn.functional.pad(w2, (0, KP - w2.shape[1]))
    return w2.contiguous()


def conv_from_columns(wc: Tensor, C: int, ks: int) -> Tensor:
    """The inverse of conv_to_columns: [Co, KP] in (ky, kx, c) order -> [Co, C, ks, ks] (a weight gradient dy^T cols)."""
    return wc[:, :ks * ks * C].reshape(wc.shape[0], ks, ks, C).permute(0, 3, 1, 2).contiguous()


def conv_images(w: Tensor, KP: int):
    """bf16 images (W, W^T) of a Conv2d weight in the unfold's feature order, padded to KP columns."""
    return K.cast_transpose(conv_to_columns(w.detach(), KP), need_t=True)


def conv_cols(src: Tensor, w: Tensor, B: int, C: int, H: int, W: int, ks: int, stride: int, pad: int, nhwc: bool):
    """One layer of a conv stem as a GEMM: (im2col rows of src, bf16 W, bf16 W^T).  The images are staged on every call."""
    cols = K.conv_unfold(src, B, C, H, W, ks, stride, pad, nhwc=nhwc)
    return (cols, *conv_images(w, cols.shape[1]))


def conv_wgrad(dy: Tensor, cols: Tensor, C: int, ks: int) -> Tensor:
    """The layer's weight gradient dy^T cols in the parameter's [Co, C, ks, ks] order."""
    return conv_from_columns(K.gemm_tn(dy, cols), C, ks)


def conv_dx(dy: Tensor, wt: Tensor, B: int, C: int, H: int, W: int, ks: int, stride: int, pad: int) -> Tensor:
    """The layer's input gradient dy W folded back to fp32 NHWC rows [B*H*W, C]."""
    return K.conv_fold(K.gemm_nt(dy, wt, out_dtype=torch.bfloat16), B, C, H, W, ks, stride, pad)


def padded_images(weight: Tensor, FP: int, need_t: bool):
    """bf16 (W, W^T) of a projection [Co, ...] of F features whose GEMM rows carry FP >= F (a patch of 3 * 14 * 14 = 588 -> 592):
    the unfold pads its rows with zero columns to the GEMM's K granularity, the projection gets matching ones.  FP == F comes
    from the weight cache; the padded image is one small cast per call, outside it."""
    F = weight[0].numel()
    if FP == F:
        return WEIGHTS.get(weight, need_t)
    w2 = torch.nn.functional.pad(weight.detach().reshape(weight.shape[0], F).to(torch.float32), (0, FP - F))
    return K.cast_transpose(w2, need_t=need_t)


def linear(x16: Tensor, w: Tensor, b: Optional[Tensor], out_dtype=torch.bfloat16) -> Tensor:
    wb, _ = WEIGHTS.get(w, True)
    if b is None:
        return K.gemm_nt(x16, wb, out_dtype=out_dtype, epilogue=EPI_NONE)
    return K.gemm_nt(x16, wb, out_dtype=out_dtype, epilogue=EPI_BIAS, bias=b.detach())


def wgrad(dys, xs, want_bias: bool):
    """sum_i dys[i]^T xs[i] (and the bias gradient): the class rows' and the patch rows' contributions to one weight."""
    dw, db = K.gemm_tn(dys[0], xs[0], want_dbias=True) if want_bias else (K.gemm_tn(dys[0], xs[0]), None)
    for dy, x in zip(dys[1:], xs[1:]):
        if want_bias:
            K.gemm_tn(dy, x, out=dw, beta=1.0, dbias=db, dbias_beta=1.0)
        else:
            K.gemm_tn(dy, x, out=dw, beta=1.0)
    return dw, db


def dx_sum(pairs, out_dtype):
    """sum_i d_i W_i: the input gradient of several Linears that read the same rows (EPI_BIAS_RESIDUAL chains the sum)."""
    acc = None
    for i, (d16, w) in enumerate(pairs):
        _, wt = WEIGHTS.get(w, True)
        dt = out_dtype if i == len(pairs) - 1 else torch.float32
        acc = K.gemm_nt(d16, wt, out_dtype=dt) if acc is None else K.gemm_nt(d16, wt, out_dtype=dt, epilogue=EPI_BIAS_RESIDUAL, aux=acc)
    return acc


class LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm on fp32 rows [R, D] through the HIP kernels; the bf16 result is returned widened to fp32 (the stream)."""

    @staticmethod
    def forward(ctx, x, w, b, eps: float):
        x = x.detach().contiguous()
        y, mean, rstd = K.layernorm_fwd(x, w, b, eps)
        ctx.save_for_backward(x, mean, rstd)
        ctx.w = w
        return y.to(torch.float32)

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd = ctx.saved_tensors
        d16 = K.cast_bf16(dy.to(torch.float32).contiguous())
        dx, _, dg, db = K.layernorm_bwd(d16, x, ctx.w, mean, rstd, want_f32=True)
        return dx, dg, db, None


@dataclass
class BlockMeta:
    heads: int
    dim_head: int
    eps: float
    robust: bool = False
    # optional gradient sink (data-parallel runtime): grad_out(param) -> (tensor, beta) or None
    sink: Optional[object] = None
    # residual / MLP dropout of the block stack (vit.py:100-101,112,125): probability for the NEXT forward (the modules set it
    # from their own p and training flag) and an optional source of keep masks, site -> uint8 tensor (tests inject the masks the
    # oracle uses; default: torch's device generator).  Sites of layer i: 3 i (attention branch), 3 i + 1 (GELU output), 3 i + 2 (MLP branch).
    dropout: float = 0.0
    mask_source: Optional[object] = None
    # dropout on the attention weights (vit.py:108): composed on the materialised [B,H,N,N] matrix (kernels.attn_composed_fwd), site -(2 + i)
    attn_dropout: float = 0.0
    # ... or, with `attn_dropout_fused`, inside the fused softmax kernels (kernels.attn_drop_fwd: the mask is a function of a 64-bit
    # seed and is regenerated in the backward; nothing of size N^2 is written) wherever those kernels apply: no mask_source, no score
    # bias, not robust, no memories.  `attn_seed_source`: site -> int64 [1] device tensor (tests inject seeds as mask_source injects
    # masks; default: torch's device generator, one draw per call, graph-safe)
    attn_dropout_fused: bool = False
    attn_seed_source: Optional[object] = None
    # additive score bias of ONE call (attention / key-padding masks of the stand-alone MultiheadAttention, utils.py:741-751): fp32,
    # broadcastable to [B, H, N, N], -inf = masked; composed path
    attn_bias: Optional[Tensor] = None


def _grad_target(meta: BlockMeta, p: Optional[Tensor]):
    """(out, beta) for a weight gradient: the sink's flat-buffer view if a sink is attached, else fresh."""
    if p is None:
        return None, 0.0
    if meta.sink is not None:
        return meta.sink.target(p)
    return None, 0.0


def sink_params(params) -> list:
    """The registered parameters behind a layer's tensors: a fused projection (`_nrv_parts`, lucid_vit.Attention) stands for
    the parameters whose rows it stacks."""
    out = []
    for q in params:
        if q is None:
            continue
        parts = getattr(q, "_nrv_parts", None)
        out += [pp for pp, _, _ in parts] if parts is not None else [q]
    return out


# Weight gradients on a second HIP stream.  dW = dy^T x only feeds the optimizer, so it can run beside the dX chain (the NT GEMM
# of the same layer reads the same dy) and take the CUs that chain leaves idle: with one 512-thread workgroup per CU a grid
# of 316 or 396 tiles (ViT-L, ViT-S, the MAE encoder) occupies 62 - 77 % of its CU-rounds.  Measured on the whole step
# (profiles/r03_wgrad_stream_ab.txt): ViT-S -2.5 %, ViT-L -2.1 %, MAE -2.6 %; ViT-B/16 at batch 256 (474 tiles, 93 %) +-0.1 %,
# where the chip is already power-limited -- so the stream is used only when the dX grid fills its rounds poorly ("auto").
WGRAD_STREAM = "auto"            # "auto" | True | False
WGRAD_MIN_IDLE = 0.15
_WGRAD_SIDE = {}
_WGRAD_KEEP: list = []


def _wgrad_side(device) -> "torch.cuda.Stream":
    s = _WGRAD_SIDE.get(device.index)
    if s is None:
        s = _WGRAD_SIDE[device.index] = torch.cuda.Stream(device=device)
    return s


@functools.lru_cache(maxsize=None)
def _dx_grid_idle(rows: int, cols: int, cus: int) -> float:
    """Share of CU-rounds the [rows x cols] dX GEMM leaves empty under the best of the NT kernel's tile heights (256-column tiles)."""
    best = 1.0
    for h in (256, 320, 192, 128):
        tiles = -(-rows // h) * -(-cols // 256)
        best = min(best, 1.0 - tiles / (-(-tiles // cus) * cus))
    return best


def _wgrad_on_side(dy16: Tensor, x16: Tensor) -> bool:
    if K._PROF is not None:                  # per-launch timing (bench.py's roofline leg): one stream, every launch timed alone
        return False
    if WGRAD_STREAM == "auto":
        # judged on the layer's narrow side (the residual width: every second GEMM of the dX chain has that many columns);
        # deciding per GEMM instead was measured 0.5 - 1 % slower on ViT-S / ViT-L than moving the whole layer's weight gradients
        cus = torch.cuda.get_device_properties(x16.device).multi_processor_count
        return _dx_grid_idle(x16.shape[0], min(x16.shape[1], dy16.shape[1]), cus) >= WGRAD_MIN_IDLE
    return bool(WGRAD_STREAM)


def wgrad_join() -> None:
    """The current stream waits for every weight gradient issued so far; their operands may be freed afterwards."""
    if _WGRAD_KEEP:
        dev = _WGRAD_KEEP[0][0].device
        torch.cuda.current_stream(dev).wait_stream(_wgrad_side(dev))
        _WGRAD_KEEP.clear()


# Weight gradients are QUEUED while a layer is differentiated and issued together when it is done (`wgrad_flush`): the four of an
# encoder block (dWqkv, dWo, dW1, dW2 and their bias gradients) are ONE stream-K launch (kernels.gemm_tn_grouped) that fills every
# CU whatever the matrices' tile counts and pays prologue, epilogue and partial-tile traffic once per layer instead of once per
# gradient (round 4; before: one split-K launch + one slab reduction per gradient).
_PENDING: list = []
WGRAD_GROUPED = False            # True: one grouped launch per layer (kernels.gemm_tn_grouped); False: every gradient is its own split-K launch, issued where it is queued (the round-3 schedule)


def _queue(meta: BlockMeta, q: dict) -> None:
    _PENDING.append(q)
    if not WGRAD_GROUPED:
        wgrad_flush(meta)


# The slab reduction of a split-K weight gradient as a side job of the dX GEMM that follows it (kernels.gemm_tn defer / gemm_nt side):
# the late-starting workgroups of the persistent NT kernel reduce the slabs where they would nap.  A token lives in a local list of
# the half's backward from the weight-gradient launch to the very next NT launch, which takes it (inside its launch, or as a
# stand-alone reduction in front of it when the library does not admit the job): nothing is ever pending across a
# `wgrad_flush`, a `wgrad_join`, `sink.layer_done` or a return to autograd, and a backward that raises drops its token with its frame.
WGRAD_DEFER = True


def _take(tok: Optional[list]):
    """The pending reduction a deferring `_dw_db` left in `tok`, once (None when it did not defer)."""
    return tok.pop() if tok else None


def _dw_db(meta: BlockMeta, dy16: Tensor, x16: Tensor, w: Tensor, b: Optional[Tensor], need=None, defer: Optional[list] = None):
    """Queue the weight and bias gradient of y = x W^T + b (dW = dy^T x on the MFMA, db = colsum(dy) fused into the same kernel).
    Returns (dW, db) as the tensors the launch of `wgrad_flush` will fill: the sink's flat-buffer views, or fresh ones.
    `need` (optional (dW wanted, db wanted)): nothing is queued when neither is wanted (a frozen layer), the bias is left out
    when only dW is.  `defer` (a list): with one split-K launch per gradient on the main stream the launch is issued here without
    its reduction, and the `kernels.PendingReduce` is appended for the caller's next `K.gemm_nt(..., side=_take(defer))`."""
    if need is not None:
        if not need[0] and not need[1]:
            return None, None
        if not need[1]:
            b = None
    parts = getattr(w, "_nrv_parts", None)
    if parts is not None and meta.sink is not None:
        # w stacks the rows of several parameters ([to_q; to_kv]): straight into their slots of the sink -- one problem when the
        # slots are adjacent (GradReducer + grad_groups), else one per parameter on the matching column block of dy
        if b is not None:
            raise NrvError("a fused projection carries no bias")
        block = meta.sink.target_block([pp for pp, _, _ in parts]) if hasattr(meta.sink, "target_block") else None
        if block is not None:
            _queue(meta, dict(A=dy16, B=x16, out=block[0], beta=block[1]))
            return None, None
        for pp, r0, r1 in parts:
            tw, bw = meta.sink.target(pp)
            _queue(meta, dict(A=dy16[:, r0:r1], B=x16, out=tw, beta=bw))
        return None, None
    tw, bw = _grad_target(meta, w)
    tb, bb = _grad_target(meta, b) if b is not None else (None, 0.0)
    M, N = dy16.shape[1], x16.shape[1]
    out = tw if tw is not None else torch.empty(M, N, dtype=torch.float32, device=dy16.device)
    dbias = None if b is None else (tb if tb is not None else torch.empty(M, dtype=torch.float32, device=dy16.device))
    if defer is not None and WGRAD_DEFER and not WGRAD_GROUPED and not (meta.sink is not None and _wgrad_on_side(dy16, x16)):
        wgrad_flush(meta)                # launch order = queue order
        defer.append(K.gemm_tn(dy16, x16, out=out, beta=bw if tw is not None else 0.0, dbias=dbias,
                               dbias_beta=bb if tb is not None else 0.0, defer=True)[-1])
        return out, dbias
    _queue(meta, dict(A=dy16, B=x16, out=out, beta=bw if tw is not None else 0.0, dbias=dbias, dbias_beta=bb if tb is not None else 0.0))
    return out, dbias


def wgrad_flush(meta: BlockMeta) -> None:
    """Issue the queued weight gradients (groups of up to 4 with the same token count).  With a gradient sink (results go to
    persistent buffers nobody reads before `wgrad_join`) the launch may go to the side stream, beside the next layer's dX chain."""
    if not _PENDING:
        return
    probs = list(_PENDING)
    _PENDING.clear()
    groups, cur = [], []
    for q in probs:
        if cur and (len(cur) == 4 or q["A"].shape[0] != cur[0]["A"].shape[0]):
            groups.append(cur)
            cur = []
        cur.append(q)
    groups.append(cur)
    dy16, x16 = probs[0]["A"], probs[0]["B"]
    if meta.sink is not None and _wgrad_on_side(dy16, x16):
        side = _wgrad_side(dy16.device)
        side.wait_stream(torch.cuda.current_stream(dy16.device))
        _WGRAD_KEEP.append(tuple(t for q in probs for t in (q["A"], q["B"])))     # alive until the join
        with torch.cuda.stream(side):
            for g in groups:
                _issue(g)
        return
    for g in groups:
        _issue(g)


def _issue(group: list) -> None:
    if WGRAD_GROUPED:
        K.gemm_tn_grouped(group)
        return
    for q in group:
        K.gemm_tn(q["A"], q["B"], out=q["out"], beta=q["beta"], dbias=q.get("dbias"), dbias_beta=q.get("dbias_beta", 0.0))


# ----------------------------------------------------------------------------------------------
# introspection: attention maps for recorder.Recorder (the fused kernels never materialise them)
# ----------------------------------------------------------------------------------------------
_RECORDING: Optional[list] = None


class record_attention:
    """Context manager: every attention layer run inside appends its fp32 [B, H, N, N] probabilities to `sink`
    (softmax, or the Sinkhorn-normalised matrix for robust=True), recomputed from q, k and the saved statistics."""

    def __init__(self, sink: list) -> None:
        self.sink = sink

    def __enter__(self):
        global _RECORDING
        self._prev, _RECORDING = _RECORDING, self.sink
        return self.sink

    def __exit__(self, *exc):
        global _RECORDING
        _RECORDING = self._prev


def _record(qkv: Tensor, att: AttnSaved, B: int, N: int, H: int, dh: int, scale: float) -> None:
    p = K.attn_probs(qkv, att.lse, B, N, H, dh, scale)
    if att.kind == "sinkhorn":                            # scalings [B, H, 7, N]: a1 b1 a2 b2 a3 b3 a4
        a, b = att.scal[:, :, 6], att.scal[:, :, 5]      # the vectors are cumulative: P = diag(a4) softmax(S) diag(b3)
        p = p * a[..., :, None] * b[..., None, :]
    _RECORDING.append(p)


# ----------------------------------------------------------------------------------------------
# attention half
# ----------------------------------------------------------------------------------------------
class AttnSaved(NamedTuple):
    """Saved attention state and the path that wrote it: "softmax" (lse), "softmax_drop" (weight dropout inside the fused kernels:
    lse of the undropped rows, and in `saved` the (seed tensor, p) the backward regenerates the mask from), "sinkhorn" (robust=True:
    lse, scal, and in `saved` the P7 dict of kernels.attn_sinkhorn_fwd) or "composed" (weight dropout / score bias on the
    materialised matrix: kernels.ComposedSaved in `saved`)."""
    kind: str
    lse: Optional[Tensor] = None
    scal: Optional[Tensor] = None
    saved: object = None


def draw_keep(meta: BlockMeta, site: int, shape, device, p: Optional[float] = None) -> Tensor:
    """uint8 keep mask of one dropout site (1 = kept); p defaults to the stack's `dropout`."""
    if meta.mask_source is not None:
        m = meta.mask_source(site, tuple(shape))
        if m.dtype != torch.uint8 or tuple(m.shape) != tuple(shape):
            raise NrvError(f"mask_source({site}): expected a uint8 mask of shape {tuple(shape)}")
        return m.to(device).contiguous()
    return (torch.rand(shape, device=device) >= (meta.dropout if p is None else p)).to(torch.uint8)


def attn_drop_fused(meta: BlockMeta, adrop) -> bool:
    """Whether the attention-weight dropout `adrop` of attn_half_fwd runs inside the fused kernels."""
    return (adrop is not None and meta.attn_dropout_fused and meta.mask_source is None and meta.attn_bias is None
            and not meta.robust and meta.dim_head in K.ATTN_FUSED_DH)


def draw_attn_seeds(meta: BlockMeta, sites, device) -> List[Tensor]:
    """One int64 [1] seed tensor per site: injected, or slices of ONE draw from torch's device generator."""
    if meta.attn_seed_source is not None:
        out = []
        for site in sites:
            t = meta.attn_seed_source(site)
            if t.dtype != torch.int64 or t.numel() != 1:
                raise NrvError(f"attn_seed_source({site}): expected an int64 tensor of one element")
            out.append(t.to(device).reshape(1))
        return out
    drawn = torch.randint(-2 ** 63, 2 ** 63 - 1, (len(sites),), dtype=torch.int64, device=device)
    return [drawn[i:i + 1] for i in range(len(sites))]


class MemKV(NamedTuple):
    """Memory keys / values and score mask of one attention layer (learnable_memory_vit.py:64-86): `rows` fp32 [M, D] (one set
    for every sample) or [B*M, D] (one set per sample), None when M == 0; they skip the LayerNorm and go through to_kv only."""
    rows: Optional[Tensor]
    M: int
    shared: bool
    mask: Optional[K.MaskBits]


def attn_half_fwd(x: Tensor, B: int, N: int, meta: BlockMeta, ln_w, ln_b, wqkv, bqkv, wo, bo, residual: bool, drop=None, adrop=None,
                  mem: Optional[MemKV] = None):
    """x fp32 [B*N, D] -> (y fp32 [B*N, D], saved).  `ln_w is None`: no LayerNorm in front of the projection (the bare
    `MultiheadAttention.forward` of the reference's forked module, utils.py:741-751).  `mem`: memory keys and / or a score
    mask (nrv_attn_mem_*); wqkv is then the bias-free [to_q; to_kv] projection."""
    H, dh = meta.heads, meta.dim_head
    if ln_w is None:
        xn, mean, rstd = K.cast_bf16(x), None, None
    else:
        xn, mean, rstd = K.layernorm_fwd(x, ln_w, ln_b, meta.eps)
    wqkv_b, _ = WEIGHTS.get(wqkv, True)
    wo_b, _ = WEIGHTS.get(wo, True)
    qkv = K.gemm_nt(xn, wqkv_b, out_dtype=torch.bfloat16,
                    epilogue=EPI_BIAS if bqkv is not None else EPI_NONE, bias=bqkv)
    scale = dh ** -0.5
    if mem is not None:
        if bqkv is not None or adrop is not None or meta.attn_bias is not None or meta.robust:
            raise NrvError("memory keys / score masks go with a bias-free projection, plain softmax and no attention dropout")
        if _RECORDING is not None:
            raise NotImplementedError("recording attention maps is not supported with memory keys / score masks")
        mem16 = mkv = None
        if mem.M > 0:
            # memories skip the LayerNorm and to_q: their k / v are the to_kv rows of the cached bf16 [to_q; to_kv] image
            mem16 = K.cast_bf16(mem.rows)
            mkv = K.gemm_nt(mem16, wqkv_b[H * dh:], out_dtype=torch.bfloat16)
        o, lse = K.attn_mem_fwd(qkv, mkv, B, N, mem.M, H, dh, scale, mem.shared, mem.mask)
        att = AttnSaved("memory", lse, saved=(mem, mem16, mkv))
    elif attn_drop_fused(meta, adrop):            # weight dropout inside the fused kernels: the mask is regenerated from the seed
        pa = adrop[2]
        seed = adrop[3] if len(adrop) > 3 and adrop[3] is not None else draw_attn_seeds(meta, [adrop[1]], x.device)[0]
        o, lse = K.attn_drop_fwd(qkv, seed, pa, B, N, H, dh, scale)
        att = AttnSaved("softmax_drop", lse, saved=(seed, pa))
    elif adrop is not None or meta.attn_bias is not None:      # weight dropout / score masks: the composed path (materialised matrix), softmax or Sinkhorn
        pscale, akeep = 1.0, None
        if adrop is not None:
            pscale, asite, pa = adrop[:3]
            akeep = draw_keep(meta, asite, (B, H, N, N), x.device, p=pa)
        o, cs = K.attn_composed_fwd(qkv, B, N, H, dh, scale, 3 if meta.robust else 0, akeep, pscale, bias=meta.attn_bias)
        att = AttnSaved("composed", saved=cs)
    elif meta.robust:                             # robust=True: softmax + Sinkhorn normalisation (utils.py:1025-1037), fused
        p7 = {}                                   # the composed path (N > 256 / dh != 64) hands its P7 to the backward through it
        o, lse, scal = K.attn_sinkhorn_fwd(qkv, B, N, H, dh, scale, saved=p7)
        att = AttnSaved("sinkhorn", lse, scal, p7)
    else:
        o, lse = K.attn_fwd(qkv, B, N, H, dh, scale)
        att = AttnSaved("softmax", lse)
    if _RECORDING is not None and att.kind not in ("composed", "memory"):
        _record(qkv, att, B, N, H, dh, scale)
    keep = None
    if residual and drop is not None:
        # dropout on the branch output (vit.py:125): the bias epilogue writes the branch, one pass adds what is kept to the stream
        scale, site = drop
        keep = draw_keep(meta, site, x.shape, x.device)
        yb = K.gemm_nt(o, wo_b, out_dtype=torch.float32, epilogue=EPI_BIAS if bo is not None else EPI_NONE, bias=bo)
        y = K.dropout_add(x, yb, keep, scale, out=yb)
    elif residual:
        y = K.gemm_nt(o, wo_b, out_dtype=torch.float32, epilogue=EPI_BIAS_RESIDUAL, bias=bo, aux=x)
    else:
        y = K.gemm_nt(o, wo_b, out_dtype=torch.float32, epilogue=EPI_BIAS if bo is not None else EPI_NONE, bias=bo)
        if drop is not None:             # stand-alone module (learnable_memory_vit.py:61): dropout on the projection's output
            scale, site = drop
            keep = draw_keep(meta, site, y.shape, x.device)
            K.mask_mul_f32(y, keep, scale, out=y)
    return y, (x, xn, mean, rstd, qkv, o, att, keep)


def attn_half_bwd(dy32: Optional[Tensor], dy16: Optional[Tensor], saved, B: int, N: int, meta: BlockMeta,
                  ln_w, ln_b, wqkv, bqkv, wo, bo, residual: bool, want_bf16: bool, want_f32: bool = True, drop_scale: float = 1.0,
                  need=None, mem_grad: Optional[list] = None):
    """Returns (dx32|None, dx16|None, [d ln_w, d ln_b, d wqkv, d bqkv, d wo, d bo]).

    The incoming gradient is given as fp32 (`dy32`), bf16 (`dy16`) or both; the residual add uses fp32 when present.
    `need` (optional, one flag per parameter): weight-gradient GEMMs of parameters without a flag are not issued.  With memory
    keys, `mem_grad` (a list) receives the fp32 gradient of the memory rows (None when M == 0); the memory rows' share of
    d wqkv is added to its to_kv rows."""
    x, xn, mean, rstd, qkv, o, att, keep = saved
    H, dh = meta.heads, meta.dim_head
    if dy16 is None:
        dy16 = K.cast_bf16(dy32)
    if keep is not None:                 # the branch sees the dropped gradient; the residual path (dres below) the whole one
        dy16 = K.mask_mul(dy16, keep, drop_scale)
    _, wo_t = WEIGHTS.get(wo, True)
    _, wqkv_t = WEIGHTS.get(wqkv, True)
    # out-proj:  y = o Wo^T (+bo) (+x)
    tok: list = []                       # the weight gradient's pending reduction, taken by the NT launch that follows
    dwo, dbo = _dw_db(meta, dy16, o, wo, bo, None if need is None else need[4:6], defer=tok)
    do = K.gemm_nt(dy16, wo_t, out_dtype=torch.bfloat16, side=_take(tok))
    scale = dh ** -0.5
    dmkv = None
    if att.kind == "memory":
        mem, mem16, mkv = att.saved
        dqkv, dmkv = K.attn_mem_bwd(qkv, o, do, att.lse, mkv, B, N, mem.M, H, dh, scale, mem.shared, mem.mask)
    elif att.kind == "composed":
        dqkv = K.attn_composed_bwd(qkv, do, att.saved, B, N, H, dh, scale)
    elif att.kind == "softmax_drop":
        seed, pa = att.saved
        dqkv = K.attn_drop_bwd(qkv, o, do, att.lse, seed, pa, B, N, H, dh, scale)
    elif att.kind == "sinkhorn":
        dqkv = K.attn_sinkhorn_bwd(qkv, do, att.lse, att.scal, B, N, H, dh, scale, saved=att.saved)
    else:
        dqkv = K.attn_bwd(qkv, o, do, att.lse, B, N, H, dh, scale)
    dwqkv, dbqkv = _dw_db(meta, dqkv, xn, wqkv, bqkv, None if need is None else need[2:4], defer=tok)
    if att.kind == "memory":
        dmem = None
        K.flush_reduce(_take(tok))       # the memory rows' launches below read dwqkv
        if dmkv is not None:
            # dmem = dKV_mem Wkv; dWkv += dKV_mem^T mem (summed over the batch already for shared memories)
            inner = H * dh
            dmkv16 = K.cast_bf16(dmkv)
            dmem = K.gemm_nt(dmkv16, wqkv_t[:, inner:], out_dtype=torch.float32)
            if dwqkv is not None:
                wgrad_flush(meta)                # the token rows' launch writes dwqkv first
                K.gemm_tn(dmkv16, mem16, out=dwqkv[inner:], beta=1.0)
        if mem_grad is not None:
            mem_grad.append(dmem)
    if ln_w is None:                     # no LayerNorm: the projection's input gradient IS the result
        if residual:
            raise NrvError("a residual attention half needs its LayerNorm")
        dx32 = K.gemm_nt(dqkv, wqkv_t, out_dtype=torch.float32, side=_take(tok))
        return dx32, None, [None, None, dwqkv, dbqkv, dwo, dbo]
    dxn = K.gemm_nt(dqkv, wqkv_t, out_dtype=torch.bfloat16, side=_take(tok))
    tg, bg = _grad_target(meta, ln_w)
    tb, _ = _grad_target(meta, ln_b)
    if residual and keep is not None and dy32 is None:
        raise NrvError("dropout needs the fp32 residual gradient")
    dres = (dy32 if dy32 is not None else dy16) if residual else None
    dx32, dx16, dg, db = K.layernorm_bwd(dxn, x, ln_w, mean, rstd, dres=dres,
                                         want_f32=want_f32, want_bf16=want_bf16, dgamma=tg, dbeta=tb, accumulate=bg != 0.0)
    return dx32, dx16, [dg, db, dwqkv, dbqkv, dwo, dbo]


# ----------------------------------------------------------------------------------------------
# MLP half
# ----------------------------------------------------------------------------------------------
GELU_STREAM_U8 = True        # False: the bf16 gelu' stream of rounds 1 - 3 (A/B, tests)


def fc1_gelu(xn: Tensor, w1_b: Tensor, b1: Tensor, q8: bool, save: bool = True):
    """h = gelu(xn W1^T + b1) on the staged bf16 image `w1_b`.  Returns (h, u): u = gelu'(pre-activation) for
    `dgelu_bwd`, or None with save=False (no gradient will be asked for).  `q8` is the caller's rule and needs
    W1 rows % 64 == 0: one byte per element in row pairs (include/nrv.h NRV_EPI_BIAS_GELU_Q8), else bf16."""
    T, F = xn.shape[0], w1_b.shape[0]
    rows, dtype = ((T + 1) // 2 * 2, torch.uint8) if q8 else (T, torch.bfloat16)
    u = torch.empty(rows, F, dtype=dtype, device=xn.device) if save else None
    h = K.gemm_nt(xn, w1_b, out_dtype=torch.bfloat16, epilogue=EPI_BIAS_GELU_Q8 if q8 else EPI_BIAS_GELU, bias=b1, aux_out=u)
    return h, u


def dgelu_bwd(dy16: Tensor, w2_t: Tensor, u: Tensor, side=None) -> Tensor:
    """du = (dy W2) o gelu', the stream as `fc1_gelu` saved it (bytes or bf16).  `side`: see `kernels.gemm_nt`."""
    return K.gemm_nt(dy16, w2_t, out_dtype=torch.bfloat16, epilogue=EPI_DGELU_Q8 if u.dtype == torch.uint8 else EPI_DGELU, aux=u,
                     side=side)


def mlp_half_fwd(x: Tensor, meta: BlockMeta, ln_w, ln_b, w1, b1, w2, b2, residual: bool, save: bool = True, drop=None):
    """`save=False` (no gradient will be asked for): the fc1 epilogue skips the gelu'(u) output -- a 310 MB store stream per
    layer on ViT-B/16 at batch 256."""
    xn, mean, rstd = K.layernorm_fwd(x, ln_w, ln_b, meta.eps)
    w1_b, _ = WEIGHTS.get(w1, True)
    w2_b, _ = WEIGHTS.get(w2, True)
    # the byte stream, unless a dropout mask is going to be multiplied into it (a scaled value leaves the byte code's range)
    q8 = GELU_STREAM_U8 and drop is None and w1.shape[0] % 64 == 0
    h, u = fc1_gelu(xn, w1_b, b1, q8, save)
    keep2 = None
    if drop is not None:
        # Dropout behind the GELU (vit.py:100) and behind the second Linear (vit.py:101).  The first mask is applied to the saved
        # activation AND to the gelu' stream, so the backward (dW2 = dY^T h, dU = dY W2 o gelu') needs no mask of its own.
        scale, site = drop
        keep1 = draw_keep(meta, site, h.shape, x.device)
        K.mask_mul(h, keep1, scale, out=h)
        if u is not None:
            K.mask_mul(u, keep1, scale, out=u)
        yb = K.gemm_nt(h, w2_b, out_dtype=torch.float32, epilogue=EPI_BIAS if b2 is not None else EPI_NONE, bias=b2)
        keep2 = draw_keep(meta, site + 1, yb.shape, x.device)
        # with a residual the kept part of the branch is added to the stream; the stand-alone module (learnable_memory_vit.py:37-39) returns it
        y = K.dropout_add(x, yb, keep2, scale, out=yb) if residual else K.mask_mul_f32(yb, keep2, scale, out=yb)
    elif residual:
        y = K.gemm_nt(h, w2_b, out_dtype=torch.float32, epilogue=EPI_BIAS_RESIDUAL, bias=b2, aux=x)
    else:
        y = K.gemm_nt(h, w2_b, out_dtype=torch.float32, epilogue=EPI_BIAS if b2 is not None else EPI_NONE, bias=b2)
    return y, (x, xn, mean, rstd, u, h, keep2)


def mlp_half_bwd(dy32: Optional[Tensor], dy16: Optional[Tensor], saved, meta: BlockMeta,
                 ln_w, ln_b, w1, b1, w2, b2, residual: bool, want_bf16: bool, want_f32: bool = True, drop_scale: float = 1.0,
                 need=None):
    x, xn, mean, rstd, u, h, keep2 = saved
    if dy16 is None:
        dy16 = K.cast_bf16(dy32)
    if keep2 is not None:
        if dy32 is None:
            raise NrvError("dropout needs the fp32 residual gradient")
        dy16 = K.mask_mul(dy16, keep2, drop_scale)
    _, w2_t = WEIGHTS.get(w2, True)
    _, w1_t = WEIGHTS.get(w1, True)
    tok: list = []                       # the weight gradient's pending reduction, taken by the NT launch that follows
    dw2, db2 = _dw_db(meta, dy16, h, w2, b2, None if need is None else need[4:6], defer=tok)
    du = dgelu_bwd(dy16, w2_t, u, side=_take(tok))
    dw1, db1 = _dw_db(meta, du, xn, w1, b1, None if need is None else need[2:4], defer=tok)
    dxn = K.gemm_nt(du, w1_t, out_dtype=torch.bfloat16, side=_take(tok))
    tg, bg = _grad_target(meta, ln_w)
    tb, _ = _grad_target(meta, ln_b)
    dres = (dy32 if dy32 is not None else dy16) if residual else None
    dx32, dx16, dg, db = K.layernorm_bwd(dxn, x, ln_w, mean, rstd, dres=dres,
                                         want_f32=want_f32, want_bf16=want_bf16, dgamma=tg, dbeta=tb, accumulate=bg != 0.0)
    return dx32, dx16, [dg, db, dw1, db1, dw2, db2]


def ls_mlp_half_fwd(x: Tensor, eps: float, ln_w, ln_b, w1, b1, w2, b2, gamma: Tensor, q8: bool):
    """The layer-scaled MLP half of CaiT and of PatchConvNet's class-token block: x + gamma * fc2(gelu(fc1(LN x))), x fp32 [R, D],
    gamma fp32 [D].  The caller decides `q8` (see `fc1_gelu`); no gradient sink.  Returns (y, saved) for `ls_mlp_half_bwd`."""
    xn, mean, rstd = K.layernorm_fwd(x, ln_w, ln_b, eps)
    w1_b, _ = WEIGHTS.get(w1, True)
    h, u = fc1_gelu(xn, w1_b, b1.detach(), q8)
    yb = linear(h, w2, b2, torch.float32)
    return K.ls_add(x, yb, gamma), (x, xn, mean, rstd, u, h, yb)


def ls_mlp_half_bwd(dy: Tensor, saved, ln_w, w1, w2, gamma: Tensor):
    """dy fp32 [R, D] -> (dx fp32, [d gamma, d ln_w, d ln_b, d w1, d b1, d w2, d b2])."""
    x, xn, mean, rstd, u, h, yb = saved
    dz, dgamma = K.ls_bwd(dy, yb, gamma)
    dw2, db2 = K.gemm_tn(dz, h, want_dbias=True)
    _, w2_t = WEIGHTS.get(w2, True)
    du = dgelu_bwd(dz, w2_t, u)
    dw1, db1 = K.gemm_tn(du, xn, want_dbias=True)
    dxn = dx_sum([(du, w1)], torch.bfloat16)
    dx, _, dg, db = K.layernorm_bwd(dxn, x, ln_w.detach(), mean, rstd, dres=dy)
    return dx, [dgamma, dg, db, dw1.reshape(w1.shape), db1, dw2.reshape(w2.shape), db2]


# ----------------------------------------------------------------------------------------------
# autograd boundary
# ----------------------------------------------------------------------------------------------
def _as_stream(x: Tensor):
    require_cuda(x)
    if x.dim() != 3:
        raise NrvError(f"expected (batch, tokens, dim), got {tuple(x.shape)}")
    B, N, D = x.shape
    x2 = x.detach().to(torch.float32).contiguous().reshape(B * N, D)
    return x2, B, N, D


def _mask_sink_grads(meta: BlockMeta, grads: List[Optional[Tensor]]) -> List[Optional[Tensor]]:
    """With a sink attached the kernels already wrote into the sink's buffers: hand autograd nothing."""
    wgrad_flush(meta)                  # autograd receives the tensors of `grads`: the queued launches must have been issued
    if meta.sink is None:
        return grads
    wgrad_join()
    return [None for _ in grads]


class EncoderStackFn(torch.autograd.Function):
    """depth x (attention half + MLP half) with residuals; params = PARAMS_PER_LAYER tensors per layer."""

    @staticmethod
    def forward(ctx, x, meta: BlockMeta, *params):
        x2, B, N, D = _as_stream(x)
        _PENDING.clear()                    # gradients queued by a backward that raised half-way never run: drop them (and their operands)
        depth = len(params) // PARAMS_PER_LAYER
        saved = []
        cur = x2
        train = any(ctx.needs_input_grad)            # inference (torch.no_grad / frozen model): keep nothing for a backward
        pdrop = float(meta.dropout)
        if not 0.0 <= pdrop < 1.0:
            raise NrvError(f"dropout probability {pdrop} outside [0, 1)")
        scale = 1.0 / (1.0 - pdrop)
        pattn = float(meta.attn_dropout)
        if not 0.0 <= pattn < 1.0:
            raise NrvError(f"attention dropout probability {pattn} outside [0, 1)")
        seeds = [None] * depth
        if pattn > 0.0 and attn_drop_fused(meta, (None,)):       # fused weight dropout: one draw of seeds for the whole stack
            seeds = draw_attn_seeds(meta, [-(2 + i) for i in range(depth)], x2.device)
        for i in range(depth):
            p = params[i * PARAMS_PER_LAYER:(i + 1) * PARAMS_PER_LAYER]
            cur, sa = attn_half_fwd(cur, B, N, meta, *p[0:6], residual=True, drop=(scale, 3 * i) if pdrop > 0.0 else None,
                                    adrop=(1.0 / (1.0 - pattn), -(2 + i), pattn, seeds[i]) if pattn > 0.0 else None)
            cur, sm = mlp_half_fwd(cur, meta, *p[6:12], residual=True, save=train, drop=(scale, 3 * i + 1) if pdrop > 0.0 else None)
            saved.append((sa, sm) if train else None)
        ctx.meta, ctx.params, ctx.saved_blocks, ctx.shape = meta, params, saved, (B, N, D)
        ctx.drop_scale = scale
        return cur.reshape(B, N, D)

    @staticmethod
    def backward(ctx, dy):
        meta, params, saved = ctx.meta, ctx.params, ctx.saved_blocks
        B, N, D = ctx.shape
        depth = len(params) // PARAMS_PER_LAYER
        d32 = dy.to(torch.float32).contiguous().reshape(B * N, D)
        d16 = None
        grads: List[Optional[Tensor]] = [None] * len(params)
        # the residual-stream gradient travels between the halves in fp32 (it is the sum of 2 x depth branch gradients; a bf16
        # stream was measured 1.9 % faster in round 1 and rejected: it rounds the running sum to 8 bits after every add)
        done = None                                          # layer whose weight gradients were issued, not yet declared final
        for i in reversed(range(depth)):
            p = params[i * PARAMS_PER_LAYER:(i + 1) * PARAMS_PER_LAYER]
            sa, sm = saved[i]
            d32, d16, gm = mlp_half_bwd(d32, d16, sm, meta, *p[6:12], residual=True, want_bf16=True, drop_scale=ctx.drop_scale)
            d32, d16, ga = attn_half_bwd(d32, d16, sa, B, N, meta, *p[0:6], residual=True, want_bf16=i > 0, drop_scale=ctx.drop_scale)
            grads[i * PARAMS_PER_LAYER:(i + 1) * PARAMS_PER_LAYER] = ga + gm
            # the previous layer's grouped weight-gradient launch (side stream: it ran beside this layer's dX chain) is joined
            # and its parameters declared final; then this layer's four gradients go out as one launch
            wgrad_join()
            if done is not None and meta.sink is not None:
                meta.sink.layer_done(done[0], done[1])
            wgrad_flush(meta)
            done = (i, sink_params(p))
            saved[i] = None                                  # free this block's activations early (queued operands are held by the launch)
        wgrad_join()
        if done is not None and meta.sink is not None:
            meta.sink.layer_done(done[0], done[1])
        grads = _mask_sink_grads(meta, grads)
        return (d32.reshape(B, N, D), None, *grads)


class AttnHalfFn(torch.autograd.Function):
    """Stand-alone `Attention.forward` (simple_vit.py:64-76): LN -> QKV -> attention -> out-proj, no residual."""

    @staticmethod
    def forward(ctx, x, meta: BlockMeta, ln_w, ln_b, wqkv, bqkv, wo, bo):
        x2, B, N, D = _as_stream(x)
        pa = float(meta.attn_dropout)
        pd = float(meta.dropout)
        y, saved = attn_half_fwd(x2, B, N, meta, ln_w, ln_b, wqkv, bqkv, wo, bo, residual=False,
                                 drop=(1.0 / (1.0 - pd), 0) if pd > 0.0 else None,
                                 adrop=(1.0 / (1.0 - pa), -2, pa) if pa > 0.0 else None)
        ctx.meta, ctx.params, ctx.saved_half, ctx.shape = meta, (ln_w, ln_b, wqkv, bqkv, wo, bo), saved, (B, N, D)
        ctx.drop_scale = 1.0 / (1.0 - pd) if pd > 0.0 else 1.0
        return y.reshape(B, N, wo.shape[0])

    @staticmethod
    def backward(ctx, dy):
        B, N, D = ctx.shape
        d32 = dy.to(torch.float32).contiguous().reshape(B * N, -1)
        dx32, _, g = attn_half_bwd(d32, None, ctx.saved_half, B, N, ctx.meta, *ctx.params, residual=False, want_bf16=False,
                                   drop_scale=ctx.drop_scale)
        return (dx32.reshape(B, N, D), None, *_mask_sink_grads(ctx.meta, g))


# ----------------------------------------------------------------------------------------------
# memory keys and score masks (learnable_memory_vit.py:64-102, the Adapter)
# ----------------------------------------------------------------------------------------------
class MaskCache:
    """bool mask -> packed bits (kernels.mask_pack), reused while the tensor is alive and unchanged: keyed on (data_ptr, version,
    shape) and the attention's geometry, like WeightCache (the Adapter's `attn_mask` buffer is packed once)."""

    def __init__(self, size: int = 16) -> None:
        self._d = {}
        self.size = size

    def get(self, mask: Tensor, B: int, H: int, Nq: int, Nk: int) -> K.MaskBits:
        key = (mask.data_ptr(), tuple(mask.shape), tuple(mask.stride()), B, H, Nq, Nk)
        ent = self._d.get(key)
        if ent is not None and ent[0]() is mask and ent[1] == mask._version:
            return ent[2]
        bits = K.mask_pack(mask, B, H, Nq, Nk)
        if len(self._d) >= self.size:
            self._d = {k: v for k, v in self._d.items() if v[0]() is not None}
            if len(self._d) >= self.size:
                self._d.clear()
        self._d[key] = (weakref.ref(mask), mask._version, bits)
        return bits


MASKS = MaskCache()


def _mem_kv(m: Optional[Tensor], B: int, D: int, M: int, mask: Optional[K.MaskBits]) -> MemKV:
    if m is None:
        return MemKV(None, 0, True, mask)
    if m.dim() not in (2, 3) or m.shape[-1] != D or m.shape[-2] != M or (m.dim() == 3 and m.shape[0] != B):
        raise NrvError(f"memories must be [M, {D}] or [{B}, M, {D}] with the same M in every layer, got {tuple(m.shape)}")
    if not m.is_cuda:
        raise NrvError("memories must be on the MI355X (HIP) device")
    rows = m.detach().to(torch.float32).contiguous().reshape(-1, D) if M > 0 else None
    return MemKV(rows, M, m.dim() == 2, mask)


class MemStackFn(torch.autograd.Function):
    """The encoder stack (EncoderStackFn) or one stand-alone attention (AttnHalfFn, `attn_only`) with memory keys and / or a
    score mask in every attention (learnable_memory_vit.py:64-102).  Inputs: x, meta, attn_only, packed mask (or None), the
    number of memory tensors (depth, or 0), those tensors ([M, D] shared / [B, M, D] per sample, one per layer), then
    PARAMS_PER_LAYER parameters per layer (6 with attn_only).  No dropout, no gradient sink.

    The backward returns gradients for the memories and issues no weight-gradient GEMM for a parameter that does not require
    one (the Adapter's frozen backbone): the flags come from autograd's needs_input_grad."""

    @staticmethod
    def forward(ctx, x, meta: BlockMeta, attn_only: bool, mask: Optional[K.MaskBits], n_mem: int, *rest):
        if meta.sink is not None:
            raise NotImplementedError("memory keys / score masks are not wired to a gradient sink (data-parallel runtime)")
        if meta.dropout > 0.0 or meta.attn_dropout > 0.0:
            raise NotImplementedError("dropout together with memory keys / score masks is not implemented")
        x2, B, N, D = _as_stream(x)
        _PENDING.clear()
        mems, params = rest[:n_mem], rest[n_mem:]
        per = 6 if attn_only else PARAMS_PER_LAYER
        depth = len(params) // per
        if n_mem and n_mem != depth:
            raise NrvError(f"{n_mem} memory tensors for {depth} layers")
        M = mems[0].shape[-2] if n_mem else 0
        if mask is not None and (mask.Nq != N or mask.Nk != N + M):
            raise NrvError(f"mask packed for [{mask.Nq}, {mask.Nk}], attention is [{N}, {N + M}]")
        train = any(ctx.needs_input_grad)
        saved, cur = [], x2
        for i in range(depth):
            p = params[i * per:(i + 1) * per]
            mk = _mem_kv(mems[i] if n_mem else None, B, D, M, mask)
            cur, sa = attn_half_fwd(cur, B, N, meta, *p[0:6], residual=not attn_only, mem=mk)
            sm = None
            if not attn_only:
                cur, sm = mlp_half_fwd(cur, meta, *p[6:12], residual=True, save=train)
            saved.append((sa, sm) if train else None)
        ctx.meta, ctx.params, ctx.saved_blocks, ctx.shape = meta, params, saved, (B, N, D)
        ctx.attn_only, ctx.n_mem, ctx.mem_shapes = attn_only, n_mem, [tuple(m.shape) for m in mems]
        return cur.reshape(B, N, -1)

    @staticmethod
    def backward(ctx, dy):
        meta, params, saved = ctx.meta, ctx.params, ctx.saved_blocks
        B, N, D = ctx.shape
        attn_only, n_mem = ctx.attn_only, ctx.n_mem
        per = 6 if attn_only else PARAMS_PER_LAYER
        depth = len(params) // per
        need_mem = ctx.needs_input_grad[5:5 + n_mem]
        need_p = ctx.needs_input_grad[5 + n_mem:]
        d32 = dy.to(torch.float32).contiguous().reshape(B * N, -1)
        d16 = None
        grads: List[Optional[Tensor]] = [None] * len(params)
        mgrads: List[Optional[Tensor]] = [None] * n_mem
        for i in reversed(range(depth)):
            p = params[i * per:(i + 1) * per]
            need = need_p[i * per:(i + 1) * per]
            sa, sm = saved[i]
            gm = []
            if not attn_only:
                d32, d16, gm = mlp_half_bwd(d32, d16, sm, meta, *p[6:12], residual=True, want_bf16=True, need=need[6:12])
            mg: list = []
            d32, d16, ga = attn_half_bwd(d32, d16, sa, B, N, meta, *p[0:6], residual=not attn_only, want_bf16=i > 0 and not attn_only,
                                         need=need[0:6], mem_grad=mg)
            wgrad_flush(meta)
            g = ga + gm
            grads[i * per:(i + 1) * per] = [t if f else None for t, f in zip(g, need)]
            if n_mem and need_mem[i] and mg[0] is not None:
                mgrads[i] = mg[0].reshape(ctx.mem_shapes[i])
            saved[i] = None
        wgrad_join()
        return (d32.reshape(B, N, D), None, None, None, None, *mgrads, *grads)


class MlpHalfFn(torch.autograd.Function):
    """Stand-alone `FeedForward.forward` (simple_vit.py:44-45): LN -> Linear -> GELU -> Linear, no residual."""

    @staticmethod
    def forward(ctx, x, meta: BlockMeta, ln_w, ln_b, w1, b1, w2, b2):
        x2, B, N, D = _as_stream(x)
        pd = float(meta.dropout)
        y, saved = mlp_half_fwd(x2, meta, ln_w, ln_b, w1, b1, w2, b2, residual=False, drop=(1.0 / (1.0 - pd), 1) if pd > 0.0 else None)
        ctx.meta, ctx.params, ctx.saved_half, ctx.shape = meta, (ln_w, ln_b, w1, b1, w2, b2), saved, (B, N, D)
        ctx.drop_scale = 1.0 / (1.0 - pd) if pd > 0.0 else 1.0
        return y.reshape(B, N, w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        B, N, D = ctx.shape
        d32 = dy.to(torch.float32).contiguous().reshape(B * N, -1)
        dx32, _, g = mlp_half_bwd(d32, None, ctx.saved_half, ctx.meta, *ctx.params, residual=False, want_bf16=False, drop_scale=ctx.drop_scale)
        return (dx32.reshape(B, N, D), None, *_mask_sink_grads(ctx.meta, g))


class PatchEmbedFn(torch.autograd.Function):
    """Patch unfold + projection + bias + positional table, written straight into the fp32 residual stream.

    SimpleViT (simple_vit.py:126-131,141-143): layout (p1 p2 c), pos = fixed sincos table [n, D], cls_slot = 0.
    VisionTransformer (vit.py:237-242,308-333,341-342, Encoder :174): layout (c p1 p2) with the Conv2d weight
    viewed [D, C*p*p]; cls_slot = 1 leaves row 0 of every sample for `class_token + pos[0]` and adds pos[1:].
    """

    @staticmethod
    def forward(ctx, img, weight, bias, pos, cls_token, patch: int, layout: int, sink):
        require_cuda(img)
        if img.requires_grad:
            raise NrvError("gradient w.r.t. the input image is not part of this hot path")
        Bn, C, H, W = img.shape
        n = (H // patch) * (W // patch)
        D = weight.shape[0]
        patches = K.patch_unfold(img.detach(), patch, layout)
        wb, _ = padded_images(weight, patches.shape[1], False)       # vit_h_14's 588 features; no BASELINE config is padded
        cls_slot = 0 if cls_token is None else 1
        S = n + cls_slot
        out = torch.empty(Bn * S, D, dtype=torch.float32, device=img.device)
        pos2 = pos.detach().reshape(-1, D).to(torch.float32)
        if pos2.shape[0] != S:
            # the GEMM epilogue reads the table through raw pointers (row = token index): a table of another grid would be
            # read out of bounds or add the wrong positions (the reference's broadcast add raises for a learned table)
            raise NrvError(f"positional table has {pos2.shape[0]} rows but the image gives {n} patches"
                           f"{' + class token' if cls_slot else ''} = {S} tokens")
        if C * patch * patch != weight[0].numel():
            raise NrvError(f"patch features {C * patch * patch} != projection in_features {weight[0].numel()}")
        if cls_slot:
            K.gemm_nt(patches, wb, epilogue=EPI_BIAS_RESIDUAL, bias=bias.detach() if bias is not None else None,
                      aux=pos2[1:], aux_row_mod=n, out=out, out_group=n, out_group_stride=S, out_row_offset=1)
            out.view(Bn, S, D)[:, 0] = (cls_token.detach().reshape(D) + pos2[0])      # B*D elements: not the hot path
        else:
            K.gemm_nt(patches, wb, epilogue=EPI_BIAS_RESIDUAL, bias=bias.detach() if bias is not None else None,
                      aux=pos2, aux_row_mod=n, out=out)
        ctx.save_for_backward(patches)
        ctx.cfg = (Bn, n, S, D, cls_slot, weight.shape, bias is not None, pos.shape, pos.requires_grad,
                   cls_token is not None and cls_token.requires_grad, sink, weight, bias)
        return out.reshape(Bn, S, D)

    @staticmethod
    def backward(ctx, dy):
        (patches,) = ctx.saved_tensors
        Bn, n, S, D, cls_slot, wshape, has_bias, pos_shape, pos_grad, cls_grad, sink, weight, bias = ctx.cfg
        d32 = dy.to(torch.float32).contiguous().reshape(Bn * S, D)
        d16 = K.cast_bf16(d32)
        tw, bw = (sink.target(weight) if sink is not None else (None, 0.0))
        if tw is not None:
            tw = tw.reshape(D, -1)
        F = weight[0].numel()
        padded = patches.shape[1] != F               # zero feature columns (patch size 14): gradient of the real columns only
        tgt = None if padded else tw
        if cls_slot:
            dw = K.gemm_tn(d16, patches, out=tgt, beta=0.0 if padded else bw, a_group=n, a_group_stride=S, a_row_offset=1, T=Bn * n)
        else:
            dw = K.gemm_tn(d16, patches, out=tgt, beta=0.0 if padded else bw)
        if padded:
            dw = dw[:, :F]
            if tw is not None:
                tw.copy_(dw) if bw == 0.0 else tw.add_(dw)
        # positional-table / class-token / bias gradients are reductions of dy over the batch
        dpos = dcls = db = None
        if pos_grad or cls_grad or cls_slot:
            dsum = K.colsum(d16.reshape(Bn, S * D)).reshape(S, D)
            dpos = dsum.reshape(pos_shape) if pos_grad else None
            dcls = dsum[0].reshape(1, 1, D) if cls_grad else None
            if has_bias:
                db = dsum[cls_slot:].sum(0)          # [S, D] -> [D]: outside the hot path
        elif has_bias:
            db = K.colsum(d16)
        if has_bias and sink is not None:
            tb, bb = sink.target(bias)
            tb.copy_(db) if bb == 0.0 else tb.add_(db)
        if sink is not None:
            sink.layer_done(-1, [weight] + ([bias] if has_bias else []))
            return (None, None, None, dpos, dcls, None, None, None)
        return (None, dw.reshape(wshape), db, dpos, dcls, None, None, None)


class LinearFn(torch.autograd.Function):
    """y = x W^T + b through the MFMA GEMM (bf16 operands, fp32 result) for projections next to the encoder
    (MAE `enc_to_dec` / `to_pixels`, mae.py:34-49).  x [..., K] fp32, K % 8 == 0, out_features % 8 == 0."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        if not x.is_cuda:
            raise NrvError("noise_robust_vit_amd runs on the MI355X (HIP) device only; there is no CPU fallback")
        shp = x.shape
        x2 = x.detach().to(torch.float32).contiguous().reshape(-1, shp[-1])
        xb = K.cast_bf16(x2)
        y = linear(xb, weight, bias, torch.float32)
        ctx.save_for_backward(xb)
        ctx.meta = (weight, bias is not None, shp)
        return y.reshape(*shp[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        (xb,) = ctx.saved_tensors
        weight, has_bias, shp = ctx.meta
        d16 = K.cast_bf16(dy.to(torch.float32).contiguous().reshape(-1, weight.shape[0]))
        _, wt = WEIGHTS.get(weight, True)
        if has_bias:
            dw, db = K.gemm_tn(d16, xb, want_dbias=True)
        else:
            dw, db = K.gemm_tn(d16, xb), None
        dx = K.gemm_nt(d16, wt, out_dtype=torch.float32)
        return dx.reshape(shp), dw, db


def _flat_token_index(index: Tensor, n: int) -> Tensor:
    B = index.shape[0]
    return (index + torch.arange(B, device=index.device)[:, None] * n).reshape(-1).contiguous()


class GatherTokensFn(torch.autograd.Function):
    """tokens[b, index[b, :]] (MAE keeps a random 25 % of the tokens, mae.py:75-76; reads the decoder's output at the masked
    positions, mae.py:112); backward scatters rows back.  Bounds-checked row kernels, no library sort in either direction."""

    @staticmethod
    def forward(ctx, tokens, index):
        B, n, D = tokens.shape
        flat = _flat_token_index(index, n)
        out = K.gather_rows(tokens.detach().to(torch.float32).contiguous().reshape(B * n, D), flat)
        ctx.save_for_backward(flat)
        ctx.shape = (B, n, D, index.shape[1])
        return out.reshape(B, index.shape[1], D)

    @staticmethod
    def backward(ctx, dy):
        (flat,) = ctx.saved_tensors
        B, n, D, k = ctx.shape
        d = K.scatter_rows(dy.to(torch.float32).contiguous().reshape(B * k, D), flat, B * n)
        return d.reshape(B, n, D), None


class ScatterTokensFn(torch.autograd.Function):
    """out[b, index[b, j]] = rows[b, j], zeros elsewhere (MAE re-assembles the full-length decoder sequence from the kept tokens,
    mae.py:103-107; indices unique per sample); backward gathers.  The counterpart of GatherTokensFn: torch's index_put / Embedding
    backward would bring library sort kernels into the step (and into its HIP graph)."""

    @staticmethod
    def forward(ctx, rows, index, n: int):
        B, k, D = rows.shape
        flat = _flat_token_index(index, n)
        out = K.scatter_rows(rows.detach().to(torch.float32).contiguous().reshape(B * k, D), flat, B * n)
        ctx.save_for_backward(flat)
        ctx.shape = (B, n, D, k)
        return out.reshape(B, n, D)

    @staticmethod
    def backward(ctx, dy):
        (flat,) = ctx.saved_tensors
        B, n, D, k = ctx.shape
        d = K.gather_rows(dy.to(torch.float32).contiguous().reshape(B * n, D), flat)
        return d.reshape(B, k, D), None, None


def flat_layer_params(layers: Sequence[Sequence[Optional[Tensor]]]) -> List[Optional[Tensor]]:
    out: List[Optional[Tensor]] = []
    for lp in layers:
        if len(lp) != PARAMS_PER_LAYER:
            raise ValueError("each layer needs PARAMS_PER_LAYER entries")
        out.extend(lp)
    return out
