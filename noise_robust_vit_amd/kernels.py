"""Tensor-level wrappers over the C ABI (include/nrv.h).  No autograd, no fallbacks.

PyTorch is used for device memory (caching allocator) and the current HIP stream only; every
arithmetic result comes from a kernel in libnrv_hip.so.

The C side sees addresses and integers only, so every wrapper checks what it hands over (tests/launch_audit.py holds them to
it): each tensor lives on a HIP device (`tensor.is_cuda`), has the dtype its kernel reads, and holds exactly the elements the
call's dimensions address (at least, where a docstring says so).  Tensors are contiguous, compared by element count and not
by shape; the exceptions are the operands documented as row-major views (GEMM operands, q / k / v views, `u` of GEGLU, ...),
whose row stride is passed on with unit stride in the last dimension.  An input that callers pass strided is copied where the
docstring or the code says `.contiguous()`; an output or a saved statistic never is.  The checks compare attributes and never
read device memory.  16-byte alignment is the C side's rule.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_Q8, EPI_BIAS_RESIDUAL, EPI_DGELU, EPI_DGELU_Q8, EPI_NONE, NRV_BF16, NRV_F32, NRV_U8,
                   PATCH_CP1P2, PATCH_P1P2C, NrvError, check)

Tensor = torch.Tensor


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(t: Tensor, name: str) -> None:
    if not t.is_cuda:
        raise NrvError(f"{name} must be on the MI355X (HIP) device; this path has no CPU implementation")


def _dt(t: Tensor, name: str) -> int:
    if t.dtype == torch.float32:
        return NRV_F32
    if t.dtype == torch.bfloat16:
        return NRV_BF16
    raise NrvError(f"{name}: dtype {t.dtype} not supported (fp32 or bf16)")


def _bf16(t: Tensor, name: str) -> None:
    _dev(t, name)
    if t.dtype != torch.bfloat16:
        raise NrvError(f"{name} must be bf16, got {t.dtype}")


def _f32(t: Tensor, name: str) -> None:
    _dev(t, name)
    if t.dtype != torch.float32:
        raise NrvError(f"{name} must be fp32, got {t.dtype}")


def _rows2d(t: Tensor, name: str) -> Tuple[int, int, int]:
    """(rows, cols, ld) of a 2-D view with unit stride in the last dim."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise NrvError(f"{name} must be 2-D with contiguous rows, got shape {tuple(t.shape)} stride {t.stride()}")
    return t.shape[0], t.shape[1], t.stride(0)


def _dense(t: Tensor, name: str, dtype: Optional[torch.dtype], n: int, by: str = "the call's dimensions") -> None:
    """`t` is on the device, of `dtype` (None: fp32 or bf16), contiguous, and holds exactly `n` elements; `by` names what `n`
    was taken from, for the message.  Element counts, not shapes: the kernels address flat buffers and callers pass reshaped
    views of them.  Attribute comparisons only."""
    _dev(t, name)
    if dtype is None:
        _dt(t, name)
    elif t.dtype != dtype:
        raise NrvError(f"{name} must be {dtype}, got {t.dtype}")
    if t.numel() != n or not t.is_contiguous():
        raise NrvError(f"{name} must be contiguous with {n} elements (by {by}), got shape {tuple(t.shape)} stride {t.stride()}")


def _view2d(t: Tensor, name: str, rows: int, width: int) -> int:
    """Row stride of a bf16 [rows, >= width] view with unit column stride (a column block of a wider buffer works)."""
    _bf16(t, name)
    if t.dim() != 2 or t.stride(1) != 1 or t.shape[0] != rows or t.shape[1] < width or (rows > 1 and t.stride(0) < t.shape[1]):
        raise NrvError(f"{name} must be a row-major bf16 [{rows}, >= {width}] view, got shape {tuple(t.shape)} stride {t.stride()}")
    return t.stride(0)


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _workspace(nbytes: int, device) -> Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def set_reserved_cus(n: int) -> int:
    """CUs the GEMM launches leave free for a collective's kernels (include/nrv.h); returns the previous value."""
    prev = _lib.load().nrv_set_reserved_cus(int(n))
    if prev < 0:
        check(prev, "nrv_set_reserved_cus")
    return prev


def gemm_nt_plan(M: int, N: int, K: int, epilogue: int = EPI_NONE, remap: bool = False) -> dict:
    """What `gemm_nt` would launch for this shape under the current CU reservation (include/nrv.h nrv_gemm_nt_plan): tile rows
    and columns, phased or plain kernel, tiles and workgroups.  Read-only; needs no GPU."""
    pl = _lib.NtPlan()
    check(_lib.load().nrv_gemm_nt_plan(int(M), int(N), int(K), int(epilogue), int(bool(remap)), ctypes.addressof(pl)),
          "nrv_gemm_nt_plan")
    return {"tile_m": pl.tile_m, "tile_n": pl.tile_n, "phased": bool(pl.phased), "tiles": pl.tiles, "grid": pl.grid}


def gemm_tn_plan(M: int, N: int, T: int, a_group: bool = False, beta: float = 0.0, dbias: bool = False) -> dict:
    """What `gemm_tn` would launch (include/nrv.h nrv_gemm_tn_plan): splits, K-tiles per split, kernel, direct or slabs."""
    pl = _lib.TnPlan()
    check(_lib.load().nrv_gemm_tn_plan(int(M), int(N), int(T), int(bool(a_group)), float(beta), int(bool(dbias)),
                                       ctypes.addressof(pl)), "nrv_gemm_tn_plan")
    return {"tiles": pl.tiles, "splits": pl.splits, "kt_q": pl.kt_q, "kt_r": pl.kt_r, "phased": bool(pl.phased),
            "direct": bool(pl.direct), "reduce": bool(pl.reduce)}


# ----------------------------------------------------------------------------------------------
# optional per-launch timing (bench.py's roofline leg): HIP events on the stream the kernel runs on
# ----------------------------------------------------------------------------------------------
_PROF = None


class LaunchProfile:
    """Collects (kernel class, algorithmic FLOPs, algorithmic bytes, start event, end event) per C-ABI call."""

    def __init__(self) -> None:
        self.records = []

    def __enter__(self):
        global _PROF
        _PROF = self
        return self

    def __exit__(self, *exc):
        global _PROF
        _PROF = None

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, flops, nbytes, s, e in self.records:
            d = out.setdefault(name, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["ms"] += s.elapsed_time(e)
            d["flops"] += flops
            d["bytes"] += nbytes
        return out


def _run(name: str, flops: float, nbytes: float, call, what: str) -> None:
    if _PROF is None:
        check(call(), what)
        return
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    code = call()
    e.record()
    check(code, what)
    _PROF.records.append((name, flops, nbytes, s, e))


# ----------------------------------------------------------------------------------------------
def layernorm_fwd(x: Tensor, gamma: Tensor, beta: Tensor, eps: float):
    """x [rows, dim] fp32|bf16 -> (y bf16, mean fp32, rstd fp32).  nn.LayerNorm (simple_vit.py:38,54; vit.py:104,115)."""
    _dev(x, "x")
    x = x.contiguous()
    rows, dim = x.shape
    _dense(gamma, "gamma", torch.float32, dim, "x"); _dense(beta, "beta", torch.float32, dim, "x")
    y = torch.empty(rows, dim, dtype=torch.bfloat16, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    _run("layernorm_fwd", 0.0, rows * dim * (x.element_size() + 2),
         lambda: lib.nrv_layernorm_fwd(x.data_ptr(), _dt(x, "x"), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                       mean.data_ptr(), rstd.data_ptr(), rows, dim, float(eps), _stream()),
         "nrv_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy: Tensor, x: Tensor, gamma: Tensor, mean: Tensor, rstd: Tensor, dres: Optional[Tensor] = None,
                  want_f32: bool = True, want_bf16: bool = False,
                  dgamma: Optional[Tensor] = None, dbeta: Optional[Tensor] = None, accumulate: bool = False):
    """Returns (dx_f32|None, dx_bf16|None, dgamma, dbeta); dx = dres + LN'(dy)."""
    _dev(x, "x")
    x = x.contiguous()                      # as layernorm_fwd took it
    rows, dim = x.shape
    _dense(dy, "dy", torch.bfloat16, rows * dim, "x"); _dense(gamma, "gamma", torch.float32, dim, "x")
    _dense(mean, "mean", torch.float32, rows, "x"); _dense(rstd, "rstd", torch.float32, rows, "x")
    if dres is not None:
        _dense(dres, "dres", None, rows * dim, "x")
    lib = _lib.load()
    dx32 = torch.empty(rows, dim, dtype=torch.float32, device=x.device) if want_f32 else None
    dx16 = torch.empty(rows, dim, dtype=torch.bfloat16, device=x.device) if want_bf16 else None
    if dgamma is None:
        dgamma = torch.empty(dim, dtype=torch.float32, device=x.device); accumulate = False
    else:
        _dense(dgamma, "dgamma", torch.float32, dim, "x")
    if dbeta is None:
        dbeta = torch.empty(dim, dtype=torch.float32, device=x.device)
    else:
        _dense(dbeta, "dbeta", torch.float32, dim, "x")
    wsb = lib.nrv_layernorm_bwd_workspace(rows, dim)
    ws = _workspace(wsb, x.device)
    nb = rows * dim * (2 + x.element_size() + (dres.element_size() if dres is not None else 0)
                       + (4 if want_f32 else 0) + (2 if want_bf16 else 0))
    _run("layernorm_bwd", 0.0, nb,
         lambda: lib.nrv_layernorm_bwd(dy.data_ptr(), x.data_ptr(), _dt(x, "x"), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                       _ptr(dres), _dt(dres, "dres") if dres is not None else 0,
                                       _ptr(dx32), _ptr(dx16), dgamma.data_ptr(), dbeta.data_ptr(), int(bool(accumulate)),
                                       ws.data_ptr(), ws.numel(), rows, dim, _stream()),
         "nrv_layernorm_bwd")
    return dx32, dx16, dgamma, dbeta


def gemm_nt_side_plan(M: int, N: int, K: int, epilogue: int = EPI_NONE, remap: bool = False, job_bytes: int = 0) -> dict:
    """How `gemm_nt(..., side=...)` would treat a reduction of `job_bytes` slab bytes (include/nrv.h nrv_gemm_nt_side_plan): the
    late-starting workgroups that take shares, the slab bytes per share, and whether the launch carries the job.  Needs no GPU."""
    pl = _lib.NtSidePlan()
    check(_lib.load().nrv_gemm_nt_side_plan(int(M), int(N), int(K), int(epilogue), int(bool(remap)), int(job_bytes),
                                            ctypes.addressof(pl)), "nrv_gemm_nt_side_plan")
    return {"late": pl.late, "share_bytes": pl.share_bytes, "admitted": bool(pl.admitted)}


class PendingReduce:
    """The reduction `gemm_tn(..., defer=True)` left behind (include/nrv.h nrv_reduce_job).  Holds the workspace, C and dbias until
    `gemm_nt(..., side=...)` or `flush_reduce` has put it on a stream; a token that is dropped instead never runs."""

    def __init__(self, job, keep) -> None:
        self.job, self.keep, self.fused = job, keep, None

    @property
    def pending(self) -> bool:
        return self.job is not None and bool(self.job.pending)

    def _consume(self):
        job, self.job, self.keep = self.job, None, None
        return job


def flush_reduce(pending: Optional[PendingReduce]) -> None:
    """Run the stand-alone reduction of a deferred weight gradient (nothing when it already ran)."""
    if pending is None or not pending.pending:
        return
    keep = pending.keep
    job = pending._consume()
    check(_lib.load().nrv_splitk_reduce(ctypes.addressof(job), _stream()), "nrv_splitk_reduce")      # no LaunchProfile class of its own
    del keep


def gemm_nt(A: Tensor, B: Tensor, *, out_dtype: torch.dtype = torch.bfloat16, epilogue: int = EPI_NONE,
            bias: Optional[Tensor] = None, aux: Optional[Tensor] = None, aux_row_mod: int = 0,
            aux_out: Optional[Tensor] = None, out: Optional[Tensor] = None,
            out_group: int = 0, out_group_stride: int = 0, out_row_offset: int = 0,
            side: Optional[PendingReduce] = None) -> Tensor:
    """C[M,N] = A[M,K] . B[N,K]^T with a fused epilogue (include/nrv.h nrv_gemm_nt_bf16).  `side`: a deferred weight-gradient
    reduction that this launch completes (nrv_gemm_nt_bf16_side): inside the GEMM launch when the library admits it, as a launch
    of its own in front of the GEMM otherwise; `side.fused` says which."""
    _bf16(A, "A"); _bf16(B, "B")
    M, K, lda = _rows2d(A, "A")
    N, K2, ldb = _rows2d(B, "B")
    if K != K2:
        raise NrvError(f"gemm_nt: K mismatch {K} vs {K2}")
    if out is None:
        if out_group:
            raise NrvError("gemm_nt: an output row remap needs a caller-provided `out`")
        out = torch.empty(M, N, dtype=out_dtype, device=A.device)
    _dev(out, "out")
    _, _, ldc = _rows2d(out, "out")
    ld_aux = 0
    aux_code = 0
    if aux is not None:
        _dev(aux, "aux")
        if (epilogue == EPI_DGELU_Q8) != (aux.dtype == torch.uint8):
            raise NrvError("gemm_nt: the 8-bit gelu' stream (uint8) goes with EPI_DGELU_Q8 and with nothing else")
        aux_code = NRV_U8 if aux.dtype == torch.uint8 else _dt(aux, "aux")
        arows, acols, ld_aux = _rows2d(aux, "aux")
        # the epilogue reads aux through raw pointers: row m % aux_row_mod, or the (remapped) output row
        need = aux_row_mod if aux_row_mod else (M if not out_group else (M - 1) // out_group * out_group_stride + (M - 1) % out_group + out_row_offset + 1)
        if epilogue == EPI_DGELU_Q8:
            need = (need + 1) // 2 * 2          # the byte stream is stored in row pairs (include/nrv.h)
        if arows < need or acols < N:
            raise NrvError(f"gemm_nt: aux is [{arows}, {acols}] but the epilogue reads rows < {need}, columns < {N}")
    if out_group:
        need = (M - 1) // out_group * out_group_stride + (M - 1) % out_group + out_row_offset + 1
        if out.shape[0] < need:
            raise NrvError(f"gemm_nt: out has {out.shape[0]} rows, the row remap writes up to row {need - 1}")
    elif out.shape[0] < M or out.shape[1] < N:
        raise NrvError(f"gemm_nt: out is {tuple(out.shape)}, result is [{M}, {N}]")
    ld_ao = 0
    if aux_out is not None:
        if epilogue == EPI_BIAS_GELU_Q8:
            _dev(aux_out, "aux_out")
            if aux_out.dtype != torch.uint8 or aux_out.shape[0] < (M + 1) // 2 * 2 or N % 64:
                raise NrvError("gemm_nt: EPI_BIAS_GELU_Q8 writes the gelu' stream as uint8 in row pairs: M rounded up to even rows, N % 64 == 0")
        else:
            _bf16(aux_out, "aux_out")
        orows, ocols, ld_ao = _rows2d(aux_out, "aux_out")
        if orows < M or ocols < N:
            raise NrvError(f"gemm_nt: aux_out is [{orows}, {ocols}], the epilogue writes [{M}, {N}]")
    if bias is not None:
        _dense(bias, "bias", torch.float32, N, "B")
    lib = _lib.load()
    nb = 2 * (M * K + N * K) + M * N * out.element_size()
    if aux is not None and not aux_row_mod:
        nb += M * N * aux.element_size()
    if aux_out is not None:
        nb += M * N * aux_out.element_size()
    if side is not None and side.pending:
        keep = side.keep
        job = side._consume()
        fused = ctypes.c_int(0)
        _run("gemm_nt", 2.0 * M * N * K, nb,
             lambda: lib.nrv_gemm_nt_bf16_side(A.data_ptr(), lda, B.data_ptr(), ldb, out.data_ptr(), _dt(out, "out"), ldc,
                                               M, N, K, int(epilogue), _ptr(bias),
                                               _ptr(aux), aux_code, ld_aux, int(aux_row_mod),
                                               _ptr(aux_out), ld_ao, int(out_group), int(out_group_stride), int(out_row_offset),
                                               ctypes.addressof(job), ctypes.addressof(fused), _stream()),
             "nrv_gemm_nt_bf16_side")
        side.fused = bool(fused.value)
        del keep
        return out
    _run("gemm_nt", 2.0 * M * N * K, nb,
         lambda: lib.nrv_gemm_nt_bf16(A.data_ptr(), lda, B.data_ptr(), ldb, out.data_ptr(), _dt(out, "out"), ldc,
                                      M, N, K, int(epilogue), _ptr(bias),
                                      _ptr(aux), aux_code, ld_aux, int(aux_row_mod),
                                      _ptr(aux_out), ld_ao, int(out_group), int(out_group_stride), int(out_row_offset),
                                      _stream()),
         "nrv_gemm_nt_bf16")
    return out


def gemm_tn(A: Tensor, B: Tensor, *, out: Optional[Tensor] = None, beta: float = 0.0,
            a_group: int = 0, a_group_stride: int = 0, a_row_offset: int = 0, T: Optional[int] = None,
            dbias: Optional[Tensor] = None, dbias_beta: float = 0.0, want_dbias: bool = False, defer: bool = False):
    """C[M,N] fp32 = beta*C + sum_t A[t,M] B[t,N]  (weight gradient).  `T` limits the token rows used (default B.shape[0]).

    With `want_dbias` (or a `dbias` output) the bias gradient sum_t A[t,:] is produced by the same kernel and the
    call returns (C, dbias).  With `defer` the slab reduction is not launched (nrv_gemm_tn_bf16_deferred): the call returns its
    usual result plus a `PendingReduce`, and C / dbias are complete only after `gemm_nt(..., side=...)` or `flush_reduce` took it."""
    _bf16(A, "A"); _bf16(B, "B")
    Ta, M, lda = _rows2d(A, "A")
    Tb, N, ldb = _rows2d(B, "B")
    T = Tb if T is None else T
    if a_group == 0 and Ta != Tb:
        raise NrvError(f"gemm_tn: token count mismatch, A has {Ta} rows and B {Tb}")
    if T > Tb:
        raise NrvError(f"gemm_tn: T = {T} token rows, B has {Tb}")
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=A.device)
        beta = 0.0
    _f32(out, "out")
    orows, ocols, ldc = _rows2d(out, "out")
    if orows < M or ocols < N:
        raise NrvError(f"gemm_tn: out is [{orows}, {ocols}], the gradient is [{M}, {N}]")
    if want_dbias and dbias is None:
        dbias = torch.empty(M, dtype=torch.float32, device=A.device)
        dbias_beta = 0.0
    if dbias is not None:
        _dense(dbias, "dbias", torch.float32, M, "A")
    lib = _lib.load()
    ws = _workspace(lib.nrv_gemm_tn_workspace(M, N, T), A.device)
    if defer:
        job = _lib.ReduceJob()
        _run("gemm_tn", 2.0 * M * N * T, 2 * T * (M + N) + 4 * M * N,
             lambda: lib.nrv_gemm_tn_bf16_deferred(A.data_ptr(), lda, B.data_ptr(), ldb, out.data_ptr(), ldc, M, N, T, float(beta),
                                                   int(a_group), int(a_group_stride), int(a_row_offset),
                                                   _ptr(dbias), float(dbias_beta), ws.data_ptr(), ws.numel(),
                                                   ctypes.addressof(job), _stream()),
             "nrv_gemm_tn_bf16_deferred")
        pending = PendingReduce(job, (ws, out, dbias))
        return (out, dbias, pending) if dbias is not None else (out, pending)
    _run("gemm_tn", 2.0 * M * N * T, 2 * T * (M + N) + 4 * M * N,
         lambda: lib.nrv_gemm_tn_bf16(A.data_ptr(), lda, B.data_ptr(), ldb, out.data_ptr(), ldc, M, N, T, float(beta),
                                      int(a_group), int(a_group_stride), int(a_row_offset),
                                      _ptr(dbias), float(dbias_beta), ws.data_ptr(), ws.numel(), _stream()),
         "nrv_gemm_tn_bf16")
    if dbias is not None:
        return out, dbias
    return out


def gemm_tn_grouped(problems) -> list:
    """ALL weight gradients of a layer in one stream-K launch (include/nrv.h nrv_gemm_tn_grouped_bf16).  `problems`: up to 4
    dicts {A: dy bf16 [T, M], B: x bf16 [T, N], out: fp32 [M, N] | None, beta, dbias: fp32 [M] | None | True (allocate),
    dbias_beta}; all with the same T.  Returns [(out, dbias | None)].  Groups the kernel does not take (tiny T) run as
    separate `gemm_tn` calls -- the same arithmetic per gradient, another summation order."""
    if not problems:
        return []
    lib = _lib.load()
    T = problems[0]["A"].shape[0]
    arr = (_lib.TnProblem * len(problems))()
    outs = []
    for i, q in enumerate(problems):
        A, B = q["A"], q["B"]
        _bf16(A, "A"); _bf16(B, "B")
        Ta, M, lda = _rows2d(A, "A")
        Tb, N, ldb = _rows2d(B, "B")
        if Ta != T or Tb != T:
            raise NrvError(f"gemm_tn_grouped: problem {i} has {Ta} / {Tb} token rows, the group has {T}")
        out, beta = q.get("out"), float(q.get("beta", 0.0))
        if out is None:
            out, beta = torch.empty(M, N, dtype=torch.float32, device=A.device), 0.0
        _f32(out, "out")
        if out.shape[0] < M or out.shape[1] < N:
            raise NrvError(f"gemm_tn_grouped: out of problem {i} is {tuple(out.shape)}, the gradient is [{M}, {N}]")
        _, _, ldc = _rows2d(out, "out")
        dbias, dbb = q.get("dbias"), float(q.get("dbias_beta", 0.0))
        if dbias is True:
            dbias, dbb = torch.empty(M, dtype=torch.float32, device=A.device), 0.0
        if dbias is not None:
            _f32(dbias, "dbias")
            if dbias.numel() < M:
                raise NrvError("gemm_tn_grouped: dbias is shorter than the gradient's rows")
        arr[i] = _lib.TnProblem(A.data_ptr(), lda, B.data_ptr(), ldb, out.data_ptr(), ldc, M, N, beta, _ptr(dbias), dbb)
        outs.append((out, dbias))
    nbytes = int(lib.nrv_gemm_tn_grouped_workspace(ctypes.addressof(arr), len(problems), T)) if len(problems) <= 4 else 0
    if nbytes == 0:                                   # not taken by the grouped kernel: one split-K launch per gradient
        for i, (q, (out, dbias)) in enumerate(zip(problems, outs)):
            given_db = q.get("dbias") is not None and q.get("dbias") is not True
            gemm_tn(q["A"], q["B"], out=out, beta=float(arr[i].beta), dbias=dbias,
                    dbias_beta=float(q.get("dbias_beta", 0.0)) if given_db else 0.0)
        return outs
    ws = _workspace(nbytes, problems[0]["A"].device)
    flops = sum(2.0 * T * q["A"].shape[1] * q["B"].shape[1] for q in problems)
    nb = sum(2 * T * (q["A"].shape[1] + q["B"].shape[1]) + 4 * q["A"].shape[1] * q["B"].shape[1] for q in problems)
    _run("gemm_tn", flops, nb,
         lambda: lib.nrv_gemm_tn_grouped_bf16(ctypes.addressof(arr), len(problems), T, ws.data_ptr(), ws.numel(), _stream()),
         "nrv_gemm_tn_grouped_bf16")
    return outs


def colsum(X: Tensor, *, out: Optional[Tensor] = None, beta: float = 0.0) -> Tensor:
    """out[n] = beta*out[n] + sum_t X[t,n]  (bias gradient)."""
    _bf16(X, "X")
    T, N, ld = _rows2d(X, "X")
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=X.device)
        beta = 0.0
    else:
        _dense(out, "out", torch.float32, N, "X")
    lib = _lib.load()
    ws = _workspace(lib.nrv_colsum_workspace(T, N), X.device)
    _run("colsum", 0.0, 2 * T * N,
         lambda: lib.nrv_colsum_bf16(X.data_ptr(), ld, out.data_ptr(), T, N, float(beta), ws.data_ptr(), ws.numel(), _stream()),
         "nrv_colsum_bf16")
    return out


ATTN_FUSED_DH = (32, 64, 80, 96, 128)    # nrv_attn_fwd's head dims (row-major qkv); nrv_attn_drop_fwd takes the same


def attn_fwd(qkv: Tensor, B: int, N: int, H: int, dh: int, scale: float, layout: int = 0):
    """qkv bf16 [B*N, 3*H*dh] -> (out bf16 [B*N, H*dh], lse fp32 [B,H,N]).  simple_vit.py:68-75.
    `layout` (include/nrv.h NRV_ATTN_*_BLOCKED): qkv given as [3*H, B*N, dh] / out returned as [H, B*N, dh]."""
    _bf16(qkv, "qkv")
    if not qkv.is_contiguous() or qkv.numel() != B * N * 3 * H * dh:
        raise NrvError("attn_fwd: qkv must be contiguous [B*N, 3*H*dh] (or [3*H, B*N, dh] with the blocked layout)")
    out = (torch.empty(H, B * N, dh, dtype=torch.bfloat16, device=qkv.device) if layout & _lib.ATTN_OUT_BLOCKED
           else torch.empty(B * N, H * dh, dtype=torch.bfloat16, device=qkv.device))
    lse = torch.empty(B, H, N, dtype=torch.float32, device=qkv.device)
    lib = _lib.load()
    _run("attn_fwd", 4.0 * B * H * N * N * dh, 2 * B * N * H * dh * 4,
         lambda: lib.nrv_attn_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, N, H, dh, float(scale), int(layout), _stream()),
         "nrv_attn_fwd")
    return out, lse


def _attn_bwd_args(qkv: Tensor, out: Tensor, dout: Tensor, lse: Tensor, B: int, N: int, H: int, dh: int) -> None:
    """What every attention backward over a packed qkv is handed: qkv [B*N, 3*H*dh], out and dout [B*N, H*dh], lse [B, H, N]."""
    _dense(qkv, "qkv", torch.bfloat16, B * N * 3 * H * dh)
    _dense(out, "out", torch.bfloat16, B * N * H * dh); _dense(dout, "dout", torch.bfloat16, B * N * H * dh)
    _dense(lse, "lse", torch.float32, B * H * N)


def attn_bwd(qkv: Tensor, out: Tensor, dout: Tensor, lse: Tensor, B: int, N: int, H: int, dh: int, scale: float,
             layout: int = 0) -> Tensor:
    _attn_bwd_args(qkv, out, dout, lse, B, N, H, dh)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty(B * H * N, dtype=torch.float32, device=qkv.device)
    lib = _lib.load()
    _run("attn_bwd", 10.0 * B * H * N * N * dh, 2 * B * N * H * dh * 8,
         lambda: lib.nrv_attn_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                  delta.data_ptr(), B, N, H, dh, float(scale), int(layout), _stream()),
         "nrv_attn_bwd")
    return dqkv


def attn_drop_peff(p: float) -> float:
    """The probability the fused attention-weight dropout actually uses: T / 2^16 for T = nrv_attn_drop_threshold(p)."""
    T = _lib.load().nrv_attn_drop_threshold(float(p))
    check(min(T, 0), "nrv_attn_drop_threshold")
    return T / 65536.0


def _seed64(seed: Tensor, what: str) -> None:
    _dev(seed, what)
    if seed.dtype != torch.int64 or seed.numel() != 1:
        raise NrvError(f"{what}: expected an int64 device tensor of one element, got {seed.dtype} {tuple(seed.shape)}")


def attn_drop_fwd(qkv: Tensor, seed: Tensor, p: float, B: int, N: int, H: int, dh: int, scale: float):
    """attn_fwd with dropout on the attention weights inside the kernel (include/nrv.h, "Attention-weight dropout"): `seed` is an
    int64 [1] device tensor read when the kernel runs.  -> (out bf16 [B*N, H*dh], lse fp32 [B,H,N] of the undropped rows)."""
    _bf16(qkv, "qkv"); _seed64(seed, "seed")
    if not qkv.is_contiguous() or qkv.numel() != B * N * 3 * H * dh:
        raise NrvError("attn_drop_fwd: qkv must be contiguous [B*N, 3*H*dh]")
    out = torch.empty(B * N, H * dh, dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty(B, H, N, dtype=torch.float32, device=qkv.device)
    lib = _lib.load()
    _run("attn_drop_fwd", 4.0 * B * H * N * N * dh, 2 * B * N * H * dh * 4,
         lambda: lib.nrv_attn_drop_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), seed.data_ptr(), float(p), B, N, H, dh,
                                       float(scale), _stream()),
         "nrv_attn_drop_fwd")
    return out, lse


def attn_drop_bwd(qkv: Tensor, out: Tensor, dout: Tensor, lse: Tensor, seed: Tensor, p: float, B: int, N: int, H: int, dh: int,
                  scale: float) -> Tensor:
    _attn_bwd_args(qkv, out, dout, lse, B, N, H, dh); _seed64(seed, "seed")
    dqkv = torch.empty_like(qkv)
    delta = torch.empty(B * H * N, dtype=torch.float32, device=qkv.device)
    lib = _lib.load()
    _run("attn_drop_bwd", 10.0 * B * H * N * N * dh, 2 * B * N * H * dh * 8,
         lambda: lib.nrv_attn_drop_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                       delta.data_ptr(), seed.data_ptr(), float(p), B, N, H, dh, float(scale), _stream()),
         "nrv_attn_drop_bwd")
    return dqkv


def attn_drop_mask(seed: Tensor, p: float, B: int, H: int, N: int) -> Tensor:
    """uint8 [B, H, N, N] keep decisions of attn_drop_fwd / _bwd for this seed and p (tests; a reference for the composed path)."""
    _seed64(seed, "seed")
    keep = torch.empty(B, H, N, N, dtype=torch.uint8, device=seed.device)
    check(_lib.load().nrv_attn_drop_mask(seed.data_ptr(), float(p), keep.data_ptr(), B, H, N, _stream()), "nrv_attn_drop_mask")
    return keep


def attn_probs(qkv: Tensor, lse: Tensor, B: int, N: int, H: int, dh: int, scale: float, layout: int = 0) -> Tensor:
    """fp32 [B, H, N, N] softmax probabilities recomputed from q, k and the saved log-sum-exp (introspection only)."""
    _dense(qkv, "qkv", torch.bfloat16, B * N * 3 * H * dh); _dense(lse, "lse", torch.float32, B * H * N)
    probs = torch.empty(B, H, N, N, dtype=torch.float32, device=qkv.device)
    check(_lib.load().nrv_attn_probs(qkv.data_ptr(), lse.data_ptr(), probs.data_ptr(), B, N, H, dh, float(scale), int(layout), _stream()),
          "nrv_attn_probs")
    return probs


@dataclass
class MaskBits:
    """A boolean score mask packed for nrv_attn_mem_*: int32 words [*, ceil(Nk / 32)] per query row, with the batch / head
    strides in words (0 = broadcast)."""
    bits: Tensor
    Nq: int
    Nk: int
    bstride: int
    hstride: int


def mask_pack(mask: Tensor, B: int, H: int, Nq: int, Nk: int) -> MaskBits:
    """bool mask broadcastable to [B, H, Nq, Nk] (True = may attend) -> MaskBits, packed on the device (no host sync)."""
    _dev(mask, "mask")
    if mask.dtype != torch.bool:
        raise NrvError(f"attention mask must be bool, got {mask.dtype}")
    if mask.dim() > 4:
        raise NrvError(f"attention mask of {mask.dim()} dims does not broadcast against [B, H, Nq, Nk]")
    m = mask.reshape((1,) * (4 - mask.dim()) + tuple(mask.shape))
    mb, mh = m.shape[0], m.shape[1]
    if mb not in (1, B) or mh not in (1, H):
        raise NrvError(f"attention mask {tuple(mask.shape)} does not broadcast against {(B, H, Nq, Nk)}")
    try:
        m = m.expand(mb, mh, Nq, Nk).contiguous()          # only the query / key dims are ever materialised
    except RuntimeError as e:
        raise NrvError(f"attention mask {tuple(mask.shape)} does not broadcast against {(B, H, Nq, Nk)}") from e
    W = (Nk + 31) // 32
    bits = torch.empty(mb * mh * Nq, W, dtype=torch.int32, device=mask.device)
    check(_lib.load().nrv_mask_pack_bits(m.data_ptr(), bits.data_ptr(), mb * mh * Nq, Nk, _stream()), "nrv_mask_pack_bits")
    return MaskBits(bits, Nq, Nk, mh * Nq * W if mb > 1 else 0, Nq * W if mh > 1 else 0)


def _mem_args(mkv: Optional[Tensor], B: int, M: int, shared: bool, mask: Optional[MaskBits], Nq: int, H: int, dh: int):
    if M > 0:
        if mkv is None:
            raise NrvError(f"mkv: {M} memory keys need their mem_kv tensor")
        _bf16(mkv, "mkv")
        rows, cols, ld = _rows2d(mkv, "mkv")
        if cols != 2 * H * dh or ld != cols or rows < (M if shared else B * M):
            raise NrvError(f"mkv (mem_kv) must be contiguous [*, {2 * H * dh}] with at least {M if shared else B * M} rows, got "
                           f"{tuple(mkv.shape)} stride {mkv.stride()}")
    if mask is not None:
        if mask.Nq != Nq or mask.Nk != Nq + M:
            raise NrvError(f"mask packed for [{mask.Nq}, {mask.Nk}], attention is [{Nq}, {Nq + M}]")
        W = (mask.Nk + 31) // 32
        bits = mask.bits
        _dev(bits, "mask.bits")
        if bits.dtype != torch.int32 or not bits.is_contiguous() or min(mask.bstride, mask.hstride) < 0 \
                or bits.numel() < (B - 1) * mask.bstride + (H - 1) * mask.hstride + Nq * W:
            raise NrvError(f"mask.bits must be contiguous int32 words covering batch stride {mask.bstride}, head stride {mask.hstride} "
                           f"and {Nq} rows of {W}, got {bits.dtype} {tuple(bits.shape)} stride {bits.stride()}")
    mptr = mkv.data_ptr() if M > 0 else None
    kptr, bs, hs = (mask.bits.data_ptr(), mask.bstride, mask.hstride) if mask is not None else (None, 0, 0)
    return mptr, 0 if shared else M, kptr, bs, hs


def attn_mem_fwd(qkv: Tensor, mkv: Optional[Tensor], B: int, Nq: int, M: int, H: int, dh: int, scale: float,
                 shared: bool = True, mask: Optional[MaskBits] = None):
    """Softmax attention of the Nq token queries over Nq token keys + M memory keys (learnable_memory_vit.py:64-86).
    qkv bf16 [B*Nq, 3*H*dh]; mkv bf16 [M, 2*H*dh] (shared) or [B*M, 2*H*dh] (per sample) -> (out bf16 [B*Nq, H*dh], lse fp32 [B,H,Nq])."""
    _bf16(qkv, "qkv")
    if not qkv.is_contiguous() or qkv.numel() != B * Nq * 3 * H * dh:
        raise NrvError("attn_mem_fwd: qkv must be contiguous [B*Nq, 3*H*dh]")
    if M > 0 and not shared and mkv is not None and mkv.shape[0] != B * M:
        raise NrvError("attn_mem_fwd: per-sample memories need B*M rows of mkv")
    mptr, mstride, kptr, bs, hs = _mem_args(mkv, B, M, shared, mask, Nq, H, dh)
    out = torch.empty(B * Nq, H * dh, dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty(B, H, Nq, dtype=torch.float32, device=qkv.device)
    Nk = Nq + M
    lib = _lib.load()
    _run("attn_mem_fwd", 4.0 * B * H * Nq * Nk * dh, 2 * B * (2 * Nq + Nk) * H * dh * 2,
         lambda: lib.nrv_attn_mem_fwd(qkv.data_ptr(), mptr, mstride, M, kptr, bs, hs, out.data_ptr(), lse.data_ptr(),
                                      B, Nq, H, dh, float(scale), _stream()),
         "nrv_attn_mem_fwd")
    return out, lse


def attn_mem_bwd(qkv: Tensor, out: Tensor, dout: Tensor, lse: Tensor, mkv: Optional[Tensor], B: int, Nq: int, M: int, H: int,
                 dh: int, scale: float, shared: bool = True, mask: Optional[MaskBits] = None):
    """-> (dqkv bf16 [B*Nq, 3*H*dh], dmem_kv fp32 [M, 2*H*dh] summed over the batch (shared) / [B*M, 2*H*dh] (per sample),
    None when M == 0)."""
    _attn_bwd_args(qkv, out, dout, lse, B, Nq, H, dh)
    mptr, mstride, kptr, bs, hs = _mem_args(mkv, B, M, shared, mask, Nq, H, dh)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty(B * H * Nq, dtype=torch.float32, device=qkv.device)
    dmem = torch.empty(B * M, 2 * H * dh, dtype=torch.float32, device=qkv.device) if M > 0 else None
    dsum = torch.empty(M, 2 * H * dh, dtype=torch.float32, device=qkv.device) if M > 0 and shared else None
    Nk = Nq + M
    lib = _lib.load()
    _run("attn_mem_bwd", 10.0 * B * H * Nq * Nk * dh, 2 * B * (4 * Nq + 2 * Nk) * H * dh * 2,
         lambda: lib.nrv_attn_mem_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), mptr, mstride, M,
                                      kptr, bs, hs, dqkv.data_ptr(), _ptr(dmem), _ptr(dsum), delta.data_ptr(),
                                      B, Nq, H, dh, float(scale), _stream()),
         "nrv_attn_mem_bwd")
    return dqkv, (dsum if dsum is not None else dmem)


def _sinkhorn_fused_shape(N: int, dh: int) -> bool:
    """Shapes the fused kernels hold on chip (csrc/nrv_sinkhorn.hip): the head's whole [N, N] matrix in registers."""
    return dh == 64 and N <= 256


# composed robust attention: the forward's normalised matrix P7 [B,H,N,N] fp32 is handed to the backward (which otherwise recomputes it:
# the scores GEMM + 5 passes over the matrix) when it is at most this many bytes per layer -- 288 GB of HBM are there to be used
SINKHORN_KEEP_P_BYTES = 2 << 30


def attn_sinkhorn_fwd(qkv: Tensor, B: int, N: int, H: int, dh: int, scale: float, saved: Optional[dict] = None):
    """robust=True attention (utils.py:1025-1037): returns (out bf16, lse fp32 [B,H,N], scalings fp32 [B,H,7,N]).
    N <= 256 and dh == 64: the fused kernel.  Any other shape (vit_h_14, 384-px checkpoints, other head dims): composed from
    the batched GEMM and the stand-alone Sinkhorn op on materialised [B,H,N,N] scores -- the reference's own structure.
    `saved` (a dict the caller keeps for the backward and passes to attn_sinkhorn_bwd): the composed path leaves P7 in it."""
    _bf16(qkv, "qkv")
    if not qkv.is_contiguous() or qkv.numel() != B * N * 3 * H * dh:
        raise NrvError("attn_sinkhorn_fwd: qkv must be contiguous [B*N, 3*H*dh]")
    if not _sinkhorn_fused_shape(N, dh):
        return _attn_sinkhorn_fwd_composed(qkv, B, N, H, dh, scale, saved)
    out = torch.empty(B * N, H * dh, dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty(B, H, N, dtype=torch.float32, device=qkv.device)
    scal = torch.empty(B, H, 7, N, dtype=torch.float32, device=qkv.device)
    lib = _lib.load()
    _run("attn_sinkhorn_fwd", 4.0 * B * H * N * N * dh, 2 * B * N * H * dh * 4,
         lambda: lib.nrv_attn_sinkhorn_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), scal.data_ptr(),
                                           B, N, H, dh, float(scale), _stream()),
         "nrv_attn_sinkhorn_fwd")
    return out, lse, scal


def attn_sinkhorn_bwd(qkv: Tensor, dout: Tensor, lse: Tensor, scal: Tensor, B: int, N: int, H: int, dh: int, scale: float,
                      saved: Optional[dict] = None) -> Tensor:
    _dense(qkv, "qkv", torch.bfloat16, B * N * 3 * H * dh); _dense(dout, "dout", torch.bfloat16, B * N * H * dh)
    _dense(lse, "lse", torch.float32, B * H * N); _dense(scal, "scal", torch.float32, B * H * 7 * N)
    if not _sinkhorn_fused_shape(N, dh):
        return _attn_sinkhorn_bwd_composed(qkv, dout, lse, scal, B, N, H, dh, scale, saved)
    dqkv = torch.empty_like(qkv)
    lib = _lib.load()
    _run("attn_sinkhorn_bwd", 10.0 * B * H * N * N * dh, 2 * B * N * H * dh * 7,
         lambda: lib.nrv_attn_sinkhorn_bwd(qkv.data_ptr(), dout.data_ptr(), lse.data_ptr(), scal.data_ptr(), dqkv.data_ptr(),
                                           B, N, H, dh, float(scale), _stream()),
         "nrv_attn_sinkhorn_bwd")
    return dqkv


# ---- batched strided GEMM + attention composed on the materialised matrix -------------------------------------------------
def bgemm(A, a_str, B_, b_str, C, c_str, G1: int, G2: int, M: int, N: int, K: int, alpha: float = 1.0) -> None:
    """C[g1,g2] = alpha * A[g1,g2] . B[g1,g2] (include/nrv.h nrv_bgemm).  A, B, C: (tensor, element offset) pairs; *_str =
    (row stride, column stride, g1 stride, g2 stride) in elements.  The tensors are only memory: the strides do the addressing,
    and the caller guarantees that every addressed element lies inside its tensor (checked below)."""
    lib = _lib.load()
    ptrs = []
    for (t, off), st, rows, cols, name in ((A, a_str, M, K, "A"), (B_, b_str, K, N, "B"), (C, c_str, M, N, "C")):
        _dev(t, name)
        last = off + (rows - 1) * st[0] + (cols - 1) * st[1] + (G1 - 1) * st[2] + (G2 - 1) * st[3]
        if off < 0 or min(st) < 0 or last >= t.numel():
            raise NrvError(f"bgemm: operand {name} addresses element {last} of a tensor with {t.numel()}")
        ptrs.append((t.data_ptr() + off * t.element_size(), _dt(t, name)))
    _run("bgemm", 2.0 * G1 * G2 * M * N * K, 0.0,
         lambda: lib.nrv_bgemm(ptrs[0][0], ptrs[0][1], *[int(v) for v in a_str], ptrs[1][0], ptrs[1][1], *[int(v) for v in b_str],
                               ptrs[2][0], ptrs[2][1], *[int(v) for v in c_str], G1, G2, M, N, K, float(alpha), _stream()),
         "nrv_bgemm")


def bgemm_plan(A, a_str, B_, b_str, C, c_str, G1: int, G2: int, M: int, N: int, K: int) -> dict:
    """What `bgemm` would launch for these arguments (include/nrv.h nrv_bgemm_plan): which operands are staged by 16-byte vectors,
    whether C rows take vector stores, the tile grid and the workgroup count.  Operands as in `bgemm`, (tensor, element offset)
    pairs, or (address of element 0, torch dtype) pairs: only the alignment of an address enters the plan, so a made-up one
    will do.  Read-only; needs no GPU.  Raises NrvError where `nrv_bgemm` would refuse the launch."""
    args = []
    for (t, off), st, name in ((A, a_str, "A"), (B_, b_str, "B"), (C, c_str, "C")):
        if isinstance(t, Tensor):
            args += [t.data_ptr() + int(off) * t.element_size(), _dt(t, name)]
        else:
            args += [int(t), _dt(torch.empty(0, dtype=off), name)]
        args += [int(v) for v in st]
    pl = _lib.BgemmPlan()
    check(_lib.load().nrv_bgemm_plan(*args, int(G1), int(G2), int(M), int(N), int(K), ctypes.addressof(pl)), "nrv_bgemm_plan")
    return {"a_vec": bool(pl.a_vec), "b_vec": bool(pl.b_vec), "c_vec": bool(pl.c_vec), "tiles_m": pl.tiles_m, "tiles_n": pl.tiles_n,
            "blocks": pl.blocks}


def _composed_strides(N: int, H: int, dh: int):
    """(row, col, batch, head) element strides of one head's [N, dh] slice of q, k or v inside qkv [B*N, 3*H*dh] (and read
    transposed), of one head's slice of out / dout [B*N, H*dh], and of one head's [N, N] block of a [B,H,N,N] matrix (and transposed)."""
    W = 3 * H * dh
    return (W, 1, N * W, dh), (1, W, N * W, dh), (H * dh, 1, N * H * dh, dh), (N, 1, H * N * N, N * N), (1, N, H * N * N, N * N)


@dataclass
class ComposedSaved:
    """What attn_composed_bwd needs from attn_composed_fwd: P, the matrix that met v (None: the backward recomputes it), the
    Sinkhorn op's statistics (lse [B*H, N], avec, bvec) and the call's keep mask, its scale, the iteration count and the bias."""
    P: Optional[Tensor]
    lse: Tensor
    avec: Tensor
    bvec: Tensor
    keep: Optional[Tensor]
    pscale: float
    iters: int
    bias: Optional[Tensor]


def _composed_scores(qkv: Tensor, B: int, N: int, H: int, dh: int, scale: float, bias: Optional[Tensor]) -> Tensor:
    """S[b,h] = scale * q k^T (+ bias), fp32 [B,H,N,N] (simple_vit.py:70)."""
    hq, hqT, _, mat, _ = _composed_strides(N, H, dh)
    S = torch.empty(B, H, N, N, dtype=torch.float32, device=qkv.device)
    bgemm((qkv, 0), hq, (qkv, H * dh), hqT, (S, 0), mat, B, H, N, N, dh, scale)
    if bias is not None:
        _f32(bias, "bias")
        S += bias                                   # broadcast over batch / heads: plumbing, once per call (not a BASELINE path)
    return S


def _composed_probs(S: Tensor, iters: int, keep: Optional[Tensor], pscale: float):
    """(P, lse, avec, bvec): the Sinkhorn op on the scores (utils.py:1031-1037; 0 iterations = softmax), then the keep mask."""
    P, lse, avec, bvec = sinkhorn_fwd(S, iters=iters)
    if keep is not None:
        mask_mul_f32(P, keep, pscale, out=P)
    return P, lse, avec, bvec


def attn_composed_fwd(qkv: Tensor, B: int, N: int, H: int, dh: int, scale: float, iters: int, keep: Optional[Tensor] = None,
                      pscale: float = 1.0, bias: Optional[Tensor] = None):
    """Attention on the materialised [B,H,N,N] matrix, for what the fused kernels do not take: robust=True beyond their shapes
    (iters = 3), dropout on the attention weights (vit.py:108; `keep` uint8 [B,H,N,N], kept weights times `pscale`) and an additive
    score bias (masks of torch's MultiheadAttention, utils.py:741-751: fp32, broadcast to [B,H,N,N], -inf = masked).  Scores (+ bias),
    the Sinkhorn op (iters = 0: softmax), the keep mask, P v -- the reference's own structure.  Returns (out bf16, ComposedSaved)."""
    _bf16(qkv, "qkv")
    if keep is not None and tuple(keep.shape) != (B, H, N, N):
        raise NrvError(f"attn_composed_fwd: keep must be a uint8 mask of shape {(B, H, N, N)}")
    hq, _, ho, mat, _ = _composed_strides(N, H, dh)
    S = _composed_scores(qkv, B, N, H, dh, scale, bias)
    P, lse, avec, bvec = _composed_probs(S, iters, keep, pscale)
    del S
    out = torch.empty(B * N, H * dh, dtype=torch.bfloat16, device=qkv.device)
    # O[b,h] = P v   (attn v, simple_vit.py:74; P enters the product in bf16 as in the fused kernels)
    bgemm((P, 0), mat, (qkv, 2 * H * dh), hq, (out, 0), ho, B, H, N, dh, N, 1.0)
    return out, ComposedSaved(P, lse, avec, bvec, keep, pscale, iters, bias)


def attn_composed_bwd(qkv: Tensor, dout: Tensor, saved: ComposedSaved, B: int, N: int, H: int, dh: int, scale: float) -> Tensor:
    """dqkv of attn_composed_fwd.  Takes P out of `saved` (freed once its two products are done); without it (the robust path did
    not keep it, or a second backward) P is recomputed from the scores the Sinkhorn backward needs anyway."""
    hq, hqT, ho, mat, matT = _composed_strides(N, H, dh)
    S = _composed_scores(qkv, B, N, H, dh, scale, saved.bias)      # masked scores are -inf: P0 = 0 there, and so is dS
    P, saved.P = saved.P, None
    if P is None:
        P = _composed_probs(S, saved.iters, saved.keep, saved.pscale)[0]
    dqkv = torch.empty_like(qkv)
    # dV = P^T dO
    bgemm((P, 0), matT, (dout, 0), ho, (dqkv, 2 * H * dh), hq, B, H, N, dh, N, 1.0)
    # dP = dO v^T, reusing P's storage would alias an operand of nothing that follows: a buffer of its own keeps it simple
    dP = torch.empty_like(P)
    bgemm((dout, 0), ho, (qkv, 2 * H * dh), hqT, (dP, 0), mat, B, H, N, N, dh, 1.0)
    del P
    if saved.keep is not None:
        mask_mul_f32(dP, saved.keep, saved.pscale, out=dP)
    dS = sinkhorn_bwd(S, dP, saved.lse, saved.avec, saved.bvec, iters=saved.iters)
    del dP, S
    # dQ = scale dS k ;  dK = scale dS^T q
    bgemm((dS, 0), mat, (qkv, H * dh), hq, (dqkv, 0), hq, B, H, N, dh, N, scale)
    bgemm((dS, 0), matT, (qkv, 0), hq, (dqkv, H * dh), hq, B, H, N, dh, N, scale)
    return dqkv


def _attn_sinkhorn_fwd_composed(qkv: Tensor, B: int, N: int, H: int, dh: int, scale: float, saved: Optional[dict] = None):
    out, cs = attn_composed_fwd(qkv, B, N, H, dh, scale, iters=SINKHORN_ITERS)
    # the model keeps ONE form of the saved statistics: [B,H,7,N] = a1 b1 a2 b2 a3 b3 a4 (cumulative), as the fused kernel writes it
    scal = torch.empty(B, H, 7, N, dtype=torch.float32, device=qkv.device)
    scal[:, :, 0::2] = cs.avec.reshape(B, H, 4, N)
    scal[:, :, 1::2] = cs.bvec.reshape(B, H, 3, N)
    if saved is not None and cs.P.numel() * 4 <= SINKHORN_KEEP_P_BYTES:
        saved["P7"] = cs.P
    return out, cs.lse.reshape(B, H, N), scal


def _attn_sinkhorn_bwd_composed(qkv: Tensor, dout: Tensor, lse: Tensor, scal: Tensor, B: int, N: int, H: int, dh: int, scale: float,
                                saved: Optional[dict] = None) -> Tensor:
    # P7 goes straight into the record (no local name here), so the backward frees it as soon as it is used
    cs = ComposedSaved(saved.pop("P7", None) if saved is not None else None, lse.reshape(B * H, N).contiguous(),
                       scal[:, :, 0::2].reshape(B * H, 4, N).contiguous(), scal[:, :, 1::2].reshape(B * H, 3, N).contiguous(),
                       keep=None, pscale=1.0, iters=SINKHORN_ITERS, bias=None)
    return attn_composed_bwd(qkv, dout, cs, B, N, H, dh, scale)


def patch_unfold(img: Tensor, p: int, layout: int) -> Tensor:
    """img [B,C,H,W] fp32|bf16 -> patches bf16 [B*(H/p)*(W/p), FP]; FP = C*p*p rounded up to a multiple of 8, the extra
    columns are zero (only patch sizes like 14 have any)."""
    _dev(img, "img")
    img = img.contiguous()
    B, C, H, W = img.shape
    out = torch.empty(B * (H // p) * (W // p), (C * p * p + 7) // 8 * 8, dtype=torch.bfloat16, device=img.device)
    lib = _lib.load()
    _run("patch_unfold", 0.0, img.numel() * (img.element_size() + 2),
         lambda: lib.nrv_patch_unfold(img.data_ptr(), _dt(img, "img"), out.data_ptr(), B, C, H, W, p, layout, _stream()),
         "nrv_patch_unfold")
    return out


def cast_transpose(w: Tensor, need_t: bool = True):
    """w fp32 [R,C] -> (w_bf16 [R,C], wT_bf16 [C,R] | None)."""
    _f32(w, "w")
    w = w.contiguous()
    R, C = w.shape
    wb = torch.empty(R, C, dtype=torch.bfloat16, device=w.device)
    wt = torch.empty(C, R, dtype=torch.bfloat16, device=w.device) if need_t else None
    lib = _lib.load()
    _run("cast_transpose", 0.0, R * C * 8,
         lambda: lib.nrv_cast_transpose(w.data_ptr(), wb.data_ptr(), _ptr(wt), R, C, _stream()), "nrv_cast_transpose")
    return wb, wt


def cast_bf16(x: Tensor, out: Optional[Tensor] = None) -> Tensor:
    _f32(x, "x")
    x = x.contiguous()
    if out is None:
        y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    else:
        _bf16(out, "out")
        if out.numel() != x.numel() or not out.is_contiguous():
            raise NrvError("cast_bf16: out must be contiguous bf16 of the same size")
        y = out
    lib = _lib.load()
    _run("cast_bf16", 0.0, x.numel() * 6,
         lambda: lib.nrv_cast_f32_bf16(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "nrv_cast_f32_bf16")
    return y


def _keep_mask(keep: Tensor, like: Tensor, what: str) -> None:
    _dev(keep, "keep")
    if keep.dtype != torch.uint8 or not keep.is_contiguous() or keep.numel() != like.numel():
        raise NrvError(f"{what}: keep must be a contiguous uint8 mask with one byte per element")
    if like.numel() % 8:
        raise NrvError(f"{what}: the element count must be a multiple of 8")


def dropout_add(x: Tensor, y: Tensor, keep: Tensor, scale: float, out: Optional[Tensor] = None) -> Tensor:
    """out = x + y * (keep ? scale : 0): the fp32 residual stream takes a dropped branch output (include/nrv.h nrv_dropout_add_f32)."""
    _dense(x, "x", torch.float32, x.numel()); _dense(y, "y", torch.float32, x.numel(), "x")
    _keep_mask(keep, x, "dropout_add")
    o = torch.empty_like(x) if out is None else out
    if out is not None:
        _dense(out, "out", torch.float32, x.numel(), "x")
    lib = _lib.load()
    _run("dropout", 0.0, x.numel() * 13,
         lambda: lib.nrv_dropout_add_f32(x.data_ptr(), y.data_ptr(), keep.data_ptr(), o.data_ptr(), float(scale), x.numel(), _stream()),
         "nrv_dropout_add_f32")
    return o


def mask_mul(a: Tensor, keep: Tensor, scale: float, out: Optional[Tensor] = None) -> Tensor:
    """out = a * (keep ? scale : 0) on bf16 tensors (include/nrv.h nrv_mask_mul_bf16); `out=a` works in place."""
    _dense(a, "a", torch.bfloat16, a.numel())
    _keep_mask(keep, a, "mask_mul")
    o = torch.empty_like(a) if out is None else out
    if out is not None:
        _dense(out, "out", torch.bfloat16, a.numel(), "a")
    lib = _lib.load()
    _run("dropout", 0.0, a.numel() * 5,
         lambda: lib.nrv_mask_mul_bf16(a.data_ptr(), keep.data_ptr(), o.data_ptr(), float(scale), a.numel(), _stream()),
         "nrv_mask_mul_bf16")
    return o


def mask_mul_f32(a: Tensor, keep: Tensor, scale: float, out: Optional[Tensor] = None) -> Tensor:
    """out = a * (keep ? scale : 0) on fp32 tensors of any size (include/nrv.h nrv_mask_mul_f32)."""
    _dense(a, "a", torch.float32, a.numel()); _dense(keep, "keep", torch.uint8, a.numel(), "a")
    o = torch.empty_like(a) if out is None else out
    if out is not None:
        _dense(out, "out", torch.float32, a.numel(), "a")
    lib = _lib.load()
    _run("dropout", 0.0, a.numel() * 9,
         lambda: lib.nrv_mask_mul_f32(a.data_ptr(), keep.data_ptr(), o.data_ptr(), float(scale), a.numel(), _stream()), "nrv_mask_mul_f32")
    return o


def gather_rows(src: Tensor, index: Tensor) -> Tensor:
    """out[r] = src[index[r]]; src fp32 [R, dim], index int64 [rows_out]."""
    _f32(src, "src"); _dev(index, "index")
    src = src.contiguous(); index = index.contiguous()
    out = torch.empty(index.numel(), src.shape[1], dtype=torch.float32, device=src.device)
    if index.dtype != torch.int64:
        raise NrvError(f"gather_rows: index must be int64, got {index.dtype}")
    check(_lib.load().nrv_gather_rows_f32(src.data_ptr(), index.data_ptr(), out.data_ptr(), index.numel(), src.shape[0], src.shape[1], _stream()),
          "nrv_gather_rows_f32")
    return out


def scatter_rows(dout: Tensor, index: Tensor, rows_src: int) -> Tensor:
    """dsrc = zeros[rows_src, dim]; dsrc[index[r]] = dout[r]  (indices unique)."""
    _f32(dout, "dout"); _dev(index, "index")
    dout = dout.contiguous(); index = index.contiguous()
    dsrc = torch.zeros(rows_src, dout.shape[1], dtype=torch.float32, device=dout.device)
    if index.dtype != torch.int64 or index.numel() != dout.shape[0]:
        raise NrvError("scatter_rows: index must be int64 with one entry per row of dout")
    check(_lib.load().nrv_scatter_rows_f32(dout.data_ptr(), index.data_ptr(), dsrc.data_ptr(), index.numel(), rows_src, dout.shape[1], _stream()),
          "nrv_scatter_rows_f32")
    return dsrc


def probe(which: int, data: Tensor, n_out: int) -> Tensor:
    _dev(data, "data")
    out = torch.zeros(n_out, dtype=torch.float32, device=data.device)
    check(_lib.load().nrv_probe(which, data.data_ptr(), out.data_ptr(), data.numel() * data.element_size(), _stream()), "nrv_probe")
    return out


def sumsq_workspace(n: int) -> int:
    return int(_lib.load().nrv_sumsq_workspace(int(n)))


def sumsq(x: Tensor, out: Tensor, ws: Tensor) -> None:
    """out[0] = sum(x^2) for a flat fp32 or bf16 buffer (deterministic); ws: fp32 scratch of nrv_sumsq_workspace bytes."""
    _dense(x, "x", None, x.numel()); _dense(out, "out", torch.float32, 1)
    lib = _lib.load()
    _dev(ws, "ws")
    if ws.dtype != torch.float32 or not ws.is_contiguous() or ws.numel() * 4 < lib.nrv_sumsq_workspace(x.numel()):
        raise NrvError(f"sumsq: ws must be contiguous fp32 scratch of nrv_sumsq_workspace({x.numel()}) bytes, got {ws.dtype} {tuple(ws.shape)}")
    _run("optimizer", 0.0, x.numel() * x.element_size(),
         lambda: lib.nrv_sumsq_f32(x.data_ptr(), _dt(x, "x"), x.numel(), out.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(), _stream()),
         "nrv_sumsq_f32")


def adamw_flat(p: Tensor, g: Tensor, m: Tensor, v: Tensor, lr: float, beta1: float, beta2: float, eps: float,
               weight_decay: float, step: int, gnorm_sq: Optional[Tensor], max_norm: float,
               step_scalars: Optional[Tensor] = None) -> None:
    """In-place clip + AdamW on flat buffers (include/nrv.h: nrv_adamw_f32): p, m, v fp32; g fp32 or bf16 (the reduced slabs of a
    bf16 gradient exchange, read in place).  `step_scalars`: device tensor of 3 floats that replaces the step-dependent scalars
    (graph replay)."""
    n = p.numel()
    _dense(p, "p", torch.float32, n); _dense(m, "m", torch.float32, n, "p"); _dense(v, "v", torch.float32, n, "p"); _dense(g, "g", None, n, "p")
    if gnorm_sq is not None:
        _dense(gnorm_sq, "gnorm_sq", torch.float32, 1)
    if step_scalars is not None:
        _dev(step_scalars, "step_scalars")
        if step_scalars.dtype != torch.float32 or not step_scalars.is_contiguous() or step_scalars.numel() < 3:
            raise NrvError(f"step_scalars must hold at least 3 contiguous fp32 values, got {step_scalars.dtype} {tuple(step_scalars.shape)}")
    lib = _lib.load()
    _run("optimizer", 0.0, p.numel() * (24 + g.element_size()),
         lambda: lib.nrv_adamw_f32(p.data_ptr(), g.data_ptr(), _dt(g, "g"), m.data_ptr(), v.data_ptr(), p.numel(),
                                   float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step),
                                   _ptr(gnorm_sq), float(max_norm), _ptr(step_scalars), _stream()),
         "nrv_adamw_f32")


SINKHORN_ITERS = 3                       # SinkhornAttention's default (utils.py:1025-1037)


def sinkhorn_fwd(scores: Tensor, iters: int = SINKHORN_ITERS):
    """SinkhornAttention(scores) on a materialised fp32 score tensor [..., R, C] (utils.py:1025-1037) -> (P, lse, avec, bvec)."""
    _f32(scores, "scores")
    if scores.dim() < 2:
        raise NrvError("sinkhorn_fwd: scores must have at least two dimensions")
    s = scores.contiguous()
    R, C = s.shape[-2], s.shape[-1]
    G = s.numel() // (R * C)
    out = torch.empty_like(s)
    lse = torch.empty(G, R, dtype=torch.float32, device=s.device)
    avec = torch.empty(G, iters + 1, R, dtype=torch.float32, device=s.device)
    bvec = torch.empty(G, max(iters, 1), C, dtype=torch.float32, device=s.device)
    lib = _lib.load()
    _run("sinkhorn_norm_fwd", 0.0, s.numel() * 4 * (2 * iters + 3),
         lambda: lib.nrv_sinkhorn_fwd(s.data_ptr(), out.data_ptr(), lse.data_ptr(), avec.data_ptr(), bvec.data_ptr(),
                                      G, R, C, int(iters), _stream()), "nrv_sinkhorn_fwd")
    return out, lse, avec, bvec


def sinkhorn_bwd(scores: Tensor, dout: Tensor, lse: Tensor, avec: Tensor, bvec: Tensor, iters: int = SINKHORN_ITERS) -> Tensor:
    _f32(scores, "scores"); _f32(dout, "dout")
    if scores.dim() < 2:
        raise NrvError("sinkhorn_bwd: scores must have at least two dimensions")
    s = scores.contiguous()
    R, C = s.shape[-2], s.shape[-1]
    G = s.numel() // (R * C)
    if dout.numel() != s.numel():
        raise NrvError(f"sinkhorn_bwd: dout has {dout.numel()} elements, scores {s.numel()}")
    d = dout.contiguous()
    _dense(lse, "lse", torch.float32, G * R, "scores"); _dense(avec, "avec", torch.float32, G * (iters + 1) * R, "scores and iters")
    _dense(bvec, "bvec", torch.float32, G * max(iters, 1) * C, "scores and iters")
    ds = torch.empty_like(s)
    lib = _lib.load()
    _run("sinkhorn_norm_bwd", 0.0, s.numel() * 4 * (4 * iters + 6),
         lambda: lib.nrv_sinkhorn_bwd(s.data_ptr(), d.data_ptr(), lse.data_ptr(), avec.data_ptr(), bvec.data_ptr(), ds.data_ptr(),
                                      G, R, C, int(iters), _stream()), "nrv_sinkhorn_bwd")
    return ds


def cast_transpose_batched(jobs) -> None:
    """Re-stage many weights in ONE launch.  jobs: list of (w fp32 [R,C], wb bf16 [R,C], wt bf16 [C,R] | None), all on one device;
    returns a reusable handle via `build_cast_jobs`."""
    handle = build_cast_jobs(jobs)
    run_cast_jobs(handle)


def build_cast_jobs(jobs):
    """Device-side job table of include/nrv.h `nrv_cast_job` (7 x int64 per entry).  The tensors must stay alive (and in place)
    for as long as the handle is used."""
    import numpy as np
    if not jobs:
        return None
    rows, start = [], 0
    for i, (w, wb, wt) in enumerate(jobs):
        if w.dim() != 2:
            raise NrvError(f"jobs[{i}]: w must be fp32 [R, C], got {tuple(w.shape)}")
        R, C = w.shape
        _dense(w, f"jobs[{i}] w", torch.float32, R * C); _dense(wb, f"jobs[{i}] wb", torch.bfloat16, R * C, "w")
        if wt is not None:
            _dense(wt, f"jobs[{i}] wt", torch.bfloat16, R * C, "w")
        tiles_c = (C + 63) // 64
        rows.append((w.data_ptr(), wb.data_ptr(), 0 if wt is None else wt.data_ptr(), R, C, start, tiles_c))
        start += ((R + 63) // 64) * tiles_c
    table = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(jobs[0][0].device)
    return table, len(rows), start


def run_cast_jobs(handle) -> None:
    if handle is None:
        return
    table, n, total = handle
    lib = _lib.load()
    _run("cast_transpose", 0.0, 0.0, lambda: lib.nrv_cast_transpose_batched(table.data_ptr(), n, total, _stream()),
         "nrv_cast_transpose_batched")


# ----------------------------------------------------------------------------------------------
# Swin: shifted-window attention and row-mode stochastic depth (include/nrv.h, ABI 15)
# ----------------------------------------------------------------------------------------------
def _window_args(qkv: Tensor, B: int, pH: int, pW: int, C: int, heads: int, Wh: int, Ww: int, sh: int, sw: int) -> None:
    _bf16(qkv, "qkv")
    if not qkv.is_contiguous() or tuple(qkv.shape) != (B * pH * pW, 3 * C):
        raise NrvError(f"window_attn: qkv must be contiguous [{B * pH * pW}, {3 * C}], got {tuple(qkv.shape)}")
    if C % heads or C // heads not in (32, 64):
        raise NrvError(f"window_attn: head dim C / heads = {C / heads} is not 32 or 64")
    if Wh * Ww > 64 or pH % Wh or pW % Ww or not (0 <= sh < Wh) or not (0 <= sw < Ww):
        raise NrvError(f"window_attn: window {Wh}x{Ww} (<= 64 slots) must tile the padded map {pH}x{pW}; shift ({sh}, {sw})")


def window_attn_fwd(qkv: Tensor, table: Tensor, B: int, pH: int, pW: int, C: int, heads: int, window, shift, robust: bool):
    """Shifted-window attention over the padded map (include/nrv.h nrv_window_attn_fwd).  Returns (out bf16 [B*pH*pW, C], stats)."""
    Wh, Ww = window
    sh, sw = shift
    _window_args(qkv, B, pH, pW, C, heads, Wh, Ww, sh, sw)
    _f32(table, "table")
    if tuple(table.shape) != ((2 * Wh - 1) * (2 * Ww - 1), heads) or not table.is_contiguous():
        raise NrvError(f"window_attn: table must be contiguous [{(2 * Wh - 1) * (2 * Ww - 1)}, {heads}], got {tuple(table.shape)}")
    T = B * pH * pW
    out = torch.empty(T, C, dtype=torch.bfloat16, device=qkv.device)
    stats = torch.empty(T, heads, 8 if robust else 1, dtype=torch.float32, device=qkv.device)
    lib = _lib.load()
    N = Wh * Ww
    _run("window_attn_fwd", 4.0 * T * N * C, T * C * 8 + stats.numel() * 4,
         lambda: lib.nrv_window_attn_fwd(qkv.data_ptr(), table.data_ptr(), out.data_ptr(), stats.data_ptr(), B, pH, pW, C, heads,
                                         Wh, Ww, sh, sw, int(bool(robust)), _stream()),
         "nrv_window_attn_fwd")
    return out, stats


def window_attn_bwd(qkv: Tensor, table: Tensor, dout: Tensor, stats: Tensor, B: int, pH: int, pW: int, C: int, heads: int,
                    window, shift, robust: bool):
    """Returns (dqkv bf16 [B*pH*pW, 3C], dtable fp32 [(2Wh-1)(2Ww-1), heads]); deterministic."""
    Wh, Ww = window
    sh, sw = shift
    _window_args(qkv, B, pH, pW, C, heads, Wh, Ww, sh, sw)
    _bf16(dout, "dout"); _f32(stats, "stats"); _f32(table, "table")
    T = B * pH * pW
    if tuple(table.shape) != ((2 * Wh - 1) * (2 * Ww - 1), heads) or not table.is_contiguous():
        raise NrvError(f"window_attn: table must be contiguous [{(2 * Wh - 1) * (2 * Ww - 1)}, {heads}], got {tuple(table.shape)}")
    if not dout.is_contiguous() or tuple(dout.shape) != (T, C):
        raise NrvError(f"window_attn_bwd: dout must be contiguous [{T}, {C}], got {tuple(dout.shape)}")
    if tuple(stats.shape) != (T, heads, 8 if robust else 1) or not stats.is_contiguous():
        raise NrvError(f"window_attn_bwd: stats {tuple(stats.shape)} stride {stats.stride()} do not belong to this call")
    lib = _lib.load()
    wsb = lib.nrv_window_attn_bwd_workspace(B, pH, pW, C, heads, Wh, Ww)
    ws = _workspace(wsb, qkv.device)
    dqkv = torch.empty(T, 3 * C, dtype=torch.bfloat16, device=qkv.device)
    dtable = torch.empty_like(table)
    N = Wh * Ww
    _run("window_attn_bwd", 10.0 * T * N * C, T * C * 16 + stats.numel() * 4,
         lambda: lib.nrv_window_attn_bwd(qkv.data_ptr(), table.data_ptr(), dout.data_ptr(), stats.data_ptr(), dqkv.data_ptr(),
                                         dtable.data_ptr(), ws.data_ptr(), wsb, B, pH, pW, C, heads, Wh, Ww, sh, sw,
                                         int(bool(robust)), _stream()),
         "nrv_window_attn_bwd")
    return dqkv, dtable


def _sd_args(x: Tensor, name: str, keep: Tensor, survival: float) -> Tuple[int, int]:
    _f32(keep, "keep")
    if not x.is_contiguous() or x.dim() != 2 or x.shape[1] % 4:
        raise NrvError(f"stochastic depth: {name} must be a contiguous [rows, dim] tensor with dim % 4 == 0, got {tuple(x.shape)}")
    if keep.dim() != 1 or not keep.is_contiguous() or x.shape[0] % keep.numel():
        raise NrvError(f"stochastic depth: keep must be one value per sample, {keep.numel()} does not divide {x.shape[0]} rows")
    if not survival > 0.0:
        raise NrvError("stochastic depth: survival probability must be > 0")
    return x.shape[0], x.shape[0] // keep.numel()


def sd_add(x: Tensor, y: Tensor, keep: Tensor, survival: float, out: Optional[Tensor] = None) -> Tensor:
    """out = x + y * keep[sample] / survival (include/nrv.h nrv_sd_add_f32)."""
    _f32(x, "x"); _f32(y, "y")
    rows, per = _sd_args(x, "x", keep, survival)
    _dense(y, "y", torch.float32, x.numel(), "x")
    o = torch.empty_like(x) if out is None else out
    if out is not None:
        _dense(out, "out", torch.float32, x.numel(), "x")
    _run("sd_add", 0.0, x.numel() * 12,
         lambda: _lib.load().nrv_sd_add_f32(x.data_ptr(), y.data_ptr(), keep.data_ptr(), o.data_ptr(), float(survival), rows, per,
                                            x.shape[1], _stream()), "nrv_sd_add_f32")
    return o


def sd_scale_bf16(dy: Tensor, keep: Tensor, survival: float) -> Tensor:
    """bf16(dy * keep[sample] / survival): the branch gradient of sd_add (include/nrv.h nrv_sd_scale_bf16)."""
    _f32(dy, "dy")
    rows, per = _sd_args(dy, "dy", keep, survival)
    o = torch.empty(dy.shape, dtype=torch.bfloat16, device=dy.device)
    _run("sd_scale", 0.0, dy.numel() * 6,
         lambda: _lib.load().nrv_sd_scale_bf16(dy.data_ptr(), keep.data_ptr(), o.data_ptr(), float(survival), rows, per,
                                               dy.shape[1], _stream()), "nrv_sd_scale_bf16")
    return o


# ----------------------------------------------------------------------------------------------
# LeViT (ABI 16): batch norm over rows, convolution as unfold + GEMM, attention with a learned offset bias
# ----------------------------------------------------------------------------------------------
def _bn_rows(y: Tensor, name: str) -> Tuple[int, int]:
    _f32(y, name)
    if y.dim() != 2 or not y.is_contiguous() or y.shape[1] % 4:
        raise NrvError(f"batch norm: {name} must be contiguous fp32 [T, C] with C % 4 == 0, got {tuple(y.shape)}")
    return y.shape[0], y.shape[1]


def _bn_keep(keep: Optional[Tensor], T: int) -> int:
    if keep is None:
        return 1
    _f32(keep, "keep")
    if keep.dim() != 1 or not keep.is_contiguous() or T % keep.numel():
        raise NrvError(f"batch norm: keep must be one value per sample, {keep.numel()} does not divide {T} rows")
    return T // keep.numel()


def bn_stats(y: Tensor, eps: float, momentum: float, running_mean: Optional[Tensor] = None,
             running_var: Optional[Tensor] = None):
    """Training-mode statistics of y [T, C] (include/nrv.h nrv_bn_stats); updates the running buffers in place when given.
    Returns (mean, invstd, stat [3, C] = the combined (count, mean, M2))."""
    T, C = _bn_rows(y, "y")
    for t, n in ((running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None:
            _f32(t, n)
            if t.numel() != C or not t.is_contiguous():
                raise NrvError(f"bn_stats: {n} must hold {C} contiguous floats")
    mean = torch.empty(C, dtype=torch.float32, device=y.device)
    invstd = torch.empty_like(mean)
    stat = torch.empty(3, C, dtype=torch.float32, device=y.device)
    lib = _lib.load()
    wsb = lib.nrv_bn_workspace(T, C)
    ws = _workspace(wsb, y.device)
    _run("bn_stats", 4.0 * T * C, 4 * T * C,
         lambda: lib.nrv_bn_stats(y.data_ptr(), T, C, float(eps), float(momentum), mean.data_ptr(), invstd.data_ptr(),
                                  stat.data_ptr(), _ptr(running_mean), _ptr(running_var), ws.data_ptr(), wsb, _stream()),
         "nrv_bn_stats")
    return mean, invstd, stat


def bn_apply(y: Tensor, mean: Tensor, scale: Tensor, gamma: Tensor, beta: Tensor, *, eps: float = 0.0, scale_is_var: bool = False,
             act: bool = False, residual: Optional[Tensor] = None, keep: Optional[Tensor] = None, survival: float = 1.0,
             want_f32: bool = False, want_bf16: bool = True):
    """z = gamma (y - mean) inv + beta [-> hardswish] [* keep / survival] [+ residual] (include/nrv.h nrv_bn_apply).
    Returns (z fp32 or None, z bf16 or None)."""
    T, C = _bn_rows(y, "y")
    for t, n in ((mean, "mean"), (scale, "scale"), (gamma, "gamma"), (beta, "beta")):
        _f32(t, n)
        if t.numel() != C or not t.is_contiguous():
            raise NrvError(f"bn_apply: {n} must hold {C} contiguous floats")
    if residual is not None:
        _f32(residual, "residual")
        if residual.shape != y.shape or not residual.is_contiguous():
            raise NrvError("bn_apply: residual must match y")
    per = _bn_keep(keep, T)
    o32 = torch.empty(T, C, dtype=torch.float32, device=y.device) if want_f32 else None
    o16 = torch.empty(T, C, dtype=torch.bfloat16, device=y.device) if want_bf16 else None
    _run("bn_apply", 4.0 * T * C, T * C * (4 + (4 if want_f32 else 0) + (2 if want_bf16 else 0) + (4 if residual is not None else 0)),
         lambda: _lib.load().nrv_bn_apply(y.data_ptr(), mean.data_ptr(), scale.data_ptr(), int(scale_is_var), float(eps),
                                          gamma.data_ptr(), beta.data_ptr(), int(bool(act)), _ptr(residual), _ptr(keep),
                                          float(survival), per, _ptr(o32), _ptr(o16), T, C, _stream()),
         "nrv_bn_apply")
    return o32, o16


def bn_bwd(dz: Tensor, y: Tensor, mean: Tensor, scale: Tensor, gamma: Tensor, beta: Tensor, *, eps: float = 0.0,
           scale_is_var: bool = False, act: bool = False, keep: Optional[Tensor] = None, survival: float = 1.0,
           training: bool = True):
    """Backward of bn_apply without the residual (include/nrv.h nrv_bn_bwd): returns (dy bf16 [T, C], dgamma, dbeta)."""
    T, C = _bn_rows(y, "y")
    _dense(dz, "dz", None, T * C, "y")
    for t, n in ((mean, "mean"), (scale, "scale"), (gamma, "gamma"), (beta, "beta")):
        _dense(t, n, torch.float32, C, "y")
    per = _bn_keep(keep, T)
    dy = torch.empty(T, C, dtype=torch.bfloat16, device=y.device)
    dg = torch.empty(C, dtype=torch.float32, device=y.device)
    db = torch.empty_like(dg)
    lib = _lib.load()
    wsb = lib.nrv_bn_workspace(T, C)
    ws = _workspace(wsb, y.device)
    _run("bn_bwd", 10.0 * T * C, T * C * (8 + 2 * dz.element_size() + 2),
         lambda: lib.nrv_bn_bwd(dz.data_ptr(), _dt(dz, "dz"), int(bool(act)), _ptr(keep), float(survival), per,
                                y.data_ptr(), mean.data_ptr(), scale.data_ptr(), int(scale_is_var), float(eps),
                                gamma.data_ptr(), beta.data_ptr(), int(bool(training)), dg.data_ptr(), db.data_ptr(),
                                dy.data_ptr(), ws.data_ptr(), wsb, T, C, _stream()),
         "nrv_bn_bwd")
    return dy, dg, db


def conv_out_size(n: int, ks: int, stride: int, pad: int) -> int:
    return (n + 2 * pad - ks) // stride + 1


def conv_unfold(src: Tensor, B: int, C: int, H: int, W: int, ks: int, stride: int, pad: int, nhwc: bool) -> Tensor:
    """cols bf16 [B*Ho*Wo, KP], feature (ky, kx, c) (include/nrv.h nrv_conv_unfold); src NCHW image or NHWC rows bf16."""
    _dev(src, "src")
    if not src.is_contiguous() or src.numel() != B * C * H * W:
        raise NrvError(f"conv_unfold: src must be contiguous with {B}x{C}x{H}x{W} elements, got {tuple(src.shape)}")
    Ho, Wo = conv_out_size(H, ks, stride, pad), conv_out_size(W, ks, stride, pad)
    KP = (ks * ks * C + 7) // 8 * 8
    cols = torch.empty(B * Ho * Wo, KP, dtype=torch.bfloat16, device=src.device)
    layout = _lib.CONV_NHWC if nhwc else _lib.CONV_NCHW
    _run("conv_unfold", 0.0, cols.numel() * 2 + src.numel() * src.element_size(),
         lambda: _lib.load().nrv_conv_unfold(src.data_ptr(), _dt(src, "src"), layout, cols.data_ptr(), B, C, H, W, ks, stride, pad,
                                             _stream()),
         "nrv_conv_unfold")
    return cols


def conv_fold(dcols: Tensor, B: int, C: int, H: int, W: int, ks: int, stride: int, pad: int) -> Tensor:
    """dx fp32 NHWC rows [B*H*W, C] (include/nrv.h nrv_conv_fold)."""
    _bf16(dcols, "dcols")
    Ho, Wo = conv_out_size(H, ks, stride, pad), conv_out_size(W, ks, stride, pad)
    KP = (ks * ks * C + 7) // 8 * 8
    if not dcols.is_contiguous() or tuple(dcols.shape) != (B * Ho * Wo, KP):
        raise NrvError(f"conv_fold: dcols must be contiguous [{B * Ho * Wo}, {KP}], got {tuple(dcols.shape)}")
    dx = torch.empty(B * H * W, C, dtype=torch.float32, device=dcols.device)
    _run("conv_fold", 0.0, dcols.numel() * 2 + dx.numel() * 4,
         lambda: _lib.load().nrv_conv_fold(dcols.data_ptr(), dx.data_ptr(), B, C, H, W, ks, stride, pad, _stream()),
         "nrv_conv_fold")
    return dx


@dataclass
class BiasIndex:
    """Device copies of one geometry's bias index: idx int32 [Nq, Nk] and its inverse (CSR over the table entries)."""
    idx: Tensor
    inv_ptr: Tensor
    inv_pos: Tensor
    n_offsets: int


def bias_index(idx: Tensor, n_offsets: int, device) -> BiasIndex:
    """Build the int32 index and its inverse from an int64 [Nq, Nk] attention_bias_idxs (host arithmetic, once per geometry).
    Entries outside [0, n_offsets) are refused here, before any kernel reads them."""
    import numpy as np
    if idx.dtype != torch.int64:
        raise NrvError(f"bias index (idx) must be int64, got {idx.dtype}")
    a = idx.detach().to("cpu").numpy()                    # numpy, not torch: nothing here is dispatched as a (capturable) op
    if a.ndim != 2:
        raise NrvError(f"bias index must be [Nq, Nk], got {a.shape}")
    if a.size and (int(a.min()) < 0 or int(a.max()) >= n_offsets):
        raise NrvError(f"bias index holds entries outside [0, {n_offsets})")
    flat = a.reshape(-1)
    order = np.argsort(flat, kind="stable").astype(np.int32)
    ptr = np.zeros(n_offsets + 1, dtype=np.int32)
    ptr[1:] = np.cumsum(np.bincount(flat, minlength=n_offsets))
    return BiasIndex(torch.from_numpy(a.astype(np.int32)).to(device), torch.from_numpy(ptr).to(device),
                     torch.from_numpy(order).to(device), int(n_offsets))


def _bias_attn_args(q: Tensor, k: Tensor, v: Tensor, hq: int, hk: int, hv: int, table: Tensor, index: BiasIndex,
                    B: int, H: int, Nq: int, Nk: int, kd: int, d: int, pre: str = "") -> Tuple[int, int, int]:
    """Row strides of the q / k / v views (or of the gradient views `pre` = "d"): head h's columns [h*step, h*step + width) must
    lie inside the view.  The table and the index belong to (H, Nq, Nk)."""
    if min(hq, hk, hv) < 0:
        raise NrvError(f"bias_attn: negative head steps ({hq}, {hk}, {hv})")
    lds = (_view2d(q, pre + "q", B * Nq, (H - 1) * hq + kd), _view2d(k, pre + "k", B * Nk, (H - 1) * hk + kd),
           _view2d(v, pre + "v", B * Nk, (H - 1) * hv + d))
    if pre:
        return lds
    _f32(table, "table")
    if tuple(table.shape) != (H, index.n_offsets) or not table.is_contiguous():
        raise NrvError(f"bias_attn: table must be contiguous [{H}, {index.n_offsets}], got {tuple(table.shape)}")
    for t, n, name in ((index.idx, Nq * Nk, "index.idx"), (index.inv_ptr, index.n_offsets + 1, "index.inv_ptr"),
                       (index.inv_pos, Nq * Nk, "index.inv_pos")):
        _dense(t, name, torch.int32, n, "Nq, Nk and the table")
    if tuple(index.idx.shape) != (Nq, Nk):
        raise NrvError(f"bias_attn: index.idx {tuple(index.idx.shape)} does not belong to ({Nq}, {Nk})")
    return lds


def bias_attn_fwd(q: Tensor, k: Tensor, v: Tensor, hq: int, hk: int, hv: int, table: Tensor, index: BiasIndex,
                  B: int, H: int, Nq: int, Nk: int, kd: int, d: int, robust: bool):
    """q / k / v: [B*Nq|Nk, *] bf16 views whose first column is head 0's q / k / v, heads hq / hk / hv columns apart
    (include/nrv.h nrv_bias_attn_fwd).  Returns (o bf16 [B*Nq, H*d], hardswish(o) bf16, stats fp32 [B*H, S])."""
    ldq, ldk, ldv = _bias_attn_args(q, k, v, hq, hk, hv, table, index, B, H, Nq, Nk, kd, d)
    lib = _lib.load()
    S = lib.nrv_bias_attn_stats_size(Nq, Nk, int(bool(robust)))
    o = torch.empty(B * Nq, H * d, dtype=torch.bfloat16, device=q.device)
    ao = torch.empty_like(o)
    stats = torch.empty(B * H, S, dtype=torch.float32, device=q.device)
    _run("bias_attn_fwd", 2.0 * B * H * Nq * Nk * (kd + d), 2 * (B * Nq * H * (kd + 2 * d) + B * Nk * H * (kd + d)),
         lambda: lib.nrv_bias_attn_fwd(q.data_ptr(), ldq, hq, k.data_ptr(), ldk, hk, v.data_ptr(), ldv, hv, table.data_ptr(),
                                       index.idx.data_ptr(), o.data_ptr(), ao.data_ptr(), stats.data_ptr(),
                                       B, H, Nq, Nk, kd, d, index.n_offsets, int(bool(robust)), _stream()),
         "nrv_bias_attn_fwd")
    return o, ao, stats


def bias_attn_bwd(q: Tensor, k: Tensor, v: Tensor, hq: int, hk: int, hv: int, table: Tensor, index: BiasIndex,
                  o: Tensor, dact: Tensor, stats: Tensor, dq: Tensor, dk: Tensor, dv: Tensor,
                  B: int, H: int, Nq: int, Nk: int, kd: int, d: int, robust: bool) -> Tensor:
    """Writes dq / dk / dv (views laid out like q / k / v) and returns dtable fp32 [H, n_offsets]; deterministic."""
    ldq, ldk, ldv = _bias_attn_args(q, k, v, hq, hk, hv, table, index, B, H, Nq, Nk, kd, d)
    if _bias_attn_args(dq, dk, dv, hq, hk, hv, table, index, B, H, Nq, Nk, kd, d, pre="d") != (ldq, ldk, ldv):
        raise NrvError("bias_attn_bwd: the gradients dq / dk / dv must be laid out (row strides) like q / k / v")
    for t, n in ((o, "o"), (dact, "dact")):
        _bf16(t, n)
        if tuple(t.shape) != (B * Nq, H * d) or not t.is_contiguous():
            raise NrvError(f"bias_attn_bwd: {n} must be contiguous [{B * Nq}, {H * d}]")
    lib = _lib.load()
    _dense(stats, "stats", torch.float32, B * H * lib.nrv_bias_attn_stats_size(Nq, Nk, int(bool(robust))), "the forward of this call")
    wsb = lib.nrv_bias_attn_bwd_workspace(B, H, index.n_offsets)
    ws = _workspace(wsb, q.device)
    dtable = torch.empty_like(table)
    _run("bias_attn_bwd", 4.0 * B * H * Nq * Nk * (kd + d), 4 * (B * Nq * H * (kd + 2 * d) + B * Nk * H * (kd + d)),
         lambda: lib.nrv_bias_attn_bwd(q.data_ptr(), ldq, hq, k.data_ptr(), ldk, hk, v.data_ptr(), ldv, hv, table.data_ptr(),
                                       index.idx.data_ptr(), index.inv_ptr.data_ptr(), index.inv_pos.data_ptr(),
                                       o.data_ptr(), dact.data_ptr(), stats.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                                       dtable.data_ptr(), ws.data_ptr(), wsb, B, H, Nq, Nk, kd, d, index.n_offsets,
                                       int(bool(robust)), _stream()),
         "nrv_bias_attn_bwd")
    return dtable


# ----------------------------------------------------------------------------------------------
# PatchConvNet (ABI 17): depthwise 3x3, squeeze-and-excitation, LayerScale residuals, class attention
# ----------------------------------------------------------------------------------------------
def _gelu_stream(g: Optional[Tensor], rows: int, C: int) -> Tuple[Optional[int], int]:
    """(pointer, dtype code) of a saved gelu' stream: bf16 [rows, C] (EPI_BIAS_GELU) or uint8 row pairs (EPI_BIAS_GELU_Q8)."""
    if g is None:
        return None, NRV_BF16
    _dev(g, "gelu_stream")
    if g.dtype == torch.uint8:
        if C % 64 or g.numel() < (rows + 1) // 2 * 2 * C or not g.is_contiguous():
            raise NrvError(f"gelu_stream: the 8-bit gelu' stream is contiguous and stored in row pairs, C % 64 == 0 and an even row "
                           f"count; got {tuple(g.shape)} stride {g.stride()} for [{rows}, {C}]")
        return g.data_ptr(), NRV_U8
    _bf16(g, "gelu_stream")
    if g.numel() != rows * C or not g.is_contiguous():
        raise NrvError(f"gelu_stream must be contiguous [{rows}, {C}], got {tuple(g.shape)} stride {g.stride()}")
    return g.data_ptr(), NRV_BF16


def _taps(w: Tensor, name: str, rows: int, cols: int, by: str = "the call's dimensions") -> Tensor:
    """A weight of rows * cols fp32 elements (Conv2d-shaped or flat) as a contiguous [rows, cols]; a strided one is copied."""
    _f32(w, name)
    if w.numel() != rows * cols:
        raise NrvError(f"{name} must hold {rows} x {cols} fp32 elements (by {by}), got {tuple(w.shape)}")
    return w.reshape(rows, cols).contiguous()


def _pcn_rows(a: Tensor, B: int, HW: int, C: int, name: str) -> None:
    _bf16(a, name)
    if not a.is_contiguous() or tuple(a.shape) != (B * HW, C):
        raise NrvError(f"{name} must be contiguous bf16 [{B * HW}, {C}], got {tuple(a.shape)}")


def dwconv3x3_fwd(a: Tensor, w: Tensor, bias: Tensor, B: int, H: int, W: int):
    """(d bf16 [B*H*W, C] = gelu(dwconv3x3(a) + bias), sq fp32 [B, C] = per-sample channel sums of d)."""
    C = a.shape[1]
    _pcn_rows(a, B, H * W, C, "a")
    w = _taps(w, "w", C, 9, "a"); _dense(bias, "bias", torch.float32, C, "a")
    d = torch.empty_like(a)
    sq = torch.empty(B, C, dtype=torch.float32, device=a.device)
    _run("dwconv3x3_fwd", 18.0 * a.numel(), 4 * a.numel(),
         lambda: _lib.load().nrv_dwconv3x3_fwd(a.data_ptr(), w.data_ptr(), bias.data_ptr(), d.data_ptr(), sq.data_ptr(), B, H, W, C,
                                               _stream()), "nrv_dwconv3x3_fwd")
    return d, sq


def dwconv3x3_bwd(a: Tensor, w: Tensor, bias: Tensor, dg: Tensor, s: Tensor, dmean: Tensor, B: int, H: int, W: int,
                  gelu_stream: Optional[Tensor] = None):
    """(da bf16 [B*H*W, C] (times gelu_stream when given), dw fp32 [C, 1, 3, 3], db fp32 [C])."""
    C = a.shape[1]
    _pcn_rows(a, B, H * W, C, "a"); _pcn_rows(dg, B, H * W, C, "dg")
    _dense(bias, "bias", torch.float32, C, "a"); _dense(s, "s", torch.float32, B * C, "B and a")
    _dense(dmean, "dmean", torch.float32, B * C, "B and a")
    gp, gdt = _gelu_stream(gelu_stream, B * H * W, C)
    w9 = _taps(w, "w", C, 9, "a")
    da = torch.empty_like(a)
    dw = torch.empty(C, 9, dtype=torch.float32, device=a.device)
    db = torch.empty(C, dtype=torch.float32, device=a.device)
    lib = _lib.load()
    ws = _workspace(lib.nrv_dwconv3x3_bwd_workspace(B, H, W, C), a.device)
    _run("dwconv3x3_bwd", 54.0 * a.numel(), 18 * a.numel(),
         lambda: lib.nrv_dwconv3x3_bwd(a.data_ptr(), w9.data_ptr(), bias.data_ptr(), dg.data_ptr(), s.data_ptr(), dmean.data_ptr(),
                                       gp, gdt, da.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), B, H, W, C,
                                       _stream()), "nrv_dwconv3x3_bwd")
    return da, dw.reshape(C, 1, 3, 3), db


def se_fwd(sq: Tensor, HW: int, wr: Tensor, br: Tensor, we: Tensor, be: Tensor):
    """(s fp32 [B, C] = sigmoid(W_e relu(W_r sq / HW + b_r) + b_e), hid fp32 [B, rd])."""
    _dense(sq, "sq", torch.float32, sq.numel())
    B, C = sq.shape
    rd = wr.shape[0]
    wr2, we2 = _taps(wr, "wr", rd, C, "sq"), _taps(we, "we", C, rd, "wr and sq")
    _dense(br, "br", torch.float32, rd, "wr"); _dense(be, "be", torch.float32, C, "sq")
    hid = torch.empty(B, rd, dtype=torch.float32, device=sq.device)
    s = torch.empty(B, C, dtype=torch.float32, device=sq.device)
    _run("se_fwd", 4.0 * B * C * rd, 8 * C * rd,
         lambda: _lib.load().nrv_se_fwd(sq.data_ptr(), int(HW), wr2.data_ptr(), br.data_ptr(), we2.data_ptr(), be.data_ptr(),
                                        hid.data_ptr(), s.data_ptr(), B, C, rd, _stream()), "nrv_se_fwd")
    return s, hid


def se_apply(d: Tensor, s: Tensor, HW: int) -> Tensor:
    """g bf16 = d * s[sample] (SqueezeExcite's x * gate)."""
    _dense(s, "s", torch.float32, s.numel())
    B, C = s.shape
    _pcn_rows(d, B, HW, C, "d")
    g = torch.empty_like(d)
    _run("se_apply", 0.0, 4 * d.numel(),
         lambda: _lib.load().nrv_se_apply(d.data_ptr(), s.data_ptr(), g.data_ptr(), B, int(HW), C, _stream()), "nrv_se_apply")
    return g


def se_bwd(dg: Tensor, d: Tensor, sq: Tensor, HW: int, s: Tensor, hid: Tensor, wr: Tensor, we: Tensor):
    """(dmean fp32 [B, C], dW_r, db_r, dW_e, db_e) with the weight gradients in the Conv2d shapes of wr / we."""
    _dense(s, "s", torch.float32, s.numel())
    B, C = s.shape
    rd = hid.shape[1]
    _pcn_rows(dg, B, HW, C, "dg"); _pcn_rows(d, B, HW, C, "d")
    _dense(sq, "sq", torch.float32, B * C, "s"); _dense(hid, "hid", torch.float32, B * rd, "s")
    wr2, we2 = _taps(wr, "wr", rd, C, "hid and s"), _taps(we, "we", C, rd, "hid and s")
    dev = d.device
    dmean = torch.empty(B, C, dtype=torch.float32, device=dev)
    dwr = torch.empty(rd, C, dtype=torch.float32, device=dev)
    dbr = torch.empty(rd, dtype=torch.float32, device=dev)
    dwe = torch.empty(C, rd, dtype=torch.float32, device=dev)
    dbe = torch.empty(C, dtype=torch.float32, device=dev)
    lib = _lib.load()
    ws = _workspace(lib.nrv_se_bwd_workspace(B, C, rd), dev)
    _run("se_bwd", 2.0 * d.numel(), 4 * d.numel(),
         lambda: lib.nrv_se_bwd(dg.data_ptr(), d.data_ptr(), sq.data_ptr(), int(HW), s.data_ptr(), hid.data_ptr(), wr2.data_ptr(),
                                we2.data_ptr(), dmean.data_ptr(), dwr.data_ptr(), dbr.data_ptr(), dwe.data_ptr(), dbe.data_ptr(),
                                ws.data_ptr(), ws.numel(), B, C, rd, _stream()), "nrv_se_bwd")
    return dmean, dwr.reshape(wr.shape), dbr, dwe.reshape(we.shape), dbe


def _ls_keep(keep: Optional[Tensor], rows: int) -> int:
    if keep is None:
        return 1
    _f32(keep, "keep")
    if keep.dim() != 1 or not keep.is_contiguous() or rows % keep.numel():
        raise NrvError(f"LayerScale drop path: keep must be one value per sample, {keep.numel()} does not divide {rows} rows")
    return rows // keep.numel()


def ls_add(x: Tensor, y: Tensor, gamma: Tensor, keep: Optional[Tensor] = None, survival: float = 1.0,
           out: Optional[Tensor] = None) -> Tensor:
    """out fp32 = x + f * gamma * y, f = keep[sample] / survival (or 1)."""
    _dense(x, "x", torch.float32, x.numel())
    rows, C = x.shape
    _dense(y, "y", torch.float32, rows * C, "x"); _dense(gamma, "gamma", torch.float32, C, "x")
    per = _ls_keep(keep, rows)
    o = torch.empty_like(x) if out is None else out
    if out is not None:
        _dense(out, "out", torch.float32, rows * C, "x")
    _run("ls_add", 0.0, 12 * x.numel(),
         lambda: _lib.load().nrv_ls_add_f32(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), _ptr(keep), float(survival), o.data_ptr(),
                                            rows, per, C, _stream()), "nrv_ls_add_f32")
    return o


def ls_bwd(dy: Tensor, y: Tensor, gamma: Tensor, keep: Optional[Tensor] = None, survival: float = 1.0):
    """(dz bf16 = dy * f * gamma, dgamma fp32 [C] = sum_rows dy * f * y)."""
    _dense(dy, "dy", torch.float32, dy.numel())
    rows, C = dy.shape
    _dense(y, "y", torch.float32, rows * C, "dy"); _dense(gamma, "gamma", torch.float32, C, "dy")
    per = _ls_keep(keep, rows)
    dz = torch.empty(rows, C, dtype=torch.bfloat16, device=dy.device)
    dgamma = torch.empty(C, dtype=torch.float32, device=dy.device)
    lib = _lib.load()
    ws = _workspace(lib.nrv_ls_bwd_workspace(rows, C), dy.device)
    _run("ls_bwd", 0.0, 10 * dy.numel(),
         lambda: lib.nrv_ls_bwd(dy.data_ptr(), y.data_ptr(), gamma.data_ptr(), _ptr(keep), float(survival), dz.data_ptr(),
                                dgamma.data_ptr(), ws.data_ptr(), ws.numel(), rows, per, C, _stream()), "nrv_ls_bwd")
    return dz, dgamma


def dgelu_rows(dx: Tensor, gelu_stream: Tensor) -> Tensor:
    """bf16(dx * gelu'), dx fp32 [rows, C], the stream as saved by EPI_BIAS_GELU (bf16) or EPI_BIAS_GELU_Q8 (uint8)."""
    _f32(dx, "dx")
    dx = dx.contiguous()
    rows, C = dx.shape
    gp, gdt = _gelu_stream(gelu_stream, rows, C)
    out = torch.empty(rows, C, dtype=torch.bfloat16, device=dx.device)
    _run("dgelu_rows", 0.0, 8 * dx.numel(),
         lambda: _lib.load().nrv_dgelu_rows(dx.data_ptr(), gp, gdt, out.data_ptr(), rows, C, _stream()), "nrv_dgelu_rows")
    return out


def _ca_view(t: Optional[Tensor], rows: int, width: int, name: str) -> int:
    if t is None:
        return 0
    _bf16(t, name)
    if t.dim() != 2 or t.stride(1) != 1 or t.shape[0] < rows or t.shape[1] < width or (t.shape[0] > 1 and t.stride(0) < width):
        raise NrvError(f"{name}: bf16 rows [>= {rows}, >= {width}] with contiguous columns, got {tuple(t.shape)} stride {t.stride()}")
    return t.stride(0)


def _cls_attn_args(q: Tensor, kc: Tensor, kp: Optional[Tensor], vc: Tensor, vp: Optional[Tensor], B: int, heads: int, Np: int, dh: int):
    if Np > 0 and (kp is None or vp is None):
        raise NrvError(f"cls_attn: {Np} patch keys need kp and vp")
    W = heads * dh
    return (_ca_view(q, B, W, "q"), _ca_view(kc, B, W, "kc"), _ca_view(vc, B, W, "vc"),
            _ca_view(kp, B * Np, W, "kp"), _ca_view(vp, B * Np, W, "vp"))


def cls_attn_fwd(q: Tensor, kc: Tensor, kp: Optional[Tensor], vc: Tensor, vp: Optional[Tensor], B: int, heads: int, Np: int,
                 dh: int, scale: float):
    """(o bf16 [B, heads*dh], lse fp32 [B*heads]): one query per sample against the class key and its Np patch keys."""
    lq, lkc, lvc, lkp, lvp = _cls_attn_args(q, kc, kp, vc, vp, B, heads, Np, dh)
    o = torch.empty(B, heads * dh, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(B * heads, dtype=torch.float32, device=q.device)
    _run("cls_attn_fwd", 4.0 * B * heads * (Np + 1) * dh, 4 * B * (Np + 1) * heads * dh,
         lambda: _lib.load().nrv_cls_attn_fwd(q.data_ptr(), lq, kc.data_ptr(), lkc, _ptr(kp), lkp, vc.data_ptr(), lvc, _ptr(vp), lvp,
                                              o.data_ptr(), o.stride(0), lse.data_ptr(), B, heads, Np, dh, float(scale), _stream()),
         "nrv_cls_attn_fwd")
    return o, lse


def cls_attn_bwd(q: Tensor, kc: Tensor, kp: Optional[Tensor], vc: Tensor, vp: Optional[Tensor], dout: Tensor, lse: Tensor,
                 B: int, heads: int, Np: int, dh: int, scale: float):
    """(dq, dkc, dkp, dvc, dvp), bf16, each shaped like its input."""
    lq, lkc, lvc, lkp, lvp = _cls_attn_args(q, kc, kp, vc, vp, B, heads, Np, dh)
    _ca_view(dout, B, heads * dh, "dout"); _dense(lse, "lse", torch.float32, B * heads, "B and heads")
    # the kernel writes each gradient with its input's leading dimension: same strides
    outs = [torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=t.device) if t is not None else None
            for t in (q, kc, kp, vc, vp)]
    dq, dkc, dkp, dvc, dvp = outs
    _run("cls_attn_bwd", 8.0 * B * heads * (Np + 1) * dh, 8 * B * (Np + 1) * heads * dh,
         lambda: _lib.load().nrv_cls_attn_bwd(q.data_ptr(), lq, kc.data_ptr(), lkc, _ptr(kp), lkp, vc.data_ptr(), lvc, _ptr(vp), lvp,
                                              dout.data_ptr(), dout.stride(0), lse.data_ptr(), dq.data_ptr(), dkc.data_ptr(),
                                              _ptr(dkp), dvc.data_ptr(), _ptr(dvp), B, heads, Np, dh, float(scale), _stream()),
         "nrv_cls_attn_bwd")
    return dq, dkc, dkp, dvc, dvp


# ---- talking-heads attention on materialised [B,H,Nq,Nk] matrices (CaiT, cait.py:107-120; include/nrv.h) ---------------
TH_MAX_HEADS, TH_MAX_KEYS = 16, 1025


def th_shape_ok(H: int, Nq: int, Nk: int) -> bool:
    """The range of the talking-heads kernels (include/nrv.h): 1 <= H <= 16, Nq >= 1, 1 <= Nk <= 1025."""
    return 1 <= H <= TH_MAX_HEADS and Nq >= 1 and 1 <= Nk <= TH_MAX_KEYS


def _th_args(t: Tensor, W: Tuple[Tensor, ...], name: str) -> Tuple[int, int, int, int]:
    _f32(t, name)
    if t.dim() != 4 or not t.is_contiguous():
        raise NrvError(f"{name} must be a contiguous fp32 [B, H, Nq, Nk] matrix, got {tuple(t.shape)}")
    B, H, Nq, Nk = t.shape
    for i, w in enumerate(W):
        wn = "W" if len(W) == 1 else f"W{i + 1}"
        _f32(w, wn)
        if tuple(w.shape) != (H, H) or not w.is_contiguous():
            raise NrvError(f"{wn}: the head-mixing matrix must be contiguous fp32 [{H}, {H}] (H by {name}), got {tuple(w.shape)} "
                           f"stride {w.stride()}")
    if not th_shape_ok(H, Nq, Nk):
        raise NotImplementedError(f"talking-heads kernels: {H} heads, {Nq} x {Nk} scores; they take at most {TH_MAX_HEADS} heads and "
                                  f"{TH_MAX_KEYS} keys")
    return B, H, Nq, Nk


def _th_like(t: Tensor, tname: str, other: Tensor, name: str) -> None:
    _f32(other, name)
    if other.shape != t.shape or not other.is_contiguous():
        raise NrvError(f"{name} must be contiguous fp32 of {tname}'s shape {tuple(t.shape)}, got {tuple(other.shape)} stride {other.stride()}")


def th_softmax_fwd(S: Tensor, W1: Tensor, W2: Tensor, a_dtype: torch.dtype = torch.bfloat16):
    """(P fp32, A): T = W1-mix of S, P = softmax(T, -1), A = W2-mix of P (cait.py:107-116)."""
    B, H, Nq, Nk = _th_args(S, (W1, W2), "S")
    P = torch.empty_like(S)
    A = torch.empty(S.shape, dtype=a_dtype, device=S.device)
    lib = _lib.load()
    _run("talking_heads_fwd", 2.0 * 2 * H * S.numel(), S.numel() * (8 + A.element_size()),
         lambda: lib.nrv_th_softmax_fwd(S.data_ptr(), W1.data_ptr(), W2.data_ptr(), P.data_ptr(), A.data_ptr(), _dt(A, "A"),
                                        B, H, Nq, Nk, _stream()), "nrv_th_softmax_fwd")
    return P, A


def th_softmax_bwd(dA: Tensor, P: Tensor, S: Tensor, W1: Tensor, W2: Tensor):
    """(dS fp32, dW1, dW2) of th_softmax_fwd from dA fp32 (= dO v^T)."""
    B, H, Nq, Nk = _th_args(S, (W1, W2), "S")
    _th_like(S, "S", dA, "dA"); _th_like(S, "S", P, "P")
    dS = torch.empty_like(S)
    dW1 = torch.empty(H, H, dtype=torch.float32, device=S.device)
    dW2 = torch.empty(H, H, dtype=torch.float32, device=S.device)
    lib = _lib.load()
    ws = _workspace(lib.nrv_th_softmax_bwd_workspace(B, H, Nq, Nk), S.device)
    _run("talking_heads_bwd", 2.0 * 4 * H * S.numel(), S.numel() * 16,
         lambda: lib.nrv_th_softmax_bwd(dA.data_ptr(), P.data_ptr(), S.data_ptr(), W1.data_ptr(), W2.data_ptr(), dS.data_ptr(),
                                        dW1.data_ptr(), dW2.data_ptr(), ws.data_ptr(), ws.numel(), B, H, Nq, Nk, _stream()),
         "nrv_th_softmax_bwd")
    return dS, dW1, dW2


def head_mix_fwd(x: Tensor, W: Tensor, out_dtype: torch.dtype = torch.float32) -> Tensor:
    """out[b,g] = sum_h W[h,g] x[b,h] (einsum 'b h i j, h g -> b g i j', cait.py:107-109, 114-116)."""
    B, H, Nq, Nk = _th_args(x, (W,), "x")
    out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    lib = _lib.load()
    _run("head_mix_fwd", 2.0 * H * x.numel(), x.numel() * (4 + out.element_size()),
         lambda: lib.nrv_head_mix_fwd(x.data_ptr(), W.data_ptr(), out.data_ptr(), _dt(out, "out"), B, H, Nq, Nk, _stream()),
         "nrv_head_mix_fwd")
    return out


def head_mix_bwd(dout: Tensor, x: Tensor, W: Tensor):
    """(din fp32, dW fp32 [H, H]) of head_mix_fwd."""
    B, H, Nq, Nk = _th_args(x, (W,), "x")
    _th_like(x, "x", dout, "dout")
    din = torch.empty_like(x)
    dW = torch.empty(H, H, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    ws = _workspace(lib.nrv_head_mix_bwd_workspace(B, H, Nq, Nk), x.device)
    _run("head_mix_bwd", 2.0 * 2 * H * x.numel(), x.numel() * 12,
         lambda: lib.nrv_head_mix_bwd(dout.data_ptr(), x.data_ptr(), W.data_ptr(), din.data_ptr(), dW.data_ptr(), ws.data_ptr(),
                                      ws.numel(), B, H, Nq, Nk, _stream()), "nrv_head_mix_bwd")
    return din, dW


# ---- re-attention on materialised [B,H,Nq,Nk] matrices (DeepViT, deepvit.py:47-53, 67-74; include/nrv.h) -----------------
def _ra_args(t: Tensor, W: Tensor, vecs: Tuple[Tensor, ...], eps: float, name: str) -> Tuple[int, int, int, int]:
    B, H, Nq, Nk = _th_args(t, (W,), name)
    for v, vn in zip(vecs, ("gamma", "beta")):
        _dense(v, vn, torch.float32, H, name)
    if not eps > 0:
        raise NotImplementedError(f"re-attention kernels: eps must be positive, got {eps}")
    return B, H, Nq, Nk


def _ra_grads(H: int, dev):
    return tuple(torch.empty(s, dtype=torch.float32, device=dev) for s in ((H, H), (H,), (H,)))


def reattn_softmax_fwd(S: Tensor, W: Tensor, gamma: Tensor, beta: Tensor, eps: float, a_dtype: torch.dtype = torch.bfloat16):
    """(P fp32, A): P = softmax(S, -1), M = W-mix of P, A = LayerNorm over the heads of M at every (i, j) (deepvit.py:67-74)."""
    B, H, Nq, Nk = _ra_args(S, W, (gamma, beta), eps, "S")
    P = torch.empty_like(S)
    A = torch.empty(S.shape, dtype=a_dtype, device=S.device)
    lib = _lib.load()
    _run("reattn_fwd", (2.0 * H + 8) * S.numel(), S.numel() * (8 + A.element_size()),
         lambda: lib.nrv_reattn_softmax_fwd(S.data_ptr(), W.data_ptr(), gamma.data_ptr(), beta.data_ptr(), P.data_ptr(), A.data_ptr(),
                                            _dt(A, "A"), B, H, Nq, Nk, float(eps), _stream()), "nrv_reattn_softmax_fwd")
    return P, A


def reattn_softmax_bwd(dA: Tensor, P: Tensor, W: Tensor, gamma: Tensor, eps: float):
    """(dS fp32, dW [H, H], dgamma [H], dbeta [H]) of reattn_softmax_fwd from dA fp32 (= dO v^T) and the kept P."""
    B, H, Nq, Nk = _ra_args(P, W, (gamma,), eps, "P")
    _th_like(P, "P", dA, "dA")
    dS = torch.empty_like(P)
    dW, dg, db = _ra_grads(H, P.device)
    lib = _lib.load()
    ws = _workspace(lib.nrv_reattn_softmax_bwd_workspace(B, H, Nq, Nk), P.device)
    _run("reattn_bwd", (2.0 * 3 * H + 16) * P.numel(), P.numel() * 12,
         lambda: lib.nrv_reattn_softmax_bwd(dA.data_ptr(), P.data_ptr(), W.data_ptr(), gamma.data_ptr(), dS.data_ptr(), dW.data_ptr(),
                                            dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), B, H, Nq, Nk, float(eps),
                                            _stream()), "nrv_reattn_softmax_bwd")
    return dS, dW, dg, db


def reattn_norm_fwd(P: Tensor, W: Tensor, gamma: Tensor, beta: Tensor, eps: float, a_dtype: torch.dtype = torch.bfloat16) -> Tensor:
    """A = LayerNorm over the heads of the W-mix of P, alone (robust=True: P comes from sinkhorn_fwd)."""
    B, H, Nq, Nk = _ra_args(P, W, (gamma, beta), eps, "P")
    A = torch.empty(P.shape, dtype=a_dtype, device=P.device)
    lib = _lib.load()
    _run("reattn_norm_fwd", (2.0 * H + 8) * P.numel(), P.numel() * (4 + A.element_size()),
         lambda: lib.nrv_reattn_norm_fwd(P.data_ptr(), W.data_ptr(), gamma.data_ptr(), beta.data_ptr(), A.data_ptr(), _dt(A, "A"),
                                         B, H, Nq, Nk, float(eps), _stream()), "nrv_reattn_norm_fwd")
    return A


def reattn_norm_bwd(dA: Tensor, P: Tensor, W: Tensor, gamma: Tensor, eps: float):
    """(dP fp32, dW [H, H], dgamma [H], dbeta [H]) of reattn_norm_fwd; dP goes to sinkhorn_bwd."""
    B, H, Nq, Nk = _ra_args(P, W, (gamma,), eps, "P")
    _th_like(P, "P", dA, "dA")
    dP = torch.empty_like(P)
    dW, dg, db = _ra_grads(H, P.device)
    lib = _lib.load()
    ws = _workspace(lib.nrv_reattn_norm_bwd_workspace(B, H, Nq, Nk), P.device)
    _run("reattn_norm_bwd", (2.0 * 3 * H + 16) * P.numel(), P.numel() * 12,
         lambda: lib.nrv_reattn_norm_bwd(dA.data_ptr(), P.data_ptr(), W.data_ptr(), gamma.data_ptr(), dP.data_ptr(), dW.data_ptr(),
                                         dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), B, H, Nq, Nk, float(eps),
                                         _stream()), "nrv_reattn_norm_bwd")
    return dP, dW, dg, db


# ----------------------------------------------------------------------------------------------
# tokens-to-token (t2t.py): soft split, LayerNorm over n of ld columns, wide-head streaming attention
# ----------------------------------------------------------------------------------------------
ATTN_WIDE_MAX_DH = 192           # include/nrv.h nrv_attn_wide_*: 128 < dh <= 192, dh % 8 == 0


def pad8(n: int) -> int:
    return (n + 7) // 8 * 8


def soft_split_fwd(src: Tensor, B: int, C: int, H: int, W: int, ks: int, stride: int, pad: int, rows: bool) -> Tensor:
    """nn.Unfold(ks, stride, pad) -> cols bf16 [B*Ho*Wo, pad8(ks*ks*C)], feature (c, ky, kx).  `rows`: src is bf16 token rows
    [B*H*W, ld >= C]; otherwise the NCHW image, fp32 | bf16."""
    _dev(src, "src")
    if rows:
        _bf16(src, "src")
        T, _, ld = _rows2d(src, "src")
        if T != B * H * W or src.shape[1] < C:
            raise NrvError(f"soft_split_fwd: src is {tuple(src.shape)}, expected [{B * H * W}, >= {C}]")
    else:
        ld = 0
        if not src.is_contiguous() or tuple(src.shape) != (B, C, H, W):
            raise NrvError(f"soft_split_fwd: src must be a contiguous [{B}, {C}, {H}, {W}] image")
    Ho, Wo = conv_out_size(H, ks, stride, pad), conv_out_size(W, ks, stride, pad)
    if Ho <= 0 or Wo <= 0:
        raise NrvError("soft_split_fwd: empty output grid")
    cols = torch.empty(B * Ho * Wo, pad8(ks * ks * C), dtype=torch.bfloat16, device=src.device)
    lib = _lib.load()
    _run("soft_split_fwd", 0.0, 4 * cols.numel(),
         lambda: lib.nrv_soft_split_fwd(src.data_ptr(), _dt(src, "src"), _lib.SPLIT_ROWS if rows else _lib.SPLIT_NCHW, ld, cols.data_ptr(),
                                        B, C, H, W, ks, stride, pad, _stream()),
         "nrv_soft_split_fwd")
    return cols


def soft_split_bwd(dcols: Tensor, B: int, C: int, H: int, W: int, ks: int, stride: int, pad: int, ld: Optional[int] = None) -> Tensor:
    """dx fp32 token rows [B*H*W, ld] (default pad8(C); columns >= C zero) of soft_split_fwd, from dcols bf16."""
    _bf16(dcols, "dcols")
    Ho, Wo = conv_out_size(H, ks, stride, pad), conv_out_size(W, ks, stride, pad)
    if not dcols.is_contiguous() or tuple(dcols.shape) != (B * Ho * Wo, pad8(ks * ks * C)):
        raise NrvError(f"soft_split_bwd: dcols is {tuple(dcols.shape)}, expected a contiguous [{B * Ho * Wo}, {pad8(ks * ks * C)}]")
    ld = pad8(C) if ld is None else ld
    dx = torch.empty(B * H * W, ld, dtype=torch.float32, device=dcols.device)
    lib = _lib.load()
    _run("soft_split_bwd", 0.0, 2 * dcols.numel() + 4 * dx.numel(),
         lambda: lib.nrv_soft_split_bwd(dcols.data_ptr(), dx.data_ptr(), ld, B, C, H, W, ks, stride, pad, _stream()),
         "nrv_soft_split_bwd")
    return dx


def layernorm_pad_fwd(x: Tensor, n: int, gamma: Tensor, beta: Tensor, eps: float):
    """x [rows, ld] fp32|bf16 with n true columns -> (y bf16 [rows, ld] with zero pad columns, mean, rstd)."""
    _dev(x, "x")
    rows, _, ld = _rows2d(x, "x")
    if x.shape[1] != ld or not 0 < n <= ld:
        raise NrvError(f"layernorm_pad_fwd: x must be dense [rows, ld] with n = {n} <= ld true columns, got {tuple(x.shape)} stride {x.stride()}")
    _dense(gamma, "gamma", torch.float32, n, "n"); _dense(beta, "beta", torch.float32, n, "n")
    y = torch.empty(rows, ld, dtype=torch.bfloat16, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    _run("layernorm_pad_fwd", 0.0, rows * ld * (x.element_size() + 2),
         lambda: lib.nrv_layernorm_pad_fwd(x.data_ptr(), _dt(x, "x"), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                           mean.data_ptr(), rstd.data_ptr(), rows, n, ld, float(eps), _stream()),
         "nrv_layernorm_pad_fwd")
    return y, mean, rstd


def layernorm_pad_bwd(dy: Tensor, x: Tensor, n: int, gamma: Tensor, mean: Tensor, rstd: Tensor, dres: Optional[Tensor] = None,
                      want_f32: bool = True, want_bf16: bool = False):
    """(dx_f32|None, dx_bf16|None, dgamma [n], dbeta [n]); dx = dres + LN'(dy) on the n true columns, zero pad columns."""
    _dev(x, "x")
    rows, _, ld = _rows2d(x, "x")
    if x.shape[1] != ld or not 0 < n <= ld:
        raise NrvError(f"layernorm_pad_bwd: x must be dense [rows, ld] with n = {n} <= ld true columns, got {tuple(x.shape)} stride {x.stride()}")
    _dense(dy, "dy", torch.bfloat16, rows * ld, "x"); _dense(gamma, "gamma", torch.float32, n, "n")
    _dense(mean, "mean", torch.float32, rows, "x"); _dense(rstd, "rstd", torch.float32, rows, "x")
    if dres is not None:
        _dense(dres, "dres", None, rows * ld, "x")
    if not (want_f32 or want_bf16):
        raise NrvError("layernorm_pad_bwd: nothing asked for")
    lib = _lib.load()
    dx32 = torch.empty(rows, ld, dtype=torch.float32, device=x.device) if want_f32 else None
    dx16 = torch.empty(rows, ld, dtype=torch.bfloat16, device=x.device) if want_bf16 else None
    dgamma = torch.empty(n, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(n, dtype=torch.float32, device=x.device)
    ws = _workspace(lib.nrv_layernorm_pad_bwd_workspace(rows, n), x.device)
    _run("layernorm_pad_bwd", 0.0, rows * ld * (2 * (2 + x.element_size()) + (dres.element_size() if dres is not None else 0) + 4),
         lambda: lib.nrv_layernorm_pad_bwd(dy.data_ptr(), x.data_ptr(), _dt(x, "x"), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                           _ptr(dres), _dt(dres, "dres") if dres is not None else 0, _ptr(dx32), _ptr(dx16),
                                           dgamma.data_ptr(), dbeta.data_ptr(), 0, ws.data_ptr(), ws.numel(), rows, n, ld, _stream()),
         "nrv_layernorm_pad_bwd")
    return dx32, dx16, dgamma, dbeta


def attn_wide_shape(dh: int) -> bool:
    return dh % 8 == 0 and 128 < dh <= ATTN_WIDE_MAX_DH


def attn_wide_fwd(qkv: Tensor, B: int, N: int, H: int, dh: int, scale: float):
    """qkv bf16 [B*N, 3*H*dh], 128 < dh <= 192 -> (out bf16 [B*N, H*dh], lse fp32 [B,H,N]); streaming softmax, no [N, N] matrix."""
    _bf16(qkv, "qkv")
    if not qkv.is_contiguous() or qkv.numel() != B * N * 3 * H * dh:
        raise NrvError("attn_wide_fwd: qkv must be contiguous [B*N, 3*H*dh]")
    out = torch.empty(B * N, H * dh, dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty(B, H, N, dtype=torch.float32, device=qkv.device)
    lib = _lib.load()
    _run("attn_wide_fwd", 4.0 * B * H * N * N * dh, 2 * B * N * H * dh * 4,
         lambda: lib.nrv_attn_wide_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, N, H, dh, float(scale), _stream()),
         "nrv_attn_wide_fwd")
    return out, lse


def attn_wide_bwd(qkv: Tensor, out: Tensor, dout: Tensor, lse: Tensor, B: int, N: int, H: int, dh: int, scale: float) -> Tensor:
    _attn_bwd_args(qkv, out, dout, lse, B, N, H, dh)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty(B * H * N, dtype=torch.float32, device=qkv.device)
    lib = _lib.load()
    _run("attn_wide_bwd", 10.0 * B * H * N * N * dh, 2 * B * N * H * dh * 8,
         lambda: lib.nrv_attn_wide_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                       delta.data_ptr(), B, N, H, dh, float(scale), _stream()),
         "nrv_attn_wide_bwd")
    return dqkv


# ----------------------------------------------------------------------------------------------
# RvT (ABI 18, added entry points): axial rotary embedding, plain depthwise ks x ks conv on rows with class rows, GEGLU
# ----------------------------------------------------------------------------------------------
def _rotary(fn: str, qkv: Tensor, sin: Tensor, cos: Tensor, B: int, N: int, lead: int, H: int, dh: int, name: str = "qkv") -> Tensor:
    _dense(qkv, name, torch.bfloat16, B * N * 3 * H * dh); _f32(sin, "sin"); _f32(cos, "cos")
    if sin.dim() != 2 or sin.shape != cos.shape or sin.shape[0] != N - lead or not (sin.is_contiguous() and cos.is_contiguous()):
        raise NrvError(f"{fn}: sin / cos must be contiguous fp32 [{N - lead}, dr / 2], got {tuple(sin.shape)} / {tuple(cos.shape)}")
    dr = 2 * sin.shape[1]
    lib = _lib.load()
    _run("rotary", 6.0 * B * (N - lead) * 2 * H * dr, 4.0 * B * (N - lead) * 2 * H * dr,
         lambda: getattr(lib, fn)(qkv.data_ptr(), sin.data_ptr(), cos.data_ptr(), B, N, lead, H, dh, dr, _stream()), fn)
    return qkv


def rotary_fwd(qkv: Tensor, sin: Tensor, cos: Tensor, B: int, N: int, lead: int, H: int, dh: int) -> Tensor:
    """In place on the packed qkv bf16 [B*N, 3*H*dh]: the first dr = 2 * sin.shape[1] features of q and k of every head are
    rotated on the rows t >= lead; class rows, features >= dr and v keep their bits (include/nrv.h nrv_rotary_fwd)."""
    return _rotary("nrv_rotary_fwd", qkv, sin, cos, B, N, lead, H, dh)


def rotary_bwd(dqkv: Tensor, sin: Tensor, cos: Tensor, B: int, N: int, lead: int, H: int, dh: int) -> Tensor:
    """The transposed rotation, in place on dqkv."""
    return _rotary("nrv_rotary_bwd", dqkv, sin, cos, B, N, lead, H, dh, "dqkv")


def _dwc_args(a: Tensor, w: Tensor, B: int, H: int, W: int, lead: int, name: str) -> Tuple[int, int, Tensor]:
    _bf16(a, name); _f32(w, "w")
    C = a.shape[-1]
    if a.dim() != 2 or not a.is_contiguous() or a.shape[0] != B * (lead + H * W):
        raise NrvError(f"{name} must be contiguous bf16 [{B * (lead + H * W)}, C], got {tuple(a.shape)}")
    if w.numel() % C:
        raise NrvError(f"w has {w.numel()} elements for {C} channels")
    kk = w.numel() // C
    ks = int(round(kk ** 0.5))
    if ks * ks != kk:
        raise NrvError(f"w must hold ks*ks taps per channel, got {kk}")
    return C, ks, w.reshape(C, kk).contiguous()


def dwconv_fwd(a: Tensor, w: Tensor, B: int, H: int, W: int, lead: int, out: Optional[Tensor] = None) -> Tensor:
    """Depthwise ks x ks (3 / 5 / 7, stride 1, zero padding, no bias) on rows [B*(lead + H*W), C]; w fp32 [C, 1, ks, ks] or
    [C, ks*ks].  The class rows of `out` are not written (a fresh `out` has zeros there)."""
    C, ks, w2 = _dwc_args(a, w, B, H, W, lead, "a")
    if out is None:
        out = torch.zeros_like(a) if lead else torch.empty_like(a)
    else:
        _bf16(out, "out")
        if out.shape != a.shape or not out.is_contiguous():
            raise NrvError("dwconv_fwd: out must be contiguous with a's shape")
    _run("dwconv_fwd", 2.0 * ks * ks * a.numel(), 4 * a.numel(),
         lambda: _lib.load().nrv_dwconv_fwd(a.data_ptr(), w2.data_ptr(), out.data_ptr(), B, H, W, lead, C, ks, _stream()), "nrv_dwconv_fwd")
    return out


def dwconv_bwd(a: Tensor, w: Tensor, dout: Tensor, B: int, H: int, W: int, lead: int, da: Optional[Tensor] = None,
               dw: Optional[Tensor] = None):
    """(da bf16 like a, class rows zero; dw fp32 of w's shape)."""
    C, ks, w2 = _dwc_args(a, w, B, H, W, lead, "a")
    _dwc_args(dout, w, B, H, W, lead, "dout")
    if dout.shape != a.shape:
        raise NrvError("dwconv_bwd: dout must have a's shape")
    if da is None:
        da = torch.empty_like(a)
    if dw is None:
        dw = torch.empty(C, ks * ks, dtype=torch.float32, device=a.device)
    _bf16(da, "da"); _f32(dw, "dw")
    if da.shape != a.shape or not da.is_contiguous() or dw.numel() != C * ks * ks or not dw.is_contiguous():
        raise NrvError("dwconv_bwd: da must be contiguous like a, dw contiguous with C*ks*ks elements")
    lib = _lib.load()
    ws = _workspace(lib.nrv_dwconv_bwd_workspace(B, H, W, C, ks), a.device)
    _run("dwconv_bwd", 4.0 * ks * ks * a.numel(), 8 * a.numel(),
         lambda: lib.nrv_dwconv_bwd(a.data_ptr(), w2.data_ptr(), dout.data_ptr(), da.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws.numel(),
                                    B, H, W, lead, C, ks, _stream()), "nrv_dwconv_bwd")
    return da, dw.reshape(w.shape)


def geglu_fwd(u: Tensor, hidden: int) -> Tensor:
    """h bf16 [rows, hidden] = u[:, :hidden] * gelu(u[:, hidden:2*hidden]); u bf16 with row stride >= 2 * hidden."""
    _bf16(u, "u")
    rows, cols, ld = _rows2d(u, "u")
    if cols < 2 * hidden:
        raise NrvError(f"geglu_fwd: u has {cols} columns, needs {2 * hidden}")
    h = torch.empty(rows, hidden, dtype=torch.bfloat16, device=u.device)
    _run("geglu_fwd", 0.0, 6 * rows * hidden,
         lambda: _lib.load().nrv_geglu_fwd(u.data_ptr(), ld, h.data_ptr(), rows, hidden, _stream()), "nrv_geglu_fwd")
    return h


def geglu_bwd(u: Tensor, dh: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """du bf16 [rows, 2*hidden] from dh bf16 [rows, hidden], gelu and gelu' recomputed from u."""
    _bf16(u, "u"); _bf16(dh, "dh")
    rows, cols, ld = _rows2d(u, "u")
    hidden = dh.shape[1]
    if not dh.is_contiguous() or dh.shape[0] != rows or cols < 2 * hidden:
        raise NrvError(f"geglu_bwd: dh must be contiguous [{rows}, hidden] with 2 * hidden <= {cols}")
    if out is None:
        out = torch.empty(rows, 2 * hidden, dtype=torch.bfloat16, device=u.device)
    _bf16(out, "out")
    if tuple(out.shape) != (rows, 2 * hidden) or not out.is_contiguous():
        raise NrvError("geglu_bwd: out must be contiguous [rows, 2 * hidden]")
    _run("geglu_bwd", 0.0, 10 * rows * hidden,
         lambda: _lib.load().nrv_geglu_bwd(u.data_ptr(), ld, dh.data_ptr(), out.data_ptr(), rows, hidden, _stream()), "nrv_geglu_bwd")
    return out


# ----------------------------------------------------------------------------------------------
# PiT (added to ABI 19): the Pool layer's stride-2 depthwise conv on the fp32 stream, nn.Unfold with overlapping patches
# ----------------------------------------------------------------------------------------------
def pool_out_size(n: int) -> int:
    return (n - 1) // 2 + 1


def _pool_args(x: Tensor, w: Tensor, B: int, H: int, W: int, lead: int, fn: str) -> Tuple[int, Tensor]:
    _f32(x, "x"); _f32(w, "w")
    if x.dim() != 2 or not x.is_contiguous() or x.shape[0] != B * (lead + H * W):
        raise NrvError(f"{fn}: x must be contiguous fp32 [{B * (lead + H * W)}, C], got {tuple(x.shape)}")
    C = x.shape[1]
    if w.numel() != 18 * C:
        raise NrvError(f"{fn}: w has {w.numel()} elements, expected [2C, 9] = {18 * C}")
    return C, w.reshape(2 * C, 9).contiguous()


def _out_buffer(t: Optional[Tensor], shape, dtype, device, name: str) -> Tensor:
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _dev(t, name)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise NrvError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t


def pool_dwconv_fwd(x: Tensor, w: Tensor, bias: Tensor, B: int, H: int, W: int, lead: int, out: Optional[Tensor] = None) -> Tensor:
    """Conv2d(C, 2C, 3, stride 2, padding 1, groups = C, bias) on the fp32 rows x [B*(lead + H*W), C] -> bf16 [B*Ho*Wo, 2C]
    without class rows; w fp32 [2C, 1, 3, 3] or [2C, 9], bias fp32 [2C] (include/nrv.h nrv_pool_dwconv_fwd)."""
    C, w2 = _pool_args(x, w, B, H, W, lead, "pool_dwconv_fwd")
    _f32(bias, "bias")
    if bias.numel() != 2 * C or not bias.is_contiguous():
        raise NrvError(f"pool_dwconv_fwd: bias must be contiguous [{2 * C}]")
    Ho, Wo = pool_out_size(H), pool_out_size(W)
    out = _out_buffer(out, (B * Ho * Wo, 2 * C), torch.bfloat16, x.device, "out")
    _run("pool_dwconv_fwd", 18.0 * out.numel(), 4 * x.numel() + 2 * out.numel(),
         lambda: _lib.load().nrv_pool_dwconv_fwd(x.data_ptr(), w2.data_ptr(), bias.data_ptr(), out.data_ptr(), B, H, W, lead, C, _stream()),
         "nrv_pool_dwconv_fwd")
    return out


def pool_dwconv_bwd(x: Tensor, w: Tensor, dout: Tensor, B: int, H: int, W: int, lead: int, dx: Optional[Tensor] = None,
                    dw: Optional[Tensor] = None, dbias: Optional[Tensor] = None):
    """(dx fp32 like x with zero class rows, dw fp32 of w's shape, dbias fp32 [2C]) from dout bf16 [B*Ho*Wo, 2C]."""
    C, w2 = _pool_args(x, w, B, H, W, lead, "pool_dwconv_bwd")
    _bf16(dout, "dout")
    Ho, Wo = pool_out_size(H), pool_out_size(W)
    if not dout.is_contiguous() or tuple(dout.shape) != (B * Ho * Wo, 2 * C):
        raise NrvError(f"pool_dwconv_bwd: dout is {tuple(dout.shape)}, expected a contiguous [{B * Ho * Wo}, {2 * C}]")
    dx = _out_buffer(dx, x.shape, torch.float32, x.device, "dx")
    dw = _out_buffer(dw, (2 * C, 9), torch.float32, x.device, "dw")
    db = _out_buffer(dbias, (2 * C,), torch.float32, x.device, "dbias")
    lib = _lib.load()
    ws = _workspace(lib.nrv_pool_dwconv_bwd_workspace(B, H, W, C), x.device)
    _run("pool_dwconv_bwd", 54.0 * dout.numel(), 8 * x.numel() + 4 * dout.numel(),
         lambda: lib.nrv_pool_dwconv_bwd(x.data_ptr(), w2.data_ptr(), dout.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                         ws.data_ptr(), ws.numel(), B, H, W, lead, C, _stream()), "nrv_pool_dwconv_bwd")
    return dx, dw.reshape(w.shape), db


def unfold_patches(img: Tensor, ks: int, stride: int, out: Optional[Tensor] = None) -> Tensor:
    """nn.Unfold(ks, stride) on a contiguous NCHW image (fp32 | bf16), 1 <= stride <= ks <= 32 -> cols bf16
    [B*Ho*Wo, pad8(ks*ks*C)], feature (c, ky, kx), zero pad columns."""
    _dev(img, "img")
    if img.dim() != 4 or not img.is_contiguous():
        raise NrvError("unfold_patches: img must be a contiguous [B, C, H, W] image")
    B, C, H, W = img.shape
    if not 1 <= stride <= ks or H < ks or W < ks:
        raise NrvError(f"unfold_patches: kernel {ks}, stride {stride} on a {H} x {W} image")
    Ho, Wo = (H - ks) // stride + 1, (W - ks) // stride + 1
    cols = _out_buffer(out, (B * Ho * Wo, pad8(ks * ks * C)), torch.bfloat16, img.device, "out")
    _run("unfold_patches", 0.0, 4 * cols.numel(),
         lambda: _lib.load().nrv_unfold_patches(img.data_ptr(), _dt(img, "img"), cols.data_ptr(), B, C, H, W, ks, stride, _stream()),
         "nrv_unfold_patches")
    return cols


# ----------------------------------------------------------------------------------------------
# CCT (added to ABI 19): ReLU + max pool on conv rows, LayerNorm on the fp32 stream, sequence pooling
# ----------------------------------------------------------------------------------------------
def maxpool_out_size(n: int, pk: int, ps: int, pp: int) -> int:
    return (n + 2 * pp - pk) // ps + 1


def _maxpool_geom(fn: str, B: int, H: int, W: int, pk: int, ps: int, pp: int) -> Tuple[int, int]:
    if pk not in (2, 3) or not 1 <= ps <= pk or not 0 <= pp <= pk // 2 or min(B, H, W) < 1 or H + 2 * pp < pk or W + 2 * pp < pk:
        raise NrvError(f"{fn}: pooling ({pk}, {ps}, {pp}) on a {H} x {W} plane: kernel 2 or 3, 1 <= stride <= kernel, padding <= kernel // 2")
    return maxpool_out_size(H, pk, ps, pp), maxpool_out_size(W, pk, ps, pp)


def relu_maxpool_fwd(y: Tensor, B: int, H: int, W: int, pk: int, ps: int, pp: int, relu: bool = True, want_f32: bool = True,
                     want_bf16: bool = False, out_f32: Optional[Tensor] = None, out_bf16: Optional[Tensor] = None,
                     idx: Optional[Tensor] = None):
    """MaxPool2d(pk, ps, pp) of (ReLU of) the NHWC rows y [B*H*W, C] (fp32 | bf16) -> (out fp32 | None, out bf16 | None,
    idx uint8), each [B*Ho*Wo, C] (include/nrv.h nrv_relu_maxpool_fwd)."""
    _dev(y, "y")
    Ho, Wo = _maxpool_geom("relu_maxpool_fwd", B, H, W, pk, ps, pp)
    if y.dim() != 2 or not y.is_contiguous() or y.shape[0] != B * H * W or y.shape[1] % 8:
        raise NrvError(f"relu_maxpool_fwd: y must be contiguous [{B * H * W}, C] with C % 8 == 0, got {tuple(y.shape)}")
    C = y.shape[1]
    if not (want_f32 or want_bf16 or out_f32 is not None or out_bf16 is not None):
        raise NrvError("relu_maxpool_fwd: at least one of the fp32 and the bf16 output")
    shape = (B * Ho * Wo, C)
    o32 = _out_buffer(out_f32, shape, torch.float32, y.device, "out_f32") if (want_f32 or out_f32 is not None) else None
    o16 = _out_buffer(out_bf16, shape, torch.bfloat16, y.device, "out_bf16") if (want_bf16 or out_bf16 is not None) else None
    ix = _out_buffer(idx, shape, torch.uint8, y.device, "idx")
    nb = y.numel() * y.element_size() + ix.numel() * (1 + (4 if o32 is not None else 0) + (2 if o16 is not None else 0))
    _run("relu_maxpool_fwd", 0.0, nb,
         lambda: _lib.load().nrv_relu_maxpool_fwd(y.data_ptr(), _dt(y, "y"), int(bool(relu)), _ptr(o32), _ptr(o16), ix.data_ptr(), B, H, W, C,
                                                  pk, ps, pp, _stream()), "nrv_relu_maxpool_fwd")
    return o32, o16, ix


def relu_maxpool_bwd(dout: Tensor, idx: Tensor, B: int, H: int, W: int, pk: int, ps: int, pp: int, dy: Optional[Tensor] = None) -> Tensor:
    """dy bf16 [B*H*W, C] from dout fp32 [B*Ho*Wo, C] and the forward's idx (include/nrv.h nrv_relu_maxpool_bwd)."""
    _f32(dout, "dout"); _dev(idx, "idx")
    Ho, Wo = _maxpool_geom("relu_maxpool_bwd", B, H, W, pk, ps, pp)
    if dout.dim() != 2 or not dout.is_contiguous() or dout.shape[0] != B * Ho * Wo or dout.shape[1] % 8:
        raise NrvError(f"relu_maxpool_bwd: dout must be contiguous [{B * Ho * Wo}, C] with C % 8 == 0, got {tuple(dout.shape)}")
    if idx.dtype != torch.uint8 or idx.shape != dout.shape or not idx.is_contiguous():
        raise NrvError("relu_maxpool_bwd: idx must be the forward's contiguous uint8 tensor of dout's shape")
    C = dout.shape[1]
    dy = _out_buffer(dy, (B * H * W, C), torch.bfloat16, dout.device, "dy")
    _run("relu_maxpool_bwd", 0.0, dout.numel() * 5 + dy.numel() * 2,
         lambda: _lib.load().nrv_relu_maxpool_bwd(dout.data_ptr(), idx.data_ptr(), dy.data_ptr(), B, H, W, C, pk, ps, pp, _stream()),
         "nrv_relu_maxpool_bwd")
    return dy


def _lnf_args(fn: str, x: Tensor, gamma: Tensor, beta: Optional[Tensor]) -> Tuple[int, int]:
    _f32(x, "x"); _f32(gamma, "gamma")
    if x.dim() != 2 or not x.is_contiguous() or x.shape[0] < 1 or x.shape[1] % 8 or not 8 <= x.shape[1] <= 4096:
        raise NrvError(f"{fn}: x must be contiguous fp32 [rows, dim] with dim % 8 == 0 and dim <= 4096, got {tuple(x.shape)}")
    for t, n in ((gamma, "gamma"), (beta, "beta")):
        if t is not None:
            _f32(t, n)
            if t.numel() != x.shape[1] or not t.is_contiguous():
                raise NrvError(f"{fn}: {n} must hold {x.shape[1]} contiguous floats")
    return x.shape[0], x.shape[1]


def layernorm_f32_fwd(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, want_bf16: bool = False, y: Optional[Tensor] = None,
                      y_bf16: Optional[Tensor] = None):
    """nn.LayerNorm with the fp32 stream on both sides: x fp32 [rows, dim] -> (y fp32, y bf16 | None, mean, rstd)
    (include/nrv.h nrv_layernorm_f32_fwd)."""
    rows, dim = _lnf_args("layernorm_f32_fwd", x, gamma, beta)
    y = _out_buffer(y, (rows, dim), torch.float32, x.device, "y")
    y16 = _out_buffer(y_bf16, (rows, dim), torch.bfloat16, x.device, "y_bf16") if (want_bf16 or y_bf16 is not None) else None
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    _run("layernorm_f32_fwd", 0.0, rows * dim * (8 + (2 if y16 is not None else 0)),
         lambda: _lib.load().nrv_layernorm_f32_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), _ptr(y16), mean.data_ptr(),
                                                   rstd.data_ptr(), rows, dim, float(eps), _stream()), "nrv_layernorm_f32_fwd")
    return y, y16, mean, rstd


def layernorm_f32_bwd(dy: Tensor, x: Tensor, gamma: Tensor, mean: Tensor, rstd: Tensor, want_bf16: bool = False,
                      dx: Optional[Tensor] = None, dx_bf16: Optional[Tensor] = None):
    """(dx fp32, dx bf16 | None, dgamma, dbeta) from an fp32 dy (include/nrv.h nrv_layernorm_f32_bwd)."""
    rows, dim = _lnf_args("layernorm_f32_bwd", x, gamma, None)
    _dense(dy, "dy", torch.float32, rows * dim, "x"); _dense(mean, "mean", torch.float32, rows, "x")
    _dense(rstd, "rstd", torch.float32, rows, "x")
    dx = _out_buffer(dx, (rows, dim), torch.float32, x.device, "dx")
    dx16 = _out_buffer(dx_bf16, (rows, dim), torch.bfloat16, x.device, "dx_bf16") if (want_bf16 or dx_bf16 is not None) else None
    dg = torch.empty(dim, dtype=torch.float32, device=x.device)
    db = torch.empty(dim, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    ws = _workspace(lib.nrv_layernorm_f32_bwd_workspace(rows, dim), x.device)
    _run("layernorm_f32_bwd", 0.0, rows * dim * (12 + (2 if dx16 is not None else 0)),
         lambda: lib.nrv_layernorm_f32_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                           _ptr(dx16), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), rows, dim, _stream()),
         "nrv_layernorm_f32_bwd")
    return dx, dx16, dg, db


def _seqpool_args(fn: str, y: Tensor, a: Tensor, B: int, n: int) -> int:
    _f32(y, "y"); _f32(a, "a")
    if y.dim() != 2 or not y.is_contiguous() or B < 1 or not 1 <= n <= 4096 or y.shape[0] != B * n or y.shape[1] % 8 or not 8 <= y.shape[1] <= 4096:
        raise NrvError(f"{fn}: y must be contiguous fp32 [B*n, D] with 1 <= n <= 4096, D % 8 == 0 and D <= 4096, got {tuple(y.shape)} "
                       f"for B {B}, n {n}")
    if a.numel() != y.shape[1] or not a.is_contiguous():
        raise NrvError(f"{fn}: a must hold {y.shape[1]} contiguous floats")
    return y.shape[1]


def seqpool_fwd(y: Tensor, a: Tensor, bias: Tensor, B: int, n: int, w: Optional[Tensor] = None, out: Optional[Tensor] = None):
    """(w fp32 [B, n], out fp32 [B, D]): w = softmax_n(y a + bias), out = sum_n w_n y_n (include/nrv.h nrv_seqpool_fwd);
    bias is a one-element device tensor."""
    D = _seqpool_args("seqpool_fwd", y, a, B, n)
    _f32(bias, "bias")
    if bias.numel() != 1:
        raise NrvError("seqpool_fwd: bias holds one float")
    w = _out_buffer(w, (B, n), torch.float32, y.device, "w")
    out = _out_buffer(out, (B, D), torch.float32, y.device, "out")
    _run("seqpool_fwd", 4.0 * y.numel(), 8 * y.numel(),
         lambda: _lib.load().nrv_seqpool_fwd(y.data_ptr(), a.data_ptr(), bias.data_ptr(), w.data_ptr(), out.data_ptr(), B, n, D, _stream()),
         "nrv_seqpool_fwd")
    return w, out


def seqpool_bwd(dout: Tensor, y: Tensor, a: Tensor, w: Tensor, B: int, n: int, dy: Optional[Tensor] = None):
    """(dy fp32 like y, da fp32 [D], dbias fp32 [1]) from dout fp32 [B, D] (include/nrv.h nrv_seqpool_bwd)."""
    D = _seqpool_args("seqpool_bwd", y, a, B, n)
    _f32(dout, "dout"); _f32(w, "w")
    if tuple(dout.shape) != (B, D) or not dout.is_contiguous() or tuple(w.shape) != (B, n) or not w.is_contiguous():
        raise NrvError(f"seqpool_bwd: dout must be contiguous [{B}, {D}] and w [{B}, {n}]")
    dy = _out_buffer(dy, y.shape, torch.float32, y.device, "dy")
    da = torch.empty(D, dtype=torch.float32, device=y.device)
    db = torch.empty(1, dtype=torch.float32, device=y.device)
    lib = _lib.load()
    ws = _workspace(lib.nrv_seqpool_bwd_workspace(B, D), y.device)
    _run("seqpool_bwd", 8.0 * y.numel(), 12 * y.numel(),
         lambda: lib.nrv_seqpool_bwd(dout.data_ptr(), y.data_ptr(), a.data_ptr(), w.data_ptr(), dy.data_ptr(), da.data_ptr(), db.data_ptr(),
                                     ws.data_ptr(), ws.numel(), B, n, D, _stream()), "nrv_seqpool_bwd")
    return dy, da, db


# ----------------------------------------------------------------------------------------------
# Twins-SVT (added to ABI 19): sub-sampled global attention with K and V on chip, PEG on the fp32 stream
# ----------------------------------------------------------------------------------------------
SUBATTN_MAX_NK = 128             # include/nrv.h nrv_subattn_*: 1 <= Nk <= 128, dh in {32, 64}


def subattn_plan(Nq: int, Nk: int, dh: int) -> dict:
    """How subattn_fwd / _bwd split this shape (include/nrv.h nrv_subattn_plan): query rows per workgroup, chunks per head and
    the keys staged on chip.  Read-only; needs no GPU.  Raises NrvError where the launch would refuse the shape."""
    pl = _lib.SubattnPlan()
    check(_lib.load().nrv_subattn_plan(int(Nq), int(Nk), int(dh), ctypes.addressof(pl)), "nrv_subattn_plan")
    return {"chunk": pl.chunk, "chunks": pl.chunks, "nk_pad": pl.nk_pad}


def _sub_view(t: Tensor, rows: int, width: int, name: str) -> int:
    _bf16(t, name)
    if t.dim() != 2 or t.stride(1) != 1 or t.shape[0] != rows or t.shape[1] < width:
        raise NrvError(f"subattn: {name} must be a row-major bf16 [{rows}, >= {width}] view, got {tuple(t.shape)} stride {t.stride()}")
    return t.stride(0) if rows > 1 else max(t.stride(0), width)


def _sub_args(q: Tensor, k: Tensor, v: Tensor, B: int, H: int, Nq: int, Nk: int, dh: int) -> Tuple[int, int, int]:
    if dh not in (32, 64) or not 1 <= Nk <= SUBATTN_MAX_NK or Nq < 1 or B < 1 or H < 1:
        raise NrvError(f"subattn: dh {dh} must be 32 or 64, 1 <= Nk <= {SUBATTN_MAX_NK} (got {Nk}), Nq {Nq} >= 1")
    return _sub_view(q, B * Nq, H * dh, "q"), _sub_view(k, B * Nk, H * dh, "k"), _sub_view(v, B * Nk, H * dh, "v")


def subattn_fwd(q: Tensor, k: Tensor, v: Tensor, B: int, H: int, Nq: int, Nk: int, dh: int, scale: float,
                out: Optional[Tensor] = None, lse: Optional[Tensor] = None):
    """softmax(scale q k^T) v with the head's K and V on chip (include/nrv.h nrv_subattn_fwd).  q / k / v: bf16 views [B*Nq|Nk, *]
    whose first column is head 0, head h at column h*dh (column blocks of wider buffers work).  Returns (out bf16 [B*Nq, H*dh],
    lse fp32 [B, H, Nq])."""
    ldq, ldk, ldv = _sub_args(q, k, v, B, H, Nq, Nk, dh)
    out = _out_buffer(out, (B * Nq, H * dh), torch.bfloat16, q.device, "out")
    lse = _out_buffer(lse, (B, H, Nq), torch.float32, q.device, "lse")
    _run("subattn_fwd", 4.0 * B * H * Nq * Nk * dh, 2.0 * H * dh * (2 * B * Nq + 2 * B * Nk) + 4.0 * B * H * Nq,
         lambda: _lib.load().nrv_subattn_fwd(q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldv, out.data_ptr(), lse.data_ptr(),
                                             B, H, Nq, Nk, dh, float(scale), _stream()),
         "nrv_subattn_fwd")
    return out, lse


def subattn_bwd(q: Tensor, k: Tensor, v: Tensor, dout: Tensor, lse: Tensor, B: int, H: int, Nq: int, Nk: int, dh: int, scale: float,
                dq: Optional[Tensor] = None, dk: Optional[Tensor] = None, dv: Optional[Tensor] = None):
    """(dq, dk, dv) bf16, laid out like q / k / v (given: views with the same row stride; else fresh [rows, H*dh] tensors with the
    layout of contiguous q / k / v).  Takes lse, not out; deterministic (include/nrv.h nrv_subattn_bwd)."""
    ldq, ldk, ldv = _sub_args(q, k, v, B, H, Nq, Nk, dh)
    _bf16(dout, "dout"); _f32(lse, "lse")
    if tuple(dout.shape) != (B * Nq, H * dh) or not dout.is_contiguous():
        raise NrvError(f"subattn_bwd: dout must be contiguous [{B * Nq}, {H * dh}], got {tuple(dout.shape)}")
    if tuple(lse.shape) != (B, H, Nq) or not lse.is_contiguous():
        raise NrvError(f"subattn_bwd: lse {tuple(lse.shape)} does not belong to this call")
    grads = []
    for g, like, rows, ld, name in ((dq, q, B * Nq, ldq, "dq"), (dk, k, B * Nk, ldk, "dk"), (dv, v, B * Nk, ldv, "dv")):
        if g is None:
            if ld != H * dh:
                raise NrvError(f"subattn_bwd: {name[1]} is a view with row stride {ld}; pass {name} as a view of the same layout")
            g = torch.empty(rows, H * dh, dtype=torch.bfloat16, device=q.device)
        elif _sub_view(g, rows, H * dh, name) != ld:
            raise NrvError(f"subattn_bwd: {name} must be laid out like {name[1]} (row stride {ld})")
        grads.append(g)
    dq, dk, dv = grads
    lib = _lib.load()
    wsb = lib.nrv_subattn_bwd_workspace(B, H, Nq, Nk, dh)
    ws = _workspace(wsb, q.device)
    _run("subattn_bwd", 10.0 * B * H * Nq * Nk * dh, 2.0 * H * dh * (4 * B * Nq + 4 * B * Nk) + 4.0 * B * H * Nq + 2.0 * wsb,
         lambda: lib.nrv_subattn_bwd(q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldv, dout.data_ptr(), lse.data_ptr(),
                                     dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr(), ws.numel(), B, H, Nq, Nk, dh,
                                     float(scale), _stream()),
         "nrv_subattn_bwd")
    return dq, dk, dv


def _peg_args(x: Tensor, w: Tensor, B: int, H: int, W: int, fn: str) -> Tuple[int, int, Tensor]:
    _f32(x, "x"); _f32(w, "w")
    if x.dim() != 2 or not x.is_contiguous() or x.shape[0] != B * H * W or x.shape[1] % 8:
        raise NrvError(f"{fn}: x must be contiguous fp32 [{B * H * W}, C] with C % 8 == 0, got {tuple(x.shape)}")
    C = x.shape[1]
    if w.numel() % C:
        raise NrvError(f"{fn}: w has {w.numel()} elements for {C} channels")
    kk = w.numel() // C
    ks = int(round(kk ** 0.5))
    if ks * ks != kk or ks not in (3, 5, 7):
        raise NrvError(f"{fn}: w must hold ks*ks taps per channel with ks in (3, 5, 7), got {kk}")
    return C, ks, w.reshape(C, kk).contiguous()


def peg_fwd(x: Tensor, w: Tensor, bias: Tensor, B: int, H: int, W: int, out: Optional[Tensor] = None) -> Tensor:
    """out fp32 = x + bias + depthwise ks x ks conv(x) (stride 1, zero padding ks / 2) on the fp32 rows x [B*H*W, C]; w fp32
    [C, 1, ks, ks] or [C, ks*ks], bias fp32 [C] (include/nrv.h nrv_peg_fwd)."""
    C, ks, w2 = _peg_args(x, w, B, H, W, "peg_fwd")
    _f32(bias, "bias")
    if bias.numel() != C or not bias.is_contiguous():
        raise NrvError(f"peg_fwd: bias must be contiguous [{C}]")
    out = _out_buffer(out, x.shape, torch.float32, x.device, "out")
    _run("peg_fwd", 2.0 * ks * ks * x.numel(), 8 * x.numel(),
         lambda: _lib.load().nrv_peg_fwd(x.data_ptr(), w2.data_ptr(), bias.data_ptr(), out.data_ptr(), B, H, W, C, ks, _stream()),
         "nrv_peg_fwd")
    return out


def peg_bwd(x: Tensor, w: Tensor, dy: Tensor, B: int, H: int, W: int, dx: Optional[Tensor] = None, dw: Optional[Tensor] = None,
            dbias: Optional[Tensor] = None):
    """(dx fp32 like x, dw fp32 of w's shape, dbias fp32 [C]) from dy fp32 like x (include/nrv.h nrv_peg_bwd)."""
    C, ks, w2 = _peg_args(x, w, B, H, W, "peg_bwd")
    _f32(dy, "dy")
    if dy.shape != x.shape or not dy.is_contiguous():
        raise NrvError(f"peg_bwd: dy must be contiguous with x's shape {tuple(x.shape)}, got {tuple(dy.shape)}")
    dx = _out_buffer(dx, x.shape, torch.float32, x.device, "dx")
    dw = _out_buffer(dw, (C, ks * ks), torch.float32, x.device, "dw")
    db = _out_buffer(dbias, (C,), torch.float32, x.device, "dbias")
    lib = _lib.load()
    ws = _workspace(lib.nrv_peg_bwd_workspace(B, H, W, C, ks), x.device)
    _run("peg_bwd", 4.0 * ks * ks * x.numel(), 16 * x.numel(),
         lambda: lib.nrv_peg_bwd(x.data_ptr(), w2.data_ptr(), dy.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                 ws.numel(), B, H, W, C, ks, _stream()), "nrv_peg_bwd")
    return dx, dw.reshape(w.shape), db
