"""The layer between tensors and the C ABI: what noise_robust_vit_amd/kernels.py lets through to a launch.

The C side sees addresses and integers; how large a tensor really is, what it holds and how it is strided is known to the wrapper
alone.  This module calls every wrapper once with tensors of exactly the documented size (CASES), then again with one tensor argument
changed at a time (`mutations`), against a stand-in library that records the C calls instead of launching them (`StandIn`).  A
changed tensor must be refused by the wrapper, by name, or change what is launched in the way its rule allows (`audit`); a launch
that equals the canonical one was not checked by anybody.

Nothing here touches a device: the tensors are CPU tensors that claim `is_cuda` (port_checks.fake_cuda), the stream is a
constant, and the entries that answer without a device (sizes, plans, thresholds) go to the built library.  The mutated calls
must never meet a real library -- a missing check would be an out-of-bounds access there.  test_launch_audit_gpu.py runs only
the column-block form of the (wrapper, argument) pairs that `audit` classifies as accepted.
"""
import dataclasses
import inspect
import re
from ctypes import c_int, c_void_p

import torch

from noise_robust_vit_amd import _lib
from noise_robust_vit_amd import kernels as K
from noise_robust_vit_amd._lib import NrvError
from port_checks import fake_cuda

STREAM = 0x5EED0
HOST_ENTRIES = ("nrv_error_string", "nrv_abi_version", "nrv_set_reserved_cus", "nrv_bias_attn_stats_size")
DTYPE_CODES = (_lib.NRV_F32, _lib.NRV_BF16, _lib.NRV_U8)
PAD = 8                        # the column-block form: columns [PAD, PAD + cols) of a buffer 2 * PAD columns wider


def needs_no_device(name):
    return name in HOST_ENTRIES or name.endswith(("_workspace", "_plan", "_threshold"))


class StandIn:
    """The library as kernels.py sees it: launching entries answer 0 and are recorded, the rest go to the built library."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        if name not in _lib.SIGNATURES:
            raise AttributeError(name)
        if needs_no_device(name):
            return getattr(self._real, name)

        def launch(*args):
            assert len(args) == len(_lib.SIGNATURES[name][1]), (name, len(args))
            self.calls.append((name, args))
            return 0
        return launch


def install(monkeypatch):
    """Put a StandIn in place of the loaded library and a constant in place of the current stream, for one test."""
    lib = StandIn(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(K, "_stream", lambda: STREAM)
    return lib


# ---- one call, reduced to what the C side is told ---------------------------------------------------
@dataclasses.dataclass
class Outcome:
    refusal: str = None            # the NrvError's text
    crash: BaseException = None    # any other exception
    launches: tuple = ()           # ((name, args), ...)
    result: object = None

    @property
    def scalars(self):
        """[(name, non-pointer args with None at the pointer positions)]: what is compared between two calls."""
        return [(n, tuple(None if ty is c_void_p else a for ty, a in zip(_lib.SIGNATURES[n][1], args))) for n, args in self.launches]

    def pointers(self):
        return [a for n, args in self.launches for ty, a in zip(_lib.SIGNATURES[n][1], args) if ty is c_void_p and a]

    def shape_of_result(self):
        """Of a wrapper that launches nothing (host arithmetic): the shapes and dtypes it hands back."""
        return [(tuple(t.shape), t.dtype) for _, t in leaves({"result": self.result})]


def _children(v):
    if dataclasses.is_dataclass(v):
        return [(f.name, getattr(v, f.name)) for f in dataclasses.fields(v)]
    if isinstance(v, (tuple, list)):
        return list(enumerate(v))
    return []


def leaves(kwargs):
    """(path, tensor) for every tensor among the arguments; path = (param,), or (param, field or index, ...) for one inside a
    dataclass, a tuple or a list (MaskBits, BiasIndex, a job list)."""
    def walk(path, v):
        if isinstance(v, torch.Tensor):
            yield path, v
        for key, child in _children(v):
            yield from walk(path + (key,), child)
    for name, v in kwargs.items():
        yield from walk((name,), v)


def replaced(kwargs, path, t):
    def put(v, rest):
        if not rest:
            return t
        if dataclasses.is_dataclass(v):
            return dataclasses.replace(v, **{rest[0]: put(getattr(v, rest[0]), rest[1:])})
        seq = list(v)
        seq[rest[0]] = put(seq[rest[0]], rest[1:])
        return type(v)(seq)
    return dict(kwargs, **{path[0]: put(kwargs[path[0]], path[1:])})


def on_fake_device(kwargs):
    for path, t in list(leaves(kwargs)):
        kwargs = replaced(kwargs, path, fake_cuda(t))
    return kwargs


def call(lib, fn, kwargs):
    del lib.calls[:]
    try:
        result = fn(**kwargs)
    except NrvError as e:
        return Outcome(refusal=str(e))
    except Exception as e:      # noqa: BLE001 -- an IndexError or a reshape's RuntimeError is a finding, reported by the caller
        return Outcome(crash=e)
    return Outcome(launches=tuple(lib.calls), result=result)


# ---- the mutations ------------------------------------------------------------------------------------
OTHER_DTYPE = {torch.float32: (torch.bfloat16, torch.float64), torch.bfloat16: (torch.float32,), torch.int64: (torch.int32,),
               torch.int32: (torch.int64,), torch.uint8: (torch.int8,), torch.bool: (torch.uint8,)}


def column_block(t, fill=0.0):
    """The same values in columns [PAD, PAD + cols) of a buffer 2 * PAD columns wider; (view, buffer)."""
    buf = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + 2 * PAD,), fill, dtype=t.dtype, device=t.device)
    view = buf[..., PAD:PAD + t.shape[-1]]
    view.copy_(t)
    return view, buf


def mutations(t):
    """(rule, variant, tensor) for one tensor argument; a form with the strides of the original is left out."""
    if t.dim() >= 1 and t.shape[0] >= 1:
        yield "shorter", "", t[:-1]
    for dt in OTHER_DTYPE.get(t.dtype, ()):
        yield "dtype", str(dt).replace("torch.", ""), t.to(dt)
    forms = []
    if t.dim() >= 2:
        forms.append(("transposed", t.transpose(-1, -2).contiguous().transpose(-1, -2)))
        forms.append(("column block", column_block(t)[0]))
    if t.dim() >= 1 and t.shape[0] > 1:
        forms.append(("stride 0", t[:1].expand(t.shape)))
    for variant, m in forms:
        if m.stride() != t.stride() and not m.is_contiguous():
            yield "strides", variant, m
    yield "host", "", t


def row_stride(t):
    return t.stride(-2) if t.dim() >= 2 else t.stride(0)


@dataclasses.dataclass
class Case:
    """One canonical call: `make(device)` -> keyword arguments with tensors of exactly the documented size on `device`.
    outs: the tensor arguments the kernel writes (a silent copy of one is a finding).  dims: the scalar dimensions that
    describe the tensors (doubling one must be refused)."""
    name: str
    make: object
    outs: tuple = ()
    dims: tuple = ()
    fn: object = None

    def function(self):
        return self.fn if self.fn is not None else getattr(K, self.name)


REFUSED, COPIED, PASSED_ON = "refused", "copied", "strides passed on"


def audit(lib, case):
    """-> (findings, classes): what is wrong, as lines "wrapper(arg) rule: ...", and how the wrapper treats the column-block
    form of each tensor argument of two or more dimensions, {path: REFUSED | COPIED | PASSED_ON}."""
    fn = case.function()
    torch.manual_seed(0)
    base = on_fake_device(case.make("cpu"))
    canon = call(lib, fn, base)
    tag = case.name
    if canon.refusal is not None or canon.crash is not None:
        return [f"{tag}: the canonical call fails: {canon.refusal or repr(canon.crash)}"], {}
    judged_by_result = not canon.launches
    same = (lambda o: o.shape_of_result() == canon.shape_of_result()) if judged_by_result else (lambda o: o.scalars == canon.scalars)
    findings, classes = [], {}

    def named(o, path, rule):
        """The refusal names the argument.  A shortened tensor that the wrapper takes its dimensions from is refused through the
        argument that no longer matches it: there any tensor argument's name will do."""
        words = {str(p) for p in path}
        if rule == "shorter":
            words |= {str(q[0]) for q, _ in leaves(base)}
        return any(re.search(r"(?<![A-Za-z0-9_])" + re.escape(w) + r"(?![A-Za-z0-9_])", o.refusal) for w in words)

    for path, t in leaves(base):
        arg = ".".join(str(p) for p in path)
        for rule, variant, m in mutations(t):
            m = m if rule == "host" else fake_cuda(m)
            if rule == "host":
                m = m.as_subclass(torch.Tensor)
            o = call(lib, fn, replaced(base, path, m))
            where = f"{tag}({arg}) {rule}{' ' + variant if variant else ''}"
            if o.crash is not None:
                findings.append(f"{where}: {type(o.crash).__name__} instead of the wrapper's own refusal: {o.crash}")
                continue
            if o.refusal is not None:
                if not named(o, path, rule):
                    findings.append(f"{where}: the refusal does not name the argument: {o.refusal}")
                if variant == "column block":
                    classes[path] = REFUSED
                continue
            if rule == "host":
                if not judged_by_result:            # host arithmetic launches nothing: a host tensor is its input
                    findings.append(f"{where}: a host tensor reaches the launch")
            elif rule == "shorter":
                if same(o):
                    findings.append(f"{where}: the same launch as the full-size tensor")
            elif rule == "dtype":
                changed = [(a, b) for (n, x), (n2, y) in zip(o.scalars, canon.scalars) if n == n2
                           for ty, a, b in zip(_lib.SIGNATURES[n][1], x, y) if ty is c_int and a != b]
                if judged_by_result:
                    if same(o):
                        findings.append(f"{where}: the same result as the documented dtype")
                elif not any(a in DTYPE_CODES and b in DTYPE_CODES for a, b in changed):
                    findings.append(f"{where}: reaches the launch and no dtype code changed")
            elif rule == "strides":
                passed = m.data_ptr() in o.pointers()
                honoured = passed and any(a != b and a == row_stride(m) for (n, x), (n2, y) in zip(o.scalars, canon.scalars) if n == n2
                                          for a, b in zip(x, y))
                if passed and not honoured:
                    findings.append(f"{where}: its own pointer is launched with the dimensions of the contiguous tensor")
                elif not passed and path[0] in case.outs and not judged_by_result:
                    findings.append(f"{where}: an output is silently copied, the caller's tensor is never written")
                if variant == "column block":
                    classes[path] = PASSED_ON if honoured else COPIED
    for d in case.dims:
        o = call(lib, fn, dict(base, **{d: 2 * base[d]}))
        if o.crash is not None:
            findings.append(f"{tag}[{d} x 2]: {type(o.crash).__name__} instead of the wrapper's own refusal: {o.crash}")
        elif o.refusal is None:
            findings.append(f"{tag}[{d} x 2]: launches with a dimension the tensors do not have")
    return findings, classes


# ---- which functions of kernels.py are wrappers --------------------------------------------------------
def wrappers():
    """The public functions of kernels.py whose own source hands a data_ptr() / _ptr(...) to the library."""
    found = []
    for name, fn in vars(K).items():
        if name.startswith("_") or not inspect.isfunction(fn) or fn.__module__ != K.__name__:
            continue
        if re.search(r"data_ptr\(|_ptr\(", inspect.getsource(fn)):
            found.append(name)
    return sorted(found)


EXEMPT = {
    "probe": "a debugging entry: `data` is any buffer and its byte count is what is passed on",
    "bgemm": "operands are (tensor, offset) pairs addressed by caller-given stride tuples; its own extent check covers every "
             "addressed element (tests/test_bgemm_ref_host.py)",
    "bgemm_plan": "as bgemm; read-only, needs no device",
    "build_cast_jobs": "job-table builder that launches nothing; audited through cast_transpose_batched, which is this plus run_cast_jobs",
    "run_cast_jobs": "takes the handle build_cast_jobs made, no tensors",
    "gemm_tn_grouped": "job-table builder: a list of dicts; checks each problem like gemm_tn",
    "flush_reduce": "takes the job a deferred gemm_tn recorded, no tensors",
}


# ---- the canonical calls ------------------------------------------------------------------------------------
def _t(dtype, *shape, device="cpu"):
    """Seeded values of magnitude around 1 (the launch audit ignores them; the GPU check computes with them)."""
    if dtype in (torch.float32, torch.bfloat16):
        return torch.randn(*shape).to(dtype).to(device)
    if dtype == torch.uint8:
        return (torch.rand(*shape) < 0.75).to(torch.uint8).to(device)
    raise AssertionError(dtype)


F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
CASES = []


def case(name, outs=(), dims=(), fn=None):
    def deco(make):
        CASES.append(Case(name, make, tuple(outs), tuple(dims), fn))
        return make
    return deco


def _pos(t):
    return t.abs() + 0.5           # a reciprocal standard deviation, a survival mask's scale: positive


@case("layernorm_fwd")
def _(dev):
    return dict(x=_t(F32, 3, 64, device=dev), gamma=_t(F32, 64, device=dev), beta=_t(F32, 64, device=dev), eps=1e-5)


@case("layernorm_bwd", outs=("dgamma", "dbeta"))
def _(dev):
    return dict(dy=_t(BF16, 3, 64, device=dev), x=_t(F32, 3, 64, device=dev), gamma=_t(F32, 64, device=dev), mean=_t(F32, 3, device=dev),
                rstd=_pos(_t(F32, 3, device=dev)), dres=_t(F32, 3, 64, device=dev), want_f32=True, want_bf16=True,
                dgamma=_t(F32, 64, device=dev), dbeta=_t(F32, 64, device=dev), accumulate=True)


@case("gemm_nt", outs=("out",))
def _(dev):
    return dict(A=_t(BF16, 16, 64, device=dev), B=_t(BF16, 64, 64, device=dev), epilogue=K.EPI_BIAS_RESIDUAL, bias=_t(F32, 64, device=dev),
                aux=_t(F32, 16, 64, device=dev), out=_t(F32, 16, 64, device=dev))


@case("gemm_nt", outs=("out", "aux_out"))
def _(dev):
    return dict(A=_t(BF16, 16, 64, device=dev), B=_t(BF16, 64, 64, device=dev), epilogue=K.EPI_BIAS_GELU, bias=_t(F32, 64, device=dev),
                aux_out=_t(BF16, 16, 64, device=dev), out=_t(BF16, 16, 64, device=dev))


@case("gemm_tn", outs=("out", "dbias"), dims=("T",))
def _(dev):
    return dict(A=_t(BF16, 32, 16, device=dev), B=_t(BF16, 32, 64, device=dev), out=_t(F32, 16, 64, device=dev), beta=1.0, T=32,
                dbias=_t(F32, 16, device=dev), dbias_beta=1.0)


@case("colsum", outs=("out",))
def _(dev):
    return dict(X=_t(BF16, 8, 64, device=dev), out=_t(F32, 64, device=dev), beta=1.0)


_ATT = dict(B=2, N=8, H=2, dh=32, scale=32 ** -0.5)


def _qkv(dev, B=2, N=8, H=2, dh=32):
    return _t(BF16, B * N, 3 * H * dh, device=dev)


@case("attn_fwd", dims=("B", "N", "H", "dh"))
def _(dev):
    return dict(qkv=_qkv(dev), **_ATT)


@case("attn_bwd", dims=("B", "N", "H", "dh"))
def _(dev):
    return dict(qkv=_qkv(dev), out=_t(BF16, 16, 64, device=dev), dout=_t(BF16, 16, 64, device=dev), lse=_t(F32, 2, 2, 8, device=dev) + 4, **_ATT)


def _seed(dev):
    return torch.tensor([1234], dtype=torch.int64).to(dev)


@case("attn_drop_fwd", dims=("B", "N", "H", "dh"))
def _(dev):
    return dict(qkv=_qkv(dev), seed=_seed(dev), p=0.25, **_ATT)


@case("attn_drop_bwd", dims=("B", "N", "H", "dh"))
def _(dev):
    return dict(qkv=_qkv(dev), out=_t(BF16, 16, 64, device=dev), dout=_t(BF16, 16, 64, device=dev), lse=_t(F32, 2, 2, 8, device=dev) + 4,
                seed=_seed(dev), p=0.25, **_ATT)


@case("attn_drop_mask")
def _(dev):
    return dict(seed=_seed(dev), p=0.25, B=2, H=2, N=8)


@case("attn_probs", dims=("B", "N", "H", "dh"))
def _(dev):
    return dict(qkv=_qkv(dev), lse=_t(F32, 2, 2, 8, device=dev) + 4, **_ATT)


@case("mask_pack", dims=("B", "H", "Nq", "Nk"))
def _(dev):
    return dict(mask=(torch.rand(2, 2, 4, 40) < 0.75).to(dev), B=2, H=2, Nq=4, Nk=40)


def _bits(dev, B, H, Nq, Nk):
    W = (Nk + 31) // 32
    return K.MaskBits(torch.full((B * H * Nq, W), -1, dtype=torch.int32).to(dev), Nq, Nk, H * Nq * W, Nq * W)


_MEM = dict(B=2, Nq=8, M=2, H=2, dh=32, scale=32 ** -0.5)


@case("attn_mem_fwd", dims=("B", "Nq", "M", "H", "dh"))
def _(dev):
    return dict(qkv=_qkv(dev), mkv=_t(BF16, 2, 128, device=dev), shared=True, mask=_bits(dev, 2, 2, 8, 10), **_MEM)


@case("attn_mem_fwd", dims=("B", "Nq", "M", "H", "dh"))
def _(dev):
    return dict(qkv=_qkv(dev), mkv=_t(BF16, 4, 128, device=dev), shared=False, mask=None, **_MEM)


@case("attn_mem_bwd", dims=("B", "Nq", "M", "H", "dh"))
def _(dev):
    return dict(qkv=_qkv(dev), out=_t(BF16, 16, 64, device=dev), dout=_t(BF16, 16, 64, device=dev), lse=_t(F32, 2, 2, 8, device=dev) + 4,
                mkv=_t(BF16, 2, 128, device=dev), shared=True, mask=_bits(dev, 2, 2, 8, 10), **_MEM)


@case("attn_mem_bwd", dims=("B", "Nq", "M", "H", "dh"))
def _(dev):
    return dict(qkv=_qkv(dev), out=_t(BF16, 16, 64, device=dev), dout=_t(BF16, 16, 64, device=dev), lse=_t(F32, 2, 2, 8, device=dev) + 4,
                mkv=_t(BF16, 4, 128, device=dev), shared=False, mask=None, **_MEM)


_SINK = dict(B=2, N=8, H=2, dh=64, scale=0.125)


@case("attn_sinkhorn_fwd", dims=("B", "N", "H"))
def _(dev):
    return dict(qkv=_qkv(dev, dh=64), **_SINK)


@case("attn_sinkhorn_bwd", dims=("B", "N", "H"))
def _(dev):
    return dict(qkv=_qkv(dev, dh=64), dout=_t(BF16, 16, 128, device=dev), lse=_t(F32, 2, 2, 8, device=dev) + 4,
                scal=_t(F32, 2, 2, 7, 8, device=dev), **_SINK)


@case("patch_unfold")
def _(dev):
    return dict(img=_t(F32, 2, 3, 8, 8, device=dev), p=4, layout=K.PATCH_P1P2C)


@case("cast_transpose")
def _(dev):
    return dict(w=_t(F32, 8, 16, device=dev), need_t=True)


@case("cast_transpose_batched", outs=("jobs",))
def _(dev):
    return dict(jobs=[(_t(F32, 8, 16, device=dev), _t(BF16, 8, 16, device=dev), _t(BF16, 16, 8, device=dev)),
                      (_t(F32, 4, 8, device=dev), _t(BF16, 4, 8, device=dev), None)])


@case("cast_bf16", outs=("out",))
def _(dev):
    return dict(x=_t(F32, 8, 16, device=dev), out=_t(BF16, 8, 16, device=dev))


@case("dropout_add", outs=("out",))
def _(dev):
    return dict(x=_t(F32, 8, 8, device=dev), y=_t(F32, 8, 8, device=dev), keep=_t(U8, 8, 8, device=dev), scale=1.25, out=_t(F32, 8, 8, device=dev))


@case("mask_mul", outs=("out",))
def _(dev):
    return dict(a=_t(BF16, 8, 8, device=dev), keep=_t(U8, 8, 8, device=dev), scale=1.25, out=_t(BF16, 8, 8, device=dev))


@case("mask_mul_f32", outs=("out",))
def _(dev):
    return dict(a=_t(F32, 8, 8, device=dev), keep=_t(U8, 8, 8, device=dev), scale=1.25, out=_t(F32, 8, 8, device=dev))


@case("gather_rows")
def _(dev):
    return dict(src=_t(F32, 6, 8, device=dev), index=torch.tensor([5, 0, 3, 2]).to(dev))


@case("scatter_rows")
def _(dev):
    return dict(dout=_t(F32, 4, 8, device=dev), index=torch.tensor([5, 0, 3, 2]).to(dev), rows_src=6)


@case("sumsq", outs=("out", "ws"))
def _(dev):
    return dict(x=_t(F32, 64, device=dev), out=_t(F32, 1, device=dev), ws=_t(F32, K.sumsq_workspace(64) // 4, device=dev))


@case("adamw_flat", outs=("p", "m", "v"))
def _(dev):
    return dict(p=_t(F32, 64, device=dev), g=_t(F32, 64, device=dev), m=_t(F32, 64, device=dev), v=_pos(_t(F32, 64, device=dev)), lr=1e-3,
                beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=1, gnorm_sq=_pos(_t(F32, 1, device=dev)), max_norm=1.0,
                step_scalars=torch.tensor([1e-3, 0.1, 0.001]).to(dev))


@case("sinkhorn_fwd")
def _(dev):
    return dict(scores=_t(F32, 2, 4, 8, device=dev), iters=3)


@case("sinkhorn_bwd")
def _(dev):
    return dict(scores=_t(F32, 2, 4, 8, device=dev), dout=_t(F32, 2, 4, 8, device=dev), lse=_t(F32, 2, 4, device=dev) + 4,
                avec=_t(F32, 2, 4, 4, device=dev), bvec=_t(F32, 2, 3, 8, device=dev), iters=3)


_WIN = dict(B=2, pH=4, pW=4, C=32, heads=1, window=(2, 2), shift=(1, 1), robust=False)


@case("window_attn_fwd", dims=("B", "pH", "pW", "C", "heads"))
def _(dev):
    return dict(qkv=_t(BF16, 32, 96, device=dev), table=_t(F32, 9, 1, device=dev), **_WIN)


@case("window_attn_bwd", dims=("B", "pH", "pW", "C", "heads"))
def _(dev):
    return dict(qkv=_t(BF16, 32, 96, device=dev), table=_t(F32, 9, 1, device=dev), dout=_t(BF16, 32, 32, device=dev),
                stats=_t(F32, 32, 1, 1, device=dev) + 4, **_WIN)


@case("sd_add", outs=("out",))
def _(dev):
    return dict(x=_t(F32, 4, 8, device=dev), y=_t(F32, 4, 8, device=dev), keep=torch.tensor([1.0, 0.0]).to(dev), survival=0.5,
                out=_t(F32, 4, 8, device=dev))


@case("sd_scale_bf16")
def _(dev):
    return dict(dy=_t(F32, 4, 8, device=dev), keep=torch.tensor([1.0, 0.0]).to(dev), survival=0.5)


@case("bn_stats", outs=("running_mean", "running_var"))
def _(dev):
    return dict(y=_t(F32, 6, 8, device=dev), eps=1e-5, momentum=0.1, running_mean=_t(F32, 8, device=dev), running_var=_pos(_t(F32, 8, device=dev)))


def _bn(dev):
    return dict(y=_t(F32, 6, 8, device=dev), mean=_t(F32, 8, device=dev), scale=_pos(_t(F32, 8, device=dev)), gamma=_t(F32, 8, device=dev),
                beta=_t(F32, 8, device=dev), act=True, keep=torch.tensor([1.0, 0.0]).to(dev), survival=0.5)


@case("bn_apply")
def _(dev):
    return dict(_bn(dev), residual=_t(F32, 6, 8, device=dev), want_f32=True, want_bf16=True)


@case("bn_bwd")
def _(dev):
    return dict(_bn(dev), dz=_t(F32, 6, 8, device=dev))


_CONV = dict(B=2, C=3, H=8, W=8, ks=3, stride=2, pad=1)


@case("conv_unfold", dims=("B", "C", "H", "W"))
def _(dev):
    return dict(src=_t(F32, 2, 3, 8, 8, device=dev), nhwc=False, **_CONV)


@case("conv_fold", dims=("B", "C", "H", "W"))
def _(dev):
    return dict(dcols=_t(BF16, 2 * 4 * 4, 32, device=dev), **_CONV)


@case("bias_index")
def _(dev):
    return dict(idx=(torch.arange(16).reshape(4, 4) % 7).to(dev), n_offsets=7, device=dev)


_BA = dict(hq=16, hk=16, hv=32, B=2, H=2, Nq=4, Nk=4, kd=16, d=32, robust=False)


def _bias_attn(dev):
    return dict(q=_t(BF16, 8, 32, device=dev), k=_t(BF16, 8, 32, device=dev), v=_t(BF16, 8, 64, device=dev), table=_t(F32, 2, 7, device=dev),
                index=K.bias_index(torch.arange(16).reshape(4, 4) % 7, 7, dev), **_BA)


@case("bias_attn_fwd", dims=("B", "H", "Nq", "Nk", "kd", "d"))
def _(dev):
    return _bias_attn(dev)


@case("bias_attn_bwd", outs=("dq", "dk", "dv"), dims=("B", "H", "Nq", "Nk", "kd", "d"))
def _(dev):
    S = _lib.load().nrv_bias_attn_stats_size(4, 4, 0)
    return dict(_bias_attn(dev), o=_t(BF16, 8, 64, device=dev), dact=_t(BF16, 8, 64, device=dev), stats=_t(F32, 4, S, device=dev) + 4,
                dq=_t(BF16, 8, 32, device=dev), dk=_t(BF16, 8, 32, device=dev), dv=_t(BF16, 8, 64, device=dev))


_PCN = dict(B=2, H=4, W=4)


@case("dwconv3x3_fwd", dims=("B", "H", "W"))
def _(dev):
    return dict(a=_t(BF16, 32, 8, device=dev), w=_t(F32, 8, 1, 3, 3, device=dev), bias=_t(F32, 8, device=dev), **_PCN)


@case("dwconv3x3_bwd", dims=("B", "H", "W"))
def _(dev):
    return dict(a=_t(BF16, 32, 8, device=dev), w=_t(F32, 8, 1, 3, 3, device=dev), bias=_t(F32, 8, device=dev), dg=_t(BF16, 32, 8, device=dev),
                s=_t(F32, 2, 8, device=dev), dmean=_t(F32, 2, 8, device=dev), gelu_stream=_t(BF16, 32, 8, device=dev), **_PCN)


def _se(dev):
    return dict(wr=_t(F32, 4, 8, 1, 1, device=dev), we=_t(F32, 8, 4, 1, 1, device=dev))


@case("se_fwd")                    # HW only divides the sums: no tensor is as large as it says
def _(dev):
    return dict(_se(dev), sq=_t(F32, 2, 8, device=dev), HW=16, br=_t(F32, 4, device=dev), be=_t(F32, 8, device=dev))


@case("se_apply", dims=("HW",))
def _(dev):
    return dict(d=_t(BF16, 32, 8, device=dev), s=_t(F32, 2, 8, device=dev), HW=16)


@case("se_bwd", dims=("HW",))
def _(dev):
    return dict(_se(dev), dg=_t(BF16, 32, 8, device=dev), d=_t(BF16, 32, 8, device=dev), sq=_t(F32, 2, 8, device=dev), HW=16,
                s=_t(F32, 2, 8, device=dev), hid=_t(F32, 2, 4, device=dev))


@case("ls_add", outs=("out",))
def _(dev):
    return dict(x=_t(F32, 4, 8, device=dev), y=_t(F32, 4, 8, device=dev), gamma=_t(F32, 8, device=dev), keep=torch.tensor([1.0, 0.0]).to(dev),
                survival=0.5, out=_t(F32, 4, 8, device=dev))


@case("ls_bwd")
def _(dev):
    return dict(dy=_t(F32, 4, 8, device=dev), y=_t(F32, 4, 8, device=dev), gamma=_t(F32, 8, device=dev), keep=torch.tensor([1.0, 0.0]).to(dev),
                survival=0.5)


@case("dgelu_rows")
def _(dev):
    return dict(dx=_t(F32, 4, 8, device=dev), gelu_stream=_t(BF16, 4, 8, device=dev))


@case("dgelu_rows")
def _(dev):
    return dict(dx=_t(F32, 4, 64, device=dev), gelu_stream=torch.randint(0, 256, (4, 64), dtype=torch.uint8).to(dev))


_CLS = dict(B=2, heads=2, Np=4, dh=32, scale=32 ** -0.5)


def _cls(dev):
    return dict(q=_t(BF16, 2, 64, device=dev), kc=_t(BF16, 2, 64, device=dev), kp=_t(BF16, 8, 64, device=dev), vc=_t(BF16, 2, 64, device=dev),
                vp=_t(BF16, 8, 64, device=dev), **_CLS)


@case("cls_attn_fwd", dims=("B", "heads", "Np", "dh"))
def _(dev):
    return _cls(dev)


@case("cls_attn_bwd", dims=("B", "heads", "Np", "dh"))
def _(dev):
    return dict(_cls(dev), dout=_t(BF16, 2, 64, device=dev), lse=_t(F32, 4, device=dev) + 4)


def _mat(dev):
    return _t(F32, 2, 2, 4, 8, device=dev)


def _prob(dev):
    return torch.softmax(_mat(dev).cpu(), -1).to(dev)


def _mix(dev):
    return _t(F32, 2, 2, device=dev)


@case("th_softmax_fwd")
def _(dev):
    return dict(S=_mat(dev), W1=_mix(dev), W2=_mix(dev))


@case("th_softmax_bwd")
def _(dev):
    return dict(dA=_mat(dev), P=_prob(dev), S=_mat(dev), W1=_mix(dev), W2=_mix(dev))


@case("head_mix_fwd")
def _(dev):
    return dict(x=_mat(dev), W=_mix(dev))


@case("head_mix_bwd")
def _(dev):
    return dict(dout=_mat(dev), x=_mat(dev), W=_mix(dev))


@case("reattn_softmax_fwd")
def _(dev):
    return dict(S=_mat(dev), W=_mix(dev), gamma=_t(F32, 2, device=dev), beta=_t(F32, 2, device=dev), eps=1e-5)


@case("reattn_softmax_bwd")
def _(dev):
    return dict(dA=_mat(dev), P=_prob(dev), W=_mix(dev), gamma=_t(F32, 2, device=dev), eps=1e-5)


@case("reattn_norm_fwd")
def _(dev):
    return dict(P=_prob(dev), W=_mix(dev), gamma=_t(F32, 2, device=dev), beta=_t(F32, 2, device=dev), eps=1e-5)


@case("reattn_norm_bwd")
def _(dev):
    return dict(dA=_mat(dev), P=_prob(dev), W=_mix(dev), gamma=_t(F32, 2, device=dev), eps=1e-5)


_SPLIT = dict(B=2, C=8, H=4, W=4, ks=3, stride=2, pad=1)


@case("soft_split_fwd", dims=("B", "C", "H", "W"))
def _(dev):
    return dict(src=_t(BF16, 32, 8, device=dev), rows=True, **_SPLIT)


@case("soft_split_fwd", dims=("B", "C", "H", "W"))
def _(dev):
    return dict(src=_t(F32, 2, 8, 4, 4, device=dev), rows=False, **_SPLIT)


@case("soft_split_bwd", dims=("B", "C", "H", "W"))
def _(dev):
    return dict(dcols=_t(BF16, 8, 72, device=dev), **_SPLIT)


@case("layernorm_pad_fwd", dims=("n",))
def _(dev):
    return dict(x=_t(F32, 3, 16, device=dev), n=12, gamma=_t(F32, 12, device=dev), beta=_t(F32, 12, device=dev), eps=1e-5)


@case("layernorm_pad_bwd", dims=("n",))
def _(dev):
    return dict(dy=_t(BF16, 3, 16, device=dev), x=_t(F32, 3, 16, device=dev), n=12, gamma=_t(F32, 12, device=dev), mean=_t(F32, 3, device=dev),
                rstd=_pos(_t(F32, 3, device=dev)), dres=_t(F32, 3, 16, device=dev), want_f32=True, want_bf16=True)


_WIDE = dict(B=2, N=8, H=1, dh=160, scale=160 ** -0.5)


@case("attn_wide_fwd", dims=("B", "N", "H"))
def _(dev):
    return dict(qkv=_qkv(dev, H=1, dh=160), **_WIDE)


@case("attn_wide_bwd", dims=("B", "N", "H"))
def _(dev):
    return dict(qkv=_qkv(dev, H=1, dh=160), out=_t(BF16, 16, 160, device=dev), dout=_t(BF16, 16, 160, device=dev),
                lse=_t(F32, 2, 1, 8, device=dev) + 4, **_WIDE)


_ROT = dict(B=2, N=5, lead=1, H=2, dh=32)


@case("rotary_fwd", outs=("qkv",), dims=("B", "N", "H", "dh"))
def _(dev):
    return dict(qkv=_qkv(dev, N=5), sin=_t(F32, 4, 8, device=dev), cos=_t(F32, 4, 8, device=dev), **_ROT)


@case("rotary_bwd", outs=("dqkv",), dims=("B", "N", "H", "dh"))
def _(dev):
    return dict(dqkv=_qkv(dev, N=5), sin=_t(F32, 4, 8, device=dev), cos=_t(F32, 4, 8, device=dev), **_ROT)


_DWC = dict(B=2, H=2, W=2, lead=1)


@case("dwconv_fwd", outs=("out",), dims=("B", "H", "W", "lead"))
def _(dev):
    return dict(a=_t(BF16, 10, 8, device=dev), w=_t(F32, 8, 1, 3, 3, device=dev), out=_t(BF16, 10, 8, device=dev), **_DWC)


@case("dwconv_bwd", outs=("da", "dw"), dims=("B", "H", "W", "lead"))
def _(dev):
    return dict(a=_t(BF16, 10, 8, device=dev), w=_t(F32, 8, 1, 3, 3, device=dev), dout=_t(BF16, 10, 8, device=dev),
                da=_t(BF16, 10, 8, device=dev), dw=_t(F32, 8, 9, device=dev), **_DWC)


@case("geglu_fwd", dims=("hidden",))
def _(dev):
    return dict(u=_t(BF16, 4, 16, device=dev), hidden=8)


@case("geglu_bwd", outs=("out",))
def _(dev):
    return dict(u=_t(BF16, 4, 16, device=dev), dh=_t(BF16, 4, 8, device=dev), out=_t(BF16, 4, 16, device=dev))


_POOL = dict(B=2, H=3, W=3, lead=1)


@case("pool_dwconv_fwd", outs=("out",), dims=("B", "H", "W", "lead"))
def _(dev):
    return dict(x=_t(F32, 20, 8, device=dev), w=_t(F32, 16, 1, 3, 3, device=dev), bias=_t(F32, 16, device=dev), out=_t(BF16, 8, 16, device=dev),
                **_POOL)


@case("pool_dwconv_bwd", outs=("dx", "dw", "dbias"), dims=("B", "H", "W", "lead"))
def _(dev):
    return dict(x=_t(F32, 20, 8, device=dev), w=_t(F32, 16, 1, 3, 3, device=dev), dout=_t(BF16, 8, 16, device=dev), dx=_t(F32, 20, 8, device=dev),
                dw=_t(F32, 16, 9, device=dev), dbias=_t(F32, 16, device=dev), **_POOL)


@case("unfold_patches", outs=("out",))
def _(dev):
    return dict(img=_t(F32, 2, 3, 5, 5, device=dev), ks=3, stride=2, out=_t(BF16, 8, 32, device=dev))


_MP = dict(B=2, H=4, W=4, pk=3, ps=2, pp=1)


@case("relu_maxpool_fwd", outs=("out_f32", "out_bf16", "idx"), dims=("B", "H", "W"))
def _(dev):
    return dict(y=_t(F32, 32, 8, device=dev), out_f32=_t(F32, 8, 8, device=dev), out_bf16=_t(BF16, 8, 8, device=dev),
                idx=torch.zeros(8, 8, dtype=torch.uint8).to(dev), **_MP)


@case("relu_maxpool_bwd", outs=("dy",), dims=("B", "H", "W"))
def _(dev):
    return dict(dout=_t(F32, 8, 8, device=dev), idx=torch.zeros(8, 8, dtype=torch.uint8).to(dev), dy=_t(BF16, 32, 8, device=dev), **_MP)


@case("layernorm_f32_fwd", outs=("y", "y_bf16"))
def _(dev):
    return dict(x=_t(F32, 3, 16, device=dev), gamma=_t(F32, 16, device=dev), beta=_t(F32, 16, device=dev), eps=1e-5, y=_t(F32, 3, 16, device=dev),
                y_bf16=_t(BF16, 3, 16, device=dev))


@case("layernorm_f32_bwd", outs=("dx", "dx_bf16"))
def _(dev):
    return dict(dy=_t(F32, 3, 16, device=dev), x=_t(F32, 3, 16, device=dev), gamma=_t(F32, 16, device=dev), mean=_t(F32, 3, device=dev),
                rstd=_pos(_t(F32, 3, device=dev)), dx=_t(F32, 3, 16, device=dev), dx_bf16=_t(BF16, 3, 16, device=dev))


@case("seqpool_fwd", outs=("w", "out"), dims=("B", "n"))
def _(dev):
    return dict(y=_t(F32, 6, 8, device=dev), a=_t(F32, 8, device=dev), bias=_t(F32, 1, device=dev), B=2, n=3, w=_t(F32, 2, 3, device=dev),
                out=_t(F32, 2, 8, device=dev))


@case("seqpool_bwd", outs=("dy",), dims=("B", "n"))
def _(dev):
    return dict(dout=_t(F32, 2, 8, device=dev), y=_t(F32, 6, 8, device=dev), a=_t(F32, 8, device=dev), w=torch.softmax(_t(F32, 2, 3), -1).to(dev),
                B=2, n=3, dy=_t(F32, 6, 8, device=dev))


_SUB = dict(B=2, H=2, Nq=4, Nk=3, dh=32, scale=32 ** -0.5)


def _sub(dev):
    return dict(q=_t(BF16, 8, 64, device=dev), k=_t(BF16, 6, 64, device=dev), v=_t(BF16, 6, 64, device=dev), **_SUB)


@case("subattn_fwd", outs=("out", "lse"), dims=("B", "H", "Nq", "Nk", "dh"))
def _(dev):
    return dict(_sub(dev), out=_t(BF16, 8, 64, device=dev), lse=_t(F32, 2, 2, 4, device=dev))


@case("subattn_bwd", outs=("dq", "dk", "dv"), dims=("B", "H", "Nq", "Nk", "dh"))
def _(dev):
    return dict(_sub(dev), dout=_t(BF16, 8, 64, device=dev), lse=_t(F32, 2, 2, 4, device=dev) + 4, dq=_t(BF16, 8, 64, device=dev),
                dk=_t(BF16, 6, 64, device=dev), dv=_t(BF16, 6, 64, device=dev))


_PEG = dict(B=2, H=2, W=2)


@case("peg_fwd", outs=("out",), dims=("B", "H", "W"))
def _(dev):
    return dict(x=_t(F32, 8, 8, device=dev), w=_t(F32, 8, 1, 3, 3, device=dev), bias=_t(F32, 8, device=dev), out=_t(F32, 8, 8, device=dev), **_PEG)


@case("peg_bwd", outs=("dx", "dw", "dbias"), dims=("B", "H", "W"))
def _(dev):
    return dict(x=_t(F32, 8, 8, device=dev), w=_t(F32, 8, 1, 3, 3, device=dev), dy=_t(F32, 8, 8, device=dev), dx=_t(F32, 8, 8, device=dev),
                dw=_t(F32, 8, 9, device=dev), dbias=_t(F32, 8, device=dev), **_PEG)


def case_ids():
    seen, ids = {}, []
    for c in CASES:
        seen[c.name] = seen.get(c.name, 0) + 1
        ids.append(c.name if seen[c.name] == 1 else f"{c.name}#{seen[c.name]}")
    return ids
