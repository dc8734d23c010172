"""GPU: LayerNorm, padded LayerNorm, batch norm and the bf16 column sums per row and per column against the fp64 references of
tests/norm_ref.py, at every reachable instantiation and at the lane, chunk, slab and dtype edges its tables list.

Every case runs through noise_robust_vit_amd.kernels and runs twice with bit-identical results.  The C ABI is called directly only where
the wrapper hides a parameter: `accumulate` of the padded LayerNorm, an over-sized workspace, and guarded outputs -- one case per entry
point whose outputs lie between guard blocks of a NaN payload no kernel produces, with the tail of the workspace guarded the same way.
The pad columns of x, dy and dres and the padding of a wide column-sum operand hold NaN: no output may see them, and the pad columns of
y and dx must come back exactly zero.  The bounds are those of tests/norm_ref.py, derived there and shown on the CPU
(tests/test_norm_ref_host.py) to hold twice over for an fp32 emulation of each kernel and to catch each of 19 wrong kernels.

Measured on an MI355X (worst error / bound over the family's cases, as test_zz_worst_ratios_per_family prints them; 205 tests in 3.3 s,
the slowest 0.09 s apart from the first, whose 0.31 s load the library):
  LayerNorm          mean 0.109  rstd 0.113  dx fp32 0.237  dgamma 0.021  dbeta 0.056                       y 0.995  dx bf16 0.995
  padded LayerNorm   mean 0.202  rstd 0.145  dx fp32 0.299  dgamma 0.160  dbeta 0.250                       y 0.993  dx bf16 0.996
  batch norm         mean 0.077  M2 0.036  invstd 0.243  running mean 0.456  running var 0.306  z fp32 0.329
                     dgamma 0.129  dbeta 0.137                                                              z bf16 0.992  dy 0.991
  column sums        0.035
The bf16 outputs use nearly all of a bound that is nearly all store term (2^-8 of the element, the unit round-off of the format); before
the store the same quantities are at 0.24 / 0.30 / 0.33 at most.  The figures equal the CPU emulation's to three digits (rstd of the
padded kernel, which uses rsqrtf, apart).  No case failed, no guard or workspace tail was touched, no pad column was nonzero and every rerun
was bit-identical: none of the gaps these cases close hid a defect in the kernels.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import norm_ref as R  # noqa: E402
from noise_robust_vit_amd import _lib  # noqa: E402
from noise_robust_vit_amd import kernels as K  # noqa: E402
from noise_robust_vit_amd._lib import NRV_BF16, NRV_F32  # noqa: E402

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
f32 = torch.float32
GUARD = 256                                  # elements on either side of an output
PATTERN = {bf: (torch.int16, 0x7FC1), f32: (torch.int32, 0x7FC00001)}     # NaNs that are not torch's nor any arithmetic's
WORST = {}


class _Out:
    """An output of `numel` elements between two guard blocks, NaN-filled or preset"""
    def __init__(self, numel, dtype, dev, preset=None):
        it, pat = PATTERN[dtype]
        self.raw = torch.full((numel + 2 * GUARD,), pat, dtype=it, device=dev)
        self.t = self.raw.view(dtype)[GUARD:GUARD + numel]
        if preset is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(preset.reshape(-1))
        self.pat = pat

    def ptr(self):
        return self.t.data_ptr()

    def done(self, what):
        assert bool((self.raw[:GUARD] == self.pat).all()) and bool((self.raw[-GUARD:] == self.pat).all()), f"{what}: a guard element was written"
        assert not bool(torch.isnan(self.t).any()), f"{what}: an output element was never written"
        return self.t


class _Workspace:
    """`need` bytes and as many again behind them, which no kernel may touch although the call is told of them"""
    def __init__(self, need, dev):
        self.need = (int(need) + 15) // 16 * 16
        self.raw = torch.full((2 * self.need + 16,), 0x5A, dtype=torch.uint8, device=dev)

    def done(self, what):
        assert bool((self.raw[self.need:] == 0x5A).all()), f"{what}: the workspace was written past what the entry point asked for"


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dev, as_bf=False):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(bf if as_bf else f32)


def _np(t):
    return None if t is None else t.detach().float().cpu().numpy()


def _same(cid, a, b):
    for n in a:
        if a[n] is not None:
            assert torch.equal(a[n], b[n]), (cid, n, "a rerun differs")


def _report(family, cid, ratios):
    print(cid, "error / bound", {k: f"{v:.3f}" for k, v in ratios.items()})
    w = WORST.setdefault(family, {})
    for k, v in ratios.items():
        if v >= w.get(k, (-1.0, ""))[0]:
            w[k] = (v, cid)
    assert max(ratios.values()) <= 1.0, (cid, ratios)


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm and padded LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------------
def _ln_run(c, i, dev, direct):
    pad = isinstance(c, R.PadCase)
    n, ld, rows = i["n"], i["ld"], c.rows
    x, dy = _dev(i["x"], dev, c.xbf), _dev(i["dy"], dev, True)
    dres = _dev(i["dres"], dev, c.dres == 2)
    gamma, beta = _dev(i["gamma"], dev), _dev(i["beta"], dev)
    want32, want16 = c.out in ("f32", "both"), c.out in ("bf16", "both")
    dg0, db0 = (_dev(i["dgamma0"], dev), _dev(i["dbeta0"], dev)) if c.acc else (None, None)
    if not direct:
        if pad:
            assert not c.acc
            y, mean, rstd = K.layernorm_pad_fwd(x, n, gamma, beta, c.eps)
            dx32, dx16, dg, db = K.layernorm_pad_bwd(dy, x, n, gamma, mean, rstd, dres, want_f32=want32, want_bf16=want16)
        else:
            y, mean, rstd = K.layernorm_fwd(x, gamma, beta, c.eps)
            dx32, dx16, dg, db = K.layernorm_bwd(dy, x, gamma, mean, rstd, dres, want_f32=want32, want_bf16=want16,
                                                 dgamma=dg0, dbeta=db0, accumulate=bool(c.acc))
        torch.cuda.synchronize()
        return {"y": y, "mean": mean, "rstd": rstd, "dx32": dx32, "dx16": dx16, "dgamma": dg, "dbeta": db}
    lib = _lib.load()
    cid = R.case_id(c)
    o = {"y": _Out(rows * ld, bf, dev), "mean": _Out(rows, f32, dev), "rstd": _Out(rows, f32, dev),
         "dgamma": _Out(n, f32, dev, dg0), "dbeta": _Out(n, f32, dev, db0)}
    if want32:
        o["dx32"] = _Out(rows * ld, f32, dev)
    if want16:
        o["dx16"] = _Out(rows * ld, bf, dev)
    xdt, rdt = (NRV_BF16 if c.xbf else NRV_F32), (NRV_BF16 if c.dres == 2 else NRV_F32)
    p32, p16 = (o["dx32"].ptr() if want32 else None), (o["dx16"].ptr() if want16 else None)
    rp = dres.data_ptr() if dres is not None else None
    if pad:
        rc = lib.nrv_layernorm_pad_fwd(x.data_ptr(), xdt, gamma.data_ptr(), beta.data_ptr(), o["y"].ptr(), o["mean"].ptr(), o["rstd"].ptr(),
                                       rows, n, ld, c.eps, _st())
        assert rc == 0, rc
        ws = _Workspace(lib.nrv_layernorm_pad_bwd_workspace(rows, n), dev)
        rc = lib.nrv_layernorm_pad_bwd(dy.data_ptr(), x.data_ptr(), xdt, gamma.data_ptr(), o["mean"].ptr(), o["rstd"].ptr(), rp, rdt, p32, p16,
                                       o["dgamma"].ptr(), o["dbeta"].ptr(), int(c.acc), ws.raw.data_ptr(), ws.raw.numel(), rows, n, ld, _st())
    else:
        rc = lib.nrv_layernorm_fwd(x.data_ptr(), xdt, gamma.data_ptr(), beta.data_ptr(), o["y"].ptr(), o["mean"].ptr(), o["rstd"].ptr(),
                                   rows, n, c.eps, _st())
        assert rc == 0, rc
        ws = _Workspace(lib.nrv_layernorm_bwd_workspace(rows, n), dev)
        rc = lib.nrv_layernorm_bwd(dy.data_ptr(), x.data_ptr(), xdt, gamma.data_ptr(), o["mean"].ptr(), o["rstd"].ptr(), rp, rdt, p32, p16,
                                   o["dgamma"].ptr(), o["dbeta"].ptr(), int(c.acc), ws.raw.data_ptr(), ws.raw.numel(), rows, n, _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    ws.done(cid)
    got = {k: v.done(f"{cid} {k}") for k, v in o.items()}
    for k in ("y", "dx32", "dx16"):
        got[k] = got[k].reshape(rows, ld) if k in got else None
    return got


def _ln_case(c, dev, direct=False):
    i = R.ln_inputs(c)
    raw = _ln_run(c, i, dev, direct)
    got = {k: _np(v) for k, v in raw.items()}
    assert all(np.isfinite(v[..., :i["n"]] if v.ndim == 2 else v).all() for v in got.values() if v is not None), R.case_id(c)
    _report("padded LayerNorm" if isinstance(c, R.PadCase) else "LayerNorm", R.case_id(c) + (" (guarded)" if direct else ""), R.ln_check(c, i, got))
    _same(R.case_id(c), raw, _ln_run(c, i, dev, direct))


@pytest.mark.parametrize("c", R.LN_CASES, ids=R.case_id)
def test_layernorm_every_row_and_column_at_every_instantiation(dev, c):
    """x fp32 | bf16 x no | fp32 | bf16 residual gradient x every (MAXJ, lanes per row), with partial, full and idle last chunks; nine rows
    of nine kinds (three workgroups of the 64-lane form, two of the half-wave form, the last pair incomplete), and 1 and 2 rows"""
    _ln_case(c, dev)


def test_layernorm_guarded_outputs_and_oversized_workspace(dev):
    _ln_case(R.LN_GUARDED, dev, direct=True)


@pytest.mark.parametrize("c", R.PAD_CASES, ids=R.case_id)
def test_padded_layernorm_every_row_and_column_with_nan_pads(dev, c):
    """n = 1 .. 4096 with ld = n, pad8(n) and wider; 1, 9, 127 and 129 rows (one slab, two slabs of 65 and 64); accumulate = 1 goes
    through the C ABI with guarded outputs, the rest through kernels.py"""
    _ln_case(c, dev, direct=bool(c.acc))


# ---------------------------------------------------------------------------------------------------------------------------------
# batch norm
# ---------------------------------------------------------------------------------------------------------------------------------
def _bn_run(c, i, dev, direct):
    T, C = c.T, c.C
    y, gamma, beta = _dev(i["y"], dev), _dev(i["gamma"], dev), _dev(i["beta"], dev)
    dz, keep, res = _dev(i["dz"], dev, c.dzbf), _dev(i["keep"], dev), _dev(i["res"], dev)
    rm, rv = _dev(i["run_mean"], dev), _dev(i["run_var"], dev)
    want32, want16 = c.out in ("f32", "both"), c.out in ("bf16", "both")
    out = {}
    if not direct:
        if c.training:
            mean, scale, stat = K.bn_stats(y, R.BN_EPS, c.mom, rm, rv)
            out.update(mean=mean, invstd=scale, stat=stat)
        else:
            mean, scale = rm, rv
        kw = dict(eps=R.BN_EPS, scale_is_var=not c.training, act=bool(c.act), keep=keep, survival=R.BN_SURVIVAL)
        out["z32"], out["z16"] = K.bn_apply(y, mean, scale, gamma, beta, residual=res, want_f32=want32, want_bf16=want16, **kw)
        out["dy"], out["dgamma"], out["dbeta"] = K.bn_bwd(dz, y, mean, scale, gamma, beta, training=bool(c.training), **kw)
        torch.cuda.synchronize()
        out.update(run_mean=rm, run_var=rv)
        return out
    lib = _lib.load()
    cid = R.case_id(c)
    assert c.training
    o = {"mean": _Out(C, f32, dev), "invstd": _Out(C, f32, dev), "stat": _Out(3 * C, f32, dev), "run_mean": _Out(C, f32, dev, rm),
         "run_var": _Out(C, f32, dev, rv), "dy": _Out(T * C, bf, dev), "dgamma": _Out(C, f32, dev), "dbeta": _Out(C, f32, dev)}
    if want32:
        o["z32"] = _Out(T * C, f32, dev)
    if want16:
        o["z16"] = _Out(T * C, bf, dev)
    ws = _Workspace(lib.nrv_bn_workspace(T, C), dev)
    rc = lib.nrv_bn_stats(y.data_ptr(), T, C, R.BN_EPS, c.mom, o["mean"].ptr(), o["invstd"].ptr(), o["stat"].ptr(), o["run_mean"].ptr(),
                          o["run_var"].ptr(), ws.raw.data_ptr(), ws.raw.numel(), _st())
    assert rc == 0, rc
    kp, per = (keep.data_ptr() if keep is not None else None), max(c.per, 1)
    rc = lib.nrv_bn_apply(y.data_ptr(), o["mean"].ptr(), o["invstd"].ptr(), 0, R.BN_EPS, gamma.data_ptr(), beta.data_ptr(), int(c.act),
                          res.data_ptr() if res is not None else None, kp, R.BN_SURVIVAL, per,
                          o["z32"].ptr() if want32 else None, o["z16"].ptr() if want16 else None, T, C, _st())
    assert rc == 0, rc
    rc = lib.nrv_bn_bwd(dz.data_ptr(), NRV_BF16 if c.dzbf else NRV_F32, int(c.act), kp, R.BN_SURVIVAL, per, y.data_ptr(), o["mean"].ptr(),
                        o["invstd"].ptr(), 0, R.BN_EPS, gamma.data_ptr(), beta.data_ptr(), 1, o["dgamma"].ptr(), o["dbeta"].ptr(), o["dy"].ptr(),
                        ws.raw.data_ptr(), ws.raw.numel(), T, C, _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    ws.done(cid)
    out = {k: v.done(f"{cid} {k}") for k, v in o.items()}
    for k in ("z32", "z16", "dy"):
        out[k] = out[k].reshape(T, C) if k in out else None
    out["stat"] = out["stat"].reshape(3, C)
    return out


def _bn_case(c, dev, direct=False):
    i = R.bn_inputs(c)
    raw = _bn_run(c, i, dev, direct)
    got = {k: _np(v) for k, v in raw.items()}
    if c.training:
        stat = got.pop("stat")
        got["count"], got["m2"] = stat[0], stat[2]
        assert np.array_equal(stat[1], got["mean"])
    _report("batch norm", R.case_id(c) + (" (guarded)" if direct else ""), R.bn_check(c, i, got))
    _same(R.case_id(c), raw, _bn_run(c, i, dev, direct))


@pytest.mark.parametrize("c", R.BN_CASES, ids=R.case_id)
def test_batchnorm_every_column_at_the_chunk_and_group_edges(dev, c):
    """T = 1, 2, 3, 5 (empty row groups), 512, 513 (a last chunk of one row), 1000, 32769 (65 chunks: a lane's second chunk); C with a
    partial 64-column block; fp32 | bf16 dz, Hardswish, keep, training | eval, momentum 0 | 0.1 | 1, every output combination"""
    _bn_case(c, dev)


def test_batchnorm_guarded_outputs_and_oversized_workspace(dev):
    _bn_case(next(c for c in R.BN_CASES if c.T == 513 and c.C == 68 and c.training), dev, direct=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------------------------------
def _cs_run(c, i, dev, direct):
    back = _dev(i["back"], dev, True)
    X = back[:c.T, :c.N]
    preset = _dev(i["out0"], dev) if c.beta != 0 else None       # beta = 0 must overwrite whatever `out` held: it holds NaN
    if not direct:
        out = preset if preset is not None else torch.full((c.N,), float("nan"), dtype=f32, device=dev)
        K.colsum(X, out=out, beta=c.beta)
        torch.cuda.synchronize()
        return {"out": out}
    lib = _lib.load()
    o = _Out(c.N, f32, dev, preset)
    ws = _Workspace(lib.nrv_colsum_workspace(c.T, c.N), dev)
    rc = lib.nrv_colsum_bf16(X.data_ptr(), c.ld, o.ptr(), c.T, c.N, c.beta, ws.raw.data_ptr(), ws.raw.numel(), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    ws.done(R.case_id(c))
    return {"out": o.done(R.case_id(c))}


def _cs_case(c, dev, direct=False):
    i = R.cs_inputs(c)
    raw = _cs_run(c, i, dev, direct)
    _report("column sums", R.case_id(c) + (" (guarded)" if direct else ""), R.cs_check(c, i, _np(raw["out"])))
    _same(R.case_id(c), raw, _cs_run(c, i, dev, direct))


@pytest.mark.parametrize("c", R.CS_CASES, ids=R.case_id)
def test_colsum_every_column_with_cancellation_and_nan_padding(dev, c):
    """T = 1, 2, 5 (row groups without a row, a second chunk of one row), N past one 512-column block and not a multiple of it, ld > N
    as a view into a NaN-filled allocation, beta 0 | 1 | -0.5 on a preset out"""
    _cs_case(c, dev)


def test_colsum_guarded_output_and_oversized_workspace(dev):
    _cs_case(R.CsCase(513, 1016, 1024, -0.5), dev, direct=True)


def test_zz_worst_ratios_per_family(dev):
    """prints what the cases above measured (the last test of the file)"""
    for fam, w in WORST.items():
        print(fam + ":", ", ".join(f"{k} {v[0]:.3f}" for k, v in sorted(w.items())))
        print("   at", {k: v[1] for k, v in sorted(w.items())})
