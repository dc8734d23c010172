"""GPU: the CCT kernels (csrc/nrv_cct.hip) per element against the fp64 references and derived bounds of tests/cct_ref.py, on
the inputs tests/test_cct_ref_host.py proves the bounds on.  Method of test_pit_kernels_gpu.py: outputs are pre-filled with NaN,
every element is compared as error / bound <= 1 (the pool forward and its idx: exact equality), and every kernel runs twice with
bit-identical results.  The kernels' grids are exact (no capped grid-stride loop); the shapes cross workgroups, the half-full
last wave of the LayerNorm backward and every chunk count the LayerNorm dispatches."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cct_ref as R  # noqa: E402

from noise_robust_vit_amd import kernels as K  # noqa: E402

pytestmark = pytest.mark.gpu
POOL_SHAPES = [(H, W, C, g) for (H, W) in R.POOL_PLANES for C in R.POOL_C for g in R.POOL_GEOMS if R.pool_valid(H, W, g)]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def _nan(shape, dtype, dev):
    if dtype == torch.uint8:
        return torch.full(tuple(shape), 77, dtype=dtype, device=dev)       # no NaN in a byte: a tap no geometry has
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device=dev)


def _same(a, b):
    return all(torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x, y.view(torch.int16) if y.dtype == torch.bfloat16 else y)
               for x, y in zip(a, b) if x is not None)


@pytest.mark.parametrize("H,W,C,geom", POOL_SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_relu_maxpool(dev, H, W, C, geom, dtype):
    B, Ho, Wo = R.POOL_B, R.pool_out(H, geom), R.pool_out(W, geom)
    for kind in R.POOL_KINDS:
        for relu in (True, False):
            y, dout = R.pool_inputs(H, W, C, geom, kind, dtype)
            out, idx, dy, bound = R.pool_ref(y, dout, H, W, geom, relu)
            yd = y.to(dev)
            shape = (B * Ho * Wo, C)
            runs = [K.relu_maxpool_fwd(yd, B, H, W, *geom, relu=relu, out_f32=_nan(shape, torch.float32, dev),
                                       out_bf16=_nan(shape, torch.bfloat16, dev), idx=_nan(shape, torch.uint8, dev)) for _ in range(2)]
            assert _same(*runs)
            o32, o16, ix = runs[0]
            assert torch.equal(o32.cpu().double(), out), (kind, relu)                       # copied values: bit for bit
            assert torch.equal(o16.cpu().view(torch.int16), out.float().to(torch.bfloat16).view(torch.int16)), (kind, relu)
            assert torch.equal(ix.cpu(), idx), (kind, relu)
            dd = dout.to(dev)
            back = [K.relu_maxpool_bwd(dd, ix, B, H, W, *geom, dy=_nan((B * H * W, C), torch.bfloat16, dev)) for _ in range(2)]
            assert torch.equal(back[0].view(torch.int16), back[1].view(torch.int16))
            r = R.ratio(back[0], dy, bound)
            print("pool", (H, W, C, geom, str(dtype), kind, relu), "dy error / bound", r)
            assert r <= 1.0, (kind, relu, r)
            assert float(back[0][(dy == 0).to(dev)].abs().max() if bool((dy == 0).any()) else 0.0) == 0.0     # nobody selected: exact zeros
            if relu and kind == "negative":
                assert int((ix != 255).sum()) == 0 and float(o32.abs().max()) == 0.0 and float(back[0].abs().max()) == 0.0


def test_relu_maxpool_single_outputs(dev):
    """only the fp32 or only the bf16 output, as the tokenizer's last and inner layers ask for them"""
    H, W, C, geom = 7, 7, 72, (3, 2, 1)
    y, _ = R.pool_inputs(H, W, C, geom)
    both = K.relu_maxpool_fwd(y.to(dev), R.POOL_B, H, W, *geom, want_f32=True, want_bf16=True)
    o32, none16, i1 = K.relu_maxpool_fwd(y.to(dev), R.POOL_B, H, W, *geom, want_f32=True, want_bf16=False)
    none32, o16, i2 = K.relu_maxpool_fwd(y.to(dev), R.POOL_B, H, W, *geom, want_f32=False, want_bf16=True)
    assert none16 is None and none32 is None
    assert torch.equal(o32, both[0]) and torch.equal(o16.view(torch.int16), both[1].view(torch.int16))
    assert torch.equal(i1, both[2]) and torch.equal(i2, both[2])


LN_SHAPES = [(rows, dim, kind) for dim in R.LN_DIMS for rows in R.LN_ROWS for kind in ("random", "constant")] + [R.LN_BIG + ("random",)]


@pytest.mark.parametrize("rows,dim,kind", LN_SHAPES)
def test_layernorm_f32(dev, rows, dim, kind):
    """R.LN_BIG: more than 8 * 4096 rows, so a backward wave walks 9 rows and 911 partial rows are reduced"""
    i = R.ln_inputs(rows, dim, kind)
    ref = R.ln_ref(i)
    bounds = R.ln_bounds(i, ref)
    x, dy, g, b = (torch.from_numpy(i[k]).to(dev) for k in ("x", "dy", "gamma", "beta"))
    for with16 in (True, False):
        fw = [K.layernorm_f32_fwd(x, g, b, R.LN_EPS, y=_nan((rows, dim), torch.float32, dev),
                                  y_bf16=_nan((rows, dim), torch.bfloat16, dev) if with16 else None) for _ in range(2)]
        assert _same(*fw)
        y32, y16, mean, rstd = fw[0]
        assert (y16 is not None) == with16
        bw = [K.layernorm_f32_bwd(dy, x, g, mean, rstd, dx=_nan((rows, dim), torch.float32, dev),
                                  dx_bf16=_nan((rows, dim), torch.bfloat16, dev) if with16 else None) for _ in range(2)]
        assert _same(*bw)
        dx32, dx16, dg, db = bw[0]
        got = {"mean": mean, "rstd": rstd, "y": y32, "dx": dx32, "dgamma": dg, "dbeta": db}
        if with16:
            got.update(y16=y16.float(), dx16=dx16.float())
            assert torch.equal(y16.view(torch.int16), y32.to(torch.bfloat16).view(torch.int16))      # the copy: one rounding of y
            assert torch.equal(dx16.view(torch.int16), dx32.to(torch.bfloat16).view(torch.int16))
        ratios = R.ln_ratios({k: v.cpu().numpy() for k, v in got.items()}, ref, bounds)
        print("ln", (dim, rows, kind, with16), {k: round(v, 3) for k, v in ratios.items()})
        assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("n", R.SP_NS)
@pytest.mark.parametrize("D", R.SP_DS)
@pytest.mark.parametrize("kind", R.SP_KINDS)
def test_seqpool(dev, n, D, kind):
    B = R.SP_B
    y, a, bias, dout = R.seqpool_inputs(n, D, kind)
    w, bw, out, bo = R.seqpool_fwd_ref(y, a, bias, n)
    yd, ad, bd, dd = y.to(dev), a.to(dev), bias.to(dev), dout.to(dev)
    fw = [K.seqpool_fwd(yd, ad, bd, B, n, w=_nan((B, n), torch.float32, dev), out=_nan((B, D), torch.float32, dev)) for _ in range(2)]
    assert _same(*fw)
    gw, gout = fw[0]
    r1, r2 = R.ratio(gw, w, bw), R.ratio(gout, out, bo)
    assert bool(torch.isfinite(gw).all()) and bool(torch.isfinite(gout).all())
    if n == 1:
        assert bool((gw == 1.0).all())
    if kind == "peaked":
        for b, t in R.sp_low_rows(n):
            assert float(gw[b, t]) == 0.0                                   # 180 nats below the maximum: an exact zero
    w32 = w.float()
    ref = R.seqpool_bwd_ref(dout, y, a, w32, n)
    bk = [K.seqpool_bwd(dd, yd, ad, w32.to(dev), B, n, dy=_nan((B * n, D), torch.float32, dev)) for _ in range(2)]
    assert _same(*bk)
    rs = {k: R.ratio(t, *ref[k]) for k, t in zip(("dy", "da", "dbias"), bk[0])}
    print("seqpool", (n, D, kind), "error / bound: w", r1, "out", r2, rs)
    assert r1 <= 1.0 and r2 <= 1.0 and all(v <= 1.0 for v in rs.values()), (r1, r2, rs)
    if n == 1:
        assert float(bk[0][1].abs().max()) == 0.0 and float(bk[0][2].abs().max()) == 0.0      # w = 1: da and dbias are exact zeros
