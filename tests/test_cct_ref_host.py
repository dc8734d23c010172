"""CPU: the references and bounds of tests/cct_ref.py.  For every kernel family the fp32 emulation of the kernel's arithmetic
stays inside the derived bound (per element, error / bound <= 1) on the inputs the GPU test uses, and wrong kernels break it:
a last-maximum tie rule, a pool backward that ignores the 255 ReLU mark, a LayerNorm backward without the mean of dy gamma and a
sequence-pool backward without the sum_m w_m t_m term.  Also: autograd's rule on tied inputs is the kernel's rule, and the
sequence-pool formulas are autograd's."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cct_ref as R  # noqa: E402

POOL_SHAPES = [(H, W, g) for (H, W) in R.POOL_PLANES for g in R.POOL_GEOMS if R.pool_valid(H, W, g)]


@pytest.mark.parametrize("H,W,geom", POOL_SHAPES)
@pytest.mark.parametrize("kind", R.POOL_KINDS)
@pytest.mark.parametrize("relu", [True, False])
def test_pool_emulation_is_the_reference(H, W, geom, kind, relu):
    C = 8
    for dtype in (torch.float32, torch.bfloat16):
        y, dout = R.pool_inputs(H, W, C, geom, kind, dtype)
        out, idx, dy, bound = R.pool_ref(y, dout, H, W, geom, relu)
        e_out, e_idx = R.pool_fwd_emul(y, H, W, geom, relu)
        assert torch.equal(e_out.double(), out) and torch.equal(e_idx, idx)
        r = R.ratio(R.pool_bwd_emul(dout, e_idx, H, W, geom), dy, bound)
        assert r <= 1.0, r
        if relu and kind == "negative":
            assert int((idx != 255).sum()) == 0 and float(out.abs().max()) == 0.0 and float(dy.abs().max()) == 0.0
        assert bool((bound[dy == 0] >= 0).all())


def test_pool_geometry_table_names_the_plane_that_does_not_fit():
    assert not R.pool_valid(1, 1, (2, 2, 0)) and len(POOL_SHAPES) == 3 * len(R.POOL_PLANES) - 1


def test_wrong_pool_kernels_break_the_checks():
    H, W, C, geom = 7, 7, 8, (3, 2, 1)
    y, dout = R.pool_inputs(H, W, C, geom, "grid")
    out, idx, dy, bound = R.pool_ref(y, dout, H, W, geom, True)
    # a last-maximum tie rule: same values, other taps, and the gradient lands on other elements
    l_out, l_idx = R.pool_fwd_emul(y, H, W, geom, True, tie="last")
    assert torch.equal(l_out.double(), out) and not torch.equal(l_idx, idx)
    assert R.ratio(R.pool_bwd_emul(dout, l_idx, H, W, geom), dy, bound) > 1.0
    # a backward that ignores the 255 mark: windows whose maximum is <= 0 pass their gradient on
    _, u_idx = R.pool_fwd_emul(y, H, W, geom, True, mark=False)
    assert int((idx == 255).sum()) > 0 and R.ratio(R.pool_bwd_emul(dout, u_idx, H, W, geom), dy, bound) > 1.0
    y, dout = R.pool_inputs(H, W, C, geom, "negative")
    out, idx, dy, bound = R.pool_ref(y, dout, H, W, geom, True)
    _, u_idx = R.pool_fwd_emul(y, H, W, geom, True, mark=False)
    assert R.ratio(R.pool_bwd_emul(dout, u_idx, H, W, geom), dy, bound) == float("inf") or \
        R.ratio(R.pool_bwd_emul(dout, u_idx, H, W, geom), dy, bound) > 1.0


@pytest.mark.parametrize("dim", R.LN_DIMS)
@pytest.mark.parametrize("rows", R.LN_ROWS)
@pytest.mark.parametrize("kind", ["random", "constant"])
def test_layernorm_emulation_is_inside_the_bounds(dim, rows, kind):
    i = R.ln_inputs(rows, dim, kind)
    ref = R.ln_ref(i)
    bounds = R.ln_bounds(i, ref)
    ratios = R.ln_ratios(R.ln_emul(i), ref, bounds)
    print(dim, rows, kind, {k: round(v, 3) for k, v in ratios.items()})
    assert all(v <= 1.0 for v in ratios.values()), ratios
    if kind == "constant":
        assert float(np.abs(ref["y"] - i["beta"].astype(np.float64)).max()) == 0.0       # variance 0: y = beta


def test_layernorm_emulation_with_the_longer_wave_loop():
    rows, dim = R.LN_BIG
    assert R.ln_rpw(rows) == (9, 911) and R.ln_rpw(37) == (8, 2) and R.ln_rpw(32768) == (8, 1024)
    i = R.ln_inputs(rows, dim)
    ref = R.ln_ref(i)
    ratios = R.ln_ratios(R.ln_emul(i), ref, R.ln_bounds(i, ref))
    assert all(v <= 1.0 for v in ratios.values()), ratios


def test_a_layernorm_backward_without_the_mean_term_breaks_the_bound():
    i = R.ln_inputs(37, 136)
    i["dy"] = (i["dy"] + 0.5).astype(np.float32)                          # a mean of dy gamma that is not small
    ref = R.ln_ref(i)
    ratios = R.ln_ratios(R.ln_emul(i, wrong="no_c2"), ref, R.ln_bounds(i, ref))
    assert ratios["dx"] > 1.0 and ratios["dx16"] > 1.0 and ratios["y"] <= 1.0 and ratios["dgamma"] <= 1.0


@pytest.mark.parametrize("n", [n for n in R.SP_NS if n <= 257])
@pytest.mark.parametrize("D", R.SP_DS)
@pytest.mark.parametrize("kind", R.SP_KINDS)
def test_seqpool_emulation_is_inside_the_bounds(n, D, kind):
    y, a, bias, dout = R.seqpool_inputs(n, D, kind)
    w, bw, out, bo = R.seqpool_fwd_ref(y, a, bias, n)
    ew, eo = R.seqpool_fwd_emul(y, a, bias, n)
    assert R.ratio(ew, w, bw) <= 1.0 and R.ratio(eo, out, bo) <= 1.0
    if n == 1:
        assert bool((ew == 1.0).all())
    if kind == "equal":
        assert float((w - 1.0 / n).abs().max()) <= 1e-15
    if kind == "peaked":
        for b, t in R.sp_low_rows(n):
            assert float(ew[b, t]) == 0.0 and 0.0 < float(w[b, t]) < 1e-70      # fp32 underflows to an exact 0, fp64 does not
    w32 = w.float()
    ref = R.seqpool_bwd_ref(dout, y, a, w32, n)
    got = R.seqpool_bwd_emul(dout, y, a, w32, n)
    for k, (r, bnd) in ref.items():
        assert R.ratio(got[k], r, bnd) <= 1.0, k
    if n == 1:
        assert float(got["da"].abs().max()) == 0.0 and float(got["dbias"].abs().max()) == 0.0


def test_a_seqpool_backward_without_the_weighted_mean_breaks_the_bound():
    n, D = 16, 72
    y, a, bias, dout = R.seqpool_inputs(n, D)
    w32 = R.seqpool_fwd_ref(y, a, bias, n)[0].float()
    ref = R.seqpool_bwd_ref(dout, y, a, w32, n)
    got = R.seqpool_bwd_emul(dout, y, a, w32, n, wrong="no_s")
    assert R.ratio(got["dy"], *ref["dy"]) > 1.0 and R.ratio(got["da"], *ref["da"]) > 1.0 and R.ratio(got["dbias"], *ref["dbias"]) > 1.0


def test_seqpool_formulas_are_autograd():
    n, D = 16, 8
    y, a, bias, dout = R.seqpool_inputs(n, D)
    y3 = y.double().reshape(R.SP_B, n, D).requires_grad_(True)
    a64, b64 = a.double().requires_grad_(True), bias.double().requires_grad_(True)
    w = torch.softmax(y3 @ a64 + b64, dim=1)
    torch.einsum("bn,bnd->bd", w, y3).backward(dout.double())
    ref = R.seqpool_bwd_ref(dout.double(), y.double(), a.double(), w.detach(), n)
    assert float((ref["dy"][0] - y3.grad.reshape(-1, D)).abs().max()) <= 1e-14
    assert float((ref["da"][0] - a64.grad).abs().max()) <= 1e-14 and float((ref["dbias"][0] - b64.grad).abs().max()) <= 1e-14
