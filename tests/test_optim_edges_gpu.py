"""GPU: nrv_sumsq_f32 and nrv_adamw_f32 (csrc/nrv_optim.hip) per element against the float64 references and derived bounds of
tests/optim_ref.py, on the cases tests/test_optim_ref_host.py proves the bounds on and shows ten wrong kernels to break.

Every call goes through kernels.sumsq / kernels.adamw_flat and runs twice from the same inputs with bit-identical results.  The
gradient (and the operand of sumsq) is a copy in the middle of a NaN-filled storage; p, m and v, the output scalar, the norm the
step reads and the workspace lie between guard blocks of a NaN payload no kernel produces (parity_tools), which must come back
untouched.  Judged as error / bound <= 1 per element; where the arithmetic is exact (all-ones and power-of-two sums, a step from
p = 1 with nothing else, a norm below max_norm against no clipping, bf16 gradients against their fp32 values) the bits are compared.
A NaN norm makes every element NaN, as clip_grad_norm_ followed by AdamW does: `c < 1 ? c : 1` in adamw_kernel let a NaN norm
through as coef = 1 (the finite elements stepped unclipped) until the clamp was turned round with these tests.

Measured on an MI355X (worst error / bound per family, as test_zz_worst_ratios prints them; 39 tests in 4.0 s, the slowest 0.37 s):
  sumsq         fp32 0.076 (n = 1025, random 1e-3)   bf16 0.068 (n = 1025, tiny)
  kernel cases  p 0.794 (spike_tail-n3073-t1-big_eps-edge-f32)   m 0.990 (random_1e-3-n3073-t2-trainer-below-f32)
                v 0.998 (spike_tail-n3073-t1000-big_eps-edge-f32)          over the 611 cases of optim_ref.CASES
The sumsq, m and v figures equal the CPU restatement's to every printed digit: the kernel adds and rounds exactly as restated.  m and
v come that close to 1 on elements whose gradient term is zero or negligible -- the bound is then the ONE rounding of the fma, u |x|,
which an x just above a power of two nearly uses up; it cannot be exceeded.  p is at 0.99 in the plain restatement and at 0.79 on the
device: the compiler contracts the last line into an fma, one of the two contractions the bound allows for.  No guard, moat, norm or
workspace tail was touched, every rerun was bit-identical and every exact count was exact: beyond the NaN clamp these cases found
no defect in the kernels.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ref as R  # noqa: E402
from parity_tools import _Out, _moated  # noqa: E402

from noise_robust_vit_amd import kernels as K  # noqa: E402
from noise_robust_vit_amd._lib import NrvError  # noqa: E402

pytestmark = pytest.mark.gpu
f32, bf = torch.float32, torch.bfloat16
WORST = {}


def _worst(family, key, r, what):
    if r >= WORST.get((family, key), (-1.0, None))[0]:
        WORST[(family, key)] = (r, what)


def _grad(g, gdt, dev):
    t = torch.from_numpy(np.ascontiguousarray(g))
    return _moated(t.to(bf) if gdt == "bf16" else t, dev)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf else torch.int32)


def _workspace(n, dev):
    return _Out(max(K.sumsq_workspace(n) // 4, 4), f32, dev)


# ---- sum of squares ------------------------------------------------------------------------------
def _sumsq(x, gdt, dev):
    """sumsq of the numpy vector x through guarded buffers, twice: the fp32 result as a Python float"""
    xd = _grad(x, gdt, dev)
    got = []
    for _ in range(2):
        out, ws = _Out(1, f32, dev), _workspace(x.size, dev)
        K.sumsq(xd, out.t, ws.t)
        got.append(out.done("sumsq out")[0].item())
        ws.done("sumsq workspace", written=False)
        assert not bool(torch.isnan(ws.t[:R.sumsq_blocks(x.size)]).any()) and bool(torch.isnan(ws.t[R.sumsq_blocks(x.size):]).all())
    assert got[0] == got[1]
    return got[0]


@pytest.mark.parametrize("gdt", R.GRAD_DTYPES)
@pytest.mark.parametrize("kind", R.SUMSQ_KINDS)
def test_sumsq_values(dev, kind, gdt):
    bad = []
    for n, k, g in R.SUMSQ_CASES:
        if (k, g) != (kind, gdt):
            continue
        x = R.sumsq_input(n, kind, gdt)
        s, b = R.sumsq_ref(x)
        got = _sumsq(x, gdt, dev)
        r = 0.0 if got == s else abs(got - s) / b
        _worst("sumsq", gdt, r, (n, kind))
        if not r <= 1.0:
            bad.append((n, r))
        if kind == "ones":                                  # every partial sum is an integer below 2^24
            assert got == float(n), (n, got)
    print("sumsq", kind, gdt, "worst error / bound so far:", WORST.get(("sumsq", gdt)))
    assert not bad, bad


@pytest.mark.parametrize("gdt", R.GRAD_DTYPES)
def test_sumsq_of_powers_of_two_at_the_loop_edges_is_exact(dev, gdt):
    for n in R.SUMSQ_LENGTHS:
        x = R.edge_powers(n)
        assert _sumsq(x, gdt, dev) == float((x.astype(np.float64) ** 2).sum()), (n, R.edge_indices(n))


# ---- AdamW ---------------------------------------------------------------------------------------
def _step(c_args, p, g, m, v, gn, mx, gdt, dev):
    """One call of adamw_flat on guarded copies of the numpy inputs, twice: (p, m, v) as CPU tensors.  `gn`: None or a float"""
    gd = _grad(g, gdt, dev)
    runs = []
    for _ in range(2):
        bufs = [_Out(p.size, f32, dev, preset=torch.from_numpy(a)) for a in (p, m, v)]
        norm = _Out(1, f32, dev, preset=torch.tensor([gn], dtype=f32)) if gn is not None else None
        K.adamw_flat(bufs[0].t, gd, bufs[1].t, bufs[2].t, *c_args, norm.t if norm is not None else None, float(mx))
        outs = [b.done("adamw " + name, written=False).cpu() for b, name in zip(bufs, "pmv")]
        if norm is not None:
            assert torch.equal(_bits(norm.done("gnorm_sq", written=False).cpu()), _bits(torch.tensor([gn], dtype=f32)))
        runs.append(outs)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*runs))
    return runs[0]


def _judge(outs, ref):
    return {k: R.ratio(o.numpy(), ref[k], ref[k + "_bound"]) for k, o in zip("pmv", outs)}


def _run_case(c, dev):
    p, g, m, v, gn, mx = c.arrays()
    outs = _step(c.args(), p, g, m, v, None if gn is None else float(gn), mx, c.gdt, dev)
    rs = _judge(outs, c.ref())
    for k, r in rs.items():
        _worst("adamw", k, r, c.name)
    if c.gdt == "bf16":                                     # the same kernel on the converted values, bit for bit
        again = _step(c.args(), p, g, m, v, None if gn is None else float(gn), mx, "f32", dev)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(outs, again)), c
    if c.clip == "above":                                   # coef is exactly 1: the bits of the unclipped call
        again = _step(c.args(), p, g, m, v, None, 0.0, c.gdt, dev)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(outs, again)), c
    return rs


@pytest.mark.parametrize("gdt", R.GRAD_DTYPES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_adamw_cases(dev, kind, gdt):
    cases = [c for c in R.CASES if (c.kind, c.gdt) == (kind, gdt)]
    assert cases
    bad = {}
    for c in cases:
        rs = _run_case(c, dev)
        if not all(r <= 1.0 for r in rs.values()):
            bad[c.name] = rs
    print("adamw", kind, gdt, len(cases), "cases; worst error / bound so far:", {k: WORST.get(("adamw", k)) for k in "pmv"})
    assert not bad, bad


@pytest.mark.parametrize("gdt", R.GRAD_DTYPES)
@pytest.mark.parametrize("clipped", [False, True])
def test_adamw_of_nothing_leaves_the_decay_everywhere(dev, gdt, clipped):
    """p = 1, g = m = v = 0: exactly float32(1 - lr wd) in every element, zeros in m and v -- an element visited twice or never
    shows at once"""
    lr, b1, b2, eps, wd = R.HYPERS["trainer"]
    want = float(np.float32(1.0 - lr * wd))
    for n in R.LENGTHS:
        z = np.zeros(n, dtype=np.float32)
        p, m, v = _step((lr, b1, b2, eps, wd, 3), np.ones(n, dtype=np.float32), z, z, z, 0.0 if clipped else None,
                        1.0 if clipped else 0.0, gdt, dev)
        assert torch.equal(p, torch.full((n,), want)) and not bool(m.any()) and not bool(v.any()), n


def test_adamw_with_an_infinite_norm_steps_with_a_zero_gradient(dev):
    for name in ("random_1-n3073-t2-trainer-below-f32", "random_1e-3-n5-t2-trainer-below-bf16"):
        c = R.CASE_BY_NAME[name]
        p, g, m, v, _, _ = c.arrays()
        outs = _step(c.args(), p, g, m, v, float("inf"), 1.0, c.gdt, dev)
        ref = R.adamw_ref(p, np.zeros_like(g), m, v, *c.args(), None, 0.0)
        rs = _judge(outs, ref)
        assert all(r <= 1.0 for r in rs.values()), rs
        again = _step(c.args(), p, np.zeros_like(g), m, v, None, 0.0, c.gdt, dev)
        assert all(torch.equal(a, b) for a, b in zip(outs, again))


@pytest.mark.parametrize("n", [1, 5, 1024, 4 * 256 * 3 + 1])
def test_adamw_with_a_nan_norm_makes_every_element_nan(dev, n):
    """what clip_grad_norm_ + AdamW do: the coefficient is NaN, so every gradient, moment and parameter is"""
    c = R.Case(n, "random_1", 2, "trainer", "below", "f32")
    p, g, m, v, _, _ = c.arrays()
    outs = _step(c.args(), p, g, m, v, float("nan"), 1.0, "f32", dev)
    assert all(bool(torch.isnan(o).all()) for o in outs)
    outs = _step(c.args(), p, g, m, v, float("nan"), 0.0, "f32", dev)         # no clipping asked for: the norm is not read
    assert all(r <= 1.0 for r in _judge(outs, R.adamw_ref(p, g, m, v, *c.args(), None, 0.0)).values())


def test_refusals(dev):
    n = 64
    x = torch.ones(n + 8, device=dev)
    x16 = torch.ones(n + 8, device=dev, dtype=bf)
    out = torch.zeros(1, device=dev)
    ws = torch.empty(max(K.sumsq_workspace(n) // 4, 4), device=dev)
    ok = (3e-3, 0.9, 0.999, 1e-8, 0.05, 1)

    def adamw(p=None, g=None, m=None, v=None, args=ok):
        a = [t if t is not None else torch.zeros(n, device=dev) for t in (p, g, m, v)]
        K.adamw_flat(*a, *args, None, 0.0)

    K.sumsq(x[:n], out, ws)
    adamw()                                                # the calls below differ from these two by one thing each
    with pytest.raises(NrvError):
        K.sumsq(x[:0], out, ws)
    with pytest.raises(NrvError):
        K.sumsq(x[:n], out, ws[:ws.numel() - 1])
    with pytest.raises(NrvError):
        K.sumsq(x[1:1 + n], out, ws)
    with pytest.raises(NrvError):
        K.sumsq(x16[2:2 + n], out, ws)
    with pytest.raises(NrvError):
        K.adamw_flat(x[:0], x[:0], x[:0], x[:0], *ok, None, 0.0)
    for bad in ((3e-3, 0.9, 0.999, 1e-8, 0.05, 0), (3e-3, 1.0, 0.999, 1e-8, 0.05, 1), (3e-3, 0.9, 1.0, 1e-8, 0.05, 1),
                (3e-3, 0.9, 0.999, -1e-8, 0.05, 1)):
        with pytest.raises(NrvError):
            adamw(args=bad)
    for which in "pgmv":
        with pytest.raises(NrvError):
            adamw(**{which: x[1:1 + n]})
    with pytest.raises(NrvError):
        adamw(g=x16[2:2 + n])
    assert out.item() == float(n)


def test_zz_worst_ratios(dev):
    """prints the figures of the docstring (after the cases above have run)"""
    for key in sorted(WORST):
        print("worst error / bound", key, WORST[key])
    assert all(r <= 1.0 for r, _ in WORST.values())
