"""CPU: the float64 AdamW reference of tests/optim_ref.py is clip_grad_norm_ + torch.optim.AdamW; its per-element bounds hold for
the fp32 restatement of `adamw_one` (plain and with either contraction of the last line) on every case the GPU test runs
(error / bound <= 1, the worst printed); each mistake of optim_ref.MISTAKES puts a named case over a bound; and the restated
summation tree of nrv_sumsq_f32 stays inside `sumsq_ref`'s bound while a tree without the tail loop leaves it on the cases that
put energy into the tail -- and passes the 2e-6 check tests/test_optim_gpu.py makes at n = 1 000 003."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ref as R  # noqa: E402

# one case per mistake that must catch it (the test prints how many of the table do)
CAUGHT_BY = {
    "omb2_in_float": "zeros_with_state-n3073-t1-trainer-none-f32",
    "eps_before_bias_correction": "tiny-n3073-t2-no_decay-none-f32",
    "decay_after_update": "zeros_with_state-n3073-t100000-big_eps-none-f32",
    "bias_correction_of_previous_step": "random_1-n3073-t2-trainer-none-f32",
    "clip_without_1e-6": "tiny-n3073-t1-no_decay-below-f32",
    "clip_not_clamped": "random_1-n3073-t2-trainer-above-f32",
    "v_from_unclipped_gradient": "random_1-n3073-t2-trainer-below-f32",
    "tail_unclipped": "spike_tail-n3073-t2-trainer-below-f32",
    "bf16_halves_swapped": "random_1e-3-n5-t2-trainer-below-bf16",
    "decay_on_moment": "zeros_with_state-n3073-t1000-trainer-below-f32",
}


@pytest.fixture(scope="module")
def refs():
    return {c.name: c.ref() for c in R.CASES}


def _ratios(out, ref):
    return {k: R.ratio(o, ref[k], ref[k + "_bound"]) for k, o in zip("pmv", out)}


def test_the_table_covers_every_axis():
    assert {c.n for c in R.CASES} == set(R.LENGTHS) and {c.t for c in R.CASES} == set(R.STEPS)
    assert {c.kind for c in R.CASES} == set(R.KINDS) and {c.hyper for c in R.CASES} == set(R.HYPERS)
    assert {c.clip for c in R.CASES} == set(R.CLIPS) and {c.gdt for c in R.CASES} == set(R.GRAD_DTYPES)
    for n in R.LENGTHS:                                      # every length with every kind and both gradient types
        for kind in R.KINDS:
            if kind == "spike_tail" and n % 4 == 0:
                continue
            assert {c.gdt for c in R.CASES if c.n == n and c.kind == kind} == set(R.GRAD_DTYPES), (n, kind)
    sweep = {(c.t, c.hyper, c.clip, c.kind) for c in R.CASES if c.n == R.SWEEP_N}
    assert len(sweep) == len(R.STEPS) * len(R.HYPERS) * len(R.CLIPS) * len(R.KINDS)
    assert R.sumsq_blocks(1048576 + 7) == 1024 and R.sumsq_blocks(1048576) == 1024 and R.sumsq_depth(1048576 + 7) == R.sumsq_depth(1048576) + 5
    for c in R.CASES:                                        # what the kinds and the max_norm settings promise
        p, g, m, v, gn, mx = c.arrays()
        coef = R.clip_coef(gn, mx)
        assert (v >= 0).all()
        if c.t == 1 and c.kind != "zeros_with_state":
            assert not m.any() and not v.any()
        if c.kind == "tiny":
            assert 1e-12 * 0.99 <= np.abs(g).min() and np.abs(g).max() <= 1e-8 * 1.01
        if c.kind == "spike_tail":
            assert not g[:c.n // 4 * 4].any() and g[c.n // 4 * 4:].all()
        if c.clip in ("none", "above"):
            assert coef == 1.0
        elif c.clip == "below":
            assert coef < 0.03 or gn == 0.0                  # n = 1 of zeros_with_state: the one gradient is the zero
        else:
            assert abs(coef - 1.0) < 1e-6


@pytest.mark.parametrize("hyper", list(R.HYPERS))
@pytest.mark.parametrize("max_norm", [0.0, 0.5])
def test_the_reference_is_torch_adamw_after_clip_grad_norm(hyper, max_norm):
    """three steps from zero state on float64 CPU tensors, 1e-12 relative per element (hyper-parameters kept in double on both
    sides); rounding them as the C entry does moves the reference by a few units of 2^-24 of its terms, no more"""
    lr, b1, b2, eps, wd = R.HYPERS[hyper]
    n = 257
    g0 = torch.Generator().manual_seed(3)
    p = torch.randn(n, generator=g0, dtype=torch.float64)
    tp = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    pn, m, v = p.numpy().copy(), np.zeros(n), np.zeros(n)
    for t in (1, 2, 3):
        g = torch.randn(n, generator=g0, dtype=torch.float64) * 0.1
        tp.grad = g.clone()
        gn = float((g * g).sum())
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([tp], max_norm)
        opt.step()
        r = R.adamw_ref(pn, g.numpy(), m, v, lr, b1, b2, eps, wd, t, gn if max_norm > 0 else None, max_norm, round_hyper=False)
        rr = R.adamw_ref(pn, g.numpy(), m, v, lr, b1, b2, eps, wd, t, gn if max_norm > 0 else None, max_norm)
        st = opt.state[tp]
        for k, want in (("p", tp.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
            want = want.numpy()
            assert np.abs(r[k] - want).max() <= 1e-12 * np.abs(want).max() and (np.abs(r[k] - want) <= 1e-12 * np.abs(want) + 1e-300).all(), (k, t)
            assert (np.abs(rr[k] - r[k]) <= 8 * r[k + "_bound"]).all(), (k, t)
        pn, m, v = r["p"], r["m"], r["v"]


def test_the_bounds_hold_for_the_restatement(refs):
    worst = {}
    for c in R.CASES:
        for con in R.CONTRACTIONS:
            rs = _ratios(R.restated(c, contract=con), refs[c.name])
            assert all(r <= 1.0 for r in rs.values()), (c, con, rs)
            for k, r in rs.items():
                if r > worst.get(k, (0.0,))[0]:
                    worst[k] = (r, c.name, con)
    print("restated adamw_one, worst error / bound over", len(R.CASES), "cases x 3 contractions:", worst)


def test_the_contractions_are_different_roundings(refs):
    """so the three restatements are three checks, not one"""
    c = R.CASE_BY_NAME["random_1-n3073-t2-trainer-below-f32"]
    a, b, d = (R.restated(c, contract=con)[0] for con in R.CONTRACTIONS)
    assert (a != b).any() and (a != d).any() and (b != d).any()


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_each_mistake_exceeds_a_bound(refs, mistake):
    caught = []
    for c in R.CASES:
        rs = _ratios(R.restated(c, mistake=mistake), refs[c.name])
        if max(rs.values()) > 1.0:
            caught.append((c.name, rs))
    names = {n for n, _ in caught}
    print(mistake, "caught by", len(caught), "of", len(R.CASES), "cases; named:", CAUGHT_BY[mistake],
          dict(caught).get(CAUGHT_BY[mistake]))
    assert CAUGHT_BY[mistake] in names, (mistake, sorted(names)[:5])
    if mistake == "eps_before_bias_correction":
        # (sqrt(v) + eps) / sqrt(1 - b2^t) differs from the kernel's by eps (1 / sqrt(1 - b2^t) - 1): 30.6 eps at t = 1 and exactly
        # nothing once b2^t has vanished in fp32 -- caught for small t only, where sqrt(v) is not far above eps
        assert not any(R.CASE_BY_NAME[n].t == 100000 for n in names)
        assert {R.CASE_BY_NAME[n].t for n in names} >= {1, 2, 10}
    if mistake == "tail_unclipped":
        assert all(R.CASE_BY_NAME[n].n % 4 for n in names)
    if mistake == "bf16_halves_swapped":
        assert all(R.CASE_BY_NAME[n].gdt == "bf16" for n in names)


def test_a_nan_or_infinite_norm_in_the_reference():
    """clip_grad_norm_ with a NaN norm multiplies every gradient by NaN; an infinite norm gives coef = 0"""
    c = R.CASE_BY_NAME["random_1-n3073-t2-trainer-below-f32"]
    p, g, m, v, _, mx = c.arrays()
    r = R.adamw_ref(p, g, m, v, *c.args(), np.float32("nan"), 1.0)
    assert all(np.isnan(r[k]).all() for k in "pmv")
    out = R.restated_step(p, g, m, v, *c.args(), np.float32("nan"), 1.0)
    assert all(np.isnan(o).all() for o in out)
    r = R.adamw_ref(p, g, m, v, *c.args(), np.float32("inf"), 1.0)
    z = R.adamw_ref(p, np.zeros_like(g), m, v, *c.args(), None, 0.0)
    assert all(np.array_equal(r[k], z[k]) for k in "pmv")
    out = R.restated_step(p, g, m, v, *c.args(), np.float32("inf"), 1.0)
    assert all(R.ratio(o, z[k], z[k + "_bound"]) <= 1.0 for k, o in zip("pmv", out))


def test_bf16_rounding_is_torchs():
    x = torch.randn(4099, generator=torch.Generator().manual_seed(1)) * 1e-3
    assert np.array_equal(R.to_bf16(x.numpy()), x.to(torch.bfloat16).float().numpy())


# ---- sum of squares ------------------------------------------------------------------------------
@pytest.mark.parametrize("gdt", R.GRAD_DTYPES)
def test_the_restated_sum_tree_is_within_the_bound(gdt):
    worst = (0.0, ())
    for n, kind, g in R.SUMSQ_CASES:
        if g != gdt:
            continue
        x = R.sumsq_input(n, kind, gdt)
        s, b = R.sumsq_ref(x)
        got = R.sumsq_restated(x)
        r = 0.0 if got == s else abs(got - s) / b
        assert r <= 1.0, (n, kind, r)
        worst = max(worst, (r, (n, kind)))
        if kind == "ones":
            assert got == float(n)
    print("restated sumsq", gdt, "worst error / bound:", worst)
    for n in R.SUMSQ_LENGTHS:
        x = R.edge_powers(n)
        assert R.sumsq_restated(x) == float((x.astype(np.float64) ** 2).sum()) and np.array_equal(R.to_bf16(x), x)


def test_a_sum_without_the_tail_loop():
    """fails the spike_tail, all-ones and edge cases of every length with a tail ..."""
    for n in R.SUMSQ_LENGTHS:
        if n % 4 == 0:
            continue
        for kind in ("spike_tail", "ones"):
            x = R.sumsq_input(n, kind, "f32")
            s, b = R.sumsq_ref(x)
            assert abs(R.sumsq_restated(x, omit_tail=True) - s) > b, (n, kind)
        x = R.edge_powers(n)
        assert R.sumsq_restated(x, omit_tail=True) != float((x.astype(np.float64) ** 2).sum())
    # ... and passes what tests/test_optim_gpu.py asserts at n = 1 000 003 (|sqrt(sum) - norm| <= 2e-6 norm, iid gradients): the
    # three tail elements are 3e-6 of the energy, 1.5e-6 of the norm
    n = 1000003
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)).numpy()
    total = math.sqrt(float((x.astype(np.float64) ** 2).sum()))
    got = math.sqrt(R.sumsq_restated(x, omit_tail=True))
    rel = abs(got - total) / total
    print("sum without its tail at n = 1000003: relative error of the norm", rel)
    assert 2e-7 < rel <= 2e-6
    s, b = R.sumsq_ref(x)
    assert abs(R.sumsq_restated(x) - s) <= b           # (three elements of a million iid ones are inside the rounding bound too)
