"""GPU: optim.FusedAdamW behind train.Trainer on a plain nn.Module (no HIP forward), every step judged per element against
tests/optim_ref.adamw_ref applied to the device's own state before that step -- so the bound needs no propagation analysis.

The module has parameters of 13, 5 x 7, 64, 3 and 9 elements (slots of 16, 40, 64, 8 and 16 in the flat buffers, in reverse
registration order); `off` names the parameters the loss leaves out, the 9-element one being the branch a flag turns off.  Covered:
all parameters with clipping (p, m, v, the norm against the float64 norm within sumsq_ref's bound, the padding between the slots
exactly zero); parameters without a gradient (`_active_ranges`: skipped at the front, at the back, two neighbours in the middle --
bits unchanged, the clip norm taken over the others, and a returning parameter stepped with the optimizer's GLOBAL step count, which
optim.py documents as its one difference from torch's per-parameter count); and state_dict / load_state_dict into a twin whose
`grad_groups()` gives other slot offsets (bit-equal continuation without clipping, within bound with it, and the refusals).

Measured on an MI355X (worst error / bound over all steps of all tests, as test_zz_worst_ratios prints them; 11 tests in 2.7 s):
  FusedAdamW    p 0.479   m 0.721   v 0.883   sum of squares 0.062
  the returning parameter at step 4: 0.43 of the bound with the global count, 10887 bounds away from the per-parameter count.
Nothing here found a defect in optim.py or parallel.py.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ref as R  # noqa: E402

from noise_robust_vit_amd._lib import NrvError  # noqa: E402
from noise_robust_vit_amd.parallel import _slot_len  # noqa: E402
from noise_robust_vit_amd.train import TrainConfig, Trainer  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = (("a", (13,)), ("b", (5, 7)), ("c", (64,)), ("d", (3,)), ("e", (9,)))
LR, WD = 3e-3, 0.05
WORST = {}


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(11)
        for name, shape in SIZES:
            setattr(self, name, torch.nn.Parameter(torch.randn(shape, generator=gen)))
        self.off = set()                      # parameters the loss leaves out this step ("e": the branch behind a flag)

    def forward(self, x):
        total = x.new_zeros(())
        for k, (name, _) in enumerate(SIZES):
            if name not in self.off:
                w = getattr(self, name)
                total = total + (torch.tanh(w * x[k]) * (k + 1.0)).sum() + (w * w).sum() * x[5 + k]
        return total


class ToyGrouped(Toy):
    """the same parameters; a and c are laid out back to back, so every slot after e and d moves"""
    def grad_groups(self):
        return [(self.a, self.c)]


def _make(cls, dev, max_norm):
    model = cls().to(dev)
    return model, Trainer(model, TrainConfig(lr=LR, weight_decay=WD, grad_max_norm=max_norm), compute_loss=lambda m, x, y: m(x))


def _inputs(steps, dev):
    g = torch.Generator().manual_seed(29)
    return [(torch.randn(10, generator=g) * 0.7).to(dev) for _ in range(steps)]


def _np(t):
    return t.detach().cpu().numpy().copy()


def _slots(tr, model):
    return {name: tr.reducer.slot(getattr(model, name)) for name, _ in SIZES}


def _step(tr, model, x, off=(), label=""):
    """One Trainer step with the parameters `off` left out of the loss, judged against adamw_ref on the state before it"""
    opt = tr.opt
    model.off = set(off)
    tr.forward_backward(x, None)
    before = {k: _np(t) for k, t in (("p", opt.param), ("m", opt.exp_avg), ("v", opt.exp_avg_sq))}
    g = _np(tr.reducer.flat)
    tr.optimizer_step()
    after = {k: _np(t) for k, t in (("p", opt.param), ("m", opt.exp_avg), ("v", opt.exp_avg_sq))}
    mx = tr.cfg.grad_max_norm
    gn = None
    slots = _slots(tr, model)
    if mx > 0:
        gn = np.float32(opt.gnorm_sq.item())
        for name in off:                                   # nothing of a parameter without a gradient enters the norm
            o, n = slots[name]
            assert not g[o:o + _slot_len(n)].any()
        active = np.concatenate([g[o:o + n] for name, (o, n) in slots.items() if name not in off]).astype(np.float64)
        want = float((active * active).sum())              # the float64 norm over the parameters that did get gradients
        _, bound = R.sumsq_ref(g)                           # the tree is that of the whole buffer; skipped slots and padding add zeros
        r = 0.0 if float(gn) == want else abs(float(gn) - want) / bound
        _worst("norm", r, label)
        assert r <= 1.0, (label, r)
        assert abs(opt.grad_norm().item() - np.sqrt(want)) <= (bound / want + 2.0 ** -23) * np.sqrt(want)
    ref = R.adamw_ref(before["p"], g, before["m"], before["v"], LR, 0.9, 0.999, 1e-8, WD, opt.step_count, gn, mx)
    used = np.zeros(g.size, dtype=bool)
    for name, (o, n) in slots.items():
        used[o:o + n] = True
        for k in "pmv":
            if name in off:                                # skipped as torch.optim.AdamW skips a parameter whose grad is None
                assert np.array_equal(after[k][o:o + n].view(np.int32), before[k][o:o + n].view(np.int32)), (label, name, k)
            else:
                r = R.ratio(after[k][o:o + n], ref[k][o:o + n], ref[k + "_bound"][o:o + n])
                _worst(k, r, (label, name))
                assert r <= 1.0, (label, name, k, r)
    for k in "pmv":                                        # the padding between the slots stays exactly zero
        assert not after[k][~used].any(), (label, k)
    return before, after, ref


def _worst(key, r, what):
    if r >= WORST.get(key, (-1.0, None))[0]:
        WORST[key] = (r, what)


def _expected_ranges(tr, model, off):
    """the complement of the skipped slots (padding included) in the flat buffer, neighbours merged"""
    total = tr.reducer.flat.numel()
    skipped = np.zeros(total, dtype=bool)
    for name in off:
        o, n = tr.reducer.slot(getattr(model, name))
        skipped[o:o + _slot_len(n)] = True
    edges = np.flatnonzero(np.diff(np.concatenate(([True], skipped, [True])).astype(np.int8)))
    return [(int(a), int(b)) for a, b in zip(edges[::2], edges[1::2])]


def test_all_parameters_with_clipping(dev):
    model, tr = _make(Toy, dev, 1.0)
    assert [tr.reducer.slot(getattr(model, n)) for n, _ in SIZES] == [(128, 13), (88, 35), (24, 64), (16, 3), (0, 9)]
    assert tr.opt.param.numel() == 144
    for i, x in enumerate(_inputs(4, dev)):
        before, after, ref = _step(tr, model, x, label=f"all/{i + 1}")
        assert ref["coef"] < 0.5                           # the clip is active at every step
        assert tr.opt.step_count == i + 1
    for name, _ in SIZES:                                  # the module reads the flat buffer
        o, n = tr.reducer.slot(getattr(model, name))
        assert torch.equal(getattr(model, name).detach().reshape(-1), tr.opt.param[o:o + n])


def test_branch_off_then_on_steps_with_the_global_count(dev):
    """Pins the optimizer's GLOBAL step count in the bias corrections of a parameter that skipped steps (optim.py; torch counts per
    parameter).  e steps at 1, is left out at 2 and 3 and returns at 4: its update follows t = 4, and t = 2 -- torch's count -- is
    further from the device than the bound, so a silent change of semantics fails here."""
    model, tr = _make(Toy, dev, 1.0)
    xs = _inputs(4, dev)
    o, n = tr.reducer.slot(model.e)
    _step(tr, model, xs[0], label="branch/1")
    kept = [t[o:o + n].clone() for t in (tr.opt.param, tr.opt.exp_avg, tr.opt.exp_avg_sq)]
    assert all(bool(t.any()) for t in kept)
    for i in (1, 2):
        _step(tr, model, xs[i], off=("e",), label=f"branch/{i + 1}")
        assert tr.opt._active_ranges() == _expected_ranges(tr, model, ("e",)) == [(16, 144)]
        for a, b in zip(kept, (tr.opt.param, tr.opt.exp_avg, tr.opt.exp_avg_sq)):
            assert torch.equal(a.view(torch.int32), b[o:o + n].view(torch.int32))
    before, after, ref = _step(tr, model, xs[3], label="branch/4")
    assert tr.opt.step_count == 4 and tr.opt._active_ranges() == [(0, 144)]
    g = _np(tr.reducer.flat)
    per_param = R.adamw_ref(before["p"], g, before["m"], before["v"], LR, 0.9, 0.999, 1e-8, WD, 2, np.float32(tr.opt.gnorm_sq.item()), 1.0)
    r_global = R.ratio(after["p"][o:o + n], ref["p"][o:o + n], ref["p_bound"][o:o + n])
    r_torch = R.ratio(after["p"][o:o + n], per_param["p"][o:o + n], per_param["p_bound"][o:o + n])
    print("returning parameter: error / bound with the global count", r_global, "with the per-parameter count", r_torch)
    assert r_global <= 1.0 < r_torch
    assert float((np.abs(per_param["p"] - ref["p"])[o:o + n] / (ref["p_bound"] + per_param["p_bound"])[o:o + n]).min()) > 1.0


@pytest.mark.parametrize("off,ranges", [(("e",), [(16, 144)]), (("a",), [(0, 128)]), (("b", "c"), [(0, 24), (128, 144)]),
                                        (("a", "e"), [(16, 128)]), (("d",), [(0, 16), (24, 144)])])
def test_parameters_without_a_gradient_are_skipped(dev, off, ranges):
    """the branches of _active_ranges: a skipped slot at the front, at the back, two neighbours, both ends, one in the middle"""
    model, tr = _make(Toy, dev, 1.0)
    xs = _inputs(3, dev)
    _step(tr, model, xs[0], label=f"skip{off}/1")
    _step(tr, model, xs[1], off=off, label=f"skip{off}/2")
    assert tr.opt._active_ranges() == ranges == _expected_ranges(tr, model, off)
    _step(tr, model, xs[2], label=f"skip{off}/3")


def _per_param(tr, model):
    out = {}
    for name, (o, n) in _slots(tr, model).items():
        for k, t in (("p", tr.opt.param), ("m", tr.opt.exp_avg), ("v", tr.opt.exp_avg_sq)):
            out[name, k] = t[o:o + n].clone()
    return out


@pytest.mark.parametrize("max_norm", [0.0, 1.0])
def test_checkpoint_into_another_slot_layout(dev, max_norm):
    xs = _inputs(5, dev)
    model, tr = _make(Toy, dev, max_norm)
    for i in range(3):
        _step(tr, model, xs[i], label=f"ckpt{max_norm}/{i + 1}")
    sd = tr.opt.state_dict()
    weights = {k: v.clone() for k, v in model.state_dict().items()}
    twin = ToyGrouped().to(dev)
    twin.load_state_dict(weights)
    tr2 = Trainer(twin, TrainConfig(lr=LR, weight_decay=WD, grad_max_norm=max_norm), compute_loss=lambda m, x, y: m(x))
    assert tr2.opt._layout() != [tuple(t) for t in sd["layout"]]
    assert [n for _, n in tr2.opt._layout()] == [n for _, n in sd["layout"]]
    assert _slots(tr2, twin)["a"] == (24, 13) and _slots(tr2, twin)["c"] == (40, 64)          # back to back, as grad_groups asks
    tr2.opt.load_state_dict(sd)
    assert tr2.opt.step_count == 3
    a, b = _per_param(tr, model), _per_param(tr2, twin)
    assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)
    for i in (3, 4):
        _step(tr, model, xs[i], label=f"ckpt{max_norm}/{i + 1}")
        _step(tr2, twin, xs[i], label=f"ckpt{max_norm}/twin{i + 1}")
    assert tr.opt.step_count == tr2.opt.step_count == 5
    a, b = _per_param(tr, model), _per_param(tr2, twin)
    if max_norm == 0.0:                                    # the update is elementwise: the layout must not change a bit
        for k in a:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    # with clipping the norm's summation order follows the layout: both runs were judged per step, within bound, by _step


def test_load_state_dict_refusals(dev):
    model, tr = _make(Toy, dev, 0.0)
    _step(tr, model, _inputs(1, dev)[0], label="refusals/1")
    sd = tr.opt.state_dict()
    twin, tr2 = _make(ToyGrouped, dev, 0.0)
    same, tr3 = _make(Toy, dev, 0.0)

    def without_layout(extra):
        d = {k: v for k, v in sd.items() if k != "layout"}
        d["exp_avg"] = torch.cat((sd["exp_avg"], torch.zeros(extra, device=dev)))
        d["exp_avg_sq"] = torch.cat((sd["exp_avg_sq"], torch.zeros(extra, device=dev)))
        return d

    with pytest.raises(NrvError, match="another size"):
        tr2.opt.load_state_dict(without_layout(8))
    with pytest.raises(NrvError, match="another parameter set"):
        tr2.opt.load_state_dict(dict(sd, layout=sd["layout"][:-1]))
    with pytest.raises(NrvError, match="another parameter set"):
        tr2.opt.load_state_dict(dict(sd, layout=[(o, n + (i == 2)) for i, (o, n) in enumerate(sd["layout"])]))
    assert tr2.opt.step_count == 0 and not bool(tr2.opt.exp_avg.any())          # a refused load changes nothing
    tr3.opt.load_state_dict(without_layout(0))                                    # written before the table existed: same layout
    assert tr3.opt.step_count == 1
    assert torch.equal(tr3.opt.exp_avg, sd["exp_avg"]) and torch.equal(tr3.opt.exp_avg_sq, sd["exp_avg_sq"])


def test_zz_worst_ratios(dev):
    """prints the figures of the docstring (after the tests above have run)"""
    for key in sorted(WORST):
        print("FusedAdamW worst error / bound", key, WORST[key])
    assert all(r <= 1.0 for r, _ in WORST.values())
