"""CPU: port_checks.judge and port_fixture.seeded_weights on synthetic tensors.  Every figure is the project's own bound taken at
0.9 and at 1.1 of itself, so nothing here is measured; distances are exact up to fp32 rounding (1e-7), far inside the margins."""
import pytest
import torch

import port_checks as PC
import port_fixture as PX


def _unit(shape, seed):
    d = torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return d / d.norm()


def _at(ref, r, seed):
    """A tensor at rel-L2 `r` from `ref`"""
    return (ref.double() + r * float(ref.double().norm()) * _unit(ref.shape, seed)).float()


def _absmax(shape, v):
    t = torch.zeros(shape)
    t.view(-1)[1] = v
    return t


class Case:
    """Three results over logits [4, 10] and gradients a, b, c; r: the low-precision restatement's own rel-L2, everywhere"""

    def __init__(self, r=0.0, s32=0.7):
        g = torch.Generator().manual_seed(0)
        self.l32 = torch.randn(4, 10, generator=g)
        self.g32 = {"a.weight": torch.randn(8, 8, generator=g), "b.bias": torch.randn(8, generator=g), "c.weight": torch.randn(3, 5, generator=g)}
        self.s32 = s32
        self.r = r
        self.bound = 2 * r + 1e-2
        self.logits, self.loss, self.grads = self.l32.clone(), s32, {k: v.clone() for k, v in self.g32.items()}

    def judge(self, **rules):
        r32 = (self.l32, torch.tensor(self.s32), self.g32)
        r16 = (_at(self.l32, self.r, 1), torch.tensor(self.s32), {k: None if v is None else _at(v, self.r, 2) for k, v in self.g32.items()})
        PC.judge((self.logits, torch.tensor(self.loss), self.grads), r32, r16, **rules)


def test_rel_is_the_relative_l2_and_detaches():
    a = torch.tensor([3.0, 0.0], requires_grad=True)
    assert PC.rel(a + torch.tensor([0.0, 4.0]), a) == pytest.approx(4.0 / 3.0)
    assert PC.rel(_at(torch.ones(50), 3e-3, 5), torch.ones(50)) == pytest.approx(3e-3, rel=1e-3)


@pytest.mark.parametrize("r", [0.0, 4e-3])
def test_logits_bound(r):
    c = Case(r)
    c.logits = _at(c.l32, 0.9 * c.bound, 3)
    c.judge()
    c.logits = _at(c.l32, 1.1 * c.bound, 3)
    with pytest.raises(AssertionError, match="logits"):
        c.judge()
    c.grads = None                                                          # an eval-mode step: the logits are still judged
    with pytest.raises(AssertionError, match="logits"):
        c.judge()


@pytest.mark.parametrize("r", [0.0, 4e-3])
def test_fixture_logits_are_held_to_the_logits_bound(r):
    c = Case(r)
    c.judge(fixture_logits=_at(c.l32, 0.9 * c.bound, 4))
    with pytest.raises(AssertionError, match="fixture logits"):
        c.judge(fixture_logits=_at(c.l32, 1.1 * c.bound, 4))


@pytest.mark.parametrize("r", [0.0, 4e-3])
def test_gradient_bound_names_the_key(r):
    c = Case(r)
    c.grads["b.bias"] = _at(c.g32["b.bias"], 0.9 * c.bound, 3)
    c.judge()
    c.grads["b.bias"] = _at(c.g32["b.bias"], 1.1 * c.bound, 3)
    with pytest.raises(AssertionError, match="b.bias"):
        c.judge()
    c.grads["b.bias"] = None
    with pytest.raises(AssertionError, match="b.bias"):
        c.judge()


@pytest.mark.parametrize("s32", [0.7, -0.7, 5.0])
def test_loss_check_is_absolute_below_one_and_relative_above(s32):
    tol = 2e-2 * max(1.0, abs(s32))
    for sign in (1, -1):
        c = Case(s32=s32)
        c.loss = s32 + sign * 0.9 * tol
        c.judge()
        c.loss = s32 + sign * 1.1 * tol
        with pytest.raises(AssertionError, match="loss"):
            c.judge()


def test_a_gradient_that_vanishes_in_the_restatement_must_vanish():
    c = Case()
    c.g32["b.bias"] = _absmax(8, 0.9e-4)
    c.grads["b.bias"] = _absmax(8, -0.9e-4)                                # rel-L2 2: only the vanishing rule lets it pass
    c.judge()
    c.judge(expect_vanished={"b.bias"})
    c.grads["b.bias"] = _absmax(8, 1.1e-4)
    with pytest.raises(AssertionError, match="b.bias"):
        c.judge()
    c.g32["b.bias"] = _absmax(8, 1.1e-4)                                    # no longer vanishing: bounded like any other
    c.judge()
    c.grads["b.bias"] = _absmax(8, -1.1e-4)
    with pytest.raises(AssertionError, match="b.bias"):
        c.judge()


def test_a_name_predicate_holds_both_sides_to_the_threshold():
    named = dict(vanishes=lambda k, r: k == "b.bias")
    c = Case()
    c.g32["b.bias"] = _absmax(8, 0.9e-4)
    c.grads["b.bias"] = _absmax(8, -0.9e-4)
    c.judge(**named)
    c.grads["b.bias"] = _absmax(8, 1.1e-4)
    with pytest.raises(AssertionError, match="b.bias"):
        c.judge(**named)
    c.grads["b.bias"] = _absmax(8, 0.9e-4)
    c.g32["b.bias"] = _absmax(8, 1.1e-4)                                    # expected to vanish, and the restatement does not
    with pytest.raises(AssertionError, match="b.bias"):
        c.judge(**named)
    # without a rule every gradient is bounded, a vanishing one included
    c.g32["b.bias"] = _absmax(8, 0.9e-4)
    c.grads["b.bias"] = _absmax(8, -0.9e-4)
    with pytest.raises(AssertionError, match="b.bias"):
        c.judge(vanishes=None)


def test_expected_vanished_set_is_exact():
    c = Case()
    c.g32["b.bias"] = c.grads["b.bias"] = _absmax(8, 0.9e-4)
    c.judge(expect_vanished={"b.bias"})
    with pytest.raises(AssertionError, match="a.weight"):
        c.judge(expect_vanished={"b.bias", "a.weight"})                    # one key fewer vanished than expected
    with pytest.raises(AssertionError, match="b.bias"):
        c.judge(expect_vanished=set())                                      # one key more


def test_key_sets_must_agree_in_both_directions():
    c = Case()
    c.grads["d.bias"] = torch.zeros(2)
    with pytest.raises(AssertionError, match="d.bias"):
        c.judge()
    c = Case()
    del c.grads["c.weight"]
    with pytest.raises(AssertionError, match="c.weight"):
        c.judge()


def test_a_dropped_layer_has_no_gradient_or_an_exactly_zero_one():
    rule = dict(skip=PC.dropped_layers({"b.", "x."}))
    c = Case()
    c.g32["b.bias"] = torch.zeros(8)                                        # the restatement leaves the layer out
    for g in (None, torch.zeros(8)):
        c.grads["b.bias"] = g
        c.judge(**rule)
    c.grads["b.bias"] = _absmax(8, 1e-30)
    with pytest.raises(AssertionError, match="b.bias"):
        c.judge(**rule)
    c.grads["b.bias"] = torch.zeros(8)
    c.grads["a.weight"] = None                                              # not under a dropped prefix: judged as usual
    with pytest.raises(AssertionError, match="a.weight"):
        c.judge(**rule)
    c = Case()
    c.judge(skip=PC.dropped_layers(set()))                                  # nothing dropped: nothing skipped
    c.grads["b.bias"] = None
    with pytest.raises(AssertionError, match="b.bias"):
        c.judge(skip=PC.dropped_layers(set()))


def test_a_frozen_table_has_no_gradient_on_either_side():
    rule = dict(skip=PC.frozen("b.bias"))
    c = Case()
    c.g32["b.bias"] = c.grads["b.bias"] = None
    c.judge(**rule)
    c.grads["b.bias"] = torch.zeros(8)
    with pytest.raises(AssertionError, match="b.bias"):
        c.judge(**rule)
    c = Case()
    c.g32["a.weight"] = c.grads["a.weight"] = None                          # no gradient, and not the table
    with pytest.raises(AssertionError, match="a.weight"):
        c.judge(**rule)
    c = Case()
    c.grads["b.bias"] = None                                                # the restatement has one: judged as usual
    with pytest.raises(AssertionError, match="b.bias"):
        c.judge(**rule)


@pytest.mark.parametrize("r", [0.0, 4e-3])
def test_fixture_gradient_samples(r):
    c = Case(r)
    big = torch.randn(50, 40, generator=torch.Generator().manual_seed(9))   # 2000 elements: stored at GRAD_SAMPLE positions
    c.g32["a.weight"] = big
    c.grads["a.weight"] = big.clone()
    stored = {k: PX.grad_sample(k, v) for k, v in c.grads.items()}
    assert stored["a.weight"].numel() == PX.GRAD_SAMPLE and stored["b.bias"].numel() == 8
    c.judge(fixture_grads=stored)
    for k in ("a.weight", "b.bias"):
        # rel(sample of the HIP gradient, stored) = x means stored = sample / (1 + x) along the sample itself
        c.judge(fixture_grads=dict(stored, **{k: stored[k] / (1 + 0.9 * (c.bound + 1e-3))}))
        with pytest.raises(AssertionError, match=k):
            c.judge(fixture_grads=dict(stored, **{k: stored[k] / (1 + 1.1 * (c.bound + 1e-3))}))


# ---- the weight recipe ------------------------------------------------------------------------------
_ENTRIES = {"fc.weight": torch.zeros(4, 6), "norm.weight": torch.zeros(6), "fc.bias": torch.zeros(4)}


def _z(seed, name, shape):
    return torch.randn(shape, generator=PX._gen(seed, name))


def test_seeded_weights_default_rule():
    w = PX.seeded_weights(_ENTRIES, 3)
    assert list(w) == list(_ENTRIES)
    assert torch.equal(w["fc.weight"], _z(3, "fc.weight", (4, 6)) / 6 ** 0.5)          # rank 2: fan-in 6
    assert torch.equal(w["norm.weight"], 1.0 + 0.1 * _z(3, "norm.weight", (6,)))
    assert torch.equal(w["fc.bias"], 0.02 * _z(3, "fc.bias", (4,)))
    assert not torch.equal(w["fc.bias"], PX.seeded_weights(_ENTRIES, 5)["fc.bias"])
    conv = PX.seeded_weights({"conv.weight": torch.zeros(8, 2, 3, 3)}, 3)["conv.weight"]
    assert torch.equal(conv, _z(3, "conv.weight", (8, 2, 3, 3)) / 18 ** 0.5)           # fan-in 2 * 3 * 3


def test_seeded_weights_special_overrides_one_entry():
    seen = []

    def special(name, leaf, t, z):
        seen.append((name, leaf, tuple(t.shape)))
        assert torch.equal(z, _z(3, name, tuple(t.shape)))
        return 0.5 * z if leaf == "bias" else None
    w = PX.seeded_weights(_ENTRIES, 3, special)
    assert seen == [("fc.weight", "weight", (4, 6)), ("norm.weight", "weight", (6,)), ("fc.bias", "bias", (4,))]
    base = PX.seeded_weights(_ENTRIES, 3)
    assert torch.equal(w["fc.bias"], 0.5 * _z(3, "fc.bias", (4,)))
    assert torch.equal(w["fc.weight"], base["fc.weight"]) and torch.equal(w["norm.weight"], base["norm.weight"])
    tokens = PX.seeded_weights({"cls_token": torch.zeros(1, 1, 4), "pos_embedding": torch.zeros(1, 3, 4), "a.weight": torch.zeros(4)},
                               3, PX.vit_tokens)
    assert torch.equal(tokens["cls_token"], 0.5 * _z(3, "cls_token", (1, 1, 4)))
    assert torch.equal(tokens["pos_embedding"], 0.2 * _z(3, "pos_embedding", (1, 3, 4)))
    assert torch.equal(tokens["a.weight"], 1.0 + 0.1 * _z(3, "a.weight", (4,)))


def test_a_skipped_entry_leaves_the_others_bits_unchanged():
    base = PX.seeded_weights(_ENTRIES, 3)
    kept = torch.arange(6.0)
    with_buffer = {"fc.weight": _ENTRIES["fc.weight"], "index": torch.zeros(5, dtype=torch.long), "norm.weight": kept,
                   "fc.bias": _ENTRIES["fc.bias"]}
    w = PX.seeded_weights(with_buffer, 3, lambda name, leaf, t, z: t.clone() if name == "norm.weight" else None)
    assert list(w) == ["fc.weight", "norm.weight", "fc.bias"]                            # the integer buffer is left out
    assert torch.equal(w["norm.weight"], kept)                                           # kept as constructed, no draw used
    assert torch.equal(w["fc.weight"], base["fc.weight"]) and torch.equal(w["fc.bias"], base["fc.bias"])
    fewer = PX.seeded_weights({"fc.bias": _ENTRIES["fc.bias"]}, 3)
    assert torch.equal(fewer["fc.bias"], base["fc.bias"])


def test_image_inputs_draw_from_the_case_generator():
    img, y = PX.image_inputs("s_train", 3, 1, 8, 6, 10)
    g = PX._gen(17, "inputs.s_train")
    assert torch.equal(img, torch.randn(3, 1, 8, 6, generator=g)) and torch.equal(y, torch.randint(0, 10, (3,), generator=g))
