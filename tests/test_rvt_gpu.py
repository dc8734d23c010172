"""GPU: RvT on the HIP kernels against the reference fixture (tests/golden/rvt_small.npz) and the fp32 restatement
tests/rvt_ref.py: logits, loss and every parameter's gradient for each fixture case; eval mode; reruns; Trainer.step and
Trainer.capture; a reference-shaped state_dict round trip.

The bound is port_checks.judge's, with both restatements (fp32, bf16 autocast) on the same GPU in the same test.  A gradient
that vanishes in the restatement (abs max < 1e-4) is checked to vanish in the HIP result, and nothing else is left out."""
import os

import numpy as np
import pytest
import torch

import port_checks as PC
import rvt_fixture as RF
import rvt_ref as R
from noise_robust_vit_amd import rvt as V

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rvt_small.npz")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


def _compare(model, x, y, **rules):
    return PC.compare(model, x, y, lambda m, x, y, low: R.rvt_loss_and_grads(m, x, y, autocast=low), **rules)


@pytest.mark.parametrize("case", list(RF.CASES))
def test_fixture_parity(dev, fx, case):
    m = RF.build(V, case)
    m.load_state_dict(RF.weights(m, 3))
    m = m.to(dev)
    img, y = RF.inputs(case)
    _compare(m, img.to(dev), y.to(dev), fixture_logits=RF.unpack(fx, case + ".logits"))


def _model(dev, cfg, **kw):
    torch.manual_seed(0)
    m = V.RvT(**dict(cfg, **kw))
    m.load_state_dict(RF.weights(m, 5))
    return m.to(dev)


def _batch(dev, B, size=48, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, size, size, generator=g).to(dev), torch.randint(0, 10, (B,), generator=g).to(dev)


def test_eval_mode_is_deterministic(dev):
    m = _model(dev, RF.SMALL, dropout=0.1, emb_dropout=0.1).eval()          # dropout is a no-op in eval
    x, y = _batch(dev, 3)
    with torch.no_grad():
        a = m(x)
        assert torch.equal(a, m(x))
    _compare(m, x, y)


@pytest.mark.parametrize("robust", [False, True])
def test_reruns_are_bit_identical(dev, robust):
    PC.check_reruns_bit_identical(_model(dev, RF.SMALL, robust=robust).train(), *_batch(dev, 2))


def test_the_layer_launches_the_new_kernels(dev):
    names = PC.profiled_step(_model(dev, RF.SMALL).train(), *_batch(dev, 2))
    for n in ("rotary", "dwconv_fwd", "dwconv_bwd", "geglu_fwd", "geglu_bwd", "attn_fwd", "attn_bwd"):
        assert n in names, sorted(names)
    assert names["rotary"]["launches"] == 4 and names["dwconv_fwd"]["launches"] == 2 and names["geglu_bwd"]["launches"] == 2
    assert "bgemm" not in names, sorted(names)


def test_trainer_step_and_capture(dev):
    x, y = _batch(dev, 8, seed=11)
    tb = PC.check_eager_vs_captured(lambda: _model(dev, RF.SMALL).train(), x, y)
    assert torch.isfinite(tb.eval_step(x, y)).all()


def test_trainer_robust_and_plain_loss_falls(dev):
    from noise_robust_vit_amd.train import TrainConfig, Trainer
    for kw in (dict(robust=True), dict(use_ds_conv=False, use_glu=False)):
        m = _model(dev, RF.SMALL, **kw).train()
        t = Trainer(m, TrainConfig(lr=1e-3))
        x, y = _batch(dev, 8, seed=5)
        losses = [t.step(x, y).item() for _ in range(21)]
        assert losses[-1] < losses[0], (kw, losses)


def test_state_dict_round_trip(dev):
    cfg = dict(RF.ONE, dim=48)
    PC.check_state_dict_round_trip(_model(dev, cfg).eval(), lambda: V.RvT(**cfg), _batch(dev, 2)[0])
