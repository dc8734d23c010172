"""GPU: CCT on the HIP kernels against the reference fixture (tests/golden/cct_small.npz) and the fp32 restatement
tests/cct_ref.py: logits, loss and every parameter's gradient for each fixture case (the dropout case with the reference's
recorded masks on both sides); eval mode; reruns; the kernels a training step launches; Trainer.step and Trainer.capture; a
reference-shaped state_dict round trip.

The bound is port_checks.judge's, with both restatements (fp32, bf16 autocast) on the same GPU in the same test.  A gradient
that vanishes in the restatement (abs max < 1e-4; attention_pool.bias, zero in exact arithmetic) is checked to vanish in the
HIP result; the frozen sine table has no gradient on either side; nothing else is left out."""
import os

import numpy as np
import pytest
import torch

import cct_fixture as CF
import cct_ref as R
import port_checks as PC
from noise_robust_vit_amd import cct as V

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cct_small.npz")
SMALL = dict(CF.BASE)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


def _compare(model, x, y, masks=None, **rules):
    """masks: the recorded keep masks, injected into the HIP model (the drop-path iterator serves one forward) and handed to
    both restatements"""
    return PC.compare(model, x, y, lambda m, x, y, low: R.cct_loss_and_grads(m, x, y, autocast=low, masks=masks),
                      pre=(lambda m: CF.inject_masks(m, masks)) if masks is not None else None,
                      skip=PC.frozen("positional_emb"), **rules)


@pytest.mark.parametrize("case", list(CF.CASES))
def test_fixture_parity(dev, fx, case):
    m = CF.build(V, case)
    m.load_state_dict(CF.weights(m, 3))
    m = m.to(dev)
    x, y = CF.inputs(case)
    masks = CF.unpack_masks(fx, case, len(CF.classifier_of(m).blocks)) if case == "drop" else None
    _compare(m, x.to(dev), y.to(dev), masks=masks, fixture_logits=CF.unpack(fx, case + ".logits"))


def _model(dev, cfg, **kw):
    torch.manual_seed(0)
    m = V.CCT(**dict(cfg, **kw))
    m.load_state_dict(CF.weights(m, 5))
    return m.to(dev)


def _batch(dev, B, size=16, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, size, size, generator=g).to(dev), torch.randint(0, 10, (B,), generator=g).to(dev)


def test_eval_mode_is_deterministic(dev):
    m = _model(dev, SMALL, stochastic_depth_rate=0.3).eval()               # attention dropout 0.1 and drop path: no-ops in eval
    x, y = _batch(dev, 3)
    with torch.no_grad():
        a = m(x)
        assert torch.equal(a, m(x))
    _compare(m, x, y)


@pytest.mark.parametrize("robust", [False, True])
def test_reruns_are_bit_identical(dev, robust):
    m = _model(dev, SMALL, robust=robust, attention_dropout=0.0, n_conv_layers=2).train()
    PC.check_reruns_bit_identical(m, *_batch(dev, 2))


def test_a_step_launches_the_new_kernels(dev):
    """relu_maxpool_fwd / _bwd once per conv layer, seqpool once, layernorm_f32_fwd num_layers + 1 times, attn_fwd num_layers
    times, and no strided batched GEMM at attention_dropout=0"""
    m = _model(dev, SMALL, attention_dropout=0.0, n_conv_layers=2).train()
    names = PC.profiled_step(m, *_batch(dev, 2))
    layers, convs = len(m.classifier.blocks), len(m.tokenizer.conv_layers)
    assert (layers, convs) == (2, 2)
    for n in ("conv_unfold", "conv_fold", "relu_maxpool_fwd", "relu_maxpool_bwd", "layernorm_f32_fwd", "layernorm_f32_bwd", "seqpool_fwd",
              "seqpool_bwd", "attn_fwd", "attn_bwd", "gemm_nt", "gemm_tn"):
        assert n in names, sorted(names)
    assert names["relu_maxpool_fwd"]["launches"] == convs and names["relu_maxpool_bwd"]["launches"] == convs
    assert names["conv_unfold"]["launches"] == convs and names["conv_fold"]["launches"] == convs - 1
    assert names["seqpool_fwd"]["launches"] == 1 and names["seqpool_bwd"]["launches"] == 1
    assert names["layernorm_f32_fwd"]["launches"] == layers + 1 and names["layernorm_f32_bwd"]["launches"] == layers + 1
    assert names["attn_fwd"]["launches"] == layers and names["attn_bwd"]["launches"] == layers
    assert "bgemm" not in names, sorted(names)


def test_the_default_attention_dropout_takes_the_composed_path(dev):
    from noise_robust_vit_amd import kernels as K
    m = _model(dev, SMALL).train()                                         # the reference's attention dropout 0.1
    x, y = _batch(dev, 2)
    names = PC.profiled_step(m, x, y)
    assert "bgemm" in names and "attn_fwd" not in names, sorted(names)
    with K.LaunchProfile() as prof:
        with torch.no_grad():
            m.eval()(x)
    assert "attn_fwd" in prof.summary() and "bgemm" not in prof.summary()


def test_trainer_step_and_capture(dev):
    kw = dict(attention_dropout=0.0, stochastic_depth_rate=0.0)
    x, y = _batch(dev, 8, seed=11)
    tb = PC.check_eager_vs_captured(lambda: _model(dev, SMALL, **kw).train(), x, y, falls=0)
    assert torch.isfinite(tb.eval_step(x, y)).all()


@pytest.mark.parametrize("captured", [False, True])
def test_trainer_loss_falls_at_the_reference_defaults(dev, captured):
    """attention dropout 0.1 (the composed path) and stochastic depth 0.1, masks drawn on the device inside the step"""
    from noise_robust_vit_amd.train import TrainConfig, Trainer
    torch.manual_seed(3)
    m = _model(dev, dict(SMALL, stochastic_depth_rate=0.1)).train()
    t = Trainer(m, TrainConfig(lr=1e-3))
    x, y = _batch(dev, 8, seed=5)
    if captured:
        t.capture(x, y)
    losses = [t.step(x, y).item() for _ in range(21)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_trainer_robust_loss_falls(dev):
    from noise_robust_vit_amd.train import TrainConfig, Trainer
    m = _model(dev, dict(SMALL, embedding_dim=128), robust=True, attention_dropout=0.0).train()
    t = Trainer(m, TrainConfig(lr=1e-3))
    x, y = _batch(dev, 8, seed=5)
    losses = [t.step(x, y).item() for _ in range(21)]
    assert losses[-1] < losses[0], losses


def test_state_dict_round_trip(dev):
    PC.check_state_dict_round_trip(_model(dev, SMALL).eval(), lambda: V.CCT(**SMALL), _batch(dev, 2)[0])
