"""GPU: PiT on the HIP kernels against the reference fixture (tests/golden/pit_small.npz) and the fp32 restatement
tests/pit_ref.py: logits, loss and every parameter's gradient for each fixture case; eval mode; reruns; the kernels a training
step launches; Trainer.step and Trainer.capture; a reference-shaped state_dict round trip.

The bound is port_checks.judge's, with both restatements (fp32, bf16 autocast) on the same GPU in the same test.  A gradient
that vanishes in the restatement (abs max < 1e-4) is checked to vanish in the HIP result, and nothing else is left out."""
import os

import numpy as np
import pytest
import torch

import pit_fixture as PF
import pit_ref as R
import port_checks as PC
from noise_robust_vit_amd import pit as V

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pit_small.npz")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


def _compare(model, x, y, **rules):
    return PC.compare(model, x, y, lambda m, x, y, low: R.pit_loss_and_grads(m, x, y, autocast=low), **rules)


@pytest.mark.parametrize("case", list(PF.CASES))
def test_fixture_parity(dev, fx, case):
    m = PF.build(V, case)
    m.load_state_dict(PF.weights(m, 3))
    m = m.to(dev)
    img, y = PF.inputs(case)
    _compare(m, img.to(dev), y.to(dev), fixture_logits=PF.unpack(fx, case + ".logits"))


def _model(dev, cfg, **kw):
    torch.manual_seed(0)
    m = V.PiT(**dict(cfg, **kw))
    m.load_state_dict(PF.weights(m, 5))
    return m.to(dev)


def _batch(dev, B, size=32, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, size, size, generator=g).to(dev), torch.randint(0, 10, (B,), generator=g).to(dev)


def test_eval_mode_is_deterministic(dev):
    m = _model(dev, PF.BASE, dropout=0.1, emb_dropout=0.1).eval()           # dropout is a no-op in eval
    x, y = _batch(dev, 3)
    with torch.no_grad():
        a = m(x)
        assert torch.equal(a, m(x))
    _compare(m, x, y)


@pytest.mark.parametrize("robust", [False, True])
def test_reruns_are_bit_identical(dev, robust):
    PC.check_reruns_bit_identical(_model(dev, PF.BASE, robust=robust).train(), *_batch(dev, 2))


def test_a_step_launches_the_new_kernels(dev):
    """pool_dwconv_fwd / _bwd once per Pool, unfold_patches once, and no strided batched GEMM on the softmax path"""
    m = _model(dev, PF.BASE).train()
    names = PC.profiled_step(m, *_batch(dev, 2))
    for n in ("unfold_patches", "pool_dwconv_fwd", "pool_dwconv_bwd", "attn_fwd", "attn_bwd", "gemm_nt", "gemm_tn"):
        assert n in names, sorted(names)
    pools = sum(isinstance(s, V.Pool) for s in m.layers)
    assert pools == 2
    assert names["pool_dwconv_fwd"]["launches"] == pools and names["pool_dwconv_bwd"]["launches"] == pools
    assert names["unfold_patches"]["launches"] == 1
    assert names["attn_fwd"]["launches"] == 3 and names["attn_bwd"]["launches"] == 3
    assert "bgemm" not in names and "patch_unfold" not in names, sorted(names)


def test_trainer_step_and_capture(dev):
    x, y = _batch(dev, 8, seed=11)
    tb = PC.check_eager_vs_captured(lambda: _model(dev, PF.BASE).train(), x, y)
    assert torch.isfinite(tb.eval_step(x, y)).all()


def test_trainer_robust_loss_falls(dev):
    from noise_robust_vit_amd.train import TrainConfig, Trainer
    m = _model(dev, PF.BASE, robust=True).train()
    t = Trainer(m, TrainConfig(lr=1e-3))
    x, y = _batch(dev, 8, seed=5)
    losses = [t.step(x, y).item() for _ in range(21)]
    assert losses[-1] < losses[0], losses


def test_state_dict_round_trip(dev):
    PC.check_state_dict_round_trip(_model(dev, PF.BASE).eval(), lambda: V.PiT(**PF.BASE), _batch(dev, 2)[0])
