"""GPU: CaiT on the HIP kernels against the reference fixture (tests/golden/cait_small.npz) and the fp32 restatement
tests/cait_ref.py: logits, loss and every parameter's gradient, softmax and robust; 224-px models with 4 and 16 heads; layer
dropout on seeded draws; eval mode; Trainer.step and Trainer.capture; reruns.

The bound is port_checks.judge's, with both restatements (fp32, bf16-rounded operands) on the CPU.  With robust=True the class
stage has one query, the Sinkhorn weights are uniform and the gradients of its to_q and mix_heads_pre_attn vanish: those are
checked to be numerically zero (abs max < 1e-4) on both sides instead, and nothing else is left out."""
import os
import random

import numpy as np
import pytest
import torch

import cait_fixture as CF
import cait_ref as R
import port_checks as PC
from noise_robust_vit_amd import cait as C

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cait_small.npz")
M224 = dict(image_size=224, patch_size=16, num_classes=10, dim=192, depth=2, cls_depth=2, heads=4, dim_head=48, mlp_dim=768)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


def _compare(model, x, y, kept=None, **rules):
    """kept: the layers a layer-dropout draw keeps, (patch stage, class stage); the others must take no part in the step"""
    robust = model.cls_transformer.layers[0][0].fn.fn.robust
    dropped = set()
    if kept is not None:
        for pre, t, ks in (("patch_transformer", model.patch_transformer, kept[0]), ("cls_transformer", model.cls_transformer, kept[1])):
            dropped |= {f"{pre}.layers.{i}." for i in range(len(t.layers)) if i not in ks}
    return PC.compare(model, x, y, lambda m, x, y, low: R.cait_loss_and_grads(m, x, y, kept=kept, bf16_operands=low), on_cpu=True,
                      vanishes=lambda k, r: robust and k.startswith("cls_transformer") and k.endswith(("to_q.weight", "mix_heads_pre_attn")),
                      skip=PC.dropped_layers(dropped), **rules)


@pytest.mark.parametrize("case", list(CF.CASES))
def test_fixture_parity(dev, fx, case):
    m = CF.build(C, case)
    m.load_state_dict(CF.weights(m, 3))
    m = m.to(dev)
    img, y = CF.inputs(case)
    _compare(m, img.to(dev), y.to(dev), fixture_logits=CF.unpack(fx, case + ".logits"),
             fixture_grads=CF.unpack_grads(fx, case) if m.training else None)


def _model(dev, cfg, **kw):
    torch.manual_seed(0)
    m = C.CaiT(**dict(cfg, **kw))
    m.load_state_dict(CF.weights(m, 5))
    return m.to(dev)


def _batch(dev, B, size=224, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, size, size, generator=g).to(dev), torch.randint(0, 10, (B,), generator=g).to(dev)


@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("heads,dim_head", [(4, 48), (16, 16)])
def test_224_matches_restatement(dev, heads, dim_head, robust):
    m = _model(dev, M224, heads=heads, dim_head=dim_head, robust=robust).train()
    x, y = _batch(dev, 2)
    _compare(m, x, y)


def test_eval_mode(dev):
    m = _model(dev, CF.SMALL, dropout=0.1, emb_dropout=0.1).eval()          # dropout is a no-op in eval
    x, y = _batch(dev, 3, 64)
    with torch.no_grad():
        a = m(x)
        assert torch.equal(a, m(x))
    _compare(m, x, y)


@pytest.mark.parametrize("robust", [False, True])
def test_layer_dropout_on_seeded_draws(dev, robust):
    cfg = dict(CF.SMALL, depth=4, cls_depth=2, layer_dropout=0.5, robust=robust)
    m = _model(dev, cfg).train()
    x, y = _batch(dev, 3, 64)

    def seed(_=None):
        torch.manual_seed(11); random.seed(11)
    seed()
    kept = ([int(i) for i in C.dropout_layers(list(range(4)), 0.5)], [int(i) for i in C.dropout_layers(list(range(2)), 0.5)])
    assert len(kept[0]) < 4 or len(kept[1]) < 2, kept                       # the seed does drop something
    _compare(m, x, y, kept=kept, pre=seed)
    # the draw is made in eval mode too (cait.py:153), from the same generator
    m.eval()
    seed()
    with torch.no_grad():
        a = m(x)
    l32, _, _ = R.cait_loss_and_grads(m.to("cpu"), x.cpu(), y.cpu(), kept=kept)
    m.to(dev)
    assert PC.rel(a, l32) <= 3e-2


@pytest.mark.parametrize("robust", [False, True])
def test_reruns_are_bit_identical(dev, robust):
    PC.check_reruns_bit_identical(_model(dev, dict(M224, robust=robust)).train(), *_batch(dev, 2))


def test_transformer_with_and_without_context(dev):
    """Transformer(robust=True) stand-alone, as the reference builds it (cait.py:123-165), more than one query with a context."""
    torch.manual_seed(0)
    t = C.Transformer(64, 1, 2, 32, 128, robust=True).to(dev)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 64, generator=g).to(dev).requires_grad_(True)
    c = torch.randn(2, 9, 64, generator=g).to(dev).requires_grad_(True)
    P = {k: v.detach().cpu() for k, v in t.named_parameters()}
    for ctx_ in (None, c):
        out = t(x, context=ctx_)
        a = t.layers[0][0].fn.fn
        x32 = x.detach().cpu().requires_grad_(True)
        c32 = ctx_.detach().cpu().requires_grad_(True) if ctx_ is not None else None
        ref = R._layer(P, "layers.0.", x32, c32, a.heads, a.scale, True, (1e-5, 1e-5))
        assert PC.rel(out, ref) <= 2e-2
        w = torch.randn(ref.shape, generator=g)
        x.grad = None; c.grad = None
        (out * w.to(dev)).sum().backward()
        (ref * w).sum().backward()
        assert PC.rel(x.grad, x32.grad) <= 3e-2
        if ctx_ is not None:
            assert PC.rel(c.grad, c32.grad) <= 3e-2


def test_trainer_step_and_capture(dev):
    PC.check_eager_vs_captured(lambda: _model(dev, M224).train(), *_batch(dev, 8, seed=11), steps=2)
    from noise_robust_vit_amd.train import TrainConfig, Trainer
    with pytest.raises(RuntimeError, match="layer_dropout"):
        Trainer(_model(dev, CF.SMALL, layer_dropout=0.2).train(), TrainConfig(lr=1e-3)).capture(*_batch(dev, 2, 64))


def test_trainer_robust_loss_falls(dev):
    from noise_robust_vit_amd.train import TrainConfig, Trainer
    m = _model(dev, CF.SMALL, robust=True).train()
    t = Trainer(m, TrainConfig(lr=1e-3))
    x, y = _batch(dev, 8, 64, seed=5)
    losses = [t.step(x, y).item() for _ in range(21)]
    assert losses[-1] < losses[0], losses
