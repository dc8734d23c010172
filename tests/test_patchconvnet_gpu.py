"""GPU: PatchConvNet on the HIP kernels against the reference fixture (tests/golden/patchconvnet_small.npz) and the fp32
restatement tests/patchconvnet_ref.py: logits, loss and every parameter's gradient; S60 at 224 px; drop path on injected keeps;
eval mode; Trainer.step and Trainer.capture; reruns.

The bound is port_checks.judge's, with both restatements (fp32, bf16-rounded operands) on the CPU.  The key bias of the class
attention has an exactly zero gradient (it adds q.b_k to every score of a sample alike, and softmax ignores a shared shift): it
is checked to be numerically zero (abs max < 1e-4) on both sides instead."""
import os

import numpy as np
import pytest
import torch

import patchconvnet_fixture as PF
import patchconvnet_ref as R
import port_checks as PC
from noise_robust_vit_amd import patch_convnet as P

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patchconvnet_small.npz")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


def _compare(model, x, y, keeps=None, **rules):
    keeps = [k.cpu() if k is not None else None for k in keeps] if keeps else None
    return PC.compare(model, x, y, lambda m, x, y, low: R.pcn_loss_and_grads(m, x, y, keeps=keeps, bf16_operands=low), on_cpu=True,
                      vanishes=lambda k, r: k.endswith("attn.k.bias"), **rules)


@pytest.mark.parametrize("case", list(PF.CASES))
def test_fixture_parity(dev, fx, case):
    m = PF.build(P, case)
    m.load_state_dict(PF.weights(m, 3))
    m = m.to(dev)
    img, y = PF.inputs(case)
    _compare(m, img.to(dev), y.to(dev), fixture_logits=PF.unpack(fx, case + ".logits"),
             fixture_grads=PF.unpack_grads(fx, case) if m.training else None)


def _s60(dev, **kw):
    torch.manual_seed(0)
    m = P.S60(num_classes=10, **kw)
    sd = PF.weights(m, 5)
    m.load_state_dict(sd)
    return m.to(dev)


def test_s60_224_matches_restatement(dev):
    m = _s60(dev).train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 224, 224, generator=g).to(dev)
    y = torch.randint(0, 10, (2,), generator=g).to(dev)
    _compare(m, x, y)


def test_drop_path_on_injected_keeps(dev):
    m = PF.build(P, "s_train")
    m2 = P.PatchConvnet(**dict(PF.SMALL, drop_path_rate=0.3))
    m2.load_state_dict(PF.weights(m, 3))
    keeps = [torch.tensor([1.0, 0.0, 1.0, 0.0]), torch.tensor([0.0, 1.0, 1.0, 1.0])]
    for blk, k in zip(m2.blocks, keeps):
        blk.keep_source = (lambda kk: (lambda b, d: kk.to(d)))(k)
    m2 = m2.to(dev).train()
    img, y = PF.inputs("s_train")
    _compare(m2, img.to(dev), y.to(dev), keeps=keeps)
    # drawn keeps (no source): per-sample values in {0, 1}, reproducible from the device RNG
    for blk in m2.blocks:
        blk.keep_source = None
    torch.manual_seed(3); torch.cuda.manual_seed(3)
    a = m2(img.to(dev))
    torch.manual_seed(3); torch.cuda.manual_seed(3)
    assert torch.equal(a, m2(img.to(dev)))


def test_eval_ignores_drop_path(dev):
    m = P.PatchConvnet(**dict(PF.SMALL, drop_path_rate=0.5))
    m.load_state_dict(PF.weights(m, 3))
    m = m.to(dev).eval()
    img, y = PF.inputs("s_eval")
    a = m(img.to(dev))
    assert torch.equal(a, m(img.to(dev)))
    _compare(m, img.to(dev), y.to(dev))


def test_backward_is_bit_identical_across_reruns(dev):
    m = PF.build(P, "g224")
    m.load_state_dict(PF.weights(m, 3))
    img, y = PF.inputs("g224")
    PC.check_reruns_bit_identical(m.to(dev), img.to(dev), y.to(dev))


def test_trainer_step_and_capture(dev):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(8, 3, 224, 224, generator=g).to(dev)
    y = torch.randint(0, 10, (8,), generator=g).to(dev)
    PC.check_eager_vs_captured(lambda: _s60(dev, drop_path_rate=0.1).train(), x, y, steps=2, cuda_seed=7)
