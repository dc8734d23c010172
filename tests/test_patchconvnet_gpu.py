"""GPU: PatchConvNet on the HIP kernels against the reference fixture (tests/golden/patchconvnet_small.npz) and the fp32
restatement tests/patchconvnet_ref.py: logits, loss and every parameter's gradient; S60 at 224 px; drop path on injected keeps;
eval mode; Trainer.step and Trainer.capture; reruns.

Bounds follow test_levit_gpu.py: the HIP result's rel-L2 to the fp32 restatement may be at most twice the bf16-operand
emulation's own error plus 1e-2."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patchconvnet_fixture as PF  # noqa: E402
import patchconvnet_ref as R  # noqa: E402

from noise_robust_vit_amd import patch_convnet as P  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patchconvnet_small.npz")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


def _rel(a, b):
    a, b = a.float().cpu().reshape(-1), b.float().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def _hip(model, x, y):
    model.zero_grad(set_to_none=True)
    logits = model(x)
    loss = torch.nn.functional.cross_entropy(logits, y)
    if model.training:
        loss.backward()
    return logits.detach(), loss.detach(), {k: p.grad for k, p in model.named_parameters()}


def _compare(model, x, y, keeps=None, fixture=None):
    """HIP vs the fp32 restatement (and the reference fixture when given), bounded by the bf16-operand emulation's error."""
    logits, loss, grads = _hip(model, x, y)
    cpu = model.to("cpu")
    l32, s32, g32 = R.pcn_loss_and_grads(cpu, x.cpu(), y.cpu(), keeps=[k.cpu() if k is not None else None for k in keeps]
                                         if keeps else None)
    l16, _, g16 = R.pcn_loss_and_grads(cpu, x.cpu(), y.cpu(), keeps=[k.cpu() if k is not None else None for k in keeps]
                                       if keeps else None, bf16_operands=True)
    model.to(x.device)
    bound = 2 * _rel(l16, l32) + 1e-2
    assert _rel(logits, l32) <= bound, (_rel(logits, l32), bound)
    assert abs(loss.item() - s32.item()) <= 2e-2 * max(1.0, abs(s32.item()))
    if fixture is not None:
        fx, case = fixture
        assert _rel(logits, PF.unpack(fx, case + ".logits")) <= bound
    if model.training:
        ref = PF.unpack_grads(fixture[0], fixture[1]) if fixture is not None else None
        for k, g in grads.items():
            assert g is not None, k
            if k.endswith("attn.k.bias"):
                # exactly zero: the key bias adds q.b_k to every score of a sample alike, and softmax ignores a shared shift
                assert float(g.abs().max()) < 1e-4, k
                continue
            b = 2 * _rel(g16[k], g32[k]) + 1e-2
            assert _rel(g, g32[k]) <= b, (k, _rel(g, g32[k]), b)
            if ref is not None:
                assert _rel(PF.grad_sample(k, g.cpu()), ref[k]) <= b + 1e-3, k
    return logits, grads


@pytest.mark.parametrize("case", list(PF.CASES))
def test_fixture_parity(dev, fx, case):
    m = PF.build(P, case)
    m.load_state_dict(PF.weights(m, 3))
    m = m.to(dev)
    img, y = PF.inputs(case)
    _compare(m, img.to(dev), y.to(dev), fixture=(fx, case))


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
    B = 4
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
    m = m.to(dev)
    img, y = PF.inputs("g224")
    runs = []
    for _ in range(2):
        lg, _, g = _hip(m, img.to(dev), y.to(dev))
        runs.append([lg] + [t.clone() for t in g.values()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def _trainer_pair(dev):
    from noise_robust_vit_amd.train import TrainConfig, Trainer
    a = _s60(dev, drop_path_rate=0.1).train()
    b = _s60(dev, drop_path_rate=0.1).train()
    cfg = TrainConfig(lr=1e-3)
    return a, b, Trainer(a, cfg), Trainer(b, cfg)


def test_trainer_step_and_capture(dev):
    a, b, ta, tb = _trainer_pair(dev)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(8, 3, 224, 224, generator=g).to(dev)
    y = torch.randint(0, 10, (8,), generator=g).to(dev)
    torch.cuda.manual_seed(7)
    ta.capture(x, y)
    torch.cuda.manual_seed(7)
    la = [ta.step(x, y) for _ in range(2)]
    torch.cuda.manual_seed(7)
    lb = [tb.step(x, y) for _ in range(2)]
    assert all(torch.equal(u, v) for u, v in zip(la, lb)), (la, lb)
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), n
    losses = [lb[-1].item()] + [tb.step(x, y).item() for _ in range(20)]
    assert losses[-1] < losses[0], losses
