"""GPU: DeepViT on the HIP kernels against the reference fixture (tests/golden/deepvit_small.npz) and the fp32 restatement
tests/deepvit_ref.py: logits, loss and every parameter's gradient, softmax and robust; 224-px models with 4 and 16 heads; mean
pooling; eval mode; a two-head model; Trainer.step and Trainer.capture; reruns.

Bounds follow test_cait_gpu.py: the HIP result's rel-L2 to the fp32 restatement may be at most twice the bf16-operand
emulation's own error plus 1e-2, per logits tensor and per parameter gradient.  Robust models have no reference recording (the
reference's DeepViT is softmax only) and are checked against the restatement.  With two heads the LayerNorm over the heads
leaves one degree of freedom per position and the gradient of reattn_weights is mostly cancellation, so the two-head model is
run and trained but no gradient parity is asserted for it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deepvit_fixture as DF  # noqa: E402
import deepvit_ref as R  # noqa: E402

from noise_robust_vit_amd import deepvit as D  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deepvit_small.npz")
M224 = dict(image_size=224, patch_size=16, num_classes=10, dim=192, depth=2, heads=4, dim_head=48, mlp_dim=768)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


def _rel(a, b):
    a, b = a.detach().float().cpu().reshape(-1), b.detach().float().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def _hip(model, x, y):
    model.zero_grad(set_to_none=True)
    logits = model(x)
    loss = torch.nn.functional.cross_entropy(logits, y)
    if model.training:
        loss.backward()
    return logits.detach(), loss.detach(), {k: p.grad for k, p in model.named_parameters()}


def _compare(model, x, y, fixture=None):
    """HIP vs the fp32 restatement (and the reference fixture when given), bounded by the bf16-operand emulation's error."""
    logits, loss, grads = _hip(model, x, y)
    cpu = model.to("cpu")
    l32, s32, g32 = R.deepvit_loss_and_grads(cpu, x.cpu(), y.cpu())
    l16, _, g16 = R.deepvit_loss_and_grads(cpu, x.cpu(), y.cpu(), bf16_operands=True)
    model.to(x.device)
    bound = 2 * _rel(l16, l32) + 1e-2
    print(f"logits rel {_rel(logits, l32):.3e} bound {bound:.3e}")
    assert _rel(logits, l32) <= bound, (_rel(logits, l32), bound)
    assert abs(loss.item() - s32.item()) <= 2e-2 * max(1.0, abs(s32.item()))
    if fixture is not None:
        fx, case = fixture
        assert _rel(logits, DF.unpack(fx, case + ".logits")) <= bound
    if model.training:
        ref = DF.unpack_grads(fixture[0], fixture[1]) if fixture is not None else None
        for k, g in grads.items():
            assert g is not None, k
            b = 2 * _rel(g16[k], g32[k]) + 1e-2
            print(f"{k}: rel {_rel(g, g32[k]):.3e} bound {b:.3e}")
            assert _rel(g, g32[k]) <= b, (k, _rel(g, g32[k]), b)
            if ref is not None:
                assert _rel(DF.grad_sample(k, g.cpu()), ref[k]) <= b + 1e-3, k
    return logits, grads


@pytest.mark.parametrize("case", list(DF.CASES))
def test_fixture_parity(dev, fx, case):
    m = DF.build(D, case)
    m.load_state_dict(DF.weights(m, 3))
    m = m.to(dev)
    img, y = DF.inputs(case)
    _compare(m, img.to(dev), y.to(dev), fixture=(fx, case))


@pytest.mark.parametrize("case", ["s_train", "h3", "g14"])
def test_robust_matches_restatement(dev, case):
    m = DF.build(D, case, robust=True)
    m.load_state_dict(DF.weights(m, 3))
    m = m.to(dev)
    img, y = DF.inputs(case)
    _compare(m, img.to(dev), y.to(dev))


def _model(dev, cfg, **kw):
    torch.manual_seed(0)
    m = D.DeepViT(**dict(cfg, **kw))
    m.load_state_dict(DF.weights(m, 5))
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


@pytest.mark.parametrize("robust", [False, True])
def test_mean_pooling(dev, robust):
    m = _model(dev, DF.SMALL, pool="mean", robust=robust).train()
    x, y = _batch(dev, 3, 64)
    _compare(m, x, y)


def test_eval_mode(dev):
    m = _model(dev, DF.SMALL, dropout=0.1, emb_dropout=0.1).eval()          # dropout is a no-op in eval
    x, y = _batch(dev, 3, 64)
    with torch.no_grad():
        a = m(x)
        assert torch.equal(a, m(x))
    _compare(m, x, y)


@pytest.mark.parametrize("robust", [False, True])
def test_two_heads_run_and_train(dev, robust):
    from noise_robust_vit_amd.train import TrainConfig, Trainer
    m = _model(dev, DF.SMALL, heads=2, dim_head=32, robust=robust).train()
    x, y = _batch(dev, 8, 64, seed=7)
    logits, _, grads = _hip(m, x, y)
    assert bool(torch.isfinite(logits).all()) and all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
    t = Trainer(m, TrainConfig(lr=1e-3))
    losses = [t.step(x, y).item() for _ in range(21)]
    assert losses[-1] < losses[0], losses


@pytest.mark.parametrize("robust", [False, True])
def test_reruns_are_bit_identical(dev, robust):
    m = _model(dev, dict(M224, robust=robust)).train()
    x, y = _batch(dev, 2)
    runs = []
    for _ in range(2):
        lg, _, g = _hip(m, x, y)
        runs.append([lg] + [t.clone() for t in g.values()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("robust", [False, True])
def test_trainer_step_and_capture(dev, robust):
    from noise_robust_vit_amd.train import TrainConfig, Trainer
    a = _model(dev, M224, robust=robust).train()
    b = _model(dev, M224, robust=robust).train()
    cfg = TrainConfig(lr=1e-3)
    ta, tb = Trainer(a, cfg), Trainer(b, cfg)
    x, y = _batch(dev, 8, seed=11)
    ta.capture(x, y)
    la = [ta.step(x, y) for _ in range(2)]
    lb = [tb.step(x, y) for _ in range(2)]
    assert all(torch.equal(u, v) for u, v in zip(la, lb)), (la, lb)
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), n
    losses = [lb[-1].item()] + [tb.step(x, y).item() for _ in range(20)]
    assert losses[-1] < losses[0], losses
