"""GPU: PiT on the HIP kernels against the reference fixture (tests/golden/pit_small.npz) and the fp32 restatement
tests/pit_ref.py: logits, loss and every parameter's gradient for each fixture case; eval mode; reruns; the kernels a training
step launches; Trainer.step and Trainer.capture; a reference-shaped state_dict round trip.

Bounds follow test_rvt_gpu.py: the HIP result's rel-L2 to the fp32 restatement may be at most twice the rel-L2 of the same
restatement under bf16 autocast plus 1e-2, per logits tensor and per parameter gradient; both restatements run on the same GPU
in the same test.  A gradient that vanishes in the restatement (abs max < 1e-4) is checked to vanish in the HIP result, and
nothing else is left out."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pit_fixture as PF  # noqa: E402
import pit_ref as R  # noqa: E402

from noise_robust_vit_amd import kernels as K  # noqa: E402
from noise_robust_vit_amd import pit as V  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pit_small.npz")


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
    logits, loss, grads = _hip(model, x, y)
    l32, s32, g32 = R.pit_loss_and_grads(model, x, y)
    l16, _, g16 = R.pit_loss_and_grads(model, x, y, autocast=True)
    bound = 2 * _rel(l16, l32) + 1e-2
    print(f"logits rel {_rel(logits, l32):.3e} bound {bound:.3e}; loss {loss.item():.5f} vs {s32.item():.5f}")
    assert _rel(logits, l32) <= bound, (_rel(logits, l32), bound)
    assert abs(loss.item() - s32.item()) <= 2e-2 * max(1.0, abs(s32.item()))
    if fixture is not None:
        fx, case = fixture
        assert _rel(logits, PF.unpack(fx, case + ".logits")) <= bound
    if model.training:
        assert set(grads) == set(g32)
        for k, g in grads.items():
            assert g is not None, k
            if float(g32[k].abs().max()) < 1e-4:
                assert float(g.abs().max()) < 1e-4, k
                continue
            b = 2 * _rel(g16[k], g32[k]) + 1e-2
            print(f"{k}: rel {_rel(g, g32[k]):.3e} bound {b:.3e}")
            assert _rel(g, g32[k]) <= b, (k, _rel(g, g32[k]), b)
    return logits, grads


@pytest.mark.parametrize("case", list(PF.CASES))
def test_fixture_parity(dev, fx, case):
    m = PF.build(V, case)
    m.load_state_dict(PF.weights(m, 3))
    m = m.to(dev)
    img, y = PF.inputs(case)
    _compare(m, img.to(dev), y.to(dev), fixture=(fx, case))


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
    m = _model(dev, PF.BASE, robust=robust).train()
    x, y = _batch(dev, 2)
    runs = []
    for _ in range(2):
        lg, _, g = _hip(m, x, y)
        runs.append([lg] + [t.clone() for t in g.values()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_a_step_launches_the_new_kernels(dev):
    """pool_dwconv_fwd / _bwd once per Pool, unfold_patches once, and no strided batched GEMM on the softmax path"""
    m = _model(dev, PF.BASE).train()
    x, y = _batch(dev, 2)
    _hip(m, x, y)
    with K.LaunchProfile() as prof:
        _hip(m, x, y)
    names = prof.summary()
    for n in ("unfold_patches", "pool_dwconv_fwd", "pool_dwconv_bwd", "attn_fwd", "attn_bwd", "gemm_nt", "gemm_tn"):
        assert n in names, sorted(names)
    pools = sum(isinstance(s, V.Pool) for s in m.layers)
    assert pools == 2
    assert names["pool_dwconv_fwd"]["launches"] == pools and names["pool_dwconv_bwd"]["launches"] == pools
    assert names["unfold_patches"]["launches"] == 1
    assert names["attn_fwd"]["launches"] == 3 and names["attn_bwd"]["launches"] == 3
    assert "bgemm" not in names and "patch_unfold" not in names, sorted(names)


def test_trainer_step_and_capture(dev):
    from noise_robust_vit_amd.train import TrainConfig, Trainer
    a = _model(dev, PF.BASE).train()
    b = _model(dev, PF.BASE).train()
    cfg = TrainConfig(lr=1e-3)
    ta, tb = Trainer(a, cfg), Trainer(b, cfg)
    x, y = _batch(dev, 8, seed=11)
    ta.capture(x, y)
    la = [ta.step(x, y) for _ in range(3)]
    lb = [tb.step(x, y) for _ in range(3)]
    assert all(torch.equal(u, v) for u, v in zip(la, lb)), (la, lb)
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), n
    losses = [lb[-1].item()] + [tb.step(x, y).item() for _ in range(20)]
    assert losses[-1] < losses[0], losses
    ev = tb.eval_step(x, y)
    assert torch.isfinite(ev).all()


def test_trainer_robust_loss_falls(dev):
    from noise_robust_vit_amd.train import TrainConfig, Trainer
    m = _model(dev, PF.BASE, robust=True).train()
    t = Trainer(m, TrainConfig(lr=1e-3))
    x, y = _batch(dev, 8, seed=5)
    losses = [t.step(x, y).item() for _ in range(21)]
    assert losses[-1] < losses[0], losses


def test_state_dict_round_trip(dev):
    """A reference-shaped state_dict (the fixture's keys and shapes) loads strictly, gives the same logits after a save / load
    cycle into a fresh model, and the bf16 weight images follow the loaded values."""
    a = _model(dev, PF.BASE).eval()
    x, _ = _batch(dev, 2)
    with torch.no_grad():
        la = a(x)
        sd = {k: v.detach().cpu().clone() for k, v in a.state_dict().items()}
        torch.manual_seed(7)
        b = V.PiT(**PF.BASE).to(dev).eval()
        lb0 = b(x)
        b.load_state_dict(sd, strict=True)
        lb = b(x)
    assert not torch.equal(la, lb0) and torch.equal(la, lb)
