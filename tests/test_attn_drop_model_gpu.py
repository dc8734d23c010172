"""GPU: `fused_attention_dropout=True` on CCT and VisionTransformer -- the weight dropout inside the fused softmax kernels against the
composed path fed the same decisions, the kernels a step launches, determinism under torch.manual_seed, and captured Trainer steps
(a new mask per replay; the loss falls at the reference defaults).

Parity: model A runs the flag with injected seeds (BlockMeta.attn_seed_source), model B the composed path with a mask_source that
returns kernels.attn_drop_mask of the same seeds.  Logits and every parameter gradient agree to the project's parameter-gradient figure,
1e-2 rel-L2.  (The composed path scales kept weights by 1 / (1 - p), the fused kernels by 1 / (1 - p_eff), p_eff = 6554 / 65536 at
p = 0.1: 7e-6 apart.)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cct_fixture as CF  # noqa: E402

from noise_robust_vit_amd import cct as C  # noqa: E402
from noise_robust_vit_amd import kernels as K  # noqa: E402
from noise_robust_vit_amd import vit as V  # noqa: E402

pytestmark = pytest.mark.gpu
P = 0.1
SEED0 = 0x1234567800000000
CCT_CFG = dict(CF.BASE, embedding_dim=128)          # 2 layers, 8 x 8 = 64 tokens, 2 heads of 64: the single-pass kernels
VIT_CFG = dict(image_size=32, patch_size=8, num_layers=2, num_heads=2, hidden_dim=64, mlp_dim=128, num_classes=10,
               attention_dropout=P)                 # 17 tokens, 2 heads of 32: the streaming kernels


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def _rel(a, b):
    a, b = a.detach().float().cpu().reshape(-1), b.detach().float().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def _seed_of(site, dev):
    return torch.tensor([SEED0 + 7 * (-site)], dtype=torch.int64, device=dev)


def _cct(dev, fused, **kw):
    torch.manual_seed(0)
    m = C.CCT(**dict(CCT_CFG, attention_dropout=P, fused_attention_dropout=fused, **kw))
    m.load_state_dict(CF.weights(m, 5))
    return m.to(dev).train()


def _vit(dev, fused):
    torch.manual_seed(0)
    m = V.VisionTransformer(**VIT_CFG, fused_attention_dropout=fused)
    sd = {k: (0.05 * torch.randn(v.shape, generator=torch.Generator().manual_seed(11 + i)) + (1.0 if k.endswith("ln_1.weight") or
          k.endswith("ln_2.weight") or k.endswith("ln.weight") else 0.0)) for i, (k, v) in enumerate(m.state_dict().items())}
    m.load_state_dict(sd)
    return m.to(dev).train()


def _metas(m):
    return [b._meta for b in m.classifier.blocks] if isinstance(m, C.CCT) else [m.encoder._meta]


def _inject(m, dev, fused):
    for meta in _metas(m):
        if fused:
            meta.attn_seed_source = lambda site: _seed_of(site, dev)
        else:
            meta.mask_source = lambda site, shape: K.attn_drop_mask(_seed_of(site, dev), P, shape[0], shape[1], shape[2])


def _batch(dev, B, size, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, size, size, generator=g).to(dev), torch.randint(0, 10, (B,), generator=g).to(dev)


def _step(m, x, y):
    m.zero_grad(set_to_none=True)
    logits = m(x)
    torch.nn.functional.cross_entropy(logits, y).backward()
    return logits.detach(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("which", ["cct", "vit"])
def test_fused_dropout_is_the_composed_path_on_the_same_decisions(dev, which):
    build, size = (_cct, 16) if which == "cct" else (_vit, 32)
    a, b = build(dev, True), build(dev, False)
    _inject(a, dev, True)
    _inject(b, dev, False)
    x, y = _batch(dev, 2, size)
    with K.LaunchProfile() as prof:
        la, ga = _step(a, x, y)
    assert "attn_drop_fwd" in prof.summary() and "bgemm" not in prof.summary(), sorted(prof.summary())
    with K.LaunchProfile() as prof:
        lb, gb = _step(b, x, y)
    assert "bgemm" in prof.summary() and "attn_drop_fwd" not in prof.summary(), sorted(prof.summary())
    print(f"{which}: logits rel {_rel(la, lb):.3e}")
    assert _rel(la, lb) <= 1e-2
    assert set(ga) == set(gb) and len(ga) > 10
    for k in ga:
        if float(gb[k].abs().max()) < 1e-4:
            assert float(ga[k].abs().max()) < 1e-4, k
            continue
        print(f"{k}: rel {_rel(ga[k], gb[k]):.3e}")
        assert _rel(ga[k], gb[k]) <= 1e-2, (k, _rel(ga[k], gb[k]))
    # other seeds, other decisions: the injected seeds are what the kernels read
    for meta in _metas(a):
        meta.attn_seed_source = lambda site: _seed_of(site - 100, dev)
    lc, _ = _step(a, x, y)
    assert not torch.equal(la, lc)


@pytest.mark.parametrize("which", ["cct", "vit"])
def test_a_step_launches_the_drop_kernels_once_per_layer(dev, which):
    build, size = (_cct, 16) if which == "cct" else (_vit, 32)
    x, y = _batch(dev, 2, size)
    m = build(dev, True)
    _step(m, x, y)
    with K.LaunchProfile() as prof:
        _step(m, x, y)
    names = prof.summary()
    assert names["attn_drop_fwd"]["launches"] == 2 and names["attn_drop_bwd"]["launches"] == 2, names
    assert "bgemm" not in names and "attn_fwd" not in names and "attn_bwd" not in names, sorted(names)
    with K.LaunchProfile() as prof:
        with torch.no_grad():
            m.eval()(x)
    assert prof.summary()["attn_fwd"]["launches"] == 2 and "attn_drop_fwd" not in prof.summary() and "bgemm" not in prof.summary()
    off = build(dev, False)                          # the flag off: today's composed path
    _step(off, x, y)
    with K.LaunchProfile() as prof:
        _step(off, x, y)
    assert "bgemm" in prof.summary() and "attn_drop_fwd" not in prof.summary() and "attn_fwd" not in prof.summary()


def test_robust_with_the_flag_stays_composed(dev):
    m = _cct(dev, True, robust=True)
    x, y = _batch(dev, 2, 16)
    with K.LaunchProfile() as prof:
        _step(m, x, y)
    assert "bgemm" in prof.summary() and "attn_drop_fwd" not in prof.summary(), sorted(prof.summary())


@pytest.mark.parametrize("which", ["cct", "vit"])
def test_eager_steps_follow_torch_manual_seed(dev, which):
    build, size = (_cct, 16) if which == "cct" else (_vit, 32)
    m = build(dev, True)
    x, y = _batch(dev, 2, size)
    runs = []
    for seed in (3, 3, 4):
        torch.manual_seed(seed)
        lg, g = _step(m, x, y)
        runs.append([lg] + list(g.values()))
    assert all(torch.equal(u, v) for u, v in zip(runs[0], runs[1]))
    assert not torch.equal(runs[0][0], runs[2][0])


def test_state_dict_is_untouched_by_the_flag(dev):
    assert list(_cct(dev, True).state_dict()) == list(_cct(dev, False).state_dict())
    assert list(_vit(dev, True).state_dict()) == list(_vit(dev, False).state_dict())


def test_captured_replays_draw_new_masks(dev):
    """lr = 0: the parameters stand still, so successive losses differ only through the masks.  A seed frozen into the graph fails."""
    from noise_robust_vit_amd.train import TrainConfig, Trainer
    torch.manual_seed(3)
    m = _cct(dev, True)
    t = Trainer(m, TrainConfig(lr=0.0))
    x, y = _batch(dev, 8, 16, seed=5)
    t.capture(x, y)
    losses = [t.step(x, y).item() for _ in range(4)]
    assert all(np.isfinite(losses)) and len(set(losses)) == len(losses), losses


def test_captured_trainer_loss_falls_at_the_reference_defaults(dev):
    """attention dropout 0.1 inside the fused kernels and stochastic depth 0.1, everything drawn on the device inside the graph"""
    from noise_robust_vit_amd.train import TrainConfig, Trainer
    torch.manual_seed(3)
    m = _cct(dev, True, stochastic_depth_rate=0.1)
    t = Trainer(m, TrainConfig(lr=1e-3))
    x, y = _batch(dev, 8, 16, seed=5)
    t.capture(x, y)
    losses = [t.step(x, y).item() for _ in range(21)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
