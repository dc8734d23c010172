"""GPU: CCT on the HIP kernels against the reference fixture (tests/golden/cct_small.npz) and the fp32 restatement
tests/cct_ref.py: logits, loss and every parameter's gradient for each fixture case (the dropout case with the reference's
recorded masks on both sides); eval mode; reruns; the kernels a training step launches; Trainer.step and Trainer.capture; a
reference-shaped state_dict round trip.

Bounds follow test_pit_gpu.py: the HIP result's rel-L2 to the fp32 restatement may be at most twice the rel-L2 of the same
restatement under bf16 autocast plus 1e-2, per logits tensor and per parameter gradient; both restatements run on the same GPU
in the same test.  A gradient that vanishes in the restatement (abs max < 1e-4; attention_pool.bias, zero in exact arithmetic)
is checked to vanish in the HIP result; the frozen sine table has no gradient on either side; nothing else is left out."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cct_fixture as CF  # noqa: E402
import cct_ref as R  # noqa: E402

from noise_robust_vit_amd import cct as V  # noqa: E402
from noise_robust_vit_amd import kernels as K  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cct_small.npz")
SMALL = dict(CF.BASE)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


def _rel(a, b):
    a, b = a.detach().float().cpu().reshape(-1), b.detach().float().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def _hip(model, x, y, masks=None):
    model.zero_grad(set_to_none=True)
    if masks is not None:
        CF.inject_masks(model, masks)                                      # the drop-path iterator serves one forward
    logits = model(x)
    loss = torch.nn.functional.cross_entropy(logits, y)
    if model.training:
        loss.backward()
    return logits.detach(), loss.detach(), {k: p.grad for k, p in model.named_parameters()}


def _compare(model, x, y, fixture=None, masks=None):
    logits, loss, grads = _hip(model, x, y, masks)
    l32, s32, g32 = R.cct_loss_and_grads(model, x, y, masks=masks)
    l16, _, g16 = R.cct_loss_and_grads(model, x, y, autocast=True, masks=masks)
    bound = 2 * _rel(l16, l32) + 1e-2
    print(f"logits rel {_rel(logits, l32):.3e} bound {bound:.3e}; loss {loss.item():.5f} vs {s32.item():.5f}")
    assert _rel(logits, l32) <= bound, (_rel(logits, l32), bound)
    assert abs(loss.item() - s32.item()) <= 2e-2 * max(1.0, abs(s32.item()))
    if fixture is not None:
        fxd, case = fixture
        assert _rel(logits, CF.unpack(fxd, case + ".logits")) <= bound
    if model.training:
        assert set(grads) == set(g32)
        for k, g in grads.items():
            if g32[k] is None:
                assert g is None and k.endswith("positional_emb"), k      # the frozen sine table: no gradient on either side
                continue
            assert g is not None, k
            if float(g32[k].abs().max()) < 1e-4:
                assert float(g.abs().max()) < 1e-4, k
                continue
            b = 2 * _rel(g16[k], g32[k]) + 1e-2
            print(f"{k}: rel {_rel(g, g32[k]):.3e} bound {b:.3e}")
            assert _rel(g, g32[k]) <= b, (k, _rel(g, g32[k]), b)
    return logits, grads


@pytest.mark.parametrize("case", list(CF.CASES))
def test_fixture_parity(dev, fx, case):
    m = CF.build(V, case)
    m.load_state_dict(CF.weights(m, 3))
    m = m.to(dev)
    x, y = CF.inputs(case)
    masks = CF.unpack_masks(fx, case, len(CF.classifier_of(m).blocks)) if case == "drop" else None
    _compare(m, x.to(dev), y.to(dev), fixture=(fx, case), masks=masks)


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
    x, y = _batch(dev, 2)
    runs = []
    for _ in range(2):
        lg, _, g = _hip(m, x, y)
        runs.append([lg] + [t.clone() for t in g.values() if t is not None])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_a_step_launches_the_new_kernels(dev):
    """relu_maxpool_fwd / _bwd once per conv layer, seqpool once, layernorm_f32_fwd num_layers + 1 times, attn_fwd num_layers
    times, and no strided batched GEMM at attention_dropout=0"""
    m = _model(dev, SMALL, attention_dropout=0.0, n_conv_layers=2).train()
    x, y = _batch(dev, 2)
    _hip(m, x, y)
    with K.LaunchProfile() as prof:
        _hip(m, x, y)
    names = prof.summary()
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
    m = _model(dev, SMALL).train()                                         # the reference's attention dropout 0.1
    x, y = _batch(dev, 2)
    _hip(m, x, y)
    with K.LaunchProfile() as prof:
        _hip(m, x, y)
    names = prof.summary()
    assert "bgemm" in names and "attn_fwd" not in names, sorted(names)
    with K.LaunchProfile() as prof:
        with torch.no_grad():
            m.eval()(x)
    assert "attn_fwd" in prof.summary() and "bgemm" not in prof.summary()


def test_trainer_step_and_capture(dev):
    from noise_robust_vit_amd.train import TrainConfig, Trainer
    kw = dict(attention_dropout=0.0, stochastic_depth_rate=0.0)
    a = _model(dev, SMALL, **kw).train()
    b = _model(dev, SMALL, **kw).train()
    cfg = TrainConfig(lr=1e-3)
    ta, tb = Trainer(a, cfg), Trainer(b, cfg)
    x, y = _batch(dev, 8, seed=11)
    ta.capture(x, y)
    la = [ta.step(x, y) for _ in range(3)]
    lb = [tb.step(x, y) for _ in range(3)]
    assert all(torch.equal(u, v) for u, v in zip(la, lb)), (la, lb)
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), n
    ev = tb.eval_step(x, y)
    assert torch.isfinite(ev).all()


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
    """A reference-shaped state_dict (the fixture's keys and shapes) loads strictly, gives the same logits after a save / load
    cycle into a fresh model, and the bf16 weight images follow the loaded values."""
    a = _model(dev, SMALL).eval()
    x, _ = _batch(dev, 2)
    with torch.no_grad():
        la = a(x)
        sd = {k: v.detach().cpu().clone() for k, v in a.state_dict().items()}
        torch.manual_seed(7)
        b = V.CCT(**SMALL).to(dev).eval()
        lb0 = b(x)
        b.load_state_dict(sd, strict=True)
        lb = b(x)
    assert not torch.equal(la, lb0) and torch.equal(la, lb)
