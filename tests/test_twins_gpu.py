"""GPU: Twins-SVT on the HIP kernels against the reference fixture (tests/golden/twins_small.npz) and the fp32 restatement
tests/twins_ref.py: logits, loss and every parameter's gradient for each fixture case and for the robust case (restatement
only: the reference has no `attend` to swap); eval mode; reruns; the kernels a training step launches; Trainer.step and
Trainer.capture; a reference-shaped state_dict round trip.

Bounds follow test_pit_gpu.py: the HIP result's rel-L2 to the fp32 restatement may be at most twice the rel-L2 of the same
restatement under bf16 autocast plus 1e-2, per logits tensor and per parameter gradient; both restatements run on the same GPU
in the same test.  A gradient that vanishes in the restatement (abs max < 1e-4) is checked to vanish in the HIP result; the
vanishing set is exactly the to_q.weight of the global attentions with a single key (softmax over one key is the constant 1),
and nothing else is left out."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import twins_fixture as TF  # noqa: E402
import twins_ref as R  # noqa: E402

from noise_robust_vit_amd import kernels as K  # noqa: E402
from noise_robust_vit_amd import twins_svt as V  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "twins_small.npz")


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


def _single_key_to_q(model, size):
    """to_q.weight of every global attention whose map is one k x k block"""
    out, g = set(), size
    for si in range(4):
        embed, t1, _, t2 = model.layers[si]
        g //= embed.patch_size
        for ti, t in ((1, t1), (3, t2)):
            for li, layer in enumerate(t.layers):
                if g // layer[2].fn.fn.k == 1:
                    out.add(f"layers.{si}.{ti}.layers.{li}.2.fn.fn.to_q.weight")
    return out


def _compare(model, x, y, fixture=None):
    logits, loss, grads = _hip(model, x, y)
    l32, s32, g32 = R.twins_loss_and_grads(model, x, y)
    l16, _, g16 = R.twins_loss_and_grads(model, x, y, autocast=True)
    bound = 2 * _rel(l16, l32) + 1e-2
    print(f"logits rel {_rel(logits, l32):.3e} bound {bound:.3e}; loss {loss.item():.5f} vs {s32.item():.5f}")
    assert _rel(logits, l32) <= bound, (_rel(logits, l32), bound)
    assert abs(loss.item() - s32.item()) <= 2e-2 * max(1.0, abs(s32.item()))
    if fixture is not None:
        fx, case = fixture
        assert _rel(logits, TF.unpack(fx, case + ".logits")) <= bound
    if model.training:
        assert set(grads) == set(g32)
        vanished = set()
        for k, g in grads.items():
            assert g is not None, k
            if float(g32[k].abs().max()) < 1e-4:
                assert float(g.abs().max()) < 1e-4, k
                vanished.add(k)
                continue
            b = 2 * _rel(g16[k], g32[k]) + 1e-2
            print(f"{k}: rel {_rel(g, g32[k]):.3e} bound {b:.3e}")
            assert _rel(g, g32[k]) <= b, (k, _rel(g, g32[k]), b)
        assert vanished == _single_key_to_q(model, x.shape[-1]), vanished
    return logits, grads


@pytest.mark.parametrize("case", list(TF.CASES))
def test_fixture_parity(dev, fx, case):
    m = TF.build(V, case)
    m.load_state_dict(TF.weights(m, 3))
    m = m.to(dev)
    img, y = TF.inputs(case)
    _, grads = _compare(m, img.to(dev), y.to(dev), fixture=(fx, case))
    if case == "s_train":
        assert _single_key_to_q(m, 56) == {"layers.2.1.layers.0.2.fn.fn.to_q.weight", "layers.2.3.layers.0.2.fn.fn.to_q.weight",
                                           "layers.2.3.layers.1.2.fn.fn.to_q.weight"}


def test_robust_parity_with_the_restatement(dev):
    m = TF.build(V, "r_train", robust=True)
    m.load_state_dict(TF.weights(m, 3))
    m = m.to(dev)
    img, y = TF.inputs("r_train")
    _compare(m, img.to(dev), y.to(dev))


def _model(dev, cfg, **kw):
    torch.manual_seed(0)
    m = V.TwinsSVT(**dict(cfg, **kw))
    m.load_state_dict(TF.weights(m, 5))
    return m.to(dev)


def _batch(dev, B, size=56, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, size, size, generator=g).to(dev), torch.randint(0, 10, (B,), generator=g).to(dev)


def test_eval_mode_is_deterministic(dev):
    m = _model(dev, TF.BASE, dropout=0.1).eval()                          # dropout is a no-op in eval
    x, y = _batch(dev, 3)
    with torch.no_grad():
        a = m(x)
        assert torch.equal(a, m(x))
    _compare(m, x, y)


@pytest.mark.parametrize("robust", [False, True])
def test_reruns_are_bit_identical(dev, robust):
    m = _model(dev, TF.BASE, robust=robust).train()
    x, y = _batch(dev, 2)
    runs = []
    for _ in range(2):
        lg, _, g = _hip(m, x, y)
        runs.append([lg] + [t.clone() for t in g.values()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_a_step_launches_the_new_kernels(dev):
    """subattn_fwd / _bwd once per global attention, peg_* once per stage, window_attn_* once per local attention, and no strided
    batched GEMM on the softmax path"""
    m = _model(dev, TF.BASE).train()
    x, y = _batch(dev, 2)
    _hip(m, x, y)
    with K.LaunchProfile() as prof:
        _hip(m, x, y)
    names = prof.summary()
    for n in ("soft_split_fwd", "soft_split_bwd", "subattn_fwd", "subattn_bwd", "peg_fwd", "peg_bwd", "window_attn_fwd", "window_attn_bwd",
              "gemm_nt", "gemm_tn"):
        assert n in names, sorted(names)
    n_global = sum(isinstance(mod, V.GlobalAttention) for mod in m.modules())
    n_local = sum(isinstance(mod, V.LocalAttention) for mod in m.modules())
    assert (n_global, n_local) == (9, 7)
    assert names["subattn_fwd"]["launches"] == n_global and names["subattn_bwd"]["launches"] == n_global
    assert names["window_attn_fwd"]["launches"] == n_local and names["window_attn_bwd"]["launches"] == n_local
    assert names["peg_fwd"]["launches"] == 4 and names["peg_bwd"]["launches"] == 4
    assert "bgemm" not in names and "sinkhorn_norm_fwd" not in names, sorted(names)


def test_the_robust_step_runs_the_composed_global_attention(dev):
    m = _model(dev, TF.BASE, robust=True).train()
    x, y = _batch(dev, 2)
    _hip(m, x, y)
    with K.LaunchProfile() as prof:
        _hip(m, x, y)
    names = prof.summary()
    assert "subattn_fwd" not in names and "subattn_bwd" not in names
    assert names["sinkhorn_norm_fwd"]["launches"] == 9 and names["sinkhorn_norm_bwd"]["launches"] == 9
    assert names["bgemm"]["launches"] == 9 * (2 + 5)                       # scores, P v; scores again, dV, dP, dQ, dK


def test_trainer_step_and_capture(dev):
    from noise_robust_vit_amd.train import TrainConfig, Trainer
    a = _model(dev, TF.BASE).train()
    b = _model(dev, TF.BASE).train()
    cfg = TrainConfig(lr=1e-3)
    ta, tb = Trainer(a, cfg), Trainer(b, cfg)
    x, y = _batch(dev, 4, seed=11)
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


def test_trainer_robust_step_and_capture(dev):
    from noise_robust_vit_amd.train import TrainConfig, Trainer
    a = _model(dev, TF.BASE, robust=True).train()
    b = _model(dev, TF.BASE, robust=True).train()
    cfg = TrainConfig(lr=1e-3)
    ta, tb = Trainer(a, cfg), Trainer(b, cfg)
    x, y = _batch(dev, 4, seed=5)
    ta.capture(x, y)
    la = [ta.step(x, y) for _ in range(3)]
    lb = [tb.step(x, y) for _ in range(3)]
    assert all(torch.equal(u, v) for u, v in zip(la, lb)), (la, lb)
    losses = [lb[-1].item()] + [tb.step(x, y).item() for _ in range(20)]
    assert losses[-1] < losses[0], losses


def test_state_dict_round_trip(dev):
    """A reference-shaped state_dict (the fixture's keys and shapes) loads strictly, gives the same logits after a save / load
    cycle into a fresh model, and the bf16 weight images follow the loaded values."""
    a = _model(dev, TF.BASE).eval()
    x, _ = _batch(dev, 2)
    with torch.no_grad():
        la = a(x)
        sd = {k: v.detach().cpu().clone() for k, v in a.state_dict().items()}
        torch.manual_seed(7)
        b = V.TwinsSVT(**TF.BASE).to(dev).eval()
        lb0 = b(x)
        b.load_state_dict(sd, strict=True)
        lb = b(x)
    assert not torch.equal(la, lb0) and torch.equal(la, lb)
