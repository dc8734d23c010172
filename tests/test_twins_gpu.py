"""GPU: Twins-SVT on the HIP kernels against the reference fixture (tests/golden/twins_small.npz) and the fp32 restatement
tests/twins_ref.py: logits, loss and every parameter's gradient for each fixture case and for the robust case (restatement
only: the reference has no `attend` to swap); eval mode; reruns; the kernels a training step launches; Trainer.step and
Trainer.capture; a reference-shaped state_dict round trip.

The bound is port_checks.judge's, with both restatements (fp32, bf16 autocast) on the same GPU in the same test.  A gradient
that vanishes in the restatement (abs max < 1e-4) is checked to vanish in the HIP result; the vanishing set is exactly the
to_q.weight of the global attentions with a single key (softmax over one key is the constant 1), and nothing else is left out."""
import os

import numpy as np
import pytest
import torch

import port_checks as PC
import twins_fixture as TF
import twins_ref as R
from noise_robust_vit_amd import twins_svt as V

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "twins_small.npz")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


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


def _compare(model, x, y, **rules):
    return PC.compare(model, x, y, lambda m, x, y, low: R.twins_loss_and_grads(m, x, y, autocast=low),
                      expect_vanished=_single_key_to_q(model, x.shape[-1]), **rules)


@pytest.mark.parametrize("case", list(TF.CASES))
def test_fixture_parity(dev, fx, case):
    m = TF.build(V, case)
    m.load_state_dict(TF.weights(m, 3))
    m = m.to(dev)
    img, y = TF.inputs(case)
    _compare(m, img.to(dev), y.to(dev), fixture_logits=TF.unpack(fx, case + ".logits"))
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
    PC.check_reruns_bit_identical(_model(dev, TF.BASE, robust=robust).train(), *_batch(dev, 2))


def test_a_step_launches_the_new_kernels(dev):
    """subattn_fwd / _bwd once per global attention, peg_* once per stage, window_attn_* once per local attention, and no strided
    batched GEMM on the softmax path"""
    m = _model(dev, TF.BASE).train()
    names = PC.profiled_step(m, *_batch(dev, 2))
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
    names = PC.profiled_step(_model(dev, TF.BASE, robust=True).train(), *_batch(dev, 2))
    assert "subattn_fwd" not in names and "subattn_bwd" not in names
    assert names["sinkhorn_norm_fwd"]["launches"] == 9 and names["sinkhorn_norm_bwd"]["launches"] == 9
    assert names["bgemm"]["launches"] == 9 * (2 + 5)                       # scores, P v; scores again, dV, dP, dQ, dK


def test_trainer_step_and_capture(dev):
    x, y = _batch(dev, 4, seed=11)
    tb = PC.check_eager_vs_captured(lambda: _model(dev, TF.BASE).train(), x, y)
    assert torch.isfinite(tb.eval_step(x, y)).all()


def test_trainer_robust_step_and_capture(dev):
    PC.check_eager_vs_captured(lambda: _model(dev, TF.BASE, robust=True).train(), *_batch(dev, 4, seed=5), same_params=False)


def test_state_dict_round_trip(dev):
    PC.check_state_dict_round_trip(_model(dev, TF.BASE).eval(), lambda: V.TwinsSVT(**TF.BASE), _batch(dev, 2)[0])
