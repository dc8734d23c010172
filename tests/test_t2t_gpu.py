"""GPU: T2TViT on the HIP kernels against the reference fixture (tests/golden/t2t_small.npz) and the fp32 restatement
tests/t2t_ref.py: logits, loss and every parameter's gradient for each fixture case; eval mode; Trainer.step and Trainer.capture;
reruns; the kernels the 224-px model launches.

The bound is port_checks.judge's, with both restatements (fp32, bf16 autocast) on the same GPU in the same test.  A gradient
that vanishes in the restatement (abs max < 1e-4) is checked to vanish in the HIP result, and nothing else is left out."""
import os

import numpy as np
import pytest
import torch

import port_checks as PC
import t2t_fixture as TF
import t2t_ref as R
from noise_robust_vit_amd import kernels as K
from noise_robust_vit_amd import t2t as T

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "t2t_small.npz")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


def _compare(model, x, y, **rules):
    return PC.compare(model, x, y, lambda m, x, y, low: R.t2t_loss_and_grads(m, x, y, autocast=low), **rules)


@pytest.mark.parametrize("case", list(TF.CASES))
def test_fixture_parity(dev, fx, case):
    m = TF.build(T, case)
    m.load_state_dict(TF.weights(m, 3))
    m = m.to(dev)
    img, y = TF.inputs(case)
    _compare(m, img.to(dev), y.to(dev), fixture_logits=TF.unpack(fx, case + ".logits"))


def _model(dev, cfg, **kw):
    torch.manual_seed(0)
    m = T.T2TViT(**dict(cfg, **kw))
    m.load_state_dict(TF.weights(m, 5))
    return m.to(dev)


def _batch(dev, B, size=64, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, size, size, generator=g).to(dev), torch.randint(0, 10, (B,), generator=g).to(dev)


def test_eval_mode_is_deterministic(dev):
    m = _model(dev, TF.SMALL, dropout=0.1, emb_dropout=0.1).eval()          # dropout is a no-op in eval
    x, y = _batch(dev, 3)
    with torch.no_grad():
        a = m(x)
        assert torch.equal(a, m(x))
    _compare(m, x, y)


@pytest.mark.parametrize("robust", [False, True])
def test_reruns_are_bit_identical(dev, robust):
    PC.check_reruns_bit_identical(_model(dev, TF.SMALL, robust=robust).train(), *_batch(dev, 2))


def test_224_runs_the_fused_wide_head_path(dev):
    """Stage 1 at 224 px (3136 tokens, one head of 147 in 152) runs nrv_attn_wide_*; the only nrv_bgemm launches are stage 2's
    (784 tokens, 1323 in 1328): no [3136, 3136] matrix is formed."""
    m = _model(dev, dict(TF.SMALL, image_size=224, depth=1)).train()
    x, y = _batch(dev, 1, 224)
    PC.hip_step(m, x, y)                           # warm
    seen = []
    orig = K.bgemm

    def spy(A, a_str, B_, b_str, C, c_str, G1, G2, M, N, Kd, alpha=1.0):
        seen.append((M, N, Kd))
        return orig(A, a_str, B_, b_str, C, c_str, G1, G2, M, N, Kd, alpha)

    K.bgemm = spy
    try:
        with K.LaunchProfile() as prof:
            PC.hip_step(m, x, y)
    finally:
        K.bgemm = orig
    names = prof.summary()
    assert names["attn_wide_fwd"]["launches"] == 1 and names["attn_wide_bwd"]["launches"] == 1, sorted(names)
    assert names["soft_split_fwd"]["launches"] == 3 and names["soft_split_bwd"]["launches"] == 2
    assert names["layernorm_pad_fwd"]["launches"] == 4 and names["layernorm_pad_bwd"]["launches"] == 4
    assert seen and all(3136 not in s for s in seen), seen
    assert all(784 in s for s in seen), seen


def test_trainer_step_and_capture(dev):
    x, y = _batch(dev, 8, seed=11)
    tb = PC.check_eager_vs_captured(lambda: _model(dev, TF.SMALL).train(), x, y)
    assert torch.isfinite(tb.eval_step(x, y)).all()


def test_trainer_robust_loss_falls(dev):
    from noise_robust_vit_amd.train import TrainConfig, Trainer
    m = _model(dev, TF.SMALL, robust=True).train()
    t = Trainer(m, TrainConfig(lr=1e-3))
    x, y = _batch(dev, 8, seed=5)
    losses = [t.step(x, y).item() for _ in range(21)]
    assert losses[-1] < losses[0], losses


def test_width_27_runs_the_head_dim_32_kernels(dev):
    """channels = 3 with 3x3 splits: a stage of width 27 stored as 32 goes to nrv_attn_fwd / _bwd (1024 tokens, streaming), as
    the backbone's two heads of 32 do; nothing is composed and the wide kernels are not used."""
    cfg = dict(TF.SMALL, depth=1, t2t_layers=((3, 2), (3, 2)))
    m = _model(dev, cfg).train()
    x, y = _batch(dev, 2)
    names = PC.profiled_step(m, x, y)
    assert names["attn_fwd"]["launches"] == 2 and names["attn_bwd"]["launches"] == 2, sorted(names)
    assert "bgemm" not in names and "attn_wide_fwd" not in names, sorted(names)
    _compare(m, x, y)


@pytest.mark.parametrize("C,N,kind", [(27, 300, "fused"), (147, 200, "wide"), (81, 100, "composed"), (9, 64, "composed")])
def test_stage_layer_keeps_the_pad_columns_zero(dev, C, N, kind):
    """One stage layer on rows of pad8(C) columns, each attention path: the output's and the input gradient's pad columns are
    exact zeros, and the true columns match the restatement's layer (2e-2 / 3e-2 rel-L2, the bounds test_cait_gpu.py uses for a
    stand-alone Transformer layer against its fp32 restatement)."""
    from noise_robust_vit_amd.lucid_vit import Transformer
    assert T._attention_kind(K.pad8(C)) == kind
    torch.manual_seed(C)
    t = Transformer(dim=C, heads=1, depth=1, dim_head=C, mlp_dim=C).to(dev)
    attn, ff = t.layers[0]
    B, Cp = 2, K.pad8(C)
    g = torch.Generator().manual_seed(1)
    x = torch.zeros(B * N, Cp)
    x[:, :C] = torch.randn(B * N, C, generator=g)
    x = x.to(dev).requires_grad_(True)
    y = T._StageFn.apply(x, (B, N, C, attn.norm.eps), attn.norm.weight, attn.norm.bias, attn.to_q.weight, attn.to_kv.weight,
                         attn.to_out[0].weight, attn.to_out[0].bias, *ff.layer_params())
    assert y.shape == (B * N, Cp) and torch.equal(y[:, C:], torch.zeros_like(y[:, C:]))
    w = torch.zeros(B * N, Cp)
    w[:, :C] = torch.randn(B * N, C, generator=g)
    (y * w.to(dev)).sum().backward()
    assert torch.equal(x.grad[:, C:], torch.zeros_like(x.grad[:, C:]))
    P = {"layers.0." + k: v.detach() for k, v in t.layers[0].named_parameters()}
    xr = x.detach()[:, :C].reshape(B, N, C).clone().requires_grad_(True)
    ref = R._layer(P, "layers.0.", xr, 1, C ** -0.5, False)
    (ref * w.to(dev)[:, :C].reshape(B, N, C)).sum().backward()
    assert PC.rel(y[:, :C], ref.reshape(B * N, C)) <= 2e-2
    assert PC.rel(x.grad[:, :C], xr.grad.reshape(B * N, C)) <= 3e-2
