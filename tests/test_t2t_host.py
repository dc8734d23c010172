"""CPU: T2TViT's module tree, state_dict contract, seeded init and refused configurations against the reference fixture
(tests/golden/t2t_small.npz), the fp32 restatement tests/t2t_ref.py against the reference's logits, loss and gradients, and the
new C-ABI prototypes.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import port_checks as PC
import t2t_fixture as TF
import t2t_ref as R
from noise_robust_vit_amd import t2t as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "t2t_small.npz")
NEW = ["nrv_soft_split_fwd", "nrv_soft_split_bwd", "nrv_layernorm_pad_fwd", "nrv_layernorm_pad_bwd_workspace",
       "nrv_layernorm_pad_bwd", "nrv_attn_wide_fwd", "nrv_attn_wide_bwd"]


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


def test_public_interface():
    import noise_robust_vit_amd as pkg
    assert pkg.T2TViT is T.T2TViT and pkg.RearrangeImage is T.RearrangeImage and pkg.conv_output_size is T.conv_output_size
    assert T.conv_output_size(224, 7, 4, 2) == 56 and T.conv_output_size(56, 3, 2, 1) == 28
    x = torch.arange(2 * 16 * 3.0).reshape(2, 16, 3)
    y = T.RearrangeImage()(x)
    assert y.shape == (2, 3, 4, 4) and torch.equal(y[1, 2, 3, 1], x[1, 13, 2])


@pytest.mark.parametrize("case", list(TF.CASES))
def test_module_tree_and_keys(fx, case):
    m = TF.build(T, case)
    PC.check_tree_and_keys(m, TF.weights(m, 3), fx, case)


@pytest.mark.parametrize("name,cfg", [("small", TF.SMALL), ("full", TF.FULL)])
def test_seeded_init_matches_reference(fx, name, cfg):
    torch.manual_seed(0)
    PC.check_seeded_init(T.T2TViT(**cfg), fx, name)


@pytest.mark.parametrize("case", list(TF.CASES))
def test_restatement_reproduces_the_reference(fx, case):
    m = TF.build(T, case)
    m.load_state_dict(TF.weights(m, 3), strict=True)
    PC.check_restatement(R.t2t_loss_and_grads(m, *TF.inputs(case)), fx, case, m.training)


def test_refused_configurations():
    base = dict(TF.SMALL)
    with pytest.raises(NotImplementedError):
        T.T2TViT(**dict(base, image_size=(64, 32)))
    with pytest.raises(NotImplementedError):
        T.T2TViT(**dict(base, t2t_layers=((9, 4), (3, 2))))
    with pytest.raises(NotImplementedError):
        T.T2TViT(**dict(base, t2t_layers=((7, 4), (7, 2), (3, 2))))          # 147 * 49 = 7203 features in a stage
    T.T2TViT(**dict(base, t2t_layers=((7, 4), (7, 2))))                       # ... but the last stage may be wider
    with pytest.raises(ValueError):
        T.T2TViT(**dict(base, robust=True, transformer=torch.nn.Identity()))
    img = torch.zeros(1, 3, 64, 64)
    for kw in (dict(dropout=0.1), dict(emb_dropout=0.1)):
        with pytest.raises(NotImplementedError):
            T.T2TViT(**dict(base, **kw)).train()(img)
    with pytest.raises(NotImplementedError):
        T.T2TViT(**base)(torch.zeros(1, 3, 64, 48))
    from noise_robust_vit_amd.encoder import record_attention
    with record_attention([]):
        with pytest.raises(NotImplementedError):
            T.T2TViT(**base)(img)
    m = T.T2TViT(**dict(base, robust=True))
    assert m.transformer._meta.robust and not m.to_patch_embedding[3]._meta.robust
    assert m.grad_groups() == m.transformer.grad_groups()


def test_user_transformer_is_used_as_given():
    from noise_robust_vit_amd.lucid_vit import Transformer
    t = Transformer(64, 1, 2, 32, 128)
    m = T.T2TViT(image_size=64, num_classes=10, dim=64, transformer=t)
    assert m.transformer is t


def test_new_prototypes_are_declared_bound_and_exported():
    PC.check_prototypes(NEW, abi=19, source="nrv_t2t.hip")


def test_shape_errors_come_back_before_any_launch():
    """Out-of-contract shapes return NRV_ERR_SHAPE from the host-side checks (no GPU is touched)."""
    from noise_robust_vit_amd import _lib
    lib = _lib.bind(__import__("noise_robust_vit_amd.build", fromlist=["build"]).build())
    p = ctypes.c_void_p(0)
    ERR_SHAPE = -2
    for dh in (128, 136 + 4, 200, 256, 64):
        assert lib.nrv_attn_wide_fwd(p, p, p, 1, 64, 1, dh, 1.0, None) == ERR_SHAPE
        assert lib.nrv_attn_wide_bwd(p, p, p, p, p, p, 1, 64, 1, dh, 1.0, None) == ERR_SHAPE
    assert lib.nrv_attn_wide_fwd(p, p, p, 0, 64, 1, 152, 1.0, None) == ERR_SHAPE
    assert lib.nrv_soft_split_fwd(p, 1, 0, 0, p, 1, 3, 8, 8, 9, 4, 2, None) == ERR_SHAPE         # kernel above 7
    assert lib.nrv_soft_split_fwd(p, 1, 1, 2, p, 1, 3, 8, 8, 3, 2, 1, None) == ERR_SHAPE         # row stride below C
    assert lib.nrv_soft_split_bwd(p, p, 2, 1, 3, 8, 8, 3, 2, 1, None) == ERR_SHAPE
    assert lib.nrv_layernorm_pad_fwd(p, 0, p, p, p, p, p, 4, 4097, 4104, 1e-5, None) == ERR_SHAPE
    assert lib.nrv_layernorm_pad_fwd(p, 0, p, p, p, p, p, 4, 147, 150, 1e-5, None) == ERR_SHAPE   # stride not a multiple of 8
    assert lib.nrv_layernorm_pad_fwd(p, 0, p, p, p, p, p, 4, 147, 144, 1e-5, None) == ERR_SHAPE
    assert lib.nrv_layernorm_pad_bwd(p, p, 0, p, p, p, p, 0, p, p, p, p, 0, p, 0, 4, 147, 150, None) == ERR_SHAPE
