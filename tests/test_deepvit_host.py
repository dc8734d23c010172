"""CPU: the DeepViT module tree, seeded init, strict state_dict loading, the robust keyword and the refusals, the fp32 restatement
against the reference fixture, and the re-attention prototypes in the header, the binding and the library's exports (no GPU)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import deepvit_fixture as DF
import deepvit_ref as R
import port_checks as PC
from noise_robust_vit_amd import deepvit as D
from noise_robust_vit_amd._lib import NrvError

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deepvit_small.npz")
NEW = ("nrv_reattn_softmax_fwd", "nrv_reattn_softmax_bwd_workspace", "nrv_reattn_softmax_bwd", "nrv_reattn_norm_fwd",
       "nrv_reattn_norm_bwd_workspace", "nrv_reattn_norm_bwd")


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


def test_package_exports_deepvit():
    import noise_robust_vit_amd
    assert noise_robust_vit_amd.deepvit is D and noise_robust_vit_amd.DeepViT is D.DeepViT
    assert {"deepvit", "DeepViT"} <= set(noise_robust_vit_amd.__all__)
    for name in ("DeepViT", "Transformer", "Attention", "FeedForward", "PreNorm", "Residual"):
        assert hasattr(D, name) and name in D.__all__, name


def test_fixture_cases_have_at_least_three_heads():
    assert all(cfg["heads"] >= 3 for cfg, _, _ in DF.CASES.values())


@pytest.mark.parametrize("case", list(DF.CASES))
def test_restatement_matches_reference_fixture(fx, case):
    m = DF.build(D, case)
    PC.check_keys_and_sums(m, DF.weights(m, 3), fx, case, rtol=1e-9)
    PC.check_restatement(R.deepvit_loss_and_grads(m, *DF.inputs(case)), fx, case, m.training, loss_tol=1e-4, grad_tol=2e-3)


@pytest.mark.parametrize("name,cfg", [("small", DF.SMALL), ("full", DF.FULL)])
def test_seeded_init_matches_reference(fx, name, cfg):
    torch.manual_seed(0)
    PC.check_seeded_init(D.DeepViT(**cfg), fx, name, rtol=1e-6, atol=0.0)
    if name == "small":
        assert int(fx[name + ".nparams"]) == DF.SMALL_NPARAMS


def test_state_dict_keys_follow_the_reference_tree():
    keys = list(D.DeepViT(**dict(DF.SMALL, depth=1)).state_dict())
    a, f = "transformer.layers.0.0.fn.", "transformer.layers.0.1.fn."
    assert keys == ["pos_embedding", "cls_token", "to_patch_embedding.1.weight", "to_patch_embedding.1.bias",
                    a + "norm.weight", a + "norm.bias", a + "fn.reattn_weights", a + "fn.to_qkv.weight",
                    a + "fn.reattn_norm.1.weight", a + "fn.reattn_norm.1.bias", a + "fn.to_out.0.weight", a + "fn.to_out.0.bias",
                    f + "norm.weight", f + "norm.bias", f + "fn.net.0.weight", f + "fn.net.0.bias", f + "fn.net.3.weight",
                    f + "fn.net.3.bias", "mlp_head.0.weight", "mlp_head.0.bias", "mlp_head.1.weight", "mlp_head.1.bias"]


def test_robust_keyword_keeps_the_state_dict_and_reaches_every_layer():
    torch.manual_seed(0)
    a = D.DeepViT(**DF.SMALL)
    torch.manual_seed(0)
    b = D.DeepViT(**DF.SMALL, robust=True)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    b.load_state_dict(sa, strict=True); a.load_state_dict(sb, strict=True)
    flags = lambda m: [l[0].fn.fn.robust for l in m.transformer.layers]  # noqa: E731
    assert flags(a) == [False] * 2 and flags(b) == [True] * 2
    assert D.Transformer(16, 1, 2, 8, 32, robust=True).layers[0][0].fn.fn.robust
    assert D.Attention(16, heads=2, dim_head=8, robust=True).robust and not D.Attention(16, heads=2, dim_head=8).robust


class _Fake:
    is_cuda = True

    def __init__(self, *shape):
        self.shape = shape

    def dim(self):
        return len(self.shape)


@pytest.mark.parametrize("kw,match", [
    (dict(heads=17, dim_head=8), "heads"),
    (dict(dim=60), "multiples of 8"),
    (dict(heads=3, dim_head=7), "multiples of 8"),
    (dict(mlp_dim=100), "multiples of 8"),
    (dict(dim=4104, heads=2, dim_head=8, mlp_dim=8, depth=1), "4096"),
])
def test_refusals_at_construction(kw, match):
    with pytest.raises(NotImplementedError, match=match):
        D.DeepViT(**dict(DF.SMALL, **kw))


@pytest.mark.parametrize("kw", [dict(dropout=0.1), dict(emb_dropout=0.1)])
def test_dropout_in_training_is_refused_and_eval_is_not(kw):
    m = D.DeepViT(**dict(DF.SMALL, **kw))
    with pytest.raises(NotImplementedError, match="dropout"):
        m.train()._check_forward(_Fake(1, 3, 64, 64))
    m.eval()._check_forward(_Fake(1, 3, 64, 64))
    if "dropout" in kw:
        with pytest.raises(NotImplementedError, match="dropout"):
            m.train().transformer._check_forward(_Fake(1, 17, 64))
        m.eval().transformer._check_forward(_Fake(1, 17, 64))


def test_shapes_outside_the_kernels_range_are_refused():
    m = D.DeepViT(**dict(DF.SMALL, image_size=528, depth=1))                     # 33 x 33 = 1089 patches
    with pytest.raises(NotImplementedError, match="1025"):
        m._check_forward(_Fake(1, 3, 528, 528))
    D.DeepViT(**dict(DF.SMALL, image_size=512, depth=1))._check_forward(_Fake(1, 3, 512, 512))      # 1024 + 1 tokens
    t = D.Transformer(16, 1, 2, 8, 32)
    with pytest.raises(NotImplementedError, match="1025"):
        t._check_forward(_Fake(1, 1026, 16))
    t._check_forward(_Fake(1, 1025, 16))
    with pytest.raises(NotImplementedError, match="multiples"):
        D.DeepViT(**DF.SMALL)._check_forward(_Fake(1, 3, 72, 64))
    with pytest.raises(NotImplementedError, match="positional"):
        D.DeepViT(**DF.SMALL)._check_forward(_Fake(1, 3, 128, 128))


def test_recording_cpu_tensors_and_direct_calls_are_refused():
    m = D.DeepViT(**DF.SMALL)
    from noise_robust_vit_amd import encoder as E
    prev, E._RECORDING = E._RECORDING, []
    try:
        with pytest.raises(NotImplementedError, match="recording"):
            m._check_forward(_Fake(1, 3, 64, 64))
        with pytest.raises(NotImplementedError, match="recording"):
            m.transformer._check_forward(_Fake(1, 17, 64))
    finally:
        E._RECORDING = prev
    with pytest.raises(NrvError, match="HIP"):
        m(torch.zeros(1, 3, 64, 64))
    with pytest.raises(NrvError, match="HIP"):
        m.transformer(torch.zeros(1, 17, 64))
    attn, ff = m.transformer.layers[0]
    for holder in (attn, attn.fn, attn.fn.fn, ff.fn.fn):
        with pytest.raises(NotImplementedError, match="holds parameters"):
            holder(torch.zeros(1, 17, 64))


def test_reattn_prototypes_in_header_binding_and_exports():
    from noise_robust_vit_amd import _lib
    PC.check_prototypes(NEW, abi=19, source="nrv_reattn.hip")
    # shapes are classified on the host, before any launch: callable without a GPU
    lib = _lib.load()
    eps, zero, big = ctypes.c_float(1e-5), ctypes.c_float(0.0), ctypes.c_size_t(1 << 30)
    assert lib.nrv_reattn_softmax_fwd(16, 16, 16, 16, 16, 16, 0, 1, 17, 4, 4, eps, None) == -2
    assert lib.nrv_reattn_softmax_fwd(16, 16, 16, 16, 16, 16, 0, 1, 4, 1, 1026, eps, None) == -2
    assert lib.nrv_reattn_softmax_fwd(16, 16, 16, 16, 16, 16, 0, 1, 4, 4, 4, zero, None) == -2
    assert lib.nrv_reattn_norm_fwd(16, 16, 16, 16, 16, 0, 1, 17, 4, 4, eps, None) == -2
    assert lib.nrv_reattn_norm_fwd(16, 16, 16, 16, 16, 0, 1, 4, 1, 1026, eps, None) == -2
    assert lib.nrv_reattn_norm_fwd(16, 16, 16, 16, 16, 0, 1, 4, 4, 4, zero, None) == -2
    for bwd in (lib.nrv_reattn_softmax_bwd, lib.nrv_reattn_norm_bwd):
        assert bwd(16, 16, 16, 16, 16, 16, 16, 16, 16, big, 1, 17, 4, 4, eps, None) == -2
        assert bwd(16, 16, 16, 16, 16, 16, 16, 16, 16, big, 1, 4, 1, 1026, eps, None) == -2
        assert bwd(16, 16, 16, 16, 16, 16, 16, 16, 16, big, 1, 4, 4, 4, zero, None) == -2
        assert bwd(16, 16, 16, 16, 16, 16, 16, 16, 16, ctypes.c_size_t(8), 4, 4, 16, 16, eps, None) == -4      # short workspace
    assert lib.nrv_reattn_softmax_bwd_workspace(4, 8, 196, 196) == 4 * 196 * (64 + 16) * 8
    assert lib.nrv_reattn_norm_bwd_workspace(4, 8, 196, 196) == 4 * 76 * (64 + 16) * 8       # ceil(196 * 196 / 512) = 76 tiles
    assert lib.nrv_reattn_softmax_bwd_workspace(64, 12, 197, 197) == 1024 * (144 + 24) * 8   # at most 1024 partial sets
