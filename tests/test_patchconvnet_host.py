"""CPU: the PatchConvNet module tree, seeded init and refusals, the fp32 restatement against the reference fixture, and the
ABI 17 prototypes in the header, the binding and the library's exports (no GPU)."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import patchconvnet_fixture as PF
import patchconvnet_ref as R
import port_checks as PC
from noise_robust_vit_amd import patch_convnet as P

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patchconvnet_small.npz")
NEW = ("nrv_dwconv3x3_fwd", "nrv_dwconv3x3_bwd_workspace", "nrv_dwconv3x3_bwd", "nrv_se_fwd", "nrv_se_apply", "nrv_se_bwd_workspace",
       "nrv_se_bwd", "nrv_ls_add_f32", "nrv_ls_bwd_workspace", "nrv_ls_bwd", "nrv_dgelu_rows", "nrv_cls_attn_fwd", "nrv_cls_attn_bwd")


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


def test_package_exports_patch_convnet():
    import noise_robust_vit_amd
    assert noise_robust_vit_amd.patch_convnet is P
    for name in PF.BUILDERS:
        assert callable(getattr(P, name))


@pytest.mark.parametrize("case", list(PF.CASES))
def test_restatement_matches_reference_fixture(fx, case):
    m = PF.build(P, case)
    PC.check_keys_and_sums(m, PF.weights(m, 3), fx, case, rtol=1e-9)
    PC.check_restatement(R.pcn_loss_and_grads(m, *PF.inputs(case)), fx, case, m.training, loss_tol=1e-4, grad_tol=2e-3)


@pytest.mark.parametrize("name", PF.BUILDERS)
def test_seeded_builders_match_reference(fx, name):
    torch.manual_seed(0)
    PC.check_seeded_init(getattr(P, name)(num_classes=100), fx, name, rtol=1e-6, atol=0.0)
    if name in PF.NPARAMS:
        assert int(fx[name + ".nparams"]) == PF.NPARAMS[name]


def test_robust_constructs_with_the_same_state_dict_and_refuses_forward():
    torch.manual_seed(0)
    a = P.PatchConvnet(**PF.SMALL)
    torch.manual_seed(0)
    b = P.PatchConvnet(**PF.SMALL, robust=True)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    with pytest.raises(NotImplementedError, match="uniform"):
        b._check_forward(_fake_cuda(1, 64))


def _fake_cuda(B, S):
    class T:
        is_cuda = True
        shape = (B, 3, S, S)

        def dim(self):
            return 4
    return T()


@pytest.mark.parametrize("kw,match", [
    (dict(multiclass=True), "multiclass"),
    (dict(act_layer=nn.ReLU), "act_layer"),
    (dict(norm_layer=nn.BatchNorm1d), "LayerNorm"),
    (dict(Attention_block=nn.Identity), "Attention_block"),
    (dict(block_layers=nn.Identity), "block_layers"),
    (dict(Patch_layer=nn.Identity), "Patch_layer"),
    (dict(embed_dim=72), "multiples of 8"),
    (dict(num_heads=3), "head dims"),
])
def test_refusals_at_construction(kw, match):
    with pytest.raises(NotImplementedError, match=match):
        P.PatchConvnet(**dict(PF.SMALL, **kw))


def test_s60_multi_is_refused():
    with pytest.raises(NotImplementedError):
        P.S60_multi()


@pytest.mark.parametrize("S,train,kw,match", [
    (64, True, dict(drop_rate=0.1), "dropout"),
    (64, True, dict(attn_drop_rate=0.1), "dropout"),
    (72, False, {}, "multiples"),
])
def test_refusals_at_forward(S, train, kw, match):
    m = P.PatchConvnet(**dict(PF.SMALL, **kw)).train(train)
    with pytest.raises(NotImplementedError, match=match):
        m._check_forward(_fake_cuda(1, S))


def test_non_square_and_recording_are_refused():
    m = P.PatchConvnet(**PF.SMALL)
    t = _fake_cuda(1, 64)
    t.shape = (1, 3, 64, 48)
    with pytest.raises(NotImplementedError, match="square"):
        m._check_forward(t)
    from noise_robust_vit_amd import encoder as E
    prev, E._RECORDING = E._RECORDING, []
    try:
        with pytest.raises(NotImplementedError, match="recording"):
            m._check_forward(_fake_cuda(1, 64))
    finally:
        E._RECORDING = prev
    # dropout in eval is a no-op in the reference: accepted
    P.PatchConvnet(**dict(PF.SMALL, drop_rate=0.1)).eval()._check_forward(_fake_cuda(1, 64))


def test_cpu_input_is_refused():
    m = P.PatchConvnet(**PF.SMALL)
    with pytest.raises(RuntimeError, match="HIP"):
        m(torch.zeros(1, 3, 64, 64))


def test_reference_helpers():
    m = P.S60(num_classes=100)
    assert m.no_weight_decay() == {"cls_token"}
    assert m.get_classifier() is m.head and m.get_num_layers() == 60
    m.reset_classifier(7)
    assert m.head.out_features == 7 and m.num_classes == 7
    assert isinstance(m.blocks[0].norm1, nn.LayerNorm) and m.blocks[0].norm1.eps == 1e-6
    q = P.PatchConvnet(**dict(PF.SMALL, qkv_bias=False, qk_scale=0.5, num_heads=2))
    assert q.blocks_token_only[0].attn.q.bias is None and q.blocks_token_only[0].attn.scale == 0.5


def test_trunc_normal_draws_like_the_reference():
    """utils.py:1040-1075 and torch.nn.init.trunc_normal_ consume the RNG identically (uniform_, erfinv_, mul_, add_, clamp_)."""
    import math
    torch.manual_seed(3)
    a = torch.empty(1000)
    nn.init.trunc_normal_(a, std=0.02)
    torch.manual_seed(3)
    b = torch.empty(1000)
    cdf = lambda x: (1.0 + math.erf(x / math.sqrt(2.0))) / 2.0   # noqa: E731
    lo, hi = cdf((-2.0 - 0.0) / 0.02), cdf((2.0 - 0.0) / 0.02)
    b.uniform_(2 * lo - 1, 2 * hi - 1).erfinv_().mul_(0.02 * math.sqrt(2.0)).add_(0.0).clamp_(min=-2.0, max=2.0)
    assert torch.equal(a, b)


def test_abi17_prototypes_in_header_binding_and_exports():
    PC.check_prototypes(NEW, abi=19)
