"""CPU: the CaiT module tree, seeded init, strict state_dict loading, layer-dropout draws and refusals, the fp32 restatement
against the reference fixture, and the talking-heads prototypes in the header, the binding and the library's exports (no GPU)."""
import os

import numpy as np
import pytest
import torch

import cait_fixture as CF
import cait_ref as R
import port_checks as PC
from noise_robust_vit_amd import cait as C
from noise_robust_vit_amd._lib import NrvError

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cait_small.npz")
NEW = ("nrv_th_softmax_fwd", "nrv_th_softmax_bwd_workspace", "nrv_th_softmax_bwd", "nrv_head_mix_fwd", "nrv_head_mix_bwd_workspace",
       "nrv_head_mix_bwd")


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


def test_package_exports_cait():
    import noise_robust_vit_amd
    assert noise_robust_vit_amd.cait is C
    for name in ("CaiT", "Transformer", "Attention", "FeedForward", "LayerScale", "PreNorm", "dropout_layers"):
        assert hasattr(C, name), name


@pytest.mark.parametrize("case", list(CF.CASES))
def test_restatement_matches_reference_fixture(fx, case):
    m = CF.build(C, case)
    PC.check_keys_and_sums(m, CF.weights(m, 3), fx, case, rtol=1e-9)

    def noise(k, g):
        # one query under Sinkhorn: uniform weights, the gradient is rounding noise on both sides
        return CF.CASES[case][1] and k.startswith("cls_transformer") and k.endswith(("to_q.weight", "mix_heads_pre_attn"))
    PC.check_restatement(R.cait_loss_and_grads(m, *CF.inputs(case)), fx, case, m.training, loss_tol=1e-4, grad_tol=2e-3, noise=noise)


@pytest.mark.parametrize("name,cfg", [("small", CF.SMALL), ("full", CF.FULL)])
def test_seeded_init_matches_reference(fx, name, cfg):
    torch.manual_seed(0)
    PC.check_seeded_init(C.CaiT(**cfg), fx, name, rtol=1e-6, atol=0.0)
    if name == "small":
        assert int(fx[name + ".nparams"]) == CF.SMALL_NPARAMS


def test_layer_scale_init_follows_the_layer_index():
    t = C.Transformer(16, 26, 2, 8, 32)
    vals = [float(a.scale.detach().flatten()[0]) for a, _ in t.layers]
    assert vals[:18] == [pytest.approx(0.1)] * 18 and vals[18:24] == [pytest.approx(1e-5)] * 6 and vals[24:] == [pytest.approx(1e-6)] * 2
    assert all(float(f.scale.detach().flatten()[0]) == v for (_, f), v in zip(t.layers, vals))


def test_robust_keyword_keeps_the_state_dict_and_reaches_both_transformers():
    torch.manual_seed(0)
    a = C.CaiT(**CF.SMALL)
    torch.manual_seed(0)
    b = C.CaiT(**CF.SMALL, robust=True)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    b.load_state_dict(sa, strict=True); a.load_state_dict(sb, strict=True)
    flags = lambda m: [l[0].fn.fn.robust for t in (m.patch_transformer, m.cls_transformer) for l in t.layers]  # noqa: E731
    assert flags(a) == [False] * 4 and flags(b) == [True] * 4
    assert C.Transformer(16, 1, 2, 8, 32, robust=True).layers[0][0].fn.fn.robust
    assert C.Attention(16, heads=2, dim_head=8, robust=True).robust and not C.Attention(16, heads=2, dim_head=8).robust


def test_dropout_layers_reproduces_the_reference_draws(fx):
    for row, d in zip(fx["draws"], CF.DRAWS):
        assert CF.draw(C, *d) == [int(i) for i in row if i >= 0], d
    layers = [object(), object()]
    assert C.dropout_layers(layers, 0) is layers


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
    (dict(dim=4104, heads=2, dim_head=8, mlp_dim=8, depth=1, cls_depth=1), "4096"),
])
def test_refusals_at_construction(kw, match):
    with pytest.raises(NotImplementedError, match=match):
        C.CaiT(**dict(CF.SMALL, **kw))


@pytest.mark.parametrize("kw", [dict(dropout=0.1), dict(emb_dropout=0.1)])
def test_dropout_in_training_is_refused_and_eval_is_not(kw):
    m = C.CaiT(**dict(CF.SMALL, **kw))
    with pytest.raises(NotImplementedError, match="dropout"):
        m.train()._check_forward(_Fake(1, 3, 64, 64))
    m.eval()._check_forward(_Fake(1, 3, 64, 64))
    if "dropout" in kw:
        with pytest.raises(NotImplementedError, match="dropout"):
            m.train().patch_transformer._check_forward(_Fake(1, 16, 64))


def test_shapes_outside_the_kernels_range_are_refused():
    m = C.CaiT(**dict(CF.SMALL, image_size=528, depth=1, cls_depth=1))          # 33 x 33 = 1089 patches
    with pytest.raises(NotImplementedError, match="1025"):
        m._check_forward(_Fake(1, 3, 528, 528))
    C.CaiT(**dict(CF.SMALL, image_size=512, depth=1, cls_depth=1))._check_forward(_Fake(1, 3, 512, 512))     # 1024 + 1 keys
    t = C.Transformer(16, 1, 2, 8, 32)
    with pytest.raises(NotImplementedError, match="1025"):
        t._check_forward(_Fake(1, 1, 16), _Fake(1, 1025, 16))
    t._check_forward(_Fake(1, 1, 16), _Fake(1, 1024, 16))
    with pytest.raises(NotImplementedError, match="multiples"):
        C.CaiT(**CF.SMALL)._check_forward(_Fake(1, 3, 72, 64))
    with pytest.raises(NotImplementedError, match="positional"):
        C.CaiT(**CF.SMALL)._check_forward(_Fake(1, 3, 128, 128))


def test_recording_cpu_tensors_and_direct_calls_are_refused():
    m = C.CaiT(**CF.SMALL)
    from noise_robust_vit_amd import encoder as E
    prev, E._RECORDING = E._RECORDING, []
    try:
        with pytest.raises(NotImplementedError, match="recording"):
            m._check_forward(_Fake(1, 3, 64, 64))
        with pytest.raises(NotImplementedError, match="recording"):
            m.patch_transformer._check_forward(_Fake(1, 16, 64))
    finally:
        E._RECORDING = prev
    with pytest.raises(NrvError, match="HIP"):
        m(torch.zeros(1, 3, 64, 64))
    with pytest.raises(NrvError, match="HIP"):
        m.cls_transformer(torch.zeros(1, 1, 64), context=torch.zeros(1, 16, 64))
    with pytest.raises(NotImplementedError, match="holds parameters"):
        m.patch_transformer.layers[0][0](torch.zeros(1, 16, 64))


def test_capture_refuses_layer_dropout():
    import inspect
    from noise_robust_vit_amd.train import Trainer
    assert C.CaiT(**dict(CF.SMALL, layer_dropout=0.2)).layer_dropout == 0.2
    src = inspect.getsource(Trainer.capture)
    assert "layer_dropout" in src


def test_talking_heads_prototypes_in_header_binding_and_exports():
    lib = PC.check_prototypes(NEW)
    # shapes are classified on the host, before any launch: callable without a GPU
    assert lib.nrv_th_softmax_fwd(16, 16, 16, 16, 16, 0, 1, 17, 4, 4, None) == -2
    assert lib.nrv_head_mix_fwd(16, 16, 16, 0, 1, 4, 1, 1026, None) == -2
    assert lib.nrv_th_softmax_bwd_workspace(4, 8, 196, 196) == 4 * 196 * 2 * 64 * 8
