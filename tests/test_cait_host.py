"""CPU: the CaiT module tree, seeded init, strict state_dict loading, layer-dropout draws and refusals, the fp32 restatement
against the reference fixture, and the talking-heads prototypes in the header, the binding and the library's exports (no GPU)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cait_fixture as CF  # noqa: E402
import cait_ref as R  # noqa: E402

from noise_robust_vit_amd import cait as C  # noqa: E402
from noise_robust_vit_amd._lib import NrvError  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "cait_small.npz")
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
    w = CF.weights(m, 3)
    m.load_state_dict(w, strict=True)
    tree = CF.unpack_tree(fx, case)
    assert list(tree) == list(m.state_dict())
    for k, (shape, s) in tree.items():
        assert tuple(m.state_dict()[k].shape) == shape, k
        assert abs(float(w[k].double().sum()) - s) <= 1e-9 * max(1.0, abs(s)), k
    img, y = CF.inputs(case)
    logits, loss, grads = R.cait_loss_and_grads(m, img, y)
    ref = CF.unpack(fx, case + ".logits")
    assert float((logits - ref).abs().max()) <= 2e-3 * float(ref.abs().max())
    assert abs(loss.item() - float(fx[case + ".loss"])) < 1e-4
    if m.training:
        G = CF.unpack_grads(fx, case)
        assert sorted(G) == sorted(grads)
        for k, g in G.items():
            a = CF.grad_sample(k, grads[k])
            if CF.CASES[case][1] and k.startswith("cls_transformer") and k.endswith(("to_q.weight", "mix_heads_pre_attn")):
                # one query under Sinkhorn: uniform weights, the gradient is rounding noise on both sides
                assert float(a.abs().max()) < 1e-6 and float(g.abs().max()) < 1e-6, k
                continue
            assert float((a - g).norm() / (g.norm() + 1e-12)) < 2e-3, k


@pytest.mark.parametrize("name,cfg", [("small", CF.SMALL), ("full", CF.FULL)])
def test_seeded_init_matches_reference(fx, name, cfg):
    torch.manual_seed(0)
    m = C.CaiT(**cfg)
    sd = m.state_dict()
    tree = CF.unpack_tree(fx, name)
    assert list(tree) == list(sd)
    for k, (shape, s) in tree.items():
        assert tuple(sd[k].shape) == shape, k
        v = float(sd[k].double().sum())
        assert abs(v - s) <= 1e-6 * max(1.0, abs(s)), (k, v, s)
    assert sum(p.numel() for p in m.parameters()) == int(fx[name + ".nparams"])
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
    from noise_robust_vit_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nrv.h")).read()
    assert int(re.search(r"#define NRV_ABI_VERSION (\d+)\b", hdr).group(1)) == _lib.ABI_VERSION
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
    from noise_robust_vit_amd import build
    import ctypes
    lib = ctypes.CDLL(build.build())
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.nrv_abi_version() == _lib.ABI_VERSION
    # shapes are classified on the host, before any launch: callable without a GPU
    assert lib.nrv_th_softmax_fwd(16, 16, 16, 16, 16, 0, 1, 17, 4, 4, None) == -2
    assert lib.nrv_head_mix_fwd(16, 16, 16, 0, 1, 4, 1, 1026, None) == -2
    assert lib.nrv_th_softmax_bwd_workspace(4, 8, 196, 196) == 4 * 196 * 2 * 64 * 8
