"""CPU: RvT's module tree, state_dict contract, seeded init and refused configurations against the reference fixture
(tests/golden/rvt_small.npz), the fp32 restatement tests/rvt_ref.py against the reference's logits, loss and gradients, the rotary
tables against stored entries, and the new C-ABI prototypes.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import port_checks as PC
import rvt_fixture as RF
import rvt_ref as R
from noise_robust_vit_amd import rvt as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "rvt_small.npz")
NEW = ["nrv_rotary_fwd", "nrv_rotary_bwd", "nrv_dwconv_fwd", "nrv_dwconv_bwd_workspace", "nrv_dwconv_bwd", "nrv_geglu_fwd",
       "nrv_geglu_bwd"]


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


def test_public_interface():
    import noise_robust_vit_amd as pkg
    assert pkg.RvT is V.RvT and pkg.rvt is V and "RvT" in pkg.__all__ and "rvt" in pkg.__all__
    for name in ("RvT", "Transformer", "Attention", "FeedForward", "GEGLU", "SpatialConv", "DepthWiseConv2d", "PreNorm",
                 "AxialRotaryEmbedding", "rotate_every_two"):
        assert name in V.__all__ and hasattr(V, name), name
    m = V.RvT(**RF.SMALL, robust=True)
    assert m.transformer.robust and m.grad_groups() == []
    m = V.RvT(**dict(RF.ONE, use_ds_conv=False))
    a = m.transformer.layers[0][0].fn
    assert m.grad_groups() == [(a.to_q.weight, a.to_kv.weight)]


@pytest.mark.parametrize("case", list(RF.CASES))
def test_module_tree_and_keys(fx, case):
    m = RF.build(V, case)
    PC.check_tree_and_keys(m, RF.weights(m, 3), fx, case)


def test_key_names_of_the_query_projection():
    keys = set(RF.build(V, "proj").state_dict())
    p = "transformer.layers.0.0.fn.to_q."
    assert {p + "conv.net.0.weight", p + "conv.net.1.weight", p + "cls_proj.weight", p + "cls_proj.bias"} <= keys
    keys = set(RF.build(V, "s_train").state_dict())
    assert p + "cls_proj.weight" not in keys                          # dim == heads * dim_head: Identity
    assert {"transformer.layers.1.1.fn.net.0.weight", "transformer.layers.1.1.fn.net.3.bias"} <= keys
    keys = set(RF.build(V, "noconv").state_dict())
    assert p + "weight" in keys and p + "conv.net.0.weight" not in keys


@pytest.mark.parametrize("name,cfg", [("small", RF.SMALL), ("full", RF.FULL)])
def test_seeded_init_matches_reference(fx, name, cfg):
    torch.manual_seed(0)
    PC.check_seeded_init(V.RvT(**cfg), fx, name)


@pytest.mark.parametrize("case", list(RF.CASES))
def test_restatement_reproduces_the_reference(fx, case):
    m = RF.build(V, case)
    m.load_state_dict(RF.weights(m, 3), strict=True)
    PC.check_restatement(R.rvt_loss_and_grads(m, *RF.inputs(case)), fx, case, m.training)


@pytest.mark.parametrize("i", range(len(RF.ROTARY_PROBES)))
def test_rotary_tables_equal_the_stored_entries(fx, i):
    n, dim, mf = RF.ROTARY_PROBES[i]
    x = RF.rotary_probe_input(n, dim)
    emb = V.AxialRotaryEmbedding(dim, max_freq=mf)
    sin, cos = emb(x)
    assert torch.equal(sin, torch.from_numpy(fx[f"rot{i}.sin"])) and torch.equal(cos, torch.from_numpy(fx[f"rot{i}.cos"]))
    assert torch.equal(V.rotate_every_two(x), torch.from_numpy(fx[f"rot{i}.rot"]))
    # the kernel's tables are the same entries, one per feature pair; the restatement's own formula agrees
    s2, c2 = V._axial_tables(n, dim, mf)
    assert s2.shape == (n * n, 2 * (dim // 4)) and torch.equal(s2.repeat_interleave(2, -1)[None], sin)
    assert torch.equal(c2.repeat_interleave(2, -1)[None], cos)
    s3, c3 = R.axial_tables(n, dim, float(mf), "cpu")
    tol = 4 * (mf / 2 * torch.pi) * 2.0 ** -24 + 1e-6                # a few fp32 roundings of the largest angle
    assert torch.allclose(s3, s2, atol=tol, rtol=0) and torch.allclose(c3, c2, atol=tol, rtol=0)
    if n == 1:
        assert torch.allclose(s2[0, 0], torch.sin(torch.tensor(-1.0 * torch.pi)), atol=1e-6)      # coordinate -1, scale 1


def test_refused_configurations():
    base = dict(RF.ONE)
    with pytest.raises(NotImplementedError):
        V.RvT(**dict(base, image_size=(48, 32)))
    for kw in (dict(dim=60), dict(dim_head=36), dict(mlp_dim=100), dict(heads=1, dim_head=20)):
        with pytest.raises(NotImplementedError):
            V.RvT(**dict(base, **kw))
    img = torch.zeros(1, 3, 48, 48)
    for kw in (dict(dropout=0.1), dict(emb_dropout=0.1)):
        with pytest.raises(NotImplementedError):
            V.RvT(**dict(base, **kw)).train()(PC.fake_cuda(img))
    with pytest.raises(NotImplementedError):
        V.RvT(**base)(PC.fake_cuda(torch.zeros(1, 3, 48, 40)))
    from noise_robust_vit_amd.encoder import record_attention
    with record_attention([]):
        with pytest.raises(NotImplementedError):
            V.RvT(**base)(PC.fake_cuda(img))
    t = V.Transformer(64, 1, 2, 32, 96, 48)
    with pytest.raises(NotImplementedError):
        t(PC.fake_cuda(torch.zeros(1, 13, 64)), fmap_dims={'h': 3, 'w': 4})
    with pytest.raises(NotImplementedError):
        t.layers[0][0].fn(torch.zeros(1, 10, 64))                     # a holder: the layer runs as a whole
    from noise_robust_vit_amd._lib import NrvError
    with pytest.raises(NrvError):
        V.RvT(**base)(img)                                            # CPU tensors: no fallback


def test_new_prototypes_are_declared_bound_and_exported():
    PC.check_prototypes(NEW, abi=19, source="nrv_rvt.hip",
                        wrappers=("rotary_fwd", "rotary_bwd", "dwconv_fwd", "dwconv_bwd", "geglu_fwd", "geglu_bwd"))


def test_shape_errors_come_back_before_any_launch():
    """Out-of-contract shapes return NRV_ERR_SHAPE from the host-side checks (no GPU is touched)."""
    from noise_robust_vit_amd import _lib
    lib = _lib.bind(__import__("noise_robust_vit_amd.build", fromlist=["build"]).build())
    p = ctypes.c_void_p(0)
    ERR_SHAPE, ERR_NULL = -2, -1
    for fn in (lib.nrv_rotary_fwd, lib.nrv_rotary_bwd):
        assert fn(p, p, p, 2, 10, 1, 2, 32, 32, None) == ERR_NULL                     # a good shape gets as far as the pointers
        assert fn(p, p, p, 2, 10, 1, 2, 32, 31, None) == ERR_SHAPE                    # dr odd
        assert fn(p, p, p, 2, 10, 1, 2, 32, 34, None) == ERR_SHAPE                    # dr > dh
        assert fn(p, p, p, 2, 10, 1, 2, 32, 0, None) == ERR_SHAPE
        assert fn(p, p, p, 2, 10, 1, 2, 36, 32, None) == ERR_SHAPE                    # dh % 8
        assert fn(p, p, p, 2, 10, 2, 2, 32, 32, None) == ERR_SHAPE                    # lead = 2
        assert fn(p, p, p, 2, 1, 1, 2, 32, 32, None) == ERR_SHAPE                     # no patch rows
        assert fn(p, p, p, 0, 10, 1, 2, 32, 32, None) == ERR_SHAPE
    assert lib.nrv_dwconv_fwd(p, p, p, 2, 3, 3, 1, 64, 5, None) == ERR_NULL
    for B, H, W, lead, C, ks in ((2, 3, 3, 1, 60, 5), (2, 3, 3, 1, 64, 4), (2, 3, 3, 1, 64, 9), (2, 3, 3, 2, 64, 5), (70000, 3, 3, 1, 64, 5),
                                 (2, 0, 3, 1, 64, 5), (2, 5000, 5000, 0, 64, 3), (2, 3, 3, -1, 64, 3)):
        assert lib.nrv_dwconv_fwd(p, p, p, B, H, W, lead, C, ks, None) == ERR_SHAPE, (B, H, W, lead, C, ks)
        assert lib.nrv_dwconv_bwd(p, p, p, p, p, p, 0, B, H, W, lead, C, ks, None) == ERR_SHAPE, (B, H, W, lead, C, ks)
    assert lib.nrv_dwconv_bwd_workspace(2, 3, 3, 64, 4) == 0 and lib.nrv_dwconv_bwd_workspace(2, 3, 3, 60, 5) == 0
    assert lib.nrv_dwconv_bwd_workspace(3, 14, 14, 384, 5) == 3 * 384 * 25 * 4
    assert lib.nrv_geglu_fwd(p, 16, p, 3, 8, None) == ERR_NULL
    for ld, rows, hidden in ((16, 3, 12), (16, 3, 4), (15, 3, 8), (24, 3, 16), (20, 3, 8), (16, 0, 8)):
        assert lib.nrv_geglu_fwd(p, ld, p, rows, hidden, None) == ERR_SHAPE, (ld, rows, hidden)
        assert lib.nrv_geglu_bwd(p, ld, p, p, rows, hidden, None) == ERR_SHAPE, (ld, rows, hidden)
