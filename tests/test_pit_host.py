"""CPU: PiT's module tree, state_dict contract, seeded init and refused configurations against the reference fixture
(tests/golden/pit_small.npz), the fp32 restatement tests/pit_ref.py against the reference's logits, loss and gradients, and the
new C-ABI prototypes with their shape / pointer / alignment answers.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pit_fixture as PF
import pit_ref as R
import port_checks as PC
from noise_robust_vit_amd import pit as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "pit_small.npz")
NEW = ["nrv_pool_dwconv_fwd", "nrv_pool_dwconv_bwd_workspace", "nrv_pool_dwconv_bwd", "nrv_unfold_patches"]
ERR_NULL, ERR_SHAPE, ERR_DTYPE, ERR_WORKSPACE, ERR_ALIGN = -1, -2, -3, -4, -5


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


@pytest.fixture(scope="module")
def lib():
    from noise_robust_vit_amd import _lib, build
    return _lib.bind(build.build())


def test_public_interface():
    import noise_robust_vit_amd as pkg
    assert pkg.PiT is V.PiT and pkg.pit is V and "PiT" in pkg.__all__ and "pit" in pkg.__all__
    for name in ("PiT", "Transformer", "Attention", "FeedForward", "PreNorm", "Pool", "DepthWiseConv2d", "cast_tuple", "conv_output_size"):
        assert name in V.__all__ and hasattr(V, name), name
    m = V.PiT(**PF.BASE, robust=True)
    stages = [s for s in m.layers if isinstance(s, V.Transformer)]
    assert len(stages) == 3 and all(s._meta.robust for s in stages) and m.grad_groups() == []
    assert [s._meta.heads for s in stages] == [2, 4, 8]
    assert not any(s._meta.robust for s in V.PiT(**PF.BASE).layers if isinstance(s, V.Transformer))
    assert V.cast_tuple(3, 2) == (3, 3) and V.cast_tuple((1, 2), 2) == (1, 2)
    assert V.conv_output_size(224, 14, 7) == 31 and V.conv_output_size(31, 3, 2, 1) == 16
    with pytest.raises(AssertionError):
        V.PiT(**dict(PF.BASE, depth=3))                                   # the reference's assert: depth is a tuple
    with pytest.raises(TypeError):
        V.PiT(32, 8, 10, 32, (1,), 2, 64)                                 # keyword-only, as in the reference


@pytest.mark.parametrize("case", list(PF.CASES))
def test_module_tree_and_keys(fx, case):
    m = PF.build(V, case)
    PC.check_tree_and_keys(m, PF.weights(m, 3), fx, case)


def test_key_names():
    keys = set(PF.build(V, "s_train").state_dict())
    assert {"to_patch_embedding.2.weight", "to_patch_embedding.2.bias", "pos_embedding", "cls_token",
            "layers.0.layers.0.0.norm.weight", "layers.0.layers.0.0.fn.to_qkv.weight", "layers.0.layers.0.0.fn.to_out.0.bias",
            "layers.0.layers.0.1.fn.net.0.weight", "layers.0.layers.0.1.fn.net.3.bias",
            "layers.1.downsample.net.0.weight", "layers.1.downsample.net.0.bias", "layers.1.downsample.net.1.weight",
            "layers.1.cls_ff.weight", "layers.3.cls_ff.bias", "layers.4.layers.0.0.fn.to_qkv.weight", "mlp_head.1.weight"} <= keys
    assert "layers.0.layers.0.0.fn.to_qkv.bias" not in keys
    m = PF.build(V, "s_train")
    assert isinstance(m.to_patch_embedding[0], torch.nn.Unfold) and not list(m.to_patch_embedding[1].parameters())
    assert tuple(m.layers[1].downsample.net[0].weight.shape) == (64, 1, 3, 3) and m.layers[1].downsample.net[0].groups == 32
    assert not any("layers.1." in k for k in PF.build(V, "d1").state_dict())       # one stage: no Pool


@pytest.mark.parametrize("name,cfg", [("small", PF.SMALL), ("full", PF.FULL)])
def test_seeded_init_matches_reference(fx, name, cfg):
    torch.manual_seed(0)
    PC.check_seeded_init(V.PiT(**cfg), fx, name)


@pytest.mark.parametrize("case", list(PF.CASES))
def test_restatement_reproduces_the_reference(fx, case):
    m = PF.build(V, case)
    m.load_state_dict(PF.weights(m, 3), strict=True)
    PC.check_restatement(R.pit_loss_and_grads(m, *PF.inputs(case)), fx, case, m.training)


def test_the_real_grid_crosses_the_attention_kernels():
    """962 -> 257 -> 65 tokens at 224 px / patch 14"""
    g = V.conv_output_size(224, 14, 7)
    counts = [1 + g * g]
    for _ in range(2):
        g = (g - 1) // 2 + 1
        counts.append(1 + g * g)
    assert counts == [962, 257, 65]
    assert tuple(PF.build(V, "g224").pos_embedding.shape) == (1, 962, 32)


def test_refused_configurations():
    base = dict(PF.BASE)
    with pytest.raises(NotImplementedError):
        V.PiT(**dict(base, image_size=(32, 24)))
    for kw in (dict(dim=36), dict(dim_head=3), dict(mlp_dim=100), dict(heads=1, dim_head=32), dict(heads=(2, 1, 2), dim_head=64)):
        with pytest.raises(NotImplementedError):
            V.PiT(**dict(base, **kw))                                     # the last: heads == 1 with dim_head == dim at stage 2
    img = torch.zeros(1, 3, 32, 32)
    for kw in (dict(dropout=0.1), dict(emb_dropout=0.1)):
        with pytest.raises(NotImplementedError):
            V.PiT(**dict(base, **kw)).train()(PC.fake_cuda(img))
    with pytest.raises(NotImplementedError):
        V.PiT(**base)(PC.fake_cuda(torch.zeros(1, 3, 32, 24)))              # not square
    with pytest.raises(NotImplementedError):
        V.PiT(**base)(PC.fake_cuda(torch.zeros(1, 3, 40, 40)))              # 81 patches, the table holds 49
    from noise_robust_vit_amd.encoder import record_attention
    with record_attention([]):
        with pytest.raises(NotImplementedError):
            V.PiT(**base)(PC.fake_cuda(img))
    t, pool = V.Transformer(32, 1, 2, 32, 64), V.Pool(32)
    for mod in (t, pool):
        with pytest.raises(NotImplementedError):
            mod(PC.fake_cuda(torch.zeros(1, 13, 32)))                       # 12 patch tokens: no square grid
    with pytest.raises(NotImplementedError):
        V.Transformer(32, 1, 2, 32, 64, dropout=0.1).train()(PC.fake_cuda(torch.zeros(1, 10, 32)))
    for holder in (t.layers[0][0], t.layers[0][0].fn, t.layers[0][1].fn, pool.downsample):
        with pytest.raises(NotImplementedError):
            holder(torch.zeros(1, 10, 32))                                # holders: a stage and a Pool run as a whole
    from noise_robust_vit_amd._lib import NrvError
    with pytest.raises(NrvError):
        V.PiT(**base)(img)                                                # CPU tensors: no fallback
    with pytest.raises(NrvError):
        pool(torch.zeros(1, 10, 32))


def test_new_prototypes_are_declared_bound_and_exported():
    PC.check_prototypes(NEW, abi=19, source="nrv_pit.hip", wrappers=("pool_dwconv_fwd", "pool_dwconv_bwd", "unfold_patches"))


def test_pool_entry_points_answer_without_a_device(lib):
    """Shapes first (NRV_ERR_SHAPE), then pointers (NRV_ERR_NULL), then the workspace and the alignment; no GPU is touched."""
    z = ctypes.c_void_p(0)
    ok, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)               # never dereferenced: every call returns before a launch
    good = (2, 3, 3, 1, 64)
    assert lib.nrv_pool_dwconv_fwd(z, z, z, z, *good, None) == ERR_NULL   # a good shape gets as far as the pointers
    assert lib.nrv_pool_dwconv_bwd(z, z, z, z, z, z, z, 0, *good, None) == ERR_NULL
    for B, H, W, lead, C in ((2, 3, 3, 1, 60), (2, 3, 3, 1, 4), (2, 3, 3, 2, 64), (2, 3, 3, -1, 64), (70000, 3, 3, 1, 64), (0, 3, 3, 1, 64),
                             (2, 0, 3, 1, 64), (2, 3, 0, 1, 64), (2, 5000, 5000, 0, 64), (2, 3, 3, 1, 0)):
        assert lib.nrv_pool_dwconv_fwd(z, z, z, z, B, H, W, lead, C, None) == ERR_SHAPE, (B, H, W, lead, C)
        assert lib.nrv_pool_dwconv_bwd(z, z, z, z, z, z, z, 0, B, H, W, lead, C, None) == ERR_SHAPE, (B, H, W, lead, C)
    assert lib.nrv_pool_dwconv_fwd(z, z, z, z, 3, 1, 1, 0, 8, None) == ERR_NULL        # a 1 x 1 plane is a shape
    for k in range(4):                                                    # any one NULL / misaligned pointer
        a = [ok] * 4
        a[k] = z
        assert lib.nrv_pool_dwconv_fwd(*a, *good, None) == ERR_NULL, k
        a[k] = odd
        assert lib.nrv_pool_dwconv_fwd(*a, *good, None) == ERR_ALIGN, k
    need = lib.nrv_pool_dwconv_bwd_workspace(2, 3, 3, 64)
    assert need == 2 * 20 * 64 * 4
    assert lib.nrv_pool_dwconv_bwd_workspace(2, 3, 3, 60) == 0 and lib.nrv_pool_dwconv_bwd_workspace(70000, 3, 3, 64) == 0
    for k in range(7):
        a = [ok] * 7
        a[k] = z
        assert lib.nrv_pool_dwconv_bwd(*a, need, *good, None) == ERR_NULL, k
    assert lib.nrv_pool_dwconv_bwd(*[ok] * 7, need - 1, *good, None) == ERR_WORKSPACE
    for k in (0, 1, 2, 3, 6):                                             # x, w, dout, dx, workspace: 16-byte accesses
        a = [ok] * 7
        a[k] = odd
        assert lib.nrv_pool_dwconv_bwd(*a, need, *good, None) == ERR_ALIGN, k
    # shapes come before pointers: a bad shape with NULL pointers is a shape error
    assert lib.nrv_pool_dwconv_bwd(z, z, z, z, z, z, z, 0, 2, 3, 3, 1, 60, None) == ERR_SHAPE


def test_unfold_patches_answers_without_a_device(lib):
    z, ok, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    F32, BF16 = 0, 1
    assert lib.nrv_unfold_patches(z, F32, z, 2, 3, 42, 42, 14, 7, None) == ERR_NULL
    assert lib.nrv_unfold_patches(z, F32, z, 2, 3, 64, 64, 32, 16, None) == ERR_NULL   # ks = 32 is a shape
    for B, C, H, W, ks, stride in ((2, 3, 66, 66, 33, 16), (2, 3, 42, 42, 14, 15), (2, 3, 42, 42, 14, 0), (2, 3, 42, 42, 0, 1),
                                   (2, 3, 13, 42, 14, 7), (2, 3, 42, 13, 14, 7), (0, 3, 42, 42, 14, 7), (2, 0, 42, 42, 14, 7)):
        assert lib.nrv_unfold_patches(z, F32, z, B, C, H, W, ks, stride, None) == ERR_SHAPE, (B, C, H, W, ks, stride)
    assert lib.nrv_unfold_patches(ok, F32, z, 2, 3, 42, 42, 14, 7, None) == ERR_NULL
    assert lib.nrv_unfold_patches(z, F32, ok, 2, 3, 42, 42, 14, 7, None) == ERR_NULL
    assert lib.nrv_unfold_patches(ok, 7, ok, 2, 3, 42, 42, 14, 7, None) == ERR_DTYPE
    assert lib.nrv_unfold_patches(ok, BF16, odd, 2, 3, 42, 42, 14, 7, None) == ERR_ALIGN
    # the shared geometry keeps ks <= 7 for the soft split and the convolutions
    assert lib.nrv_soft_split_fwd(z, F32, 0, 0, z, 2, 3, 42, 42, 8, 4, 0, None) == ERR_SHAPE
    assert lib.nrv_soft_split_bwd(z, z, 8, 2, 3, 42, 42, 8, 4, 0, None) == ERR_SHAPE
    assert lib.nrv_conv_unfold(z, F32, 0, z, 2, 3, 42, 42, 8, 4, 0, None) == ERR_SHAPE
    assert lib.nrv_conv_fold(z, z, 2, 3, 42, 42, 8, 4, 0, None) == ERR_SHAPE
    assert lib.nrv_soft_split_fwd(z, F32, 0, 0, z, 2, 3, 42, 42, 7, 4, 2, None) == ERR_NULL


def test_the_unfold_call_site_keeps_the_split_grid_cap():
    src = open(os.path.join(ROOT, "noise_robust_vit_amd", "csrc", "nrv_misc.hip")).read()
    body = src[src.index('extern "C" int nrv_unfold_patches'):]
    body = body[:body.index("\n}\n")]
    assert re.search(r"launch_unfold<UF_CHANNEL_MAJOR>\([^;]*\bSPLIT_GRID_CAP\b", body)
    assert "constexpr int CONV_GRID_CAP = 4096, SPLIT_GRID_CAP = 16384;" in src
