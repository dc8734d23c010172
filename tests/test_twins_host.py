"""CPU: Twins-SVT's public interface, module tree, state_dict contract, seeded init and refused configurations against the
reference fixture (tests/golden/twins_small.npz), and the new C-ABI prototypes with their shape / pointer / alignment answers
and the plan query.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import port_checks as PC
import twins_fixture as TF
from noise_robust_vit_amd import twins_svt as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "twins_small.npz")
NEW = ["nrv_subattn_plan", "nrv_subattn_fwd", "nrv_subattn_bwd_workspace", "nrv_subattn_bwd", "nrv_peg_fwd", "nrv_peg_bwd_workspace",
       "nrv_peg_bwd"]
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
    assert pkg.TwinsSVT is V.TwinsSVT and pkg.twins_svt is V and "TwinsSVT" in pkg.__all__ and "twins_svt" in pkg.__all__
    for name in ("TwinsSVT", "Transformer", "LocalAttention", "GlobalAttention", "FeedForward", "PatchEmbedding", "PEG", "PreNorm",
                 "Residual", "LayerNorm", "group_dict_by_key", "group_by_key_prefix_and_remove_prefix"):
        assert name in V.__all__ and hasattr(V, name), name
    m = V.TwinsSVT(**TF.BASE, robust=True)
    attn = [mod for mod in m.modules() if isinstance(mod, (V.LocalAttention, V.GlobalAttention))]
    assert len(attn) == 4 + 4 + 6 + 2 and all(a.robust for a in attn) and m.grad_groups() == []
    assert all((a.heads, a.dim_head) == (8, 64) for a in attn)            # TwinsSVT passes neither heads nor dim_head on
    assert not any(a.robust for a in V.TwinsSVT(**TF.BASE).modules() if isinstance(a, (V.LocalAttention, V.GlobalAttention)))
    assert V.Transformer(16, 1, robust=True).layers[0][0].fn.fn.robust and V.LocalAttention(16, robust=True).robust
    assert V.GlobalAttention(16, robust=True).robust
    with pytest.raises(TypeError):
        V.TwinsSVT(10)                                                    # keyword-only, as in the reference
    a, b = V.group_by_key_prefix_and_remove_prefix("s1_", {"s1_depth": 1, "s2_depth": 2, "dropout": 0.})
    assert a == {"depth": 1} and b == {"s2_depth": 2, "dropout": 0.}
    assert V.group_dict_by_key(lambda k: k.startswith("a"), {"ab": 1, "b": 2}) == ({"ab": 1}, {"b": 2})


@pytest.mark.parametrize("case", list(TF.CASES))
def test_module_tree_and_keys(fx, case):
    m = TF.build(V, case)
    PC.check_tree_and_keys(m, TF.weights(m, 3), fx, case)


def test_key_names_and_shapes():
    m = TF.build(V, "s_train")
    sd = m.state_dict()
    assert {"layers.0.0.proj.weight", "layers.0.0.proj.bias", "layers.0.1.layers.0.0.fn.norm.g", "layers.0.1.layers.0.0.fn.norm.b",
            "layers.0.1.layers.0.0.fn.fn.to_q.weight", "layers.0.1.layers.0.0.fn.fn.to_kv.weight", "layers.0.1.layers.0.0.fn.fn.to_out.0.bias",
            "layers.0.1.layers.0.1.fn.fn.net.0.weight", "layers.0.1.layers.0.3.fn.fn.net.3.bias", "layers.0.2.proj.fn.weight",
            "layers.0.2.proj.fn.bias", "layers.2.3.layers.1.2.fn.fn.to_kv.weight", "layers.3.1.layers.0.2.fn.fn.to_q.weight",
            "layers.6.weight", "layers.6.bias"} <= set(sd)
    assert not any(k.startswith("layers.3.1.layers.0.0.") or k.startswith("layers.3.1.layers.0.1.") for k in sd)   # s4: no local half
    assert tuple(sd["layers.0.1.layers.0.0.fn.norm.g"].shape) == (1, 16, 1, 1)
    assert tuple(sd["layers.0.1.layers.0.0.fn.fn.to_kv.weight"].shape) == (1024, 16, 1, 1)
    assert tuple(sd["layers.0.1.layers.0.2.fn.fn.to_kv.weight"].shape) == (1024, 16, 7, 7)
    assert tuple(sd["layers.1.0.proj.weight"].shape) == (24, 64, 1, 1) and tuple(sd["layers.0.2.proj.fn.weight"].shape) == (16, 1, 3, 3)
    assert "layers.0.1.layers.0.0.fn.fn.to_q.bias" not in sd
    assert isinstance(m.layers[4], torch.nn.AdaptiveAvgPool2d) and not list(m.layers[5].parameters())


@pytest.mark.parametrize("name,cfg", [("small", TF.SMALL), ("full", TF.FULL)])
def test_seeded_init_matches_reference(fx, name, cfg):
    torch.manual_seed(0)
    PC.check_seeded_init(V.TwinsSVT(**cfg), fx, name)


def test_refused_configurations():
    base = dict(TF.BASE)
    for kw in (dict(s1_emb_dim=20), dict(s4_emb_dim=4104), dict(s2_global_k=8), dict(s3_patch_size=8), dict(peg_kernel_size=9),
               dict(peg_kernel_size=4), dict(s1_local_patch_size=9)):
        with pytest.raises(NotImplementedError):
            V.TwinsSVT(**dict(base, **kw))
    img = torch.zeros(1, 3, 56, 56)
    with pytest.raises(NotImplementedError):
        V.TwinsSVT(**dict(base, dropout=0.1)).train()(PC.fake_cuda(img))
    with pytest.raises(NotImplementedError):
        V.TwinsSVT(**base)(PC.fake_cuda(torch.zeros(1, 3, 56, 28)))         # not square
    with pytest.raises(NotImplementedError):
        V.TwinsSVT(**base)(PC.fake_cuda(torch.zeros(1, 3, 48, 48)))         # a 24 x 24 map: windows of 7 do not tile it
    with pytest.raises(NotImplementedError):
        V.TwinsSVT(**dict(base, s1_local_patch_size=4, s1_global_k=5))(PC.fake_cuda(img))     # 28 x 28: k = 5 does not tile it
    from noise_robust_vit_amd.encoder import record_attention
    with record_attention([]):
        with pytest.raises(NotImplementedError):
            V.TwinsSVT(**base)(PC.fake_cuda(img))
    t = V.Transformer(16, 1)
    with pytest.raises(NotImplementedError):
        t(PC.fake_cuda(torch.zeros(1, 16, 7, 14)))
    with pytest.raises(NotImplementedError):
        V.Transformer(16, 1, dropout=0.1).train()(PC.fake_cuda(torch.zeros(1, 16, 7, 7)))
    res = t.layers[0][0]
    for holder in (res, res.fn, res.fn.norm, res.fn.fn, t.layers[0][1].fn.fn, t.layers[0][2].fn.fn, V.PEG(16), V.PEG(16).proj,
                   V.PatchEmbedding(dim=3, dim_out=16, patch_size=2)):
        with pytest.raises(NotImplementedError):
            holder(torch.zeros(1, 16, 7, 7))                              # holders: a Transformer or TwinsSVT runs them
    from noise_robust_vit_amd._lib import NrvError
    with pytest.raises(NrvError):
        V.TwinsSVT(**base)(img)                                           # CPU tensors: no fallback
    with pytest.raises(NrvError):
        t(torch.zeros(1, 16, 7, 7))


def test_new_prototypes_are_declared_bound_and_exported():
    PC.check_prototypes(NEW, abi=19, source="nrv_twins.hip",
                        wrappers=("subattn_fwd", "subattn_bwd", "subattn_plan", "peg_fwd", "peg_bwd"))


def test_subattn_plan(lib):
    from noise_robust_vit_amd import kernels as K
    from noise_robust_vit_amd._lib import NrvError
    p = K.subattn_plan(3136, 64, 64)
    chunk = p["chunk"]
    assert chunk >= 64 and chunk % 64 == 0                                # whole backward steps of 4 waves x 16 rows
    assert p == {"chunk": chunk, "chunks": -(-3136 // chunk), "nk_pad": 64}
    for Nq in (1, chunk, chunk + 1, 2 * chunk + 17):
        assert K.subattn_plan(Nq, 1, 32) == {"chunk": chunk, "chunks": -(-Nq // chunk), "nk_pad": 32}
    assert [K.subattn_plan(49, n, 64)["nk_pad"] for n in (1, 32, 33, 64, 65, 96, 97, 128)] == [32, 32, 64, 64, 96, 96, 128, 128]
    for bad in ((49, 0, 64), (49, 129, 64), (49, 4, 48), (0, 4, 64)):
        with pytest.raises(NrvError):
            K.subattn_plan(*bad)
    assert lib.nrv_subattn_plan(49, 4, 64, None) == ERR_NULL
    # the chunk length is a constant of the source, not a function of the device
    src = open(os.path.join(ROOT, "noise_robust_vit_amd", "csrc", "nrv_twins.hip")).read()
    assert re.search(r"constexpr int SA_CHUNK = %d;" % chunk, src)


def test_subattn_entry_points_answer_without_a_device(lib):
    """Shapes first (NRV_ERR_SHAPE), then pointers (NRV_ERR_NULL), then the workspace and the alignment; no GPU is touched."""
    z, ok, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4100)      # never dereferenced
    sc = ctypes.c_float(0.125)

    def fwd(ptrs, ld=(512, 1024, 1024), shape=(2, 8, 49, 4, 64)):
        q, k, v, o, lse = ptrs
        return lib.nrv_subattn_fwd(q, ld[0], k, ld[1], v, ld[2], o, lse, *shape, sc, None)

    def bwd(ptrs, wsb, ld=(512, 1024, 1024), shape=(2, 8, 49, 4, 64)):
        q, k, v, do, lse, dq, dk, dv, ws = ptrs
        return lib.nrv_subattn_bwd(q, ld[0], k, ld[1], v, ld[2], do, lse, dq, dk, dv, ws, wsb, *shape, sc, None)

    assert fwd([z] * 5) == ERR_NULL and bwd([z] * 9, 0) == ERR_NULL        # a good shape gets as far as the pointers
    for shape in ((2, 8, 49, 0, 64), (2, 8, 49, 129, 64), (2, 8, 49, 4, 48), (2, 8, 49, 4, 128), (2, 8, 0, 4, 64), (0, 8, 49, 4, 64),
                  (2, 0, 49, 4, 64), (70000, 8, 49, 4, 64)):
        assert fwd([z] * 5, shape=shape) == ERR_SHAPE, shape
        assert bwd([z] * 9, 0, shape=shape) == ERR_SHAPE, shape
        assert lib.nrv_subattn_bwd_workspace(*shape) == 0, shape
    for ld in ((504, 1024, 1024), (512, 1020, 1024), (512, 1024, 508), (516, 1024, 1024)):       # narrower than H*dh, or not % 8
        assert fwd([z] * 5, ld=ld) == ERR_SHAPE, ld
        assert bwd([z] * 9, 0, ld=ld) == ERR_SHAPE, ld
    assert fwd([z] * 5, shape=(2, 8, 1, 1, 32), ld=(256, 256, 256)) == ERR_NULL           # one query, one key
    assert fwd([z] * 5, shape=(2, 8, 100000, 128, 64)) == ERR_NULL                        # any Nq
    for i in range(5):
        a = [ok] * 5
        a[i] = z
        assert fwd(a) == ERR_NULL, i
        a[i] = odd if i < 4 else ctypes.c_void_p(4098)                    # lse: fp32 alignment
        assert fwd(a) == ERR_ALIGN, i
    need = lib.nrv_subattn_bwd_workspace(2, 8, 49, 4, 64)
    assert need == 2 * 8 * 1 * 2 * 32 * 64 * 4
    plan = ctypes.create_string_buffer(12)
    assert lib.nrv_subattn_plan(1200, 65, 64, ctypes.addressof(plan)) == 0
    chunk, chunks, nkp = np.frombuffer(plan.raw, dtype=np.int32)
    assert lib.nrv_subattn_bwd_workspace(3, 5, 1200, 65, 64) == 3 * 5 * chunks * 2 * nkp * 64 * 4 and nkp == 96
    for i in range(9):
        a = [ok] * 9
        a[i] = z
        assert bwd(a, need) == ERR_NULL, i
    assert bwd([ok] * 9, need - 1) == ERR_WORKSPACE
    for i in (0, 1, 2, 3, 5, 6, 7, 8):
        a = [ok] * 9
        a[i] = odd
        assert bwd(a, need) == ERR_ALIGN, i
    assert bwd([z] * 9, 0, shape=(2, 8, 49, 129, 64)) == ERR_SHAPE        # shapes come before pointers


def test_peg_entry_points_answer_without_a_device(lib):
    z, ok, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    good = (2, 3, 5, 40, 3)
    assert lib.nrv_peg_fwd(z, z, z, z, *good, None) == ERR_NULL
    assert lib.nrv_peg_bwd(z, z, z, z, z, z, z, 0, *good, None) == ERR_NULL
    for shape in ((2, 3, 5, 36, 3), (2, 3, 5, 40, 4), (2, 3, 5, 40, 9), (2, 3, 5, 40, 1), (0, 3, 5, 40, 3), (70000, 3, 5, 40, 3),
                  (2, 0, 5, 40, 3), (2, 3, 0, 40, 3), (2, 5000, 5000, 40, 3), (2, 3, 5, 0, 3)):
        assert lib.nrv_peg_fwd(z, z, z, z, *shape, None) == ERR_SHAPE, shape
        assert lib.nrv_peg_bwd(z, z, z, z, z, z, z, 0, *shape, None) == ERR_SHAPE, shape
        assert lib.nrv_peg_bwd_workspace(*shape) == 0, shape
    assert lib.nrv_peg_fwd(z, z, z, z, 3, 1, 1, 8, 7, None) == ERR_NULL   # a 1 x 1 plane under a 7 x 7 kernel is a shape
    for i in range(4):
        a = [ok] * 4
        a[i] = z
        assert lib.nrv_peg_fwd(*a, *good, None) == ERR_NULL, i
    for i in (0, 2, 3):                                                   # x, bias, out: 16-byte accesses
        a = [ok] * 4
        a[i] = odd
        assert lib.nrv_peg_fwd(*a, *good, None) == ERR_ALIGN, i
    need = lib.nrv_peg_bwd_workspace(*good)
    assert need == 2 * 10 * 40 * 4 and lib.nrv_peg_bwd_workspace(2, 3, 5, 40, 7) == 2 * 50 * 40 * 4
    for i in range(7):
        a = [ok] * 7
        a[i] = z
        assert lib.nrv_peg_bwd(*a, need, *good, None) == ERR_NULL, i
    assert lib.nrv_peg_bwd(*[ok] * 7, need - 1, *good, None) == ERR_WORKSPACE
    for i in (0, 2, 3, 6):                                                # x, dy, dx, workspace
        a = [ok] * 7
        a[i] = odd
        assert lib.nrv_peg_bwd(*a, need, *good, None) == ERR_ALIGN, i
    assert lib.nrv_peg_bwd(z, z, z, z, z, z, z, 0, 2, 3, 5, 36, 3, None) == ERR_SHAPE


def test_wrappers_refuse_bad_arguments_before_a_launch():
    """kernels.subattn_* / peg_* check dtypes, views and shapes on the host (fake device tensors: nothing is launched)."""
    from noise_robust_vit_amd import kernels as K
    from noise_robust_vit_amd._lib import NrvError
    q = PC.fake_cuda(torch.zeros(2 * 49, 512, dtype=torch.bfloat16))
    kv = PC.fake_cuda(torch.zeros(2 * 4, 1024, dtype=torch.bfloat16))
    for args in ((q, kv[:, :512], kv[:, 512:], 2, 8, 49, 0, 64), (q, kv[:, :512], kv[:, 512:], 2, 8, 49, 129, 64),
                 (q, kv[:, :512], kv[:, 512:], 2, 8, 49, 4, 48), (q.float(), kv[:, :512], kv[:, 512:], 2, 8, 49, 4, 64),
                 (q, kv[:, :512], kv[:, 512:], 2, 8, 50, 4, 64), (q[:, :256], kv[:, :512], kv[:, 512:], 2, 8, 49, 4, 64)):
        with pytest.raises(NrvError):
            K.subattn_fwd(*args, 0.125)
    with pytest.raises(NrvError):
        K.subattn_fwd(torch.zeros(98, 512, dtype=torch.bfloat16), kv[:, :512], kv[:, 512:], 2, 8, 49, 4, 64, 0.125)     # CPU tensor
    x = PC.fake_cuda(torch.zeros(2 * 15, 40))
    for w in (torch.zeros(40, 4), torch.zeros(40, 81), torch.zeros(39, 9)):
        with pytest.raises(NrvError):
            K.peg_fwd(x, PC.fake_cuda(w), PC.fake_cuda(torch.zeros(40)), 2, 3, 5)
    with pytest.raises(NrvError):
        K.peg_fwd(x, PC.fake_cuda(torch.zeros(40, 9)), PC.fake_cuda(torch.zeros(40)), 2, 3, 4)       # 30 rows are not 2 x 3 x 4
    with pytest.raises(NrvError):
        K.peg_fwd(PC.fake_cuda(torch.zeros(30, 36)), PC.fake_cuda(torch.zeros(36, 9)), PC.fake_cuda(torch.zeros(36)), 2, 3, 5)   # C % 8
