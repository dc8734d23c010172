"""CPU: the LeViT modules against the reference fixture (module trees and seeded init of all five builders, bias indices, a
reference checkpoint), the fp32 restatement tests/levit_ref.py against the reference's logits, loss, gradients and running
statistics, refusals, and the host-side argument checks of the new C entry points (no GPU)."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch
from torch import nn

import levit_fixture as LF
import levit_ref
from noise_robust_vit_amd import levit as L

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "levit_small.npz")


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLD)


@pytest.mark.parametrize("name", LF.BUILDERS)
def test_builder_tree_and_seeded_init_match_reference(fx, name):
    torch.manual_seed(0)
    m = getattr(L, name)()
    sd = m.state_dict()
    tree = LF.unpack_tree(fx, name)
    assert list(sd) == list(tree)
    for k, v in sd.items():
        assert tuple(v.shape) == tree[k][0], k
        assert float(v.double().sum()) == pytest.approx(tree[k][1], rel=1e-12, abs=1e-9), k
    assert int(fx[name + ".nparams"]) == sum(p.numel() for p in m.parameters())


def test_reference_checkpoint_loads_strictly(fx):
    """A state_dict with the reference's keys and shapes (the fixture's 128S tree) loads strictly and lands where it should."""
    tree = LF.unpack_tree(fx, "LeViT_128S")
    torch.manual_seed(0)
    m = L.LeViT_128S()
    ref = {k: (torch.full(shape, 0.5) if m.state_dict()[k].is_floating_point() else m.state_dict()[k].clone())
           for k, (shape, _) in tree.items()}
    m.load_state_dict(ref, strict=True)
    assert torch.equal(m.blocks[0].m.qkv.c.weight, torch.full_like(m.blocks[0].m.qkv.c.weight, 0.5))


@pytest.mark.parametrize("case", list(LF.CASES))
def test_case_tree_and_bias_indices_match_reference(fx, case):
    m = LF.build(L, case)
    tree = LF.unpack_tree(fx, case)
    sd = m.state_dict()
    assert list(sd) == list(tree)
    w = LF.weights(m, seed=3)
    for k, v in w.items():
        assert float(v.double().sum()) == pytest.approx(tree[k][1], rel=1e-12, abs=1e-9), k
    if case == "g224":
        idx = [v for k, v in sd.items() if k.endswith("attention_bias_idxs")]
        geoms = {tuple(t.shape) for t in idx}
        assert {(196, 196), (49, 196), (49, 49), (16, 49), (16, 16)} <= geoms
        for i, t in enumerate(idx):
            assert torch.equal(t, torch.from_numpy(fx[f"g224.idx.{i}"].astype(np.int64))), i


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@pytest.mark.parametrize("case", list(LF.CASES))
def test_restatement_reproduces_reference(fx, case):
    """levit_ref (the GPU oracle) on CPU against what the reference's levit.py computed (float16-relative storage)."""
    m = LF.build(L, case)
    m.load_state_dict(LF.weights(m, seed=3), strict=False)
    img, y = LF.inputs(case)
    logits, loss, grads, bufs = levit_ref.levit_loss_and_grads(m, img, y)
    assert _rel(logits, LF.unpack(fx, case + ".logits")) < 1e-3
    assert abs(loss.item() - float(fx[case + ".loss"])) < 1e-5
    if m.training:
        ref = LF.unpack_grads(fx, case)
        assert sorted(ref) == sorted(grads)
        for n, g in grads.items():
            assert _rel(LF.grad_sample(n, g), ref[n]) < 2e-3, n
    ref_buf = LF.unpack_grads(fx, case + ".buf")
    for n, v in ref_buf.items():
        assert _rel(bufs[n].reshape(-1), v) < 2e-3, n

# parameter / state_dict counts of the reference builders (levit.py:560-587) at 1000 classes, seeded
NPARAMS = {"LeViT_128S": 7391290, "LeViT_128": 8828168, "LeViT_192": 10561301, "LeViT_256": 18379852, "LeViT_384": 38358300}
NKEYS = {"LeViT_128S": 329, "LeViT_128": 407, "LeViT_192": 407, "LeViT_256": 407, "LeViT_384": 407}


@pytest.mark.parametrize("name", list(NPARAMS))
def test_builders_parameter_and_key_counts(name):
    torch.manual_seed(0)
    m = getattr(L, name)()
    assert sum(p.numel() for p in m.parameters()) == NPARAMS[name]
    sd = m.state_dict()
    assert len(sd) == NKEYS[name]
    idx = [k for k in sd if k.endswith("attention_bias_idxs")]
    assert idx and all(sd[k].dtype == torch.int64 for k in idx)
    assert all(k.endswith(("running_mean", "running_var", "num_batches_tracked")) for k in sd
               if k not in dict(m.named_parameters()) and not k.endswith("attention_bias_idxs"))
    assert m.no_weight_decay() == {k for k in sd if "attention_biases" in k}


def test_levit_128s_at_100_classes_and_zero_branches():
    torch.manual_seed(0)
    m = L.LeViT_128S(num_classes=100, robust=True)
    assert sum(p.numel() for p in m.parameters()) == 7044790
    # bn_weight_init=0 on every proj and on the second MLP Linear: every residual branch starts at exactly 0
    for blk in m.blocks:
        if isinstance(blk, L.Residual):
            last = blk.m.proj[1] if isinstance(blk.m, L.Attention) else blk.m[2]
            assert torch.equal(last.bn.weight, torch.zeros_like(last.bn.weight))
    # the head's Linear is trunc_normal_(std=.02), seeded: all draws inside +-2 (the reference's truncation bounds)
    w = m.head.l.weight
    assert w.abs().max() <= 2.0 and 0.015 < w.std().item() < 0.025


def test_state_dict_round_trip_between_instances():
    torch.manual_seed(0)
    a = L.LeViT_128S(num_classes=10)
    torch.manual_seed(1)
    b = L.LeViT_128S(num_classes=10)
    b.load_state_dict(a.state_dict(), strict=True)
    assert all(torch.equal(u, v) for u, v in zip(a.state_dict().values(), b.state_dict().values()))


def _ref_offsets(points_q, points_k, stride):
    """The reference's rule, restated (levit.py:235-244 and 338-353: float offsets with size = 1, first appearance)."""
    offsets, idxs = {}, []
    for p1 in points_q:
        for p2 in points_k:
            off = (abs(p1[0] * stride - p2[0] + 0.0), abs(p1[1] * stride - p2[1] + 0.0))
            if off not in offsets:
                offsets[off] = len(offsets)
            idxs.append(offsets[off])
    return idxs, len(offsets)


@pytest.mark.parametrize("rq,rk,s", [(14, 14, 1), (7, 14, 2), (7, 7, 1), (4, 7, 2), (4, 4, 1), (2, 4, 2)])
def test_bias_index_matches_reference_rule(rq, rk, s):
    pq = list(itertools.product(range(rq), range(rq)))
    pk = list(itertools.product(range(rk), range(rk)))
    assert L.attention_offsets(pq, pk, s) == _ref_offsets(pq, pk, s)
    idx, n = L.attention_offsets(pq, pk, s)
    assert n <= 256 and len(idx) == len(pq) * len(pk)


def test_subsample_index_is_the_strided_view():
    B, r, s, C = 3, 7, 2, 5
    x = torch.arange(B * r * r * C, dtype=torch.float32).view(B, r * r, C)
    ref = x.view(B, r, r, C)[:, ::s, ::s].reshape(B, -1, C).reshape(-1, C)
    assert torch.equal(x.reshape(-1, C)[L.subsample_index(B, r, s)], ref)


def test_refused_configurations():
    act = nn.Hardswish
    kw = dict(img_size=224, patch_size=16, embed_dim=[128, 256, 384], key_dim=[16] * 3, depth=[1, 1, 1], num_heads=[4, 6, 8],
              attn_ratio=[2, 2, 2], mlp_ratio=[2, 2, 2], down_ops=[["Subsample", 16, 8, 4, 2, 2], ["Subsample", 16, 16, 4, 2, 2]],
              attention_activation=act, mlp_activation=act, hybrid_backbone=L.b16(128, activation=act))
    L.LeViT(**kw)
    with pytest.raises(NotImplementedError):
        L.LeViT(**{**kw, "attention_activation": nn.GELU})
    with pytest.raises(NotImplementedError):
        L.LeViT(**{**kw, "mlp_activation": nn.ReLU})
    with pytest.raises(NotImplementedError):
        L.LeViT(**{**kw, "hybrid_backbone": nn.Sequential(nn.Conv2d(3, 128, 16, 16))})
    with pytest.raises(NotImplementedError):
        L.LeViT(**{**kw, "down_ops": [["AvgPool", 16, 8, 4, 2, 2], ["Subsample", 16, 16, 4, 2, 2]]})
    with pytest.raises(NotImplementedError):
        L.LeViT(**{**kw, "key_dim": [64] * 3})                       # kd 64
    with pytest.raises(NotImplementedError):
        L.LeViT(**{**kw, "attn_ratio": [3, 2, 2]})                   # value dim 48
    with pytest.raises(NotImplementedError):
        L.LeViT(**{**kw, "img_size": 288})                           # 18 x 18 = 324 keys > 256
    m = L.LeViT(**kw)
    m.blocks[0].m.qkv.bn.momentum = None
    with pytest.raises(NotImplementedError):
        L._bn_check(m.blocks[0].m.qkv.bn)
    from noise_robust_vit_amd._lib import NrvError
    with pytest.raises(NrvError):
        m(torch.randn(1, 3, 224, 224))                                # CPU input
    with pytest.raises(NotImplementedError):
        m.blocks[0](torch.randn(1, 196, 128))


def test_new_entry_points_reject_bad_arguments():
    from noise_robust_vit_amd import _lib
    lib = _lib.load()
    f = ctypes.c_float
    assert lib.nrv_bn_stats(16, 100, 6, f(1e-5), f(0.1), 16, 16, 16, None, None, 16, 1 << 20, None) == -2        # C % 4
    assert lib.nrv_bn_stats(16, 0, 8, f(1e-5), f(0.1), 16, 16, 16, None, None, 16, 1 << 20, None) == -2          # T = 0
    assert lib.nrv_bn_stats(16, 100, 8, f(1e-5), f(1.5), 16, 16, 16, None, None, 16, 1 << 20, None) == -2        # momentum
    assert lib.nrv_bn_stats(16, 100, 8, f(1e-5), f(0.1), 16, 16, 16, 16, None, 16, 1 << 20, None) == -1          # one running buffer
    assert lib.nrv_bn_stats(16, 100, 8, f(1e-5), f(0.1), 16, 16, 16, None, None, 16, 4, None) == -4              # workspace
    assert lib.nrv_bn_apply(16, 16, 16, 0, f(0), 16, 16, 2, None, None, f(1), 1, 16, None, 100, 8, None) == -6    # act
    assert lib.nrv_bn_apply(16, 16, 16, 0, f(0), 16, 16, 0, None, 16, f(1), 3, 16, None, 100, 8, None) == -2      # rows % per
    assert lib.nrv_bn_bwd(16, 7, 0, None, f(1), 1, 16, 16, 16, 0, f(0), 16, 16, 1, 16, 16, 16, 16, 1 << 20, 100, 8, None) == -3
    assert lib.nrv_conv_unfold(16, 0, 0, 16, 1, 3, 8, 8, 3, 2, 3, None) == -2                                     # pad >= ks
    assert lib.nrv_conv_unfold(16, 0, 1, 16, 1, 3, 8, 8, 3, 2, 1, None) == -3                                     # NHWC fp32
    assert lib.nrv_conv_fold(16, 16, 1, 3, 0, 8, 3, 2, 1, None) == -2
    A = (16, 64, 64, 32, 64, 64, 48, 64, 64)          # q, ldq, hq, k, ldk, hk, v, ldv, hv
    ok = (2, 1, 16, 16, 16, 32, 4, 0)                 # B, heads, Nq, Nk, kd, dv, n_offsets, robust
    bad = [(2, 1, 16, 300, 16, 32, 4, 0), (2, 1, 32, 16, 16, 32, 4, 0), (2, 1, 16, 16, 64, 32, 4, 0), (2, 1, 16, 16, 16, 48, 4, 0),
           (2, 1, 16, 16, 16, 32, 300, 0), (2, 1, 16, 16, 16, 32, 4, 2), (2, 1, 200, 200, 16, 32, 4, 0)]
    for b in bad:
        assert lib.nrv_bias_attn_fwd(*A, 16, 16, 16, 16, 16, *b, None) == -2, b
        assert lib.nrv_bias_attn_bwd(*A, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 1 << 20, *b, None) == -2, b
    assert lib.nrv_bias_attn_fwd(*A[:1], 60, *A[2:], 16, 16, 16, 16, 16, *ok, None) == -5                       # ld % 8
    assert lib.nrv_bias_attn_fwd(*A, 16, None, 16, 16, 16, *ok, None) == -1
    assert lib.nrv_bias_attn_stats_size(49, 196, 1) == 5 * 49 + 3 * 196
