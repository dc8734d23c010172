"""lucid_vit.Adapter on the host (no GPU): drop-in module tree against the reference fixture, frozen backbone, the mask
buffer, and the argument checks of the memory / mask attention entry points."""
import ctypes
import os

import numpy as np
import torch

import adapter_fixture as AF

TRAINABLE = {"memory_cls_token", "memories_per_layer", "mlp_head.0.weight", "mlp_head.0.bias", "mlp_head.1.weight", "mlp_head.1.bias"}


def _adapter():
    from noise_robust_vit_amd.lucid_vit import Adapter, ViT
    return Adapter(vit=ViT(**AF.ADAPTER_VIT), num_memories_per_layer=AF.ADAPTER_M, num_classes=AF.ADAPTER_CLASSES)


def _fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "adapter_small.npz"))


def test_adapter_is_exported():
    from noise_robust_vit_amd import lucid_vit
    assert hasattr(lucid_vit, "Adapter")


def test_state_dict_matches_reference(golden_dir):
    fx = _fixture(golden_dir)
    sd = _adapter().state_dict()
    assert list(sd.keys()) == list(fx["a.keys"])
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(fx["a.shape." + k]) for k in fx["a.keys"]}


def test_fixture_weights_rebuild_identically(golden_dir):
    """The seeded weights the GPU parity tests load are the ones the reference ran with."""
    fx = _fixture(golden_dir)
    w = AF.weights(_adapter().state_dict(), seed=0)
    assert sorted(w) == sorted(k[len("a.wsum."):] for k in fx.files if k.startswith("a.wsum."))
    for k, t in w.items():
        assert t.double().sum().item() == float(fx["a.wsum." + k]), k


def test_attn_mask_buffer_matches_reference(golden_dir):
    fx = _fixture(golden_dir)
    ad = _adapter()
    assert ad.attn_mask.dtype == torch.bool
    assert np.array_equal(ad.attn_mask.numpy(), fx["a.attn_mask"])
    S = ad.vit.pos_embedding.shape[-2]
    assert tuple(ad.attn_mask.shape) == (S + 1, S + 1 + 3)


def test_backbone_is_frozen():
    ad = _adapter()
    train = {k for k, p in ad.named_parameters() if p.requires_grad}
    assert train == TRAINABLE
    assert all(not p.requires_grad for p in ad.vit.parameters())


def test_attn_mem_entry_points_check_arguments():
    from noise_robust_vit_amd import _lib
    lib = _lib.load()
    f = ctypes.c_float(0.125)
    # shapes are checked before the (bogus, unaligned) pointers: accepted shapes fail on alignment (-5)
    assert lib.nrv_attn_mem_fwd(1, 1, 0, 3, None, 0, 0, 1, 1, 2, 197, 2, 64, f, None) == -5
    assert lib.nrv_attn_mem_fwd(1, 1, 3, 3, None, 0, 0, 1, 1, 2, 197, 2, 80, f, None) == -5      # per-sample memories
    assert lib.nrv_attn_mem_fwd(1, None, 0, 0, 1, 0, 0, 1, 1, 2, 17, 2, 32, f, None) == -5       # masks only, M = 0
    assert lib.nrv_attn_mem_fwd(1, 1, 0, 3, None, 0, 0, 1, 1, 2, 197, 2, 72, f, None) == -2      # head dim
    assert lib.nrv_attn_mem_fwd(1, 1, 2, 3, None, 0, 0, 1, 1, 2, 197, 2, 64, f, None) == -2      # memory stride not 0 / M
    assert lib.nrv_attn_mem_fwd(1, 1, 0, -1, None, 0, 0, 1, 1, 2, 197, 2, 64, f, None) == -2     # M < 0
    assert lib.nrv_attn_mem_fwd(1, 1, 0, 3, 4, -1, 0, 1, 1, 2, 197, 2, 64, f, None) == -2        # negative mask stride
    assert lib.nrv_attn_mem_fwd(1, 1, 0, 3, None, 0, 0, 1, 1, 0, 197, 2, 64, f, None) == -2      # B = 0
    assert lib.nrv_attn_mem_fwd(1, None, 0, 3, None, 0, 0, 1, 1, 2, 197, 2, 64, f, None) == -1   # memories missing
    assert lib.nrv_attn_mem_fwd(16, 16, 0, 3, 2, 0, 0, 16, 16, 2, 197, 2, 64, f, None) == -5     # mask word unaligned
    bwd = lib.nrv_attn_mem_bwd
    assert bwd(1, 1, 1, 1, 1, 0, 3, None, 0, 0, 1, 1, 1, 1, 2, 197, 2, 64, f, None) == -5
    assert bwd(1, 1, 1, 1, 1, 3, 3, None, 0, 0, 1, 1, 1, 1, 2, 197, 2, 64, f, None) == -2         # batch sum of per-sample memories
    assert bwd(1, 1, 1, 1, 1, 0, 3, None, 0, 0, 1, None, None, 1, 2, 197, 2, 64, f, None) == -1   # dmem missing
    assert bwd(1, 1, 1, 1, 1, 0, 3, None, 0, 0, 1, 1, None, 1, 2, 197, 2, 96, f, None) == -5      # dh 96 accepted
    assert bwd(1, 1, 1, 1, 1, 0, 3, None, 0, 0, 1, 1, None, 1, 2, 197, 2, 48, f, None) == -2
    assert lib.nrv_mask_pack_bits(1, 4, 0, 10, None) == -2
    assert lib.nrv_mask_pack_bits(1, None, 3, 10, None) == -1
    assert lib.nrv_mask_pack_bits(1, 2, 3, 10, None) == -5
