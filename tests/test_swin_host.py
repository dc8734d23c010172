"""CPU: the Swin modules against the reference fixture (module tree, seeded init, index builders, refusals), the fp32
restatement tests/swin_ref.py against the reference's outputs and gradients, and the host-side argument checks of the new
C entry points (no GPU)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import swin_fixture as SF
import swin_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swin_small.npz")


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLD)


def _model(case):
    from noise_robust_vit_amd.swin import SwinTransformer
    return SwinTransformer(**SF.model_kwargs(case))


@pytest.mark.parametrize("case", list(SF.CASES))
def test_module_tree_and_keys(fx, case):
    m = _model(case)
    sd = m.state_dict()
    tree = SF.unpack_tree(fx, case)
    assert list(sd.keys()) == list(tree)
    assert len(sd) == 67
    for k, v in sd.items():
        assert tuple(v.shape) == tree[k][0], k
    w = SF.weights(sd, seed=3)
    m.load_state_dict(w, strict=False)
    for k, v in w.items():
        assert float(v.double().sum()) == pytest.approx(tree[k][1], rel=1e-12, abs=1e-12), k


def test_swin_t_seeded_init_matches_reference(fx):
    from noise_robust_vit_amd import swin_t
    torch.manual_seed(0)
    m = swin_t()
    sd = m.state_dict()
    tree = SF.unpack_tree(fx, "swin_t")
    assert list(sd.keys()) == list(tree)
    assert sum(p.numel() for p in m.parameters()) == int(fx["swin_t.nparams"]) == SF.SWIN_T_PARAMS
    for k, v in sd.items():
        assert tuple(v.shape) == tree[k][0], k
        assert float(v.double().sum()) == pytest.approx(tree[k][1], rel=1e-9, abs=1e-9), k


def test_reference_checkpoint_loads(fx):
    """A reference state_dict (same keys, the integer index buffer included) loads strictly."""
    from noise_robust_vit_amd.swin import SwinTransformer
    m = _model("s56")
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m2 = SwinTransformer(**SF.model_kwargs("s56"))
    m2.load_state_dict(sd, strict=True)


def test_relative_position_index_matches_reference_rule():
    from noise_robust_vit_amd.swin import ShiftedWindowAttention
    for ws in ([7, 7], [8, 8], [4, 6]):
        a = ShiftedWindowAttention(32, ws, [0, 0], 1)
        Wh, Ww = ws
        coords = torch.stack(torch.meshgrid(torch.arange(Wh), torch.arange(Ww), indexing="ij")).flatten(1)
        rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0)
        idx = (rel[..., 0] + Wh - 1) * (2 * Ww - 1) + rel[..., 1] + Ww - 1
        assert torch.equal(a.relative_position_index, idx.flatten())


@pytest.mark.parametrize("H,W", [(14, 14), (7, 9), (5, 4), (1, 3)])
def test_merge_index_matches_reference_slicing(H, W):
    from noise_robust_vit_amd.swin import merge_index
    B, C = 2, 3
    x = torch.randn(B, H, W, C)
    xp = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    ref = torch.cat([xp[:, 0::2, 0::2], xp[:, 1::2, 0::2], xp[:, 0::2, 1::2], xp[:, 1::2, 1::2]], -1)
    idx = merge_index(B, H, W)
    flat = x.reshape(B * H * W, C)
    got = torch.where(idx[:, None] >= 0, flat[idx.clamp(min=0)], torch.zeros(1, C)).reshape(ref.shape)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("H,W", [(16, 16), (14, 14), (7, 10)])
def test_pad_and_real_index_match_reference_padding(H, W):
    from noise_robust_vit_amd.swin import pad_index, real_index, window_geometry
    B, C = 2, 4
    pH, pW, _, _ = window_geometry(H, W, [7, 7], [3, 3])
    x = torch.randn(B, H, W, C)
    ref = F.pad(x, (0, 0, 0, pW - W, 0, pH - H))
    pi = pad_index(B, H, W, pH, pW)
    flat = x.reshape(-1, C)
    got = torch.where(pi[:, None] >= 0, flat[pi.clamp(min=0)], torch.zeros(1, C)).reshape(ref.shape)
    assert torch.equal(got, ref)
    ri = real_index(B, H, W, pH, pW)
    assert torch.equal(ref.reshape(-1, C)[ri], flat)


def test_shift_rule():
    from noise_robust_vit_amd.swin import window_geometry
    assert window_geometry(7, 7, [7, 7], [3, 3]) == (7, 7, 0, 0)          # swin_t's last stage at 224 px: unshifted
    assert window_geometry(7, 14, [7, 7], [3, 3]) == (7, 14, 0, 3)
    assert window_geometry(16, 16, [7, 7], [3, 3]) == (21, 21, 3, 3)


def test_refused_configurations():
    from noise_robust_vit_amd import swin
    with pytest.raises(NotImplementedError):
        swin.swin_v2_t()
    m = swin.SwinTransformer(**dict(SF.MODEL, dropout=0.1))
    with pytest.raises(NotImplementedError, match="eval"):
        m.features[1][0]._check()
    m = swin.SwinTransformer(**dict(SF.MODEL, attention_dropout=0.1))
    with pytest.raises(NotImplementedError):
        m.features[1][0]._check()
    from noise_robust_vit_amd.encoder import record_attention
    m = swin.SwinTransformer(**SF.MODEL)
    with record_attention([]):
        with pytest.raises(NotImplementedError, match="recording"):
            m.features[1][0]._check()
    with pytest.raises(NotImplementedError):
        swin.SwinTransformer(**dict(SF.MODEL, block=torch.nn.Identity))
    with pytest.raises(NotImplementedError):
        m.features[1][0].attn(torch.zeros(1, 7, 7, 32))


def test_cpu_input_is_refused():
    from noise_robust_vit_amd.swin import SwinTransformer
    from noise_robust_vit_amd._lib import NrvError
    m = SwinTransformer(**SF.MODEL)
    with pytest.raises(NrvError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 56, 56))


@pytest.mark.parametrize("case", list(SF.CASES))
def test_restatement_reproduces_reference(fx, case):
    m = _model(case)
    sd = dict(m.state_dict())
    sd.update(SF.weights(sd, seed=3))
    img, y = SF.inputs(case)
    logits, loss, grads = swin_ref.loss_and_grads(sd, SF.model_kwargs(case), img, y)
    ref = SF.unpack(fx, case + ".logits")
    assert (logits - ref).abs().max() <= 2e-3 * ref.abs().max()
    assert abs(loss.item() - float(fx[case + ".loss"])) < 1e-4
    ref_grads = SF.unpack_grads(fx, case)
    assert sorted(ref_grads) == sorted(grads)
    for name, r in ref_grads.items():
        g = SF.grad_sample(name, grads[name])
        err = ((g - r).norm() / r.norm().clamp(min=1e-30)).item()
        assert err < 2e-3, (name, err)


def test_window_attn_entry_points_reject_bad_arguments():
    from noise_robust_vit_amd import _lib
    lib = _lib.load()
    f = lib.nrv_window_attn_fwd
    ok = dict(B=1, pH=14, pW=14, C=64, heads=2, Wh=7, Ww=7, sh=3, sw=3)

    def call(**kw):
        a = dict(ok, **kw)
        return f(24, 16, 16, 16, a["B"], a["pH"], a["pW"], a["C"], a["heads"], a["Wh"], a["Ww"], a["sh"], a["sw"], 0, None)

    assert call() == -5                         # valid shape; the unaligned qkv pointer fails the alignment check
    assert call(C=96, heads=2) == -2            # dh 48
    assert call(C=128, heads=1) == -2           # dh 128
    assert call(Wh=9, Ww=8, pH=18, pW=16) == -2 # 72 slots
    assert call(pH=15) == -2                    # not a multiple of the window
    assert call(sh=7) == -2                     # shift >= window
    assert call(sw=-1) == -2
    assert f(None, 16, 16, 16, 1, 14, 14, 64, 2, 7, 7, 0, 0, 0, None) == -1
    assert lib.nrv_window_attn_bwd(16, 16, 16, 16, 16, 16, 16, 0, 1, 14, 14, 64, 2, 7, 7, 0, 0, 0, None) == -4   # workspace
    assert lib.nrv_window_attn_bwd_workspace(2, 14, 14, 64, 2, 7, 7) == 1 * 2 * 169 * 4     # 8 windows -> one chunk
    assert lib.nrv_window_attn_bwd_workspace(2, 14, 14, 48, 1, 7, 7) == 0
    assert lib.nrv_sd_add_f32(16, 16, 16, 16, ctypes.c_float(0.8), 10, 3, 8, None) == -2      # rows % rows_per_sample
    assert lib.nrv_sd_add_f32(16, 16, 16, 16, ctypes.c_float(0.0), 10, 5, 8, None) == -2      # survival 0
    assert lib.nrv_sd_scale_bf16(16, 16, 16, ctypes.c_float(0.8), 10, 5, 6, None) == -2       # dim % 4
    assert lib.nrv_sd_scale_bf16(None, 16, 16, ctypes.c_float(0.8), 10, 5, 8, None) == -1
