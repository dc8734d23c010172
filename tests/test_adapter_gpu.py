"""lucid_vit.Adapter and Transformer(x, attn_mask, memories) on the HIP path: parity with the reference's fixture
(tests/golden/gen_golden_adapter.py), the frozen backbone (no gradients, no weight-gradient launches), mask isolation and a
ViT-B/16-shaped Adapter against an fp32 restatement."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import adapter_fixture as AF

pytestmark = pytest.mark.gpu

TRAINABLE = {"memory_cls_token", "memories_per_layer", "mlp_head.0.weight", "mlp_head.0.bias", "mlp_head.1.weight", "mlp_head.1.bias"}


def _fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "adapter_small.npz"))


def _rel_l2(a, b):
    a, b = a.detach().float().cpu(), torch.as_tensor(b).detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _rel_max(a, b):
    a, b = a.detach().float().cpu(), torch.as_tensor(b).detach().float().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


def _small_adapter(fixture_weights=False):
    from noise_robust_vit_amd.lucid_vit import Adapter, ViT
    ad = Adapter(vit=ViT(**AF.ADAPTER_VIT), num_memories_per_layer=AF.ADAPTER_M, num_classes=AF.ADAPTER_CLASSES)
    if fixture_weights:
        missing, unexpected = ad.load_state_dict(AF.weights(ad.state_dict(), seed=0), strict=False)
        assert missing == ["attn_mask"] and not unexpected      # the bool buffer is the module's own
    return ad


def test_adapter_matches_fixture(dev, golden_dir):
    fx = _fixture(golden_dir)
    ad = _small_adapter(True).to(dev)
    img, y = AF.adapter_inputs()
    logits = ad(img.to(dev))
    loss = F.cross_entropy(logits, y.to(dev))
    loss.backward()
    assert _rel_max(logits, AF.unpack(fx, "a.logits")) <= 6e-3
    assert abs(loss.item() - float(fx["a.loss"])) < 2e-3
    for k, p in ad.named_parameters():
        if p.requires_grad:
            ref = AF.unpack(fx, "a.g." + k)
            assert _rel_l2(p.grad, ref) <= 1e-2, (k, _rel_l2(p.grad, ref))


def test_transformer_masks_and_memories_match_fixture(dev, golden_dir):
    from noise_robust_vit_amd.lucid_vit import Transformer
    fx = _fixture(golden_dir)
    tr = Transformer(*AF.TR_ARGS)
    tr.load_state_dict(AF.weights(tr.state_dict(), seed=1))
    tr = tr.to(dev)
    x, mems, mask, dy = AF.transformer_inputs()
    x = x.to(dev).requires_grad_(True)
    mems = mems.to(dev).requires_grad_(True)
    y = tr(x, attn_mask=mask.to(dev), memories=mems)
    (y * dy.to(dev)).sum().backward()
    assert _rel_max(y, AF.unpack(fx, "t.y")) <= 6e-3
    assert _rel_l2(x.grad, AF.unpack(fx, "t.gx")) <= 1e-2
    assert _rel_l2(mems.grad, AF.unpack(fx, "t.gmems")) <= 1e-2
    for k, p in tr.named_parameters():
        ref = AF.unpack(fx, "t.g." + k)
        assert _rel_l2(p.grad, ref) <= 1e-2, (k, _rel_l2(p.grad, ref))


def test_frozen_backbone_issues_no_weight_gradients(dev, monkeypatch):
    from noise_robust_vit_amd import kernels
    ad = _small_adapter(True).to(dev)
    img, y = AF.adapter_inputs()
    calls = []
    for name in ("gemm_tn", "gemm_tn_grouped"):
        orig = getattr(kernels, name)
        monkeypatch.setattr(kernels, name, lambda *a, _o=orig, _n=name, **kw: (calls.append(_n), _o(*a, **kw))[1])
    logits = ad(img.to(dev))
    F.cross_entropy(logits, y.to(dev)).backward()
    assert calls == []
    for k, p in ad.named_parameters():
        if k.startswith("vit."):
            assert p.grad is None, k
        else:
            assert k in TRAINABLE and p.grad is not None, k


def test_adapter_mask_isolates_backbone_tokens(dev):
    torch.manual_seed(3)
    ad = _small_adapter().to(dev).eval()
    img = torch.randn(3, 3, 64, 64, device=dev)
    with torch.no_grad():
        tokens = ad.vit.img_to_tokens(img)
        outs = []
        for seed in (0, 1):
            g = torch.Generator().manual_seed(seed)
            cls = torch.randn(128, generator=g).to(dev)
            mems = torch.randn(2, 3, 128, generator=g).to(dev)
            t = torch.cat((cls.reshape(1, 1, -1).expand(3, 1, -1), tokens), dim=1)
            outs.append(ad.vit.transformer(t, memories=mems, attn_mask=ad.attn_mask))
    assert not torch.equal(outs[0][:, 0], outs[1][:, 0])
    assert torch.equal(outs[0][:, 1:], outs[1][:, 1:])


def _ref_adapter_logits(ad, img, cls, mems):
    """fp32 restatement of learnable_memory_vit.py:30-205 on the same weights."""
    vit = ad.vit
    b, c, hh, ww = img.shape
    p = vit.patch
    x = img.reshape(b, c, hh // p, p, ww // p, p).permute(0, 2, 4, 3, 5, 1).reshape(b, (hh // p) * (ww // p), p * p * c)
    lin = vit.to_patch_embedding[1]
    x = x @ lin.weight.T + lin.bias
    x = torch.cat((vit.cls_token.expand(b, -1, -1), x), dim=1) + vit.pos_embedding
    x = torch.cat((cls.reshape(1, 1, -1).expand(b, 1, -1), x), dim=1)
    mask = ad.attn_mask
    for i, (attn, ff) in enumerate(vit.transformer.layers):
        xn = F.layer_norm(x, (x.shape[-1],), attn.norm.weight, attn.norm.bias, attn.norm.eps)
        kv_in = torch.cat((xn, mems[i].expand(b, -1, -1)), dim=1)
        h = attn.heads
        q = (xn @ attn.to_q.weight.T).reshape(b, xn.shape[1], h, -1).transpose(1, 2)
        k, v = (kv_in @ attn.to_kv.weight.T).chunk(2, dim=-1)
        k = k.reshape(b, kv_in.shape[1], h, -1).transpose(1, 2)
        v = v.reshape(b, kv_in.shape[1], h, -1).transpose(1, 2)
        s = (q @ k.transpose(-1, -2)) * attn.scale
        s = s.masked_fill(~mask, -torch.finfo(s.dtype).max)
        o = (s.softmax(-1) @ v).transpose(1, 2).reshape(b, xn.shape[1], -1)
        x = o @ attn.to_out[0].weight.T + attn.to_out[0].bias + x
        n = ff.net
        y = F.layer_norm(x, (x.shape[-1],), n[0].weight, n[0].bias, n[0].eps)
        y = F.gelu(y @ n[1].weight.T + n[1].bias)
        x = y @ n[4].weight.T + n[4].bias + x
    hd = ad.mlp_head
    return F.layer_norm(x[:, 0], (x.shape[-1],), hd[0].weight, hd[0].bias, hd[0].eps) @ hd[1].weight.T + hd[1].bias


def test_adapter_vit_b16_against_fp32(dev):
    from noise_robust_vit_amd.lucid_vit import Adapter, ViT
    torch.manual_seed(5)
    vit = ViT(image_size=224, patch_size=16, num_classes=1000, dim=768, depth=12, heads=12, mlp_dim=3072)
    with torch.no_grad():                       # keep the residual stream at a trained network's scale
        vit.pos_embedding.mul_(0.02)
        vit.cls_token.mul_(0.02)
    ad = Adapter(vit=vit, num_memories_per_layer=10, num_classes=100)
    with torch.no_grad():
        ad.memory_cls_token.mul_(0.02)
        ad.memories_per_layer.mul_(0.02)
    ad = ad.to(dev)
    img = torch.randn(4, 3, 224, 224, device=dev)
    y = torch.randint(0, 100, (4,), device=dev)
    logits = ad(img)
    F.cross_entropy(logits, y).backward()
    cls = ad.memory_cls_token.detach().clone().requires_grad_(True)
    mems = ad.memories_per_layer.detach().clone().requires_grad_(True)
    ref = _ref_adapter_logits(ad, img, cls, mems)
    F.cross_entropy(ref, y).backward()
    assert _rel_max(logits, ref) <= 6e-3 * 2, _rel_max(logits, ref)
    assert _rel_l2(ad.memory_cls_token.grad, cls.grad) <= 2e-2, _rel_l2(ad.memory_cls_token.grad, cls.grad)
    assert _rel_l2(ad.memories_per_layer.grad, mems.grad) <= 2e-2, _rel_l2(ad.memories_per_layer.grad, mems.grad)
