#!/usr/bin/env python3
"""Golden fixture for the learnable-memory Adapter, produced by running the reference's learnable_memory_vit.py itself on CPU
(development container only; the module is loaded through a stub package, as gen_golden_mae.py does).

Weights and inputs are rebuilt from seeds by tests/adapter_fixture.py on both sides, so only what the reference computes is
stored (float16 relative to max-abs), with the module tree (state_dict keys and shapes), the Adapter's attn_mask and the
sums of the weights (a guard that both sides rebuilt the same tensors).  Two cases, written to adapter_small.npz:
  a.*  Adapter(ViT(image_size=64, patch_size=16, dim=128, depth=2, heads=2, dim_head=64, mlp_dim=256), M=3, num_classes=5),
       batch 4: logits, CE loss, gradients of the six trainable parameters.
  t.*  a bare Transformer(dim=64, depth=2, heads=2, dim_head=32, mlp_dim=128) called with a random bool attn_mask
       [Nq, Nq + M] (one query row fully masked) and per-sample memories [depth, B, M, dim], all weights trainable: the
       output and every gradient.
"""
import importlib, os, sys, types
import numpy as np
import torch

REF = "/root/reference/vit_pytorch_robust"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import adapter_fixture as AF  # noqa: E402

pkg = types.ModuleType("vit_pytorch_robust"); pkg.__path__ = [REF]
sys.modules["vit_pytorch_robust"] = pkg
lm = importlib.import_module("vit_pytorch_robust.learnable_memory_vit")

out = {"meta": np.array("reference learnable_memory_vit.py (ViT + Adapter; Transformer with attn_mask and memories), CPU fp32; "
                        "weights / inputs from tests/adapter_fixture.py")}

# --- Adapter case
vit = lm.ViT(**AF.ADAPTER_VIT)
ad = lm.Adapter(vit=vit, num_memories_per_layer=AF.ADAPTER_M, num_classes=AF.ADAPTER_CLASSES)
w = AF.weights(ad.state_dict(), seed=0)
ad.load_state_dict(w, strict=False)
img, y = AF.adapter_inputs()
logits = ad(img)
loss = torch.nn.functional.cross_entropy(logits, y)
loss.backward()
AF.pack(out, "a.logits", logits)
out["a.loss"] = loss.detach().numpy()
out["a.keys"] = np.array(list(ad.state_dict().keys()))
for k, v in ad.state_dict().items():
    out["a.shape." + k] = np.array(v.shape, dtype=np.int64)
    if k in w:
        out["a.wsum." + k] = np.float64(w[k].double().sum())
out["a.attn_mask"] = ad.attn_mask.numpy()
for k, p in ad.named_parameters():
    if p.requires_grad:
        AF.pack(out, "a.g." + k, p.grad)

# --- masks-and-memories case
tr = lm.Transformer(*AF.TR_ARGS)
tr.load_state_dict(AF.weights(tr.state_dict(), seed=1))
x, mems, mask, dy = AF.transformer_inputs()
x.requires_grad_(True)
mems.requires_grad_(True)
yo = tr(x, attn_mask=mask, memories=mems)
(yo * dy).sum().backward()
AF.pack(out, "t.y", yo)
AF.pack(out, "t.gx", x.grad)
AF.pack(out, "t.gmems", mems.grad)
for k, p in tr.named_parameters():
    AF.pack(out, "t.g." + k, p.grad)

np.savez_compressed(os.path.join(OUT, "adapter_small.npz"), **out)
print("adapter_small.npz", os.path.getsize(os.path.join(OUT, "adapter_small.npz")), "loss", loss.item())
