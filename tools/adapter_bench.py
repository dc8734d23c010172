#!/usr/bin/env python3
"""Adapter step against the full training step of the same ViT-B/16-shaped lucid ViT (one process, alternating).

    python tools/adapter_bench.py [--batch 256] [--steps 20] [--warmup 5] [--memories 10]

Adapter step: forward + CE + backward + AdamW on the six trainable tensors (memory CLS token, memories, head), frozen
backbone.  Full step: forward + CE + backward + AdamW on every parameter of the plain ViT.  Both use torch.optim.AdamW
(foreach), so the optimizer is priced alike; prints one JSON line with the median ms of each and their ratio."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from noise_robust_vit_amd.lucid_vit import Adapter, ViT  # noqa: E402


def vit_b16():
    return ViT(image_size=224, patch_size=16, num_classes=1000, dim=768, depth=12, heads=12, mlp_dim=3072)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--memories", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    full = vit_b16().to(dev).train()
    ad = Adapter(vit=vit_b16(), num_memories_per_layer=a.memories, num_classes=1000).to(dev).train()
    opt_full = torch.optim.AdamW(full.parameters(), lr=1e-4, foreach=True)
    opt_ad = torch.optim.AdamW([p for p in ad.parameters() if p.requires_grad], lr=1e-4, foreach=True)
    img = torch.randn(a.batch, 3, 224, 224, device=dev)
    y = torch.randint(0, 1000, (a.batch,), device=dev)

    def step(model, opt):
        opt.zero_grad(set_to_none=True)
        F.cross_entropy(model(img), y).backward()
        opt.step()

    times = {"adapter": [], "full": []}
    for i in range(a.warmup + a.steps):
        for name, model, opt in (("adapter", ad, opt_ad), ("full", full, opt_full)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            step(model, opt)
            e.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times[name].append(s.elapsed_time(e))
    ma, mf = statistics.median(times["adapter"]), statistics.median(times["full"])
    print(json.dumps({"batch": a.batch, "memories": a.memories, "adapter_ms": round(ma, 3), "full_ms": round(mf, 3),
                      "adapter_over_full": round(ma / mf, 3), "adapter_img_s": round(a.batch / ma * 1e3, 1),
                      "full_img_s": round(a.batch / mf * 1e3, 1)}))


if __name__ == "__main__":
    main()
