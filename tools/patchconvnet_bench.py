#!/usr/bin/env python3
"""PatchConvNet S60 224 px training-step throughput (fwd + CE + bwd + clip + AdamW through train.Trainer) at the given batch
sizes, eager and captured (Trainer.capture); for comparison the fp32 restatement tests/patchconvnet_ref.py run eagerly under
bf16 autocast on the same GPU (forward + backward + torch AdamW).  Prints one JSON line per configuration.

    python tools/patchconvnet_bench.py [--batches 64 256] [--steps 10] [--warmup 3] [--no-eager]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    from noise_robust_vit_amd import patch_convnet
    from noise_robust_vit_amd.train import Trainer, TrainConfig
    import patchconvnet_ref
    dev = torch.device("cuda:0")
    for B in a.batches:
        torch.manual_seed(0)
        x = torch.randn(B, 3, 224, 224, device=dev)
        y = torch.randint(0, 100, (B,), device=dev)
        for captured in (False, True):
            torch.manual_seed(0)
            m = patch_convnet.S60(num_classes=100).to(dev).train()
            tr = Trainer(m, TrainConfig(lr=1e-3, grad_max_norm=5.0))
            if captured:
                tr.capture(x, y)
            dt = _time(lambda: tr.step(x, y), a.steps, a.warmup)
            print(json.dumps({"model": "S60", "batch": B, "captured": captured, "hip_step_ms": round(dt * 1e3, 2),
                              "hip_img_per_s": round(B / dt, 1)}), flush=True)
            if captured or a.no_eager:
                del m, tr
                torch.cuda.empty_cache()
                continue
            P = {n: p.detach().clone().float().requires_grad_(True) for n, p in m.named_parameters()}
            params = list(P.values())
            opt = torch.optim.AdamW(params, lr=1e-3)

            def eager():
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    logits = patchconvnet_ref.forward(m, P, x)
                    loss = torch.nn.functional.cross_entropy(logits.float(), y)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(params, 5.0)
                opt.step()
                opt.zero_grad(set_to_none=True)
            rec = {"model": "S60", "batch": B, "restatement": "fp32 under bf16 autocast, eager"}
            try:
                de = _time(eager, max(2, a.steps // 2), 1)
                rec.update(eager_step_ms=round(de * 1e3, 2), eager_img_per_s=round(B / de, 1))
            except torch.cuda.OutOfMemoryError:
                rec.update(eager_step_ms=None, eager_note="out of memory")
            print(json.dumps(rec), flush=True)
            del P, params, opt, m, tr
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
