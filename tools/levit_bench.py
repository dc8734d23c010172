#!/usr/bin/env python3
"""LeViT_128S 224 px training-step throughput (fwd + CE + bwd + clip + AdamW through train.Trainer), softmax and robust, at the
given batch sizes; for comparison the fp32 restatement tests/levit_ref.py run eagerly under bf16 autocast on the same GPU
(forward + backward + torch AdamW).  Prints one JSON line per configuration.

    python tools/levit_bench.py [--batches 64 256] [--steps 10] [--warmup 3] [--no-eager]
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
    ap.add_argument("--robust", choices=["both", "0", "1"], default="both")
    a = ap.parse_args()
    from noise_robust_vit_amd import levit
    from noise_robust_vit_amd.train import Trainer, TrainConfig
    import levit_ref
    dev = torch.device("cuda:0")
    for robust in {"both": (False, True), "0": (False,), "1": (True,)}[a.robust]:
        for B in a.batches:
            torch.manual_seed(0)
            m = levit.LeViT_128S(num_classes=1000, robust=robust).to(dev).train()
            x = torch.randn(B, 3, 224, 224, device=dev)
            y = torch.randint(0, 1000, (B,), device=dev)
            tr = Trainer(m, TrainConfig(lr=1e-3, grad_max_norm=5.0))
            dt = _time(lambda: tr.step(x, y), a.steps, a.warmup)
            rec = {"model": "LeViT_128S", "robust": robust, "batch": B, "hip_step_ms": round(dt * 1e3, 2),
                   "hip_img_per_s": round(B / dt, 1)}
            if not a.no_eager:
                P = {n: p.detach().clone().float().requires_grad_(True) for n, p in m.named_parameters()}
                Bf = {n: b.detach().clone() for n, b in m.named_buffers()}
                params = list(P.values())
                opt = torch.optim.AdamW(params, lr=1e-3)

                def eager():
                    with torch.autocast("cuda", dtype=torch.bfloat16):
                        logits = levit_ref.levit_forward(m, P, Bf, x)
                        loss = torch.nn.functional.cross_entropy(logits.float(), y)
                    loss.backward()
                    torch.nn.utils.clip_grad_norm_(params, 5.0)
                    opt.step()
                    opt.zero_grad(set_to_none=True)
                try:
                    de = _time(eager, max(2, a.steps // 2), 1)
                    rec.update(eager_step_ms=round(de * 1e3, 2), eager_img_per_s=round(B / de, 1))
                except torch.cuda.OutOfMemoryError:
                    rec.update(eager_step_ms=None, eager_note="out of memory")
                del P, Bf, params, opt
            print(json.dumps(rec), flush=True)
            del m, tr
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
