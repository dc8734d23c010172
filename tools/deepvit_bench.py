#!/usr/bin/env python3
"""DeepViT 224 px / patch 16 training-step throughput (fwd + CE + bwd + clip + AdamW through train.Trainer) for a DeepViT-S-like
(dim 384, depth 16, 12 heads of 32, mlp_dim 1152) and a smaller (dim 256, depth 8, 8 heads of 32, mlp_dim 768) model, softmax
and robust, eager and captured (Trainer.capture); for comparison the fp32 restatement tests/deepvit_ref.py run eagerly under
bf16 autocast on the same GPU (forward + backward + torch AdamW).  Every configuration -- and the restatement of every
configuration -- runs in a child process of its own under a time limit, and the run stops at the first one that fails.  Prints
one JSON line per measurement.

    python tools/deepvit_bench.py [--models s small] [--batches 64 256] [--steps 10] [--warmup 3] [--no-eager] [--no-capture] [--limit 300]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MODELS = {
    "s": dict(dim=384, depth=16, heads=12, dim_head=32, mlp_dim=1152),
    "small": dict(dim=256, depth=8, heads=8, dim_head=32, mlp_dim=768),
}


def _time(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def _setup(name, B, robust):
    import torch
    from noise_robust_vit_amd.deepvit import DeepViT
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x = torch.randn(B, 3, 224, 224, device=dev)
    y = torch.randint(0, 100, (B,), device=dev)
    torch.manual_seed(0)
    m = DeepViT(image_size=224, patch_size=16, num_classes=100, robust=robust, **MODELS[name]).to(dev).train()
    return m, x, y, {"model": name, "batch": B, "robust": robust}


def hip(name, B, robust, steps, warmup, captured):
    from noise_robust_vit_amd.train import Trainer, TrainConfig
    m, x, y, tag = _setup(name, B, robust)
    tr = Trainer(m, TrainConfig(lr=1e-3, grad_max_norm=5.0))
    if captured:
        tr.capture(x, y)
    dt = _time(lambda: tr.step(x, y), steps, warmup)
    print(json.dumps(dict(tag, captured=captured, hip_step_ms=round(dt * 1e3, 2), hip_img_per_s=round(B / dt, 1))), flush=True)


def ref(name, B, robust, steps):
    import torch
    import deepvit_ref
    m, x, y, tag = _setup(name, B, robust)
    P = {n: p.detach().clone().float().requires_grad_(True) for n, p in m.named_parameters()}
    params = list(P.values())
    opt = torch.optim.AdamW(params, lr=1e-3)

    def eager():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = deepvit_ref.forward(m, P, x)
            loss = torch.nn.functional.cross_entropy(logits.float(), y)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 5.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
    rec = dict(tag, restatement="fp32 under bf16 autocast, eager")
    try:
        de = _time(eager, max(2, steps // 2), 1)
        rec.update(eager_step_ms=round(de * 1e3, 2), eager_img_per_s=round(B / de, 1))
    except torch.cuda.OutOfMemoryError:
        rec.update(eager_step_ms=None, eager_note="out of memory")
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=list(MODELS), choices=list(MODELS))
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true", help="skip the autocast restatement")
    ap.add_argument("--no-capture", action="store_true", help="eager steps only (profiler runs)")
    ap.add_argument("--limit", type=int, default=300, help="seconds per child process")
    ap.add_argument("--one", nargs=4, metavar=("MODEL", "BATCH", "ROBUST", "KIND"),
                    help="run one measurement in this process; KIND = eager | captured | ref")
    a = ap.parse_args()
    if a.one:
        name, B, robust, kind = a.one[0], int(a.one[1]), a.one[2] == "1", a.one[3]
        if kind == "ref":
            ref(name, B, robust, a.steps)
        else:
            hip(name, B, robust, a.steps, a.warmup, kind == "captured")
        return 0
    kinds = ["eager"] + ([] if a.no_capture else ["captured"]) + ([] if a.no_eager else ["ref"])
    for name in a.models:
        for B in a.batches:
            for robust in (False, True):
                for kind in kinds:
                    cmd = [sys.executable, os.path.abspath(__file__), "--one", name, str(B), "1" if robust else "0", kind,
                           "--steps", str(a.steps), "--warmup", str(a.warmup)]
                    try:
                        rc = subprocess.run(cmd, timeout=a.limit).returncode
                    except subprocess.TimeoutExpired:
                        rc = 124
                    if rc != 0:
                        print(json.dumps({"model": name, "batch": B, "robust": robust, "kind": kind, "failed": rc}), flush=True)
                        return rc                   # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
