#!/usr/bin/env python3
"""PiT 224 px / patch 14 training-step throughput (fwd + CE + bwd + clip + AdamW through train.Trainer) for a PiT-S-like (dim 144,
depth (2, 6, 4), heads (3, 6, 12), dim_head 64, mlp_dim 576) and a smaller (dim 64, depth (2, 4, 2), heads (2, 4, 8), dim_head 32,
mlp_dim 256) model, softmax and robust, eager and captured (Trainer.capture); for comparison, at one batch size, the fp32
restatement tests/pit_ref.py run
eagerly under bf16 autocast on the same GPU (forward + backward + clip + torch AdamW) in a process of its own that launches no
HIP kernel of the library.  Every configuration runs in a child process of its own under a time limit, and the run stops at the
first one that fails.  Prints one JSON line per measurement.

    python tools/pit_bench.py [--models s small] [--batches 64 256] [--steps 10] [--warmup 3] [--no-eager] [--eager-batch 64] [--chunk 64] [--no-capture] [--limit 300]
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
    "s": dict(dim=144, depth=(2, 6, 4), heads=(3, 6, 12), dim_head=64, mlp_dim=576),
    "small": dict(dim=64, depth=(2, 4, 2), heads=(2, 4, 8), dim_head=32, mlp_dim=256),
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


def one(name, B, robust, steps, warmup, no_capture=False):
    """The HIP legs of one configuration: Trainer.step eager, then captured.  A batch that does not fit is reported, not an error."""
    import torch
    from noise_robust_vit_amd.pit import PiT
    from noise_robust_vit_amd.train import Trainer, TrainConfig
    dev = torch.device("cuda:0")
    tag = {"model": name, "batch": B, "robust": robust}
    try:
        torch.manual_seed(0)
        x = torch.randn(B, 3, 224, 224, device=dev)
        y = torch.randint(0, 100, (B,), device=dev)
        for captured in ((False,) if no_capture else (False, True)):
            torch.manual_seed(0)
            m = PiT(image_size=224, patch_size=14, num_classes=100, robust=robust, **MODELS[name]).to(dev).train()
            tr = Trainer(m, TrainConfig(lr=1e-3, grad_max_norm=5.0))
            if captured:
                tr.capture(x, y)
            dt = _time(lambda: tr.step(x, y), steps, warmup)
            print(json.dumps(dict(tag, captured=captured, hip_step_ms=round(dt * 1e3, 2), hip_img_per_s=round(B / dt, 1),
                                  peak_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1))), flush=True)
            del m, tr
            torch.cuda.empty_cache()
    except torch.cuda.OutOfMemoryError:
        print(json.dumps(dict(tag, fits=False, note="out of memory")), flush=True)


def restatement(name, B, robust, steps, chunk):
    """tests/pit_ref.py, fp32 masters under bf16 autocast, forward + backward + clip + torch AdamW, in a process that launches no
    kernel of libnrv_hip.so (the model object is walked for its structure only).  The batch goes through in chunks of `chunk`
    images whose gradients accumulate (loss weighted chunk / B: the same step as one pass over the batch)."""
    import torch
    from noise_robust_vit_amd import _lib
    from noise_robust_vit_amd.pit import PiT
    import pit_ref
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x = torch.randn(B, 3, 224, 224, device=dev)
    y = torch.randint(0, 100, (B,), device=dev)
    m = PiT(image_size=224, patch_size=14, num_classes=100, robust=robust, **MODELS[name]).train()
    P = {n: p.detach().to(dev, torch.float32).requires_grad_(True) for n, p in m.named_parameters()}
    params = list(P.values())
    opt = torch.optim.AdamW(params, lr=1e-3)

    def step():
        for i in range(0, B, chunk):
            xs, ys = x[i:i + chunk], y[i:i + chunk]
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits = pit_ref.forward(m, P, xs)
            (torch.nn.functional.cross_entropy(logits.float(), ys) * (xs.shape[0] / B)).backward()
        torch.nn.utils.clip_grad_norm_(params, 5.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
    de = _time(step, max(2, steps // 2), 1)
    assert _lib._lib is None, "the restatement's process must not load libnrv_hip.so"
    print(json.dumps({"model": name, "batch": B, "robust": robust, "restatement": f"fp32 under bf16 autocast, eager, chunks of {chunk}",
                      "eager_step_ms": round(de * 1e3, 2), "eager_img_per_s": round(B / de, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=list(MODELS), choices=list(MODELS))
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true", help="skip the torch restatement")
    ap.add_argument("--eager-batch", type=int, default=64, help="the restatement is timed at this batch only")
    ap.add_argument("--chunk", type=int, default=64, help="images per pass of the restatement")
    ap.add_argument("--one-eager", nargs=3, metavar=("MODEL", "BATCH", "ROBUST"), help="run one restatement in this process")
    ap.add_argument("--no-capture", action="store_true", help="eager steps only (profiler runs)")
    ap.add_argument("--limit", type=int, default=300, help="seconds per configuration")
    ap.add_argument("--one", nargs=3, metavar=("MODEL", "BATCH", "ROBUST"), help="run one configuration in this process")
    a = ap.parse_args()
    if a.one:
        one(a.one[0], int(a.one[1]), a.one[2] == "1", a.steps, a.warmup, a.no_capture)
        return 0
    if a.one_eager:
        restatement(a.one_eager[0], int(a.one_eager[1]), a.one_eager[2] == "1", a.steps, a.chunk)
        return 0
    for name in a.models:
        for B in a.batches:
            for robust in (False, True):
                base = [sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup), "--chunk", str(a.chunk)]
                cmds = [base + ["--one", name, str(B), "1" if robust else "0"] + (["--no-capture"] if a.no_capture else [])]
                if not a.no_eager and B == a.eager_batch:
                    cmds.append(base + ["--one-eager", name, str(B), "1" if robust else "0"])
                for cmd in cmds:
                    try:
                        rc = subprocess.run(cmd, timeout=a.limit).returncode
                    except subprocess.TimeoutExpired:
                        rc = 124
                    if rc != 0:
                        print(json.dumps({"model": name, "batch": B, "robust": robust, "failed": rc, "leg": "restatement" if "--one-eager" in cmd else "hip"}), flush=True)
                        return rc                       # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
