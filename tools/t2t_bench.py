#!/usr/bin/env python3
"""T2T-ViT 224 px training-step throughput (fwd + CE + bwd + clip + AdamW through train.Trainer) for a T2T-ViT-14-like
(dim 384, depth 14, heads 6, mlp_dim 1152) and a smaller (dim 256, depth 7, heads 4, mlp_dim 512) model, softmax and robust,
eager and captured (Trainer.capture); for comparison, at one batch size, the fp32 restatement tests/t2t_ref.py run eagerly under
bf16 autocast on the same GPU (forward + backward + torch AdamW) in a process of its own that launches no HIP kernel of the
library, the batch in chunks of 8 images.  `--attn` times stage-1 attention alone (3136 tokens, one head of 147 stored
as 152), forward + backward, on the fused nrv_attn_wide_* kernels and on the composed path (nrv_bgemm + softmax on the matrix)
in one process.  Every configuration runs in a child process of its own under a time limit, and the run stops at the first one
that fails.  Prints one JSON line per measurement.

    python tools/t2t_bench.py [--models t2t14 small] [--batches 64 256] [--steps 10] [--warmup 3] [--no-eager] [--eager-batch 64] [--chunk 8] [--no-capture] [--limit 300]
    python tools/t2t_bench.py --attn [--batches 8 64]
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
    "t2t14": dict(dim=384, depth=14, heads=6, mlp_dim=1152),
    "small": dict(dim=256, depth=7, heads=4, mlp_dim=512),
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
    from noise_robust_vit_amd.t2t import T2TViT
    from noise_robust_vit_amd.train import Trainer, TrainConfig
    dev = torch.device("cuda:0")
    tag = {"model": name, "batch": B, "robust": robust}
    try:
        torch.manual_seed(0)
        x = torch.randn(B, 3, 224, 224, device=dev)
        y = torch.randint(0, 100, (B,), device=dev)
        for captured in ((False,) if no_capture else (False, True)):
            torch.manual_seed(0)
            m = T2TViT(image_size=224, num_classes=100, robust=robust, **MODELS[name]).to(dev).train()
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
    """tests/t2t_ref.py, fp32 masters under bf16 autocast, forward + backward + clip + torch AdamW, in a process that launches no
    kernel of libnrv_hip.so (the model object is walked for its structure only).  The batch goes through in chunks of `chunk`
    images whose gradients accumulate (loss weighted chunk / B: the same step as one pass over the batch), so that the largest
    tensor, stage 1's fp32 [chunk, 1, 3136, 3136] attention matrix, stays at 0.3 GB for chunk = 8 instead of 2.5 GB for 64."""
    import torch
    from noise_robust_vit_amd import _lib
    from noise_robust_vit_amd.t2t import T2TViT
    import t2t_ref
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x = torch.randn(B, 3, 224, 224, device=dev)
    y = torch.randint(0, 100, (B,), device=dev)
    m = T2TViT(image_size=224, num_classes=100, robust=robust, **MODELS[name]).train()
    P = {n: p.detach().to(dev, torch.float32).requires_grad_(True) for n, p in m.named_parameters()}
    params = list(P.values())
    opt = torch.optim.AdamW(params, lr=1e-3)

    def step():
        for i in range(0, B, chunk):
            xs, ys = x[i:i + chunk], y[i:i + chunk]
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits = t2t_ref.forward(m, P, xs)
            (torch.nn.functional.cross_entropy(logits.float(), ys) * (xs.shape[0] / B)).backward()
        torch.nn.utils.clip_grad_norm_(params, 5.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
    de = _time(step, max(2, steps // 2), 1)
    assert _lib._lib is None, "the restatement's process must not load libnrv_hip.so"
    print(json.dumps({"model": name, "batch": B, "robust": robust, "restatement": f"fp32 under bf16 autocast, eager, chunks of {chunk}",
                      "eager_step_ms": round(de * 1e3, 2), "eager_img_per_s": round(B / de, 1)}), flush=True)


def attn(B, steps, warmup):
    """Stage-1 attention alone, forward + backward: the fused wide-head kernels and the composed path, same process, same q / k / v."""
    import torch
    from noise_robust_vit_amd import kernels as K
    dev = torch.device("cuda:0")
    N, dh, scale = 3136, 152, 147 ** -0.5
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B * N, 3, dh, generator=g)
    qkv[..., 147:] = 0
    qkv = qkv.reshape(B * N, 3 * dh).to(torch.bfloat16).to(dev)
    dout = torch.randn(B * N, dh, generator=g).to(torch.bfloat16).to(dev)

    def fused():
        o, lse = K.attn_wide_fwd(qkv, B, N, 1, dh, scale)
        K.attn_wide_bwd(qkv, o, dout, lse, B, N, 1, dh, scale)

    def composed():
        o, saved = K.attn_composed_fwd(qkv, B, N, 1, dh, scale, 0)
        K.attn_composed_bwd(qkv, dout, saved, B, N, 1, dh, scale)
    tf = _time(fused, steps, warmup)
    tc = _time(composed, steps, warmup)
    print(json.dumps({"stage1_attention": True, "batch": B, "tokens": N, "head_dim": 147, "fused_ms": round(tf * 1e3, 3),
                      "composed_ms": round(tc * 1e3, 3), "composed_over_fused": round(tc / tf, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=list(MODELS), choices=list(MODELS))
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true", help="skip the torch restatement")
    ap.add_argument("--eager-batch", type=int, default=64, help="the restatement is timed at this batch only")
    ap.add_argument("--chunk", type=int, default=8, help="images per pass of the restatement")
    ap.add_argument("--one-eager", nargs=3, metavar=("MODEL", "BATCH", "ROBUST"), help="run one restatement in this process")
    ap.add_argument("--no-capture", action="store_true", help="eager steps only (profiler runs)")
    ap.add_argument("--limit", type=int, default=300, help="seconds per configuration")
    ap.add_argument("--attn", action="store_true", help="stage-1 attention alone: fused against composed")
    ap.add_argument("--one-attn", type=int, metavar="BATCH", help="run one stage-1 attention measurement in this process")
    ap.add_argument("--one", nargs=3, metavar=("MODEL", "BATCH", "ROBUST"), help="run one configuration in this process")
    a = ap.parse_args()
    if a.one:
        one(a.one[0], int(a.one[1]), a.one[2] == "1", a.steps, a.warmup, a.no_capture)
        return 0
    if a.one_eager:
        restatement(a.one_eager[0], int(a.one_eager[1]), a.one_eager[2] == "1", a.steps, a.chunk)
        return 0
    if a.one_attn:
        attn(a.one_attn, a.steps, a.warmup)
        return 0
    if a.attn:
        for B in a.batches:
            cmd = [sys.executable, os.path.abspath(__file__), "--one-attn", str(B), "--steps", str(a.steps), "--warmup", str(a.warmup)]
            try:
                rc = subprocess.run(cmd, timeout=a.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(json.dumps({"stage1_attention": True, "batch": B, "failed": rc}), flush=True)
                return rc
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
