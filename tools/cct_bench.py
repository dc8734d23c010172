#!/usr/bin/env python3
"""CCT training-step throughput (fwd + CE + bwd + clip + AdamW through train.Trainer) for CCT-7/3x1 at 32 px (256 tokens),
CCT-14/7x2 at 224 px (196 tokens) and CCT-7/7x1 at 224 px (3136 tokens): softmax and robust, attention dropout 0.1 (the
reference's default: the composed path) and 0.0 (the fused kernels), eager and captured (Trainer.capture); `--fused-adrop` adds, beside
every softmax configuration with attention dropout > 0, the same one with fused_attention_dropout=True (the dropout inside the fused
kernels).  For comparison, at
one batch size, the fp32 restatement tests/cct_ref.py run eagerly under bf16 autocast on the same GPU (forward + backward + clip
+ torch AdamW, without attention dropout and drop path: less work than the HIP leg does) in a process of its own that launches
no HIP kernel of the library.  `--profile` times every C-ABI launch of one eager step with HIP events (kernels.LaunchProfile) and
prints, per kernel class, the time, the bytes computed from the shapes and their share of the HBM peak.  Every configuration runs
in a child process of its own under a time limit, and the run stops at the first one that fails.  One JSON line per measurement.

    python tools/cct_bench.py [--models 7_3x1_32 ...] [--batches 64 256] [--adrop 0.1 0.0] [--steps 10] [--warmup 3] [--no-eager]
                              [--eager-batch 64] [--chunk 64] [--no-capture] [--no-robust] [--limit 300] [--profile MODEL BATCH]
                              [--fused-adrop]
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

# name -> (builder, keyword arguments, image size)
MODELS = {
    "7_3x1_32": ("cct_7", dict(img_size=32, n_conv_layers=1, kernel_size=3, num_classes=100), 32),
    "14_7x2_224": ("cct_14", dict(img_size=224, n_conv_layers=2, kernel_size=7, num_classes=100), 224),
    "7_7x1_224": ("cct_7", dict(img_size=224, n_conv_layers=1, kernel_size=7, num_classes=100), 224),
}
HBM_PEAK = 8.0e12            # bytes / s, MI355X


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


def _build(name, robust, adrop, fused=False):
    from noise_robust_vit_amd import cct
    fn, kw, size = MODELS[name]
    return getattr(cct, fn)(robust=robust, attention_dropout=adrop, fused_attention_dropout=fused, **kw), size


def one(name, B, robust, adrop, steps, warmup, no_capture=False, fused=False):
    """The HIP legs of one configuration: Trainer.step eager, then captured.  A batch that does not fit is reported, not an error."""
    import torch
    from noise_robust_vit_amd.train import Trainer, TrainConfig
    dev = torch.device("cuda:0")
    tag = {"model": name, "batch": B, "robust": robust, "attention_dropout": adrop, "fused_attention_dropout": fused}
    try:
        for captured in ((False,) if no_capture else (False, True)):
            torch.manual_seed(0)
            m, size = _build(name, robust, adrop, fused)
            m = m.to(dev).train()
            x = torch.randn(B, 3, size, size, device=dev)
            y = torch.randint(0, 100, (B,), device=dev)
            tr = Trainer(m, TrainConfig(lr=1e-3, grad_max_norm=5.0))
            if captured:
                tr.capture(x, y)
            dt = _time(lambda: tr.step(x, y), steps, warmup)
            print(json.dumps(dict(tag, tokens=m.classifier.sequence_length, captured=captured, hip_step_ms=round(dt * 1e3, 2),
                                  hip_img_per_s=round(B / dt, 1), peak_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1))), flush=True)
            del m, tr
            torch.cuda.empty_cache()
    except torch.cuda.OutOfMemoryError:
        print(json.dumps(dict(tag, fits=False, note="out of memory")), flush=True)


def profile(name, B, fused=False):
    """One eager forward + backward at attention_dropout 0 (with `fused`: 0.1 inside the fused kernels) with every launch timed alone: per kernel class launches, ms, the
    bytes the wrapper computes from the shapes, GB/s and the share of the HBM peak."""
    import torch
    from noise_robust_vit_amd import kernels as K
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m, size = _build(name, False, 0.1 if fused else 0.0, fused)
    m = m.to(dev).train()
    x = torch.randn(B, 3, size, size, device=dev)
    y = torch.randint(0, 100, (B,), device=dev)

    def fb():
        m.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(m(x), y).backward()
    fb()
    fb()
    with K.LaunchProfile() as prof:
        fb()
    s = prof.summary()
    total = sum(v["ms"] for v in s.values())
    for k, v in sorted(s.items(), key=lambda kv: -kv[1]["ms"]):
        gbs = v["bytes"] / (v["ms"] * 1e-3) / 1e9 if v["ms"] > 0 else 0.0
        print(json.dumps({"model": name, "batch": B, "kernel": k, "launches": v["launches"], "ms": round(v["ms"], 4),
                          "share_of_launch_time": round(v["ms"] / total, 4), "mbytes": round(v["bytes"] / 1e6, 2), "gb_per_s": round(gbs, 1),
                          "share_of_hbm_peak": round(gbs * 1e9 / HBM_PEAK, 4)}), flush=True)


def restatement(name, B, robust, steps, chunk):
    """tests/cct_ref.py, fp32 masters under bf16 autocast, forward + backward + clip + torch AdamW, in a process that launches no
    kernel of libnrv_hip.so (the model object is walked for its structure only); no attention dropout, no drop path.  The batch
    goes through in chunks of `chunk` images whose gradients accumulate."""
    import torch
    from noise_robust_vit_amd import _lib
    import cct_ref
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m, size = _build(name, robust, 0.0)
    m.train()
    for blk in m.classifier.blocks:
        blk.drop_path.drop_prob = 0.0
    x = torch.randn(B, 3, size, size, device=dev)
    y = torch.randint(0, 100, (B,), device=dev)
    P = {n: p.detach().to(dev, torch.float32).requires_grad_(p.requires_grad) for n, p in m.named_parameters()}
    params = [p for p in P.values() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-3)

    def step():
        for i in range(0, B, chunk):
            xs, ys = x[i:i + chunk], y[i:i + chunk]
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits = cct_ref.forward(m, P, xs)
            (torch.nn.functional.cross_entropy(logits.float(), ys) * (xs.shape[0] / B)).backward()
        torch.nn.utils.clip_grad_norm_(params, 5.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
    de = _time(step, max(2, steps // 2), 1)
    assert _lib._lib is None, "the restatement's process must not load libnrv_hip.so"
    print(json.dumps({"model": name, "batch": B, "robust": robust, "restatement": f"fp32 under bf16 autocast, eager, chunks of {chunk}, no dropout",
                      "eager_step_ms": round(de * 1e3, 2), "eager_img_per_s": round(B / de, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=list(MODELS), choices=list(MODELS))
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--adrop", type=float, nargs="+", default=[0.1, 0.0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true", help="skip the torch restatement")
    ap.add_argument("--no-robust", action="store_true", help="softmax only")
    ap.add_argument("--eager-batch", type=int, default=64, help="the restatement is timed at this batch only")
    ap.add_argument("--chunk", type=int, default=64, help="images per pass of the restatement")
    ap.add_argument("--no-capture", action="store_true", help="eager steps only (profiler runs)")
    ap.add_argument("--limit", type=int, default=300, help="seconds per configuration")
    ap.add_argument("--one", nargs=4, metavar=("MODEL", "BATCH", "ROBUST", "ADROP"), help="run one configuration in this process")
    ap.add_argument("--one-eager", nargs=3, metavar=("MODEL", "BATCH", "ROBUST"), help="run one restatement in this process")
    ap.add_argument("--fused-adrop", action="store_true", help="add the fused_attention_dropout=True configurations (softmax, dropout > 0)")
    ap.add_argument("--fused", action="store_true", help="with --one / --profile: fused_attention_dropout=True")
    ap.add_argument("--profile", nargs=2, metavar=("MODEL", "BATCH"), help="per-launch timing of one eager step in this process")
    a = ap.parse_args()
    if a.one:
        one(a.one[0], int(a.one[1]), a.one[2] == "1", float(a.one[3]), a.steps, a.warmup, a.no_capture, a.fused)
        return 0
    if a.one_eager:
        restatement(a.one_eager[0], int(a.one_eager[1]), a.one_eager[2] == "1", a.steps, a.chunk)
        return 0
    if a.profile:
        profile(a.profile[0], int(a.profile[1]), a.fused)
        return 0
    base = [sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup), "--chunk", str(a.chunk)]
    for name in a.models:
        for B in a.batches:
            for robust in ((False,) if a.no_robust else (False, True)):
                cmds = [base + ["--one", name, str(B), "1" if robust else "0", str(p)] + (["--no-capture"] if a.no_capture else [])
                        for p in a.adrop]
                if a.fused_adrop and not robust:
                    cmds += [base + ["--one", name, str(B), "0", str(p), "--fused"] + (["--no-capture"] if a.no_capture else [])
                             for p in a.adrop if p > 0.0]
                if not a.no_eager and B == a.eager_batch:
                    cmds.append(base + ["--one-eager", name, str(B), "1" if robust else "0"])
                for cmd in cmds:
                    try:
                        rc = subprocess.run(cmd, timeout=a.limit).returncode
                    except subprocess.TimeoutExpired:
                        rc = 124
                    if rc != 0:
                        print(json.dumps({"model": name, "batch": B, "robust": robust, "failed": rc,
                                          "leg": "restatement" if "--one-eager" in cmd else "hip"}), flush=True)
                        return rc                       # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
