#!/usr/bin/env python3
"""Twins-SVT at 224 px with the reference's default arguments (emb 64 / 128 / 256 / 512, depths 1 / 1 / 5 / 4, heads 8 x 64):
training-step throughput (fwd + CE + bwd + clip + AdamW through train.Trainer), softmax and robust, eager and captured
(Trainer.capture); for comparison, at one batch size, the fp32 restatement tests/twins_ref.py run eagerly under bf16 autocast on
the same GPU (forward + backward + clip + torch AdamW) in a process of its own that launches no HIP kernel of the library.
`--kernels` times, in ONE process, nrv_subattn_fwd + _bwd against the composed path (nrv_bgemm -> nrv_sinkhorn_fwd with 0
iterations -> nrv_bgemm and its backward, the model's own fallback) at the four stage shapes of the 224 px model.  `--profile`
times every C-ABI launch of one eager forward + backward with HIP events (kernels.LaunchProfile) and writes the kernel-time
shares as CSV.  Every configuration runs in a child process of its own under a time limit, and the run stops at the first one
that fails.  Prints one JSON line per measurement.

    python tools/twins_bench.py [--batches 64 256] [--steps 10] [--warmup 3] [--no-eager] [--eager-batch 64] [--chunk 16] [--no-capture]
                                [--no-robust] [--limit 300] [--kernels] [--kernel-batches 64 8] [--profile BATCH [--csv PATH]]
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

# (Nq, Nk) of the global attention in the four stages at 224 px: maps 56 / 28 / 14 / 7, k = 7
STAGE_SHAPES = ((3136, 64), (784, 16), (196, 4), (49, 1))
HEADS, DH = 8, 64


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


def one(B, robust, steps, warmup, no_capture=False):
    """The HIP legs of one configuration: Trainer.step eager, then captured.  A batch that does not fit is reported, not an error."""
    import torch
    from noise_robust_vit_amd.twins_svt import TwinsSVT
    from noise_robust_vit_amd.train import Trainer, TrainConfig
    dev = torch.device("cuda:0")
    tag = {"model": "twins_svt_default", "batch": B, "robust": robust}
    try:
        torch.manual_seed(0)
        x = torch.randn(B, 3, 224, 224, device=dev)
        y = torch.randint(0, 100, (B,), device=dev)
        for captured in ((False,) if no_capture else (False, True)):
            torch.manual_seed(0)
            m = TwinsSVT(num_classes=100, robust=robust).to(dev).train()
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


def restatement(B, robust, steps, chunk):
    """tests/twins_ref.py, fp32 masters under bf16 autocast, forward + backward + clip + torch AdamW, in a process that launches
    no kernel of libnrv_hip.so (the model object is walked for its structure only).  The batch goes through in chunks of `chunk`
    images whose gradients accumulate (loss weighted chunk / B: the same step as one pass over the batch)."""
    import torch
    from noise_robust_vit_amd import _lib
    from noise_robust_vit_amd.twins_svt import TwinsSVT
    import twins_ref
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x = torch.randn(B, 3, 224, 224, device=dev)
    y = torch.randint(0, 100, (B,), device=dev)
    m = TwinsSVT(num_classes=100, robust=robust).train()
    P = {n: p.detach().to(dev, torch.float32).requires_grad_(True) for n, p in m.named_parameters()}
    params = list(P.values())
    opt = torch.optim.AdamW(params, lr=1e-3)

    def step():
        for i in range(0, B, chunk):
            xs, ys = x[i:i + chunk], y[i:i + chunk]
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits = twins_ref.forward(m, P, xs)
            (torch.nn.functional.cross_entropy(logits.float(), ys) * (xs.shape[0] / B)).backward()
        torch.nn.utils.clip_grad_norm_(params, 5.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
    de = _time(step, max(2, steps // 2), 1)
    assert _lib._lib is None, "the restatement's process must not load libnrv_hip.so"
    print(json.dumps({"model": "twins_svt_default", "batch": B, "robust": robust,
                      "restatement": f"fp32 under bf16 autocast, eager, chunks of {chunk}", "eager_step_ms": round(de * 1e3, 2),
                      "eager_img_per_s": round(B / de, 1)}), flush=True)


def kernels(batches, steps, warmup):
    """subattn forward + backward against the composed path on the same q / kv / dout, one process, every stage shape."""
    import torch
    from noise_robust_vit_amd import kernels as K
    from noise_robust_vit_amd import twins_svt as V
    dev = torch.device("cuda:0")
    inner, scale = HEADS * DH, DH ** -0.5
    for B in batches:
        for Nq, Nk in STAGE_SHAPES:
            g = torch.Generator(device="cpu").manual_seed(Nq + Nk)
            q = torch.randn(B * Nq, inner, generator=g).to(dev, torch.bfloat16)
            kv = torch.randn(B * Nk, 2 * inner, generator=g).to(dev, torch.bfloat16)
            do = torch.randn(B * Nq, inner, generator=g).to(dev, torch.bfloat16)
            k, v = kv[:, :inner], kv[:, inner:]
            dkv = torch.empty_like(kv)

            def fused():
                o, lse = K.subattn_fwd(q, k, v, B, HEADS, Nq, Nk, DH, scale)
                K.subattn_bwd(q, k, v, do, lse, B, HEADS, Nq, Nk, DH, scale, dk=dkv[:, :inner], dv=dkv[:, inner:])

            sq, kvs, kvT, mat, matT = V._global_strides(Nq, Nk, HEADS, DH)

            def composed():
                S, P, lse, avec, bvec = V._composed_probs(q, kv, B, HEADS, Nq, Nk, DH, scale, 0)
                o = torch.empty_like(q)
                K.bgemm((P, 0), mat, (kv, inner), kvs, (o, 0), sq, B, HEADS, Nq, DH, Nk, 1.0)
                del S
                S = torch.empty_like(P)                                                         # the backward recomputes the scores
                K.bgemm((q, 0), sq, (kv, 0), kvT, (S, 0), mat, B, HEADS, Nq, Nk, DH, scale)
                K.bgemm((P, 0), matT, (do, 0), sq, (dkv, inner), kvs, B, HEADS, Nk, DH, Nq, 1.0)
                dP = torch.empty_like(P)
                K.bgemm((do, 0), sq, (kv, inner), kvT, (dP, 0), mat, B, HEADS, Nq, Nk, DH, 1.0)
                dS = K.sinkhorn_bwd(S, dP, lse, avec, bvec, iters=0)
                dq = torch.empty_like(q)
                K.bgemm((dS, 0), mat, (kv, 0), kvs, (dq, 0), sq, B, HEADS, Nq, DH, Nk, scale)
                K.bgemm((dS, 0), matT, (q, 0), sq, (dkv, 0), kvs, B, HEADS, Nk, DH, Nq, scale)

            tf, tc = _time(fused, steps, warmup), _time(composed, steps, warmup)
            qo_mb = 4 * B * Nq * inner * 2 / 1e6
            print(json.dumps({"kernel": "subattn fwd+bwd vs composed", "batch": B, "Nq": Nq, "Nk": Nk, "heads": HEADS, "dh": DH,
                              "subattn_ms": round(tf * 1e3, 4), "composed_ms": round(tc * 1e3, 4), "speedup": round(tc / tf, 2),
                              "q_o_dq_do_mbytes": round(qo_mb, 1), "subattn_gb_per_s_on_those": round(qo_mb / 1e3 / tf, 1)}), flush=True)


def profile(B, csv):
    """One eager forward + backward, softmax, with every launch of the library timed alone; kernel classes as shares of the
    summed launch time (torch's own kernels -- the head, the loss, the final mean -- are not in it)."""
    import torch
    from noise_robust_vit_amd import kernels as K
    from noise_robust_vit_amd.twins_svt import TwinsSVT
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = TwinsSVT(num_classes=100).to(dev).train()
    x = torch.randn(B, 3, 224, 224, device=dev)
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
    rows = sorted(s.items(), key=lambda kv: -kv[1]["ms"])
    for k, v in rows:
        print(json.dumps({"model": "twins_svt_default", "batch": B, "kernel": k, "launches": v["launches"], "ms": round(v["ms"], 4),
                          "share_of_launch_time": round(v["ms"] / total, 4)}), flush=True)
    if csv:
        os.makedirs(os.path.dirname(os.path.abspath(csv)), exist_ok=True)
        with open(csv, "w") as f:
            f.write("family,calls,total_ms,share\n")
            for k, v in rows:
                f.write(f"{k},{v['launches']},{v['ms']:.3f},{v['ms'] / total:.4f}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true", help="skip the torch restatement")
    ap.add_argument("--no-robust", action="store_true")
    ap.add_argument("--eager-batch", type=int, default=64, help="the restatement is timed at this batch only")
    ap.add_argument("--chunk", type=int, default=16, help="images per pass of the restatement")
    ap.add_argument("--one-eager", nargs=2, metavar=("BATCH", "ROBUST"), help="run one restatement in this process")
    ap.add_argument("--no-capture", action="store_true", help="eager steps only (profiler runs)")
    ap.add_argument("--limit", type=int, default=300, help="seconds per configuration")
    ap.add_argument("--one", nargs=2, metavar=("BATCH", "ROBUST"), help="run one configuration in this process")
    ap.add_argument("--kernels", action="store_true", help="subattn against the composed path, in this process")
    ap.add_argument("--kernel-batches", type=int, nargs="+", default=[64, 8])
    ap.add_argument("--profile", type=int, metavar="BATCH", help="per-launch timing of one eager step in this process")
    ap.add_argument("--csv", help="with --profile: write the kernel-time shares here")
    a = ap.parse_args()
    if a.one:
        one(int(a.one[0]), a.one[1] == "1", a.steps, a.warmup, a.no_capture)
        return 0
    if a.one_eager:
        restatement(int(a.one_eager[0]), a.one_eager[1] == "1", a.steps, a.chunk)
        return 0
    if a.kernels:
        kernels(a.kernel_batches, a.steps, a.warmup)
        return 0
    if a.profile:
        profile(a.profile, a.csv)
        return 0
    for B in a.batches:
        for robust in ((False,) if a.no_robust else (False, True)):
            base = [sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup), "--chunk", str(a.chunk)]
            cmds = [base + ["--one", str(B), "1" if robust else "0"] + (["--no-capture"] if a.no_capture else [])]
            if not a.no_eager and B == a.eager_batch:
                cmds.append(base + ["--one-eager", str(B), "1" if robust else "0"])
            for cmd in cmds:
                try:
                    rc = subprocess.run(cmd, timeout=a.limit).returncode
                except subprocess.TimeoutExpired:
                    rc = 124
                if rc != 0:
                    print(json.dumps({"batch": B, "robust": robust, "failed": rc, "leg": "restatement" if "--one-eager" in cmd else "hip"}), flush=True)
                    return rc                       # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
