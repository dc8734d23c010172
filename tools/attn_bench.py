#!/usr/bin/env python3
"""Attention kernels only.  Without arguments: ViT-B/16, batch 256 (B / N / H from the environment), forward + backward in a loop, for
rocprofv3 --kernel-trace --stats.  With --drop P: the plain entries and the attention-weight dropout entries (nrv_attn_drop_*) timed
with HIP events in this process at each of --shapes B,N,H,dh, one JSON line per shape with the drop / plain ratios.  Dev tool, GPU only.

    python tools/attn_bench.py --drop 0.1 [--shapes 256,197,12,64 256,256,4,64 64,577,12,64 64,3136,4,64] [--iters 20]
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from noise_robust_vit_amd import kernels as K
dev = torch.device("cuda:0")
SHAPES = ["256,197,12,64", "256,256,4,64", "64,577,12,64", "64,3136,4,64"]


def _ms(fn, iters):
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def drop_ab(shape, p, iters):
    B, N, H, dh = shape
    scale = dh ** -0.5
    qkv = (torch.randn(B * N, 3 * H * dh, device=dev) * 0.5).bfloat16()
    do = (torch.randn(B * N, H * dh, device=dev) * 0.5).bfloat16()
    seed = torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64, device=dev)
    o, lse = K.attn_fwd(qkv, B, N, H, dh, scale)
    od, lsed = K.attn_drop_fwd(qkv, seed, p, B, N, H, dh, scale)
    t = {"fwd": _ms(lambda: K.attn_fwd(qkv, B, N, H, dh, scale), iters),
         "drop_fwd": _ms(lambda: K.attn_drop_fwd(qkv, seed, p, B, N, H, dh, scale), iters),
         "bwd": _ms(lambda: K.attn_bwd(qkv, o, do, lse, B, N, H, dh, scale), iters),
         "drop_bwd": _ms(lambda: K.attn_drop_bwd(qkv, od, do, lsed, seed, p, B, N, H, dh, scale), iters)}
    print(json.dumps({"B": B, "N": N, "H": H, "dh": dh, "p": p, **{k + "_ms": round(v, 4) for k, v in t.items()},
                      "fwd_ratio": round(t["drop_fwd"] / t["fwd"], 3), "bwd_ratio": round(t["drop_bwd"] / t["bwd"], 3),
                      "fwd_bwd_ratio": round((t["drop_fwd"] + t["drop_bwd"]) / (t["fwd"] + t["bwd"]), 3)}), flush=True)


ap = argparse.ArgumentParser()
ap.add_argument("--drop", type=float, default=None)
ap.add_argument("--shapes", nargs="+", default=SHAPES)
ap.add_argument("--iters", type=int, default=20)
a = ap.parse_args()
if a.drop is not None:
    for sh in a.shapes:
        drop_ab(tuple(int(v) for v in sh.split(",")), a.drop, a.iters)
else:
    B, N, H = int(os.environ.get("B", 256)), int(os.environ.get("N", 197)), int(os.environ.get("H", 12))
    qkv = (torch.randn(B * N, 3 * H * 64, device=dev) * 0.5).bfloat16()
    do = (torch.randn(B * N, H * 64, device=dev) * 0.5).bfloat16()
    for _ in range(20):
        o, lse = K.attn_fwd(qkv, B, N, H, 64, 0.125)
        K.attn_bwd(qkv, o, do, lse, B, N, H, 64, 0.125)
    torch.cuda.synchronize()
