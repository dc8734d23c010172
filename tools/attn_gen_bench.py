#!/usr/bin/env python3
"""Streaming attention kernels of nrv_attn_gen.hip (N > 256 or head dim != 64; memory keys and masks) of several builds,
interleaved.  Dev tool, GPU only.
    python tools/attn_gen_bench.py base,product"""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import _devlib
from noise_robust_vit_amd import kernels as K
libs = (sys.argv[1] if len(sys.argv) > 1 else "product").split(",")
dev = torch.device("cuda:0")
def timeit(fn, n=6):
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / n
def flat(x):
    return [t for t in (x if isinstance(x, tuple) else (x,)) if t is not None]
def gen_case(B, N, H, dh):
    qkv = (torch.randn(B * N, 3 * H * dh, device=dev) * 0.5).bfloat16()
    do = (torch.randn(B * N, H * dh, device=dev) * 0.5).bfloat16()
    return (lambda: K.attn_fwd(qkv, B, N, H, dh, dh ** -0.5),
            lambda o, aux: K.attn_bwd(qkv, o, do, aux, B, N, H, dh, dh ** -0.5))
def mem_case(B, N, H, dh, M, shared):
    # the mask of lucid_vit.Adapter (as in tools/attn_mem_profile.py): query 0 attends to every key, the other queries to
    # token keys 1 .. N - 1 only
    qkv = (torch.randn(B * N, 3 * H * dh, device=dev) * 0.5).bfloat16()
    do = (torch.randn(B * N, H * dh, device=dev) * 0.5).bfloat16()
    mkv = (torch.randn((1 if shared else B) * M, 2 * H * dh, device=dev) * 0.5).bfloat16()
    mask = torch.zeros(N, N + M, dtype=torch.bool, device=dev)
    mask[0] = True
    mask[1:, 1:N] = True
    bits = K.mask_pack(mask, B, H, N, N + M)
    sc = dh ** -0.5
    return (lambda: K.attn_mem_fwd(qkv, mkv, B, N, M, H, dh, sc, shared, bits),
            lambda o, l: K.attn_mem_bwd(qkv, o, do, l, mkv, B, N, M, H, dh, sc, shared, bits))
for name, shape, make in [("vit_b_16 @ 384 px", "B32 N577 H12 dh64", lambda: gen_case(32, 577, 12, 64)),
                          ("vit_h_14", "B32 N257 H16 dh80", lambda: gen_case(32, 257, 16, 80)),
                          ("simplevit dh 32", "B64 N196 H24 dh32", lambda: gen_case(64, 196, 24, 32)),
                          ("dh 128, N 1024", "B8 N1024 H8 dh128", lambda: gen_case(8, 1024, 8, 128)),
                          ("adapter, shared", "B256 N197 M10 H12 dh64", lambda: mem_case(256, 197, 12, 64, 10, True)),
                          ("memories per sample", "B32 N257 M10 H16 dh80", lambda: mem_case(32, 257, 16, 80, 10, False)),
                          ("memories per sample", "B8 N1024 M10 H8 dh128", lambda: mem_case(8, 1024, 8, 128, 10, False))]:
    fwd, bwd = make()
    res = {l: ([], []) for l in libs}
    outs = {}
    for l in libs:
        _devlib.use_library(l)
        o, aux = fwd()
        outs[l] = [t.float().clone() for t in flat((o, aux)) + flat(bwd(o, aux))]
    for l in libs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[l], outs[libs[0]])), f"{name}: {l} differs from {libs[0]}"
    for _ in range(4):
        for l in libs:
            _devlib.use_library(l)
            res[l][0].append(timeit(fwd))
            o, aux = fwd()
            res[l][1].append(timeit(lambda: bwd(o, aux)))
    for l in libs:
        print(f"{name:20s} {shape:22s}: {l:8s} fwd {statistics.median(res[l][0]):7.3f} ms   bwd {statistics.median(res[l][1]):7.3f} ms   "
              f"(rounds fwd {' '.join(f'{t:.3f}' for t in res[l][0])}, bwd {' '.join(f'{t:.3f}' for t in res[l][1])})", flush=True)
