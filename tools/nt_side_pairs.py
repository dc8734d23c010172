#!/usr/bin/env python3
"""The four (weight gradient, dX GEMM) pairs of an encoder block's backward, timed two ways in ONE process, arm by arm:

    arm A   gemm_tn (its reduction a launch of its own) + gemm_nt                  three launches
    arm B   gemm_tn(defer=True) + gemm_nt(side=pending)                            the reduction rides in the NT launch when admitted

One HIP event pair per call, the arms alternating call by call, `--rounds` rounds of `--calls` calls each; per round and arm the
median.  Reported per pair: the medians over the rounds, the spread (max - min) of arm A's rounds, B - A, whether the library
admitted the job, the share and the smallest bytes-per-K-step constant that admits it.

    python tools/nt_side_pairs.py [--lib NAME] [--dim 768 --mlp 3072 --tokens 50432] [--probe K ...]

`--lib NAME`: a tools/build_dev.py build, e.g. one that admits every job with late workgroups
    python tools/build_dev.py side --instrument -DNRV_DEV_NO_STAMPS -DNRV_FORCE_NT_SIDE_ADMIT
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch

import _devlib
from noise_robust_vit_amd import kernels as K
from noise_robust_vit_amd._lib import EPI_DGELU_Q8, EPI_NONE


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--mlp", type=int, default=3072)
    ap.add_argument("--tokens", type=int, default=50432)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--probe", type=int, nargs="*", default=None, help="K values: the dW1 job in front of [tokens x dim x K] launches")
    a = ap.parse_args()
    _devlib.use_library(a.lib)
    dev = torch.device("cuda")
    T, D, F = a.tokens, a.dim, a.mlp
    g = torch.Generator(device=dev).manual_seed(0)

    def bf(r, c):
        return (torch.randn(r, c, device=dev, generator=g) * 0.05).to(torch.bfloat16)

    dy, h, xn, o = bf(T, D), bf(T, F), bf(T, D), bf(T, D)
    du, dqkv = bf(T, F), bf(T, 3 * D)
    u = torch.randint(0, 256, ((T + 1) // 2 * 2, F), device=dev, dtype=torch.uint8, generator=g)
    w2_t, w1_t, wo_t, wqkv_t = bf(F, D), bf(D, F), bf(D, D), bf(D, 3 * D)
    # name, TN operands (A [T, M], B [T, N]), NT operands (A [T, K], B [N, K]), NT epilogue, aux
    pairs = [("dW2 -> dU", dy, h, dy, w2_t, EPI_DGELU_Q8, u),
             ("dW1 -> dXn2", du, xn, du, w1_t, EPI_NONE, None),
             ("dWo -> dO", dy, o, dy, wo_t, EPI_NONE, None),
             ("dWqkv -> dXn", dqkv, xn, dqkv, wqkv_t, EPI_NONE, None)]
    if a.probe:
        # the same 7-split job in front of dX launches of other depths: a slab job of a full split-K launch is always about one
        # 256 x 256 fp32 tile per CU, so what a launch can hide is set by its K-steps alone
        pairs = [(f"dW1 -> K {kk}", du, xn, bf(T, kk), bf(D, kk), EPI_NONE, None) for kk in a.probe]
    print(f"T {T} D {D} mlp {F}  lib {a.lib or 'product'}  rounds {a.rounds} x {a.calls} calls per arm")
    total_gap = 0.0
    for name, ta, tb, na, nb, epi, aux in pairs:
        M, N = ta.shape[1], tb.shape[1]
        dW = torch.zeros(M, N, device=dev)
        db = torch.zeros(M, device=dev)
        out = torch.empty(T, nb.shape[0], dtype=torch.bfloat16, device=dev)
        tn = K.gemm_tn_plan(M, N, T, dbias=True)
        job_bytes = 0 if tn["direct"] else tn["splits"] * M * N * 4
        sp = K.gemm_nt_side_plan(T, nb.shape[0], na.shape[1], epi, False, job_bytes)
        npl = K.gemm_nt_plan(T, nb.shape[0], na.shape[1], epi)
        fused = [None]

        def arm_a():
            K.gemm_tn(ta, tb, out=dW, beta=1.0, dbias=db, dbias_beta=1.0)
            K.gemm_nt(na, nb, out=out, epilogue=epi, aux=aux)

        def arm_b():
            pend = K.gemm_tn(ta, tb, out=dW, beta=1.0, dbias=db, dbias_beta=1.0, defer=True)[-1]
            K.gemm_nt(na, nb, out=out, epilogue=epi, aux=aux, side=pend)
            fused[0] = pend.fused

        def timed(fn):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); fn(); e.record()
            return s, e

        for _ in range(5):
            arm_a(); arm_b()
        torch.cuda.synchronize()
        med = {"A": [], "B": []}
        for _ in range(a.rounds):
            ev = {"A": [], "B": []}
            for _ in range(a.calls):
                ev["A"].append(timed(arm_a))
                ev["B"].append(timed(arm_b))
            torch.cuda.synchronize()
            for k in ev:
                med[k].append(statistics.median(s.elapsed_time(e) * 1e3 for s, e in ev[k]))
        ma, mb = statistics.median(med["A"]), statistics.median(med["B"])
        spread = max(med["A"]) - min(med["A"])
        nk = na.shape[1] // 64
        need = sp["share_bytes"] / (nk * npl["tile_m"] / 256) if sp["late"] else float("inf")
        print(f"{name:14s} splits {tn['splits']:3d}  nt tiles {npl['tiles']} x {npl['tile_m']} rows on {npl['grid']}  late {sp['late']:3d}  "
              f"share {sp['share_bytes'] / 1024:7.1f} KiB  admitted {int(sp['admitted'])} fused {fused[0]}  constant needed {need / 1024:6.1f} KiB/K-step")
        print(f"{'':14s} A {ma:8.1f} us  (rounds {' '.join(f'{v:.1f}' for v in med['A'])}; spread {spread:.1f})   "
              f"B {mb:8.1f} us  (rounds {' '.join(f'{v:.1f}' for v in med['B'])})   B - A {mb - ma:+7.1f} us")
        if fused[0]:
            total_gap += ma - mb
    print(f"sum of the fused pairs' gaps: {total_gap:.1f} us per layer, x 12 layers = {total_gap * 12 / 1e3:.3f} ms per step")


if __name__ == "__main__":
    main()
