#!/usr/bin/env python3
"""Launches for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/attn_mem_profile.py): the memory / mask
attention forward and backward (nrv_attn_mem_*) against nrv_attn_fwd / nrv_attn_bwd at N = 197 (ViT-B/16: B 256, H 12, dh 64;
the single-pass kernels) with M = 0 and with M = 10 plus the Adapter mask, and at N = 300 (which nrv_attn_fwd takes to the
streaming kernels of nrv_attn_gen.hip) with M = 0.  nrv_attn_mem_* run the MEM = false instantiation of those streaming
kernels when M = 0 and there is no mask, the MEM = true one otherwise."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from noise_robust_vit_amd import kernels as K  # noqa: E402


def main(reps: int = 20):
    dev = torch.device("cuda:0")
    B, N, H, dh, M = 256, 197, 12, 64, 10
    sc = dh ** -0.5
    qkv = (torch.randn(B * N, 3 * H * dh, device=dev) * 0.5).to(torch.bfloat16)
    dout = torch.randn(B * N, H * dh, device=dev).to(torch.bfloat16)
    mkv = (torch.randn(M, 2 * H * dh, device=dev) * 0.5).to(torch.bfloat16)
    mask = torch.zeros(N, N + M, dtype=torch.bool, device=dev)
    mask[0] = True
    mask[1:, 1:N] = True
    bits = K.mask_pack(mask, B, H, N, N + M)
    N2 = 300
    qkv2 = (torch.randn(B * N2, 3 * H * dh, device=dev) * 0.5).to(torch.bfloat16)
    dout2 = torch.randn(B * N2, H * dh, device=dev).to(torch.bfloat16)
    for _ in range(reps):
        o, l = K.attn_fwd(qkv, B, N, H, dh, sc)
        K.attn_bwd(qkv, o, dout, l, B, N, H, dh, sc)
        o, l = K.attn_fwd(qkv2, B, N2, H, dh, sc)                  # streaming kernels
        K.attn_bwd(qkv2, o, dout2, l, B, N2, H, dh, sc)
        o, l = K.attn_mem_fwd(qkv2, None, B, N2, 0, H, dh, sc)
        K.attn_mem_bwd(qkv2, o, dout2, l, None, B, N2, 0, H, dh, sc)
        o, l = K.attn_mem_fwd(qkv, None, B, N, 0, H, dh, sc)
        K.attn_mem_bwd(qkv, o, dout, l, None, B, N, 0, H, dh, sc)
        o, l = K.attn_mem_fwd(qkv, mkv, B, N, M, H, dh, sc, True, bits)
        K.attn_mem_bwd(qkv, o, dout, l, mkv, B, N, M, H, dh, sc, True, bits)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
