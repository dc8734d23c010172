"""ctypes binding of libnrv_hip.so (the C ABI declared in include/nrv.h).

The library is the product: there is NO fallback.  If it cannot be loaded, or a call returns a
non-zero code, a RuntimeError is raised -- nothing here ever routes through PyTorch eager maths or
the CPU oracle.
"""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import c_char_p, c_float, c_int, c_int64, c_size_t, c_void_p, c_double

_HERE = os.path.dirname(os.path.abspath(__file__))
_DEFAULT_LIB = os.path.join(_HERE, "lib", "libnrv_hip.so")
LIB_PATH = _DEFAULT_LIB       # no environment override: what runs is the in-tree library (tools/_devlib.py swaps it for A/B runs)

NRV_F32, NRV_BF16, NRV_U8 = 0, 1, 2
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESIDUAL, EPI_DGELU, EPI_BIAS_GELU_Q8, EPI_DGELU_Q8 = 0, 1, 2, 3, 4, 5, 6
PATCH_P1P2C, PATCH_CP1P2 = 0, 1
ABI_VERSION = 19
ATTN_QKV_BLOCKED, ATTN_OUT_BLOCKED = 1, 2      # include/nrv.h: NRV_ATTN_*_BLOCKED
CONV_NCHW, CONV_NHWC = 0, 1                    # include/nrv.h: NRV_CONV_*
SPLIT_NCHW, SPLIT_ROWS = 0, 1                  # include/nrv.h: NRV_SPLIT_*



class TnProblem(ctypes.Structure):
    """include/nrv.h `nrv_tn_problem`: one weight gradient of a grouped launch."""
    _fields_ = [("A", c_void_p), ("lda", c_int64), ("B", c_void_p), ("ldb", c_int64), ("C", c_void_p), ("ldc", c_int64),
                ("M", c_int64), ("N", c_int64), ("beta", c_float), ("dbias", c_void_p), ("dbias_beta", c_float)]

class NtPlan(ctypes.Structure):
    """include/nrv.h `nrv_nt_plan`: what nrv_gemm_nt_bf16 would launch."""
    _fields_ = [("tile_m", c_int), ("tile_n", c_int), ("phased", c_int), ("tiles", c_int), ("grid", c_int)]


class TnPlan(ctypes.Structure):
    """include/nrv.h `nrv_tn_plan`: what nrv_gemm_tn_bf16 would launch."""
    _fields_ = [("tiles", c_int), ("splits", c_int), ("kt_q", c_int), ("kt_r", c_int), ("phased", c_int), ("direct", c_int),
                ("reduce", c_int)]

class ReduceJob(ctypes.Structure):
    """include/nrv.h `nrv_reduce_job`: the reduction a deferred weight-gradient launch leaves behind."""
    _fields_ = [("slabs", c_void_p), ("slab_stride", c_int64), ("C", c_void_p), ("ldc", c_int64),
                ("bias_ws", c_void_p), ("dbias", c_void_p), ("M", c_int64), ("N", c_int64),
                ("splits", c_int), ("beta", c_float), ("dbias_beta", c_float), ("pending", c_int)]


class NtSidePlan(ctypes.Structure):
    """include/nrv.h `nrv_nt_side_plan`: the shares a side job would be cut into, and whether nrv_gemm_nt_bf16_side takes it."""
    _fields_ = [("late", c_int), ("admitted", c_int), ("share_bytes", c_int64)]


class BgemmPlan(ctypes.Structure):
    """include/nrv.h `nrv_bgemm_plan_t`: what nrv_bgemm would launch."""
    _fields_ = [("a_vec", c_int), ("b_vec", c_int), ("c_vec", c_int), ("tiles_m", c_int), ("tiles_n", c_int),
                ("blocks", ctypes.c_longlong)]


class SubattnPlan(ctypes.Structure):
    """include/nrv.h `nrv_subattn_plan_t`: how nrv_subattn_fwd / _bwd split the query rows and pad the keys."""
    _fields_ = [("chunk", c_int), ("chunks", c_int), ("nk_pad", c_int)]


# name -> (restype, argtypes); every symbol include/nrv.h declares (tests/test_abi.py checks the two agree)
SIGNATURES = {
    "nrv_abi_version": (c_int, []),
    "nrv_error_string": (c_char_p, [c_int]),
    "nrv_layernorm_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_int64, c_int, c_float, c_void_p]),
    "nrv_layernorm_bwd_workspace": (c_size_t, [c_int64, c_int]),
    "nrv_layernorm_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                  c_void_p, c_size_t, c_int64, c_int, c_void_p]),
    "nrv_gemm_nt_bf16": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int, c_int64,
                                 c_int64, c_int64, c_int64, c_int, c_void_p,
                                 c_void_p, c_int, c_int64, c_int64, c_void_p, c_int64,
                                 c_int64, c_int64, c_int64, c_void_p]),
    "nrv_gemm_tn_workspace": (c_size_t, [c_int64, c_int64, c_int64]),
    "nrv_gemm_nt_plan": (c_int, [c_int64, c_int64, c_int64, c_int, c_int, c_void_p]),
    "nrv_gemm_tn_plan": (c_int, [c_int64, c_int64, c_int64, c_int, c_float, c_int, c_void_p]),
    "nrv_gemm_tn_bf16": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                 c_int64, c_int64, c_int64, c_float, c_int64, c_int64, c_int64,
                                 c_void_p, c_float, c_void_p, c_size_t, c_void_p]),
    "nrv_gemm_tn_bf16_deferred": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                          c_int64, c_int64, c_int64, c_float, c_int64, c_int64, c_int64,
                                          c_void_p, c_float, c_void_p, c_size_t, c_void_p, c_void_p]),
    "nrv_splitk_reduce": (c_int, [c_void_p, c_void_p]),
    "nrv_gemm_nt_bf16_side": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int, c_int64,
                                      c_int64, c_int64, c_int64, c_int, c_void_p,
                                      c_void_p, c_int, c_int64, c_int64, c_void_p, c_int64,
                                      c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "nrv_gemm_nt_side_plan": (c_int, [c_int64, c_int64, c_int64, c_int, c_int, c_int64, c_void_p]),
    "nrv_gemm_tn_grouped_workspace": (c_size_t, [c_void_p, c_int, c_int64]),
    "nrv_gemm_tn_grouped_bf16": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_size_t, c_void_p]),
    "nrv_colsum_workspace": (c_size_t, [c_int64, c_int64]),
    "nrv_colsum_bf16": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_float, c_void_p, c_size_t, c_void_p]),
    "nrv_attn_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_void_p]),
    "nrv_attn_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_int, c_int, c_int, c_int, c_float, c_int, c_void_p]),
    "nrv_attn_drop_threshold": (c_int, [c_float]),
    "nrv_attn_drop_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "nrv_attn_drop_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                  c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "nrv_attn_drop_mask": (c_int, [c_void_p, c_float, c_void_p, c_int, c_int, c_int, c_void_p]),
    "nrv_attn_probs": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_void_p]),
    "nrv_attn_mem_fwd": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_int64,
                                 c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "nrv_attn_mem_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_int64,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "nrv_mask_pack_bits": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "nrv_attn_sinkhorn_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "nrv_attn_sinkhorn_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "nrv_window_attn_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                    c_int, c_int, c_int, c_void_p]),
    "nrv_window_attn_bwd_workspace": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "nrv_window_attn_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                    c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_sd_add_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int64, c_int64, c_int, c_void_p]),
    "nrv_sd_scale_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_int64, c_int64, c_int, c_void_p]),
    "nrv_patch_unfold": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_cast_transpose": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "nrv_cast_transpose_batched": (c_int, [c_void_p, c_int, c_int64, c_void_p]),
    "nrv_cast_f32_bf16": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "nrv_dropout_add_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int64, c_void_p]),
    "nrv_mask_mul_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_int64, c_void_p]),
    "nrv_mask_mul_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_int64, c_void_p]),
    "nrv_gather_rows_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p]),
    "nrv_scatter_rows_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p]),
    "nrv_sumsq_workspace": (c_size_t, [c_int64]),
    "nrv_sumsq_f32": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "nrv_adamw_f32": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int64,
                              c_double, c_double, c_double, c_double, c_double, c_int, c_void_p, c_float, c_void_p, c_void_p]),
    "nrv_bn_workspace": (c_size_t, [c_int64, c_int]),
    "nrv_bn_stats": (c_int, [c_void_p, c_int64, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_size_t, c_void_p]),
    "nrv_bn_apply": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_int,
                             c_void_p, c_void_p, c_float, c_int64, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "nrv_bn_bwd": (c_int, [c_void_p, c_int, c_int, c_void_p, c_float, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_float,
                           c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int64, c_int, c_void_p]),
    "nrv_conv_unfold": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_conv_fold": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_bias_attn_stats_size": (c_size_t, [c_int, c_int, c_int]),
    "nrv_bias_attn_fwd": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int64, c_int, c_void_p, c_int64, c_int, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_bias_attn_bwd_workspace": (c_size_t, [c_int, c_int, c_int]),
    "nrv_bias_attn_bwd": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int64, c_int, c_void_p, c_int64, c_int, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_size_t, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_dwconv3x3_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_dwconv3x3_bwd_workspace": (c_size_t, [c_int, c_int, c_int, c_int]),
    "nrv_dwconv3x3_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_se_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "nrv_se_apply": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "nrv_se_bwd_workspace": (c_size_t, [c_int, c_int, c_int]),
    "nrv_se_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_void_p]),
    "nrv_ls_add_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int64, c_int64, c_int, c_void_p]),
    "nrv_ls_bwd_workspace": (c_size_t, [c_int64, c_int]),
    "nrv_ls_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_int64, c_int64,
                           c_int, c_void_p]),
    "nrv_dgelu_rows": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_int, c_void_p]),
    "nrv_cls_attn_fwd": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                 c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "nrv_cls_attn_bwd": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                 c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "nrv_sinkhorn_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    "nrv_sinkhorn_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    "nrv_th_softmax_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_th_softmax_bwd_workspace": (c_size_t, [c_int, c_int, c_int, c_int]),
    "nrv_th_softmax_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                   c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_head_mix_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_head_mix_bwd_workspace": (c_size_t, [c_int, c_int, c_int, c_int]),
    "nrv_head_mix_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_int,
                                 c_void_p]),
    "nrv_reattn_softmax_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                       c_float, c_void_p]),
    "nrv_reattn_softmax_bwd_workspace": (c_size_t, [c_int, c_int, c_int, c_int]),
    "nrv_reattn_softmax_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_size_t, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "nrv_reattn_norm_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                                    c_void_p]),
    "nrv_reattn_norm_bwd_workspace": (c_size_t, [c_int, c_int, c_int, c_int]),
    "nrv_reattn_norm_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_size_t, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "nrv_soft_split_fwd": (c_int, [c_void_p, c_int, c_int, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_soft_split_bwd": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_layernorm_pad_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_int64, c_int, c_int64, c_float, c_void_p]),
    "nrv_layernorm_pad_bwd_workspace": (c_size_t, [c_int64, c_int]),
    "nrv_layernorm_pad_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_int64, c_int, c_int64, c_void_p]),
    "nrv_attn_wide_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "nrv_attn_wide_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float,
                                  c_void_p]),
    "nrv_bgemm": (c_int, [c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64,
                          c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "nrv_bgemm_plan": (c_int, [c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64,
                               c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_rotary_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_rotary_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_dwconv_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_dwconv_bwd_workspace": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "nrv_dwconv_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_int,
                               c_int, c_int, c_void_p]),
    "nrv_geglu_fwd": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p]),
    "nrv_geglu_bwd": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "nrv_pool_dwconv_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_pool_dwconv_bwd_workspace": (c_size_t, [c_int, c_int, c_int, c_int]),
    "nrv_pool_dwconv_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int,
                                    c_int, c_int, c_int, c_void_p]),
    "nrv_unfold_patches": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_relu_maxpool_fwd": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                     c_void_p]),
    "nrv_relu_maxpool_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_layernorm_f32_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float,
                                      c_void_p]),
    "nrv_layernorm_f32_bwd_workspace": (c_size_t, [c_int64, c_int]),
    "nrv_layernorm_f32_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_size_t, c_int64, c_int, c_void_p]),
    "nrv_seqpool_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "nrv_seqpool_bwd_workspace": (c_size_t, [c_int, c_int]),
    "nrv_seqpool_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int,
                                c_int, c_void_p]),
    "nrv_subattn_plan": (c_int, [c_int, c_int, c_int, c_void_p]),
    "nrv_subattn_fwd": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                c_int, c_float, c_void_p]),
    "nrv_subattn_bwd_workspace": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "nrv_subattn_bwd": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_size_t, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "nrv_peg_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nrv_peg_bwd_workspace": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "nrv_peg_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_int,
                            c_int, c_void_p]),
    "nrv_set_reserved_cus": (c_int, [c_int]),
    "nrv_probe": (c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p]),
}

_lock = threading.Lock()
_lib = None


class NrvError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load libnrv_hip.so once; raise loudly if it is missing (run `python -m noise_robust_vit_amd.build`)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH) and LIB_PATH == _DEFAULT_LIB:
            # the in-tree library is a build product (git-ignored): compile it if the toolchain is here.  This is
            # the same HIP code path, not a fallback; without hipcc the error below is raised.
            try:
                from . import build as _build
                _build.build()
            except Exception as e:        # noqa: BLE001 -- reported below
                raise NrvError(f"{LIB_PATH} is missing and building it failed ({e}); the HIP kernels are the product "
                               "and there is no fallback path") from e
        if not os.path.exists(LIB_PATH):
            raise NrvError(
                f"{LIB_PATH} not found: the HIP kernels are the product and there is no fallback path. "
                "Build them with `python -m noise_robust_vit_amd.build` (needs hipcc, gfx950 target).")
        _lib = bind(LIB_PATH)
    return _lib


def bind(path: str) -> ctypes.CDLL:
    """dlopen `path` and set the prototype of every symbol include/nrv.h declares."""
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    got = lib.nrv_abi_version()
    if got != ABI_VERSION:
        raise NrvError(f"{path}: ABI version {got} != binding version {ABI_VERSION}; rebuild the library")
    return lib


def check(code: int, what: str) -> None:
    if code != 0:
        msg = load().nrv_error_string(code)
        raise NrvError(f"{what} failed with code {code}: {msg.decode() if msg else '?'}")
