"""GPU: the fused Sinkhorn attention pair (csrc/nrv_sinkhorn.hip) per row at its tile, slot and walk edges against the fp64 reference
of tests/sinkhorn_edges_ref.py: 51 values of N at B = H = 2 (six edges of every NP = 32 .. 256, N <= 16, N = 1), five N at three scales
other than 0.125, and seven walk cases in which every workgroup reaches `it` = 2 (3 cus + 7 heads at N = 17, 33; ceil(2.25 cus) + 3 heads
at N = 129, 197 and, forward only, 225), every head checked.

Every call goes through the C ABI with buffers the test owns: out, lse, scal and dqkv are pre-filled with NaN between guard blocks of a
NaN payload no kernel produces (parity_tools._Out); no NaN may remain -- scal is [B, H, 7, N] with row stride N, so a row written with
stride NP leaves one -- the guards must come back bit-identical, and every case runs twice with bit-identical results.

Bounds (sinkhorn_edges_ref.check; none of them new, all of tests/test_peaked_attn_gpu.py):
  dq / dk / dv   every (batch, head, token) row within PER_ROW_BOUND = 3e-2 relative L2 of fp64; no row skipped.  The host test shows that
                 rounding at the kernels' points alone costs at most 8.3e-3 per row on these inputs (P0 resident as bf16; P7, dS and the
                 outputs in bf16), and plain emulate_bf16 5.8e-3
  o              every row within 2^-6 of the tensor's maximum (P7 and o are bf16)
  lse            1e-4 max(1, |lse|_max): fp32 from bf16 operands
  saved vectors  element-wise relative <= 1e-3: fp32 sums of N exponentials over seven compounding steps (b3 of the weak key is ~ 1e5)
  N = 1          o == v and dv == dO bit for bit; dq and dk, exactly zero in the definition, within 8 x 2 dh 2^-24 |dO| |v| scale |k or q|:
                 the one-key cancellation bound of attn_edges_ref.check, once for each of the seven normalisation steps and the softmax
                 backward, which each leave at most one fp32 rounding of G
tests/test_sinkhorn_edges_ref_host.py shows on the CPU that each of eight one-line mistakes puts a named case over these bounds, and that
a K image slot not refilled after the swap is invisible below three passes per workgroup and fails every walk case here.

Measured on an MI355X (worst error / bound over the family's cases; 79 tests in 6.7 s):
  family                                              o      dq     dk     dv     lse    saved vectors
  edges, NP 32 .. 128 (27 N; one chunk slot)           0.307  0.195  0.205  0.195  0.001  0.001
  edges, NP 160 .. 224 (18 N; second slot 32 .. 96)    0.392  0.196  0.203  0.202  0.002  0.001
  edges, NP 256 (6 N; the two-slot backward)           0.227  0.187  0.178  0.179  0.001  0.001
  scales 0.1 / 0.2 / 0.0625, 5 N                       0.322  0.190  0.213  0.225  0.002  0.001
  walk, 3 cus + 7 heads, N 17 / 33, H 1 / 5            0.361  0.277  0.229  0.221  0.001  0.001
  walk, ceil(2.25 cus) + 3 heads, N 129 / 197 / 225    0.372  0.232  0.220  0.225  0.001  0.001
  one key (N = 1): o == v and dv == dO bit for bit; dq and dk come back exactly zero (ratio 0 of the cancellation bound): with P0 = 1
  and every scaling 1 the first row step subtracts G from itself
The walk figures are, to the three digits shown, those of restated(kernel_rounding=True) on the CPU: with the same rounding points the
kernels and the restatement round the same fp32 values.
Scale refusal: before this change both entry points launched with scale <= 0 and with NaN (the row maximum is taken on the raw scores
and scaled afterwards, which is only the maximum for scale > 0); sk_check now returns NRV_ERR_SHAPE.  No other case failed before or after it,
no guard was touched, no output element stayed unwritten and every rerun was bit-identical: none of the gaps these cases close
hid a defect in the kernels.
"""
import ctypes

import pytest
import torch

import sinkhorn_edges_ref as R
from noise_robust_vit_amd import _lib
from noise_robust_vit_amd import kernels as K
from parity_tools import _Out

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
NRV_ERR_SHAPE = -2


def _st():
    return torch.cuda.current_stream().cuda_stream


def _cus(dev) -> int:
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _buffers(c, dev):
    B, N, H = c.B, c.N, c.H
    outs = {"out": _Out(B * N * H * R.DH, bf, dev), "lse": _Out(B * H * N, torch.float32, dev), "scal": _Out(B * H * 7 * N, torch.float32, dev)}
    if not c.fwd_only:
        outs["dqkv"] = _Out(B * N * 3 * H * R.DH, bf, dev)
    return outs


def _run(c, dev):
    """One forward and (unless the case is forward only) one backward of case `c` through the C ABI -> the raw outputs, on the device."""
    lib = _lib.load()
    i = R.inputs(c)
    B, N, H, scale = c.B, c.N, c.H, float(c.scale)
    qkv, dout = i["qkv"].to(dev), i["dout"].to(dev)
    outs = _buffers(c, dev)
    rc = lib.nrv_attn_sinkhorn_fwd(qkv.data_ptr(), outs["out"].ptr(), outs["lse"].ptr(), outs["scal"].ptr(), B, N, H, R.DH, scale, _st())
    assert rc == 0, rc
    if not c.fwd_only:
        rc = lib.nrv_attn_sinkhorn_bwd(qkv.data_ptr(), dout.data_ptr(), outs["lse"].ptr(), outs["scal"].ptr(), outs["dqkv"].ptr(),
                                       B, N, H, R.DH, scale, _st())
        assert rc == 0, rc
    torch.cuda.synchronize()
    return {n: o.done(f"{R.case_id(c)} {n}") for n, o in outs.items()}


def _shaped(c, raw):
    """the raw outputs in the reference's shapes"""
    B, N, H = c.B, c.N, c.H
    got = {"o": R.heads(raw["out"].cpu().double().reshape(B * N, H * R.DH), B, N, H, R.DH)[0],
           "lse": raw["lse"].cpu().double().reshape(B, H, N), "scal": raw["scal"].cpu().double().reshape(B, H, 7, N)}
    if not c.fwd_only:
        got["dq"], got["dk"], got["dv"] = R.heads(raw["dqkv"].cpu().double().reshape(B * N, 3 * H * R.DH), B, N, H, R.DH)
    return got


def _case(c, dev, ref=None, grid=None):
    raw = _run(c, dev)
    where = {}
    ratios = R.check(c, _shaped(c, raw), ref=ref, grid=grid, where=where)
    print(R.case_id(c), "error / bound", {k: f"{v:.3f}" for k, v in ratios.items()})
    if c.N == 1:
        print(R.case_id(c), "one key: |dq|, |dk| over the cancellation bound", f"{ratios['dq']:.3e}", f"{ratios['dk']:.3e}")
    assert max(ratios.values()) <= 1.0, (R.case_id(c), ratios, where)
    again = _run(c, dev)
    for n in raw:
        assert torch.equal(raw[n], again[n]), (R.case_id(c), n, "a rerun differs")
    return raw


@pytest.mark.parametrize("c", R.EDGE_CASES, ids=R.case_id)
def test_every_row_at_the_tile_and_slot_edges(dev, c):
    """Per NP = 32 k: the first N of the NP, a last key tile of padding only behind a partial and behind a full one, one real key in the
    last tile, one padding key, and N = NP; N = 1, 2, 3, 5 (wave 0 alone).  NP >= 160 fills the second chunk slot of the backward with
    32, 64, 96 and 128 queries; NP = 256 takes the two-slot backward.  Key N - 1 is twelve nats down for every query (N >= 8)."""
    _case(c, dev)


@pytest.mark.parametrize("c", R.SCALE_CASES, ids=R.case_id)
def test_every_row_at_scales_other_than_an_eighth(dev, c):
    """The forward scales the maximum of the raw scores; the backward multiplies dS by the scale.  0.1, 0.2 and 0.0625."""
    _case(c, dev)


@pytest.mark.parametrize("spec", R.WALK_SPECS, ids=R.spec_id)
def test_every_head_of_a_walk_that_reuses_its_slots(dev, spec):
    """Three passes and more per workgroup: the forward's image pair and b vector of `it & 1` are reused at it = 2, the backward's K and
    V slots have swapped twice and the K slot was refilled by the previous head.  Heads as (heads, 1) and as (ceil(heads / 5), 5)."""
    cus = _cus(dev)
    c = R.walk_case(spec, cus)
    gf, gb = R.grids(c.N, c.B * c.H, cus)
    assert gf == cus and -(-c.B * c.H // cus) >= 3
    _case(c, dev, ref=R.reference(c, device=dev), grid={"fwd": gf, "bwd": gb})


@pytest.mark.parametrize("c", R.WRAPPER_CASES, ids=R.case_id)
def test_wrappers_agree_with_the_abi_call_bit_for_bit(dev, c):
    raw = _run(c, dev)
    i = R.inputs(c)
    qkv, dout = i["qkv"].to(dev), i["dout"].to(dev)
    out, lse, scal = K.attn_sinkhorn_fwd(qkv, c.B, c.N, c.H, R.DH, c.scale)
    dqkv = K.attn_sinkhorn_bwd(qkv, dout, lse, scal, c.B, c.N, c.H, R.DH, c.scale)
    for name, t in (("out", out), ("lse", lse), ("scal", scal), ("dqkv", dqkv)):
        assert torch.equal(raw[name], t.reshape(-1)), (R.case_id(c), name)


@pytest.mark.parametrize("scale", [0.0, -0.125, float("nan")], ids=["zero", "negative", "nan"])
def test_a_scale_that_is_not_positive_is_refused_without_a_launch(dev, scale):
    lib = _lib.load()
    c = R.WRAPPER_CASES[0]
    i = R.inputs(c)
    qkv, dout = i["qkv"].to(dev), i["dout"].to(dev)
    outs = _buffers(c, dev)
    before = {n: o.raw.clone() for n, o in outs.items()}
    args = (c.B, c.N, c.H, R.DH, ctypes.c_float(scale), _st())
    assert lib.nrv_attn_sinkhorn_fwd(qkv.data_ptr(), outs["out"].ptr(), outs["lse"].ptr(), outs["scal"].ptr(), *args) == NRV_ERR_SHAPE
    assert lib.nrv_attn_sinkhorn_bwd(qkv.data_ptr(), dout.data_ptr(), outs["lse"].ptr(), outs["scal"].ptr(), outs["dqkv"].ptr(),
                                     *args) == NRV_ERR_SHAPE
    torch.cuda.synchronize()
    for n, o in outs.items():
        assert torch.equal(o.raw, before[n]), (n, "written by a refused call")
    with pytest.raises(_lib.NrvError):
        K.attn_sinkhorn_fwd(qkv, c.B, c.N, c.H, R.DH, scale)
    with pytest.raises(_lib.NrvError):
        K.attn_sinkhorn_bwd(qkv, dout, outs["lse"].t.reshape(c.B, c.H, c.N), outs["scal"].t.reshape(c.B, c.H, 7, c.N), c.B, c.N, c.H, R.DH, scale)
