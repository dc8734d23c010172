"""GPU: attention-weight dropout inside the fused softmax attention kernels (nrv_attn_drop_*) against tests/attn_drop_ref.py -- the
exported mask bit for bit against the numpy restatement, every case per row against fp64 with the restated mask, the three probes that
decode each kernel's own mask exactly, T = 0 against the plain entries and the fused result against the composed path fed the exported
mask.

Every call goes through the C ABI into NaN-pre-filled buffers between guard blocks (parity_tools._Out).  Bounds, none of them new:
o / dq / dk / dv rows within PER_ROW_BOUND (3e-2) relative L2 of fp64, lse within LSE_TOL and bit-identical to nrv_attn_fwd's, rows
with no kept key exactly zero, a rerun bit-identical.  tests/test_attn_drop_ref_host.py shows that rounding at the kernels' points
costs at most 0.9e-2 per row on these inputs and that each of seven mistakes is seen.

Measured on an MI355X (worst error / bound over the family's cases; 126 tests in 3.8 s):
  family                               o      dq     dk     dv     lse
  single pass, 32 N (nine tile counts) 0.124  0.296  0.187  0.136  0.002
  streaming, KS 1..4, N 1..300         0.147  0.220  0.165  0.144  0.001
  one key (N = 1, p = 0.5): dq and dk at most 0.001 of the cancellation bound; o, dv exact
Every probe decoded each kernel's mask bit for bit, every rerun was bit-identical, T = 0 matched the plain entries bit for bit, and
the fused result lay within 5.9e-3 per row of the composed path fed the exported mask (N 197 and 300)."""
import numpy as np
import pytest
import torch

import attn_drop_ref as R
from noise_robust_vit_amd import _lib
from noise_robust_vit_amd import kernels as K
from parity_tools import _Out

pytestmark = pytest.mark.gpu
bf = torch.bfloat16


def _st():
    return torch.cuda.current_stream().cuda_stream


def _seed(seed: int, dev):
    return torch.tensor([seed - (1 << 64) if seed >= (1 << 63) else seed], dtype=torch.int64, device=dev)


def _run(c, dev, qkv=None, dout=None, p=None, plain=False):
    """One forward and one backward through the C ABI -> raw out, lse, dqkv on the device"""
    lib = _lib.load()
    i = R.inputs(c)
    qkv = (i["qkv"] if qkv is None else qkv).to(dev)
    dout = (i["dout"] if dout is None else dout).to(dev)
    p = c.p if p is None else p
    B, N, H, dh, scale = c.B, c.N, c.H, c.dh, float(c.dh ** -0.5)
    T = B * N
    out, lse, dqkv = _Out(T * H * dh, bf, dev), _Out(B * H * N, torch.float32, dev), _Out(T * 3 * H * dh, bf, dev)
    delta = torch.empty(B * H * N, dtype=torch.float32, device=dev)
    seed = _seed(c.seed, dev)
    if plain:
        rc = lib.nrv_attn_fwd(qkv.data_ptr(), out.ptr(), lse.ptr(), B, N, H, dh, scale, 0, _st())
        assert rc == 0, rc
        rc = lib.nrv_attn_bwd(qkv.data_ptr(), out.ptr(), dout.data_ptr(), lse.ptr(), dqkv.ptr(), delta.data_ptr(), B, N, H, dh, scale, 0, _st())
    else:
        rc = lib.nrv_attn_drop_fwd(qkv.data_ptr(), out.ptr(), lse.ptr(), seed.data_ptr(), p, B, N, H, dh, scale, _st())
        assert rc == 0, rc
        rc = lib.nrv_attn_drop_bwd(qkv.data_ptr(), out.ptr(), dout.data_ptr(), lse.ptr(), dqkv.ptr(), delta.data_ptr(), seed.data_ptr(),
                                   p, B, N, H, dh, scale, _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {n: o.done(f"{R.case_id(c)} {n}") for n, o in (("out", out), ("lse", lse), ("dqkv", dqkv))}


def _shaped(c, raw):
    B, N, H, dh = c.B, c.N, c.H, c.dh
    got = {"o": R.heads(raw["out"].cpu().double().reshape(B * N, H * dh), B, N, H, dh)[0], "lse": raw["lse"].cpu().double().reshape(B, H, N)}
    got["dq"], got["dk"], got["dv"] = R.heads(raw["dqkv"].cpu().double().reshape(B * N, 3 * H * dh), B, N, H, dh)
    return got


@pytest.mark.parametrize("B,H,N,p", [(2, 3, 257, 0.1), (1, 2, 40, 0.5), (3, 1, 64, 0.9)])
def test_exported_mask_is_the_numpy_restatement(dev, B, H, N, p):
    for seed in (R.BASE_SEED, R.BASE_SEED ^ (1 << 40), 0xFEDCBA9876543210):          # the first two differ in the upper word only
        got = K.attn_drop_mask(_seed(seed, dev), p, B, H, N).cpu().numpy()
        want = R.keep_mask(seed, p, B, H, N)
        assert set(np.unique(got)) <= {0, 1}
        assert np.array_equal(got.astype(bool), want), (seed, int((got.astype(bool) != want).sum()))
    assert K.attn_drop_peff(p) == R.p_eff(p)


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_every_row_against_fp64_with_the_restated_mask(dev, c):
    raw = _run(c, dev)
    got, ref = _shaped(c, raw), R.reference(c)
    ratios = R.check(c, got, ref)
    print(R.case_id(c), "error / bound", {k: f"{v:.3f}" for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, (R.case_id(c), ratios)
    none = ref["none"]
    assert bool((got["o"][none] == 0).all()) and bool((got["dq"][none] == 0).all())
    again = _run(c, dev)
    for n in raw:
        assert torch.equal(raw[n], again[n]), (R.case_id(c), n, "a rerun differs")
    assert torch.equal(raw["lse"], _run(c, dev, plain=True)["lse"]), "lse is not the undropped row's, bit for bit"


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_probes_decode_each_kernels_mask_exactly(dev, c):
    def run(qkv, dout):
        got = _shaped(c, _run(c, dev, qkv, dout))
        return {n: got[n] for n in ("o", "dq", "dv")}
    dec = R.probe_decode(c, run)
    m = R.case_mask(c)
    for n in ("fwd", "dv", "dq"):
        assert torch.equal(dec[n], m), (R.case_id(c), n, int((dec[n] != m).sum()), "decisions differ")


@pytest.mark.parametrize("c", [k for k in R.CASES if k.N in (17, 208, 300) or (k.N == 129 and k.dh in (32, 128))], ids=R.case_id)
def test_threshold_zero_is_the_plain_entry_bit_for_bit(dev, c):
    a, b = _run(c, dev, p=1e-6), _run(c, dev, plain=True)
    for n in a:
        assert torch.equal(a[n], b[n]), (R.case_id(c), n)


@pytest.mark.parametrize("B,N,H,dh", [(2, 197, 2, 64), (2, 300, 2, 64)])
def test_fused_agrees_with_the_composed_path_fed_the_exported_mask(dev, B, N, H, dh):
    p, scale = 0.1, dh ** -0.5
    g = torch.Generator().manual_seed(7 + N)
    qkv = torch.randn(B * N, 3 * H * dh, generator=g).to(bf).to(dev)
    dout = torch.randn(B * N, H * dh, generator=g).to(bf).to(dev)
    seed = _seed(R.BASE_SEED + N, dev)
    keep = K.attn_drop_mask(seed, p, B, H, N)
    rs = 1.0 / (1.0 - K.attn_drop_peff(p))
    o, lse = K.attn_drop_fwd(qkv, seed, p, B, N, H, dh, scale)
    dqkv = K.attn_drop_bwd(qkv, o, dout, lse, seed, p, B, N, H, dh, scale)
    oc, cs = K.attn_composed_fwd(qkv, B, N, H, dh, scale, 0, keep, rs)
    dqkvc = K.attn_composed_bwd(qkv, dout, cs, B, N, H, dh, scale)
    torch.cuda.synchronize()
    worst = {}
    a = R.heads(o.cpu().double(), B, N, H, dh)[0], R.heads(oc.cpu().double().reshape(B * N, H * dh), B, N, H, dh)[0]
    worst["o"] = R.per_row_rel(*a).max().item()
    for name, x, y in zip(("dq", "dk", "dv"), R.heads(dqkv.cpu().double(), B, N, H, dh),
                          R.heads(dqkvc.cpu().double().reshape(B * N, 3 * H * dh), B, N, H, dh)):
        worst[name] = R.per_row_rel(x, y).max().item()
    print(f"N {N}: fused against composed, worst row", {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= R.PER_ROW_BOUND, worst
