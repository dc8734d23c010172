"""GPU: softmax attention per row at its tile, mask-word and batch-sum edges against the fp64 reference of tests/attn_edges_ref.py --
the nine single-pass instantiations of csrc/nrv_attn.hip in both layouts, and the streaming (KS 1..4), wide-head (KS 5, 6) and memory-key
+ bit-mask kernels of csrc/nrv_attn_gen.hip with the two-level batch sum of the shared memories' gradient.

Every call goes through the C ABI with buffers the test owns: out, lse, dqkv, the per-sample dmem and dmem_sum are pre-filled with NaN
between guard blocks of a NaN payload no kernel produces; no NaN may remain, the guards must come back bit-identical, and every case runs
twice with bit-identical results.  Bounds (tests/attn_edges_ref.check, none of them new): every o / dq / dk / dv / memory row within
PER_ROW_BOUND (3e-2) relative L2 of fp64, lse within 1e-4 max(1, |lse|_max), a fully masked row's lse exactly -FLT_MAX, a row that is
exactly zero in the definition exactly zero.  tests/test_attn_edges_ref_host.py shows that rounding at the kernels' documented points costs
at most 1.4e-2 per row on these inputs and that each of seven index mistakes puts a case over these bounds.

Measured on an MI355X (worst error / bound over the family's cases; 133 tests in 3.9 s):
  family                                   o      dq     dk     dv     memory rows   lse
  single pass, 32 N x 2 layouts            0.118  0.453  0.253  0.134  -             0.002     (both layouts bit for bit the same figures)
  streaming, KS 1..4, N 1..129 and 257     0.132  0.562  0.276  0.143  -             0.003
  wide heads, KS 5, 6                      0.101  0.512  0.194  0.120  -             0.003
  memory keys + mask, 10 shapes            0.122  0.251  0.372  0.101  0.254         0.002
  batch sum, B 16 / 17 / 35                0.119  0.310  0.745  0.139  0.255         0.001     (dk 0.745: B 17 with a mask)
  one key (N = 1): dq and dk at most 0.002 of the cancellation bound of attn_edges_ref.check; o, dv exact
No case failed, no guard was touched, every rerun was bit-identical: none of the gaps these cases close hid a defect in the kernels.
"""
import pytest
import torch

import attn_edges_ref as R
from noise_robust_vit_amd import _lib
from noise_robust_vit_amd import kernels as K
from parity_tools import _Out                 # the guarded, NaN-pre-filled output (shared with test_sinkhorn_edges_gpu.py)

pytestmark = pytest.mark.gpu
bf = torch.bfloat16


def _st():
    return torch.cuda.current_stream().cuda_stream


def _blocked(x, rows, heads, dh):
    """[rows, heads*dh] -> [heads, rows, dh] (include/nrv.h NRV_ATTN_QKV_BLOCKED / NRV_ATTN_OUT_BLOCKED), and back with _rowmajor"""
    return x.reshape(rows, heads, dh).permute(1, 0, 2).contiguous()


def _rowmajor(x, rows, heads, dh):
    return x.reshape(heads, rows, dh).permute(1, 0, 2).reshape(rows, heads * dh)


def _run(c, dev, mask_override=None):
    """One forward and one backward of case `c` -> the raw outputs (row-major, on the device)."""
    lib = _lib.load()
    i = R.inputs(c)
    B, Nq, M, H, dh, scale = c.B, c.Nq, c.M, c.H, c.dh, float(i["scale"])
    T = B * Nq
    qkv, dout = i["qkv"].to(dev), i["dout"].to(dev)
    if c.layout == R.LAYOUT_BLOCKED:
        qkv, dout = _blocked(qkv, T, 3 * H, dh), _blocked(dout, T, H, dh)
    out, lse, dqkv = _Out(T * H * dh, bf, dev), _Out(B * H * Nq, torch.float32, dev), _Out(T * 3 * H * dh, bf, dev)
    delta = torch.empty(B * H * Nq, dtype=torch.float32, device=dev)
    outs = {"out": out, "lse": lse, "dqkv": dqkv}
    if c.entry == "attn":
        rc = lib.nrv_attn_fwd(qkv.data_ptr(), out.ptr(), lse.ptr(), B, Nq, H, dh, scale, c.layout, _st())
        assert rc == 0, rc
        rc = lib.nrv_attn_bwd(qkv.data_ptr(), out.ptr(), dout.data_ptr(), lse.ptr(), dqkv.ptr(), delta.data_ptr(), B, Nq, H, dh, scale,
                              c.layout, _st())
    elif c.entry == "wide":
        rc = lib.nrv_attn_wide_fwd(qkv.data_ptr(), out.ptr(), lse.ptr(), B, Nq, H, dh, scale, _st())
        assert rc == 0, rc
        rc = lib.nrv_attn_wide_bwd(qkv.data_ptr(), out.ptr(), dout.data_ptr(), lse.ptr(), dqkv.ptr(), delta.data_ptr(), B, Nq, H, dh, scale, _st())
    else:
        mkv = i["mkv"].to(dev) if M > 0 else None
        mask = i["mask"] if mask_override is None else mask_override
        bits, bs, hs = (None, 0, 0)
        if mask is not None:
            bits, bs, hs = R.pack_bits(mask, Nq, Nq + M)
            bits = bits.to(dev)
        mptr, kptr = (mkv.data_ptr() if M > 0 else None), (bits.data_ptr() if bits is not None else None)
        mstride = 0 if c.shared else M
        rc = lib.nrv_attn_mem_fwd(qkv.data_ptr(), mptr, mstride, M, kptr, bs, hs, out.ptr(), lse.ptr(), B, Nq, H, dh, scale, _st())
        assert rc == 0, rc
        dmem = dsum = None
        if M > 0:
            dmem = outs["dmem"] = _Out(B * M * 2 * H * dh, torch.float32, dev)
            if c.shared:
                dsum = outs["dmem_sum"] = _Out(M * 2 * H * dh, torch.float32, dev)
        rc = lib.nrv_attn_mem_bwd(qkv.data_ptr(), out.ptr(), dout.data_ptr(), lse.ptr(), mptr, mstride, M, kptr, bs, hs, dqkv.ptr(),
                                  dmem.ptr() if dmem else None, dsum.ptr() if dsum else None, delta.data_ptr(), B, Nq, H, dh, scale, _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    # after a shared call the per-sample dmem is scratch (partial sums): its guards are checked, its contents are not
    raw = {n: o.done(f"{R.case_id(c)} {n}", written=not (n == "dmem" and c.shared)) for n, o in outs.items()}
    if c.layout == R.LAYOUT_BLOCKED:
        raw["out"], raw["dqkv"] = _rowmajor(raw["out"], T, H, dh), _rowmajor(raw["dqkv"], T, 3 * H, dh)
    return raw


def _shaped(c, raw):
    """the raw outputs in the reference's shapes"""
    B, Nq, M, H, dh = c.B, c.Nq, c.M, c.H, c.dh
    got = {"o": R.heads(raw["out"].cpu().double().reshape(B * Nq, H * dh), B, Nq, H, dh)[0], "lse": raw["lse"].cpu().double().reshape(B, H, Nq)}
    got["dq"], got["dk"], got["dv"] = R.heads(raw["dqkv"].cpu().double().reshape(B * Nq, 3 * H * dh), B, Nq, H, dh)
    if M > 0:
        d = raw["dmem_sum"] if c.shared else raw["dmem"]
        got["dmem_k"], got["dmem_v"] = d.cpu().double().reshape(-1, M, 2, H, dh).permute(2, 0, 3, 1, 4)
    return got


def _same(c, a, b):
    for n in a:
        if not (n == "dmem" and c.shared):
            assert torch.equal(a[n], b[n]), (R.case_id(c), n, "a rerun differs")


def _case(c, dev):
    raw = _run(c, dev)
    ratios = R.check(c, _shaped(c, raw))
    print(R.case_id(c), "error / bound", {k: f"{v:.3f}" for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, (R.case_id(c), ratios)
    _same(c, raw, _run(c, dev))
    return raw


@pytest.mark.parametrize("c", R.SINGLE_PASS_CASES, ids=R.case_id)
def test_single_pass_every_row_at_the_tile_edges(dev, c):
    """N = 16 NT (no padding), 16 NT - 15 (one real key in the last tile), 16 (NT - 1) and 16 (NT - 2) + 1 (a last tile of padding only)
    for every instantiated NT, row-major and blocked; every real key 8 nats down, so a padding key in the softmax takes the row."""
    _case(c, dev)


@pytest.mark.parametrize("c", R.STREAM_CASES, ids=R.case_id)
def test_streaming_every_row_at_the_tile_edges(dev, c):
    """KS 1..4 at N = 1, 63, 64, 65, 129 through nrv_attn_mem_* with no memory and no mask (MEM = false at any N; dh 80 | 96 | 128 take
    the prefetching dK / dV pass, dh 32 | 64 the other), and N = 257 at dh 64 through nrv_attn_*'s own dispatch."""
    _case(c, dev)


@pytest.mark.parametrize("c", R.WIDE_CASES, ids=R.case_id)
def test_wide_heads_every_row_at_the_tile_edges(dev, c):
    """KS 5, 6; width 147 stored as 152 with zero pad columns, which must come back exactly zero in o, dq, dk and dv."""
    _case(c, dev)


@pytest.mark.parametrize("c", R.MEM_CASES, ids=R.case_id)
def test_memory_keys_and_mask_every_row_at_the_word_and_tile_edges(dev, c):
    """Loud keys at bit 31 / bit 0 of a mask word and row 63 / row 0 of a key tile, masked for even queries; a fully masked query, a
    masked first and last key tile, a two-key query; every mask shape (both broadcast strides), shared and per-sample memories."""
    _case(c, dev)


@pytest.mark.parametrize("c", R.SUM_CASES, ids=R.case_id)
def test_shared_memory_gradient_summed_over_more_than_one_group(dev, c):
    """B = 16 (one full group), 17 (a remainder of one), 35 (two groups and a remainder of three): dmem_sum per row against fp64; the
    per-sample case checks every sample's rows."""
    _case(c, dev)


def test_all_true_mask_is_bit_identical_to_no_mask_at_a_batch_sum_case(dev):
    c = next(k for k in R.SUM_CASES if k.B == 17 and k.shared and k.mask is None)
    a = _run(c, dev)
    b = _run(c, dev, mask_override=torch.ones(c.Nq, c.Nq + c.M, dtype=torch.bool))
    _same(c, a, b)


@pytest.mark.parametrize("c", R.MEM_CASES[:4] + R.SUM_CASES[4:5], ids=R.case_id)
def test_device_mask_packing_is_the_host_packing(dev, c):
    m = R.inputs(c)["mask"]
    bits, bs, hs = R.pack_bits(m, c.Nq, c.Nq + c.M)
    mb = K.mask_pack(m.to(dev), c.B, c.H, c.Nq, c.Nq + c.M)
    assert (mb.bstride, mb.hstride) == (bs, hs) and torch.equal(mb.bits.cpu(), bits)
