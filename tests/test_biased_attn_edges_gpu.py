"""GPU: the shifted-window kernels (csrc/nrv_window_attn.hip) and the offset-biased kernels (csrc/nrv_bias_attn.hip) per element, per
statistic and per table entry against the fp64 restatement of biased_attn_ref.py, at the geometry edges its case lists name
(non-square windows, idle lanes, every tacc slot count, row-only and extreme shifts, partial and straddling chunks, heads 3; Nq = 1,
Nk = 256, the LDS limit, T = 1 and 256, unused and once-used table entries, arbitrary index matrices, padded strides).

Every entry point is called through the C ABI so that the test owns the buffers: outputs are pre-filled with NaN and workspaces
with 0xFF bytes (a NaN as fp32), so an element the kernel does not write fails; strided gradient buffers are filled with a NaN of a
payload no kernel produces and their gap columns must come back bit-identical.  The bounds are those of biased_attn_ref.py, shown
by tests/test_biased_attn_ref_host.py to hold for an fp32 emulation of the kernels' arithmetic on these same inputs and to
catch that emulation with any one index mistake in it."""
import pytest
import torch

import biased_attn_ref as R
from noise_robust_vit_amd import _lib
from noise_robust_vit_amd import kernels as K

pytestmark = pytest.mark.gpu
dev = "cuda"
bf = torch.bfloat16
SENTINEL = 0x7FC1          # a bf16 NaN that is not torch's (0x7FC0) nor any arithmetic's
NRV_ERR_SHAPE = -2         # include/nrv.h


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _sentinel(shape):
    return torch.full(tuple(shape), SENTINEL, dtype=torch.int16, device=dev).view(bf)


def _ws(nbytes):
    return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device=dev)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _done(rc, *outs):
    assert rc == 0, rc
    torch.cuda.synchronize()
    for o in outs:
        assert not bool(torch.isnan(o).any()), "an output element was never written"
    return outs


def _inside(r, what):
    print(what, {k: f"{v:.3f}" for k, v in r.items()})
    assert max(r.values()) <= 1.0, (what, r)


# ---- shifted-window attention ---------------------------------------------------------------------------------------------------
def _window_bwd(lib, qkv, table, dout, stats, case, robust):
    B, pH, pW, C, heads, (Wh, Ww), (sh, sw) = case
    T = (2 * Wh - 1) * (2 * Ww - 1)
    dqkv, dtable = _nan(B * pH * pW, 3 * C, dtype=bf), _nan(T, heads)
    nbytes = lib.nrv_window_attn_bwd_workspace(B, pH, pW, C, heads, Wh, Ww)
    chunks = -(-B * (pH // Wh) * (pW // Ww) // 8)
    assert nbytes == chunks * heads * T * 4
    ws = _ws(nbytes)
    _done(lib.nrv_window_attn_bwd(qkv.data_ptr(), table.data_ptr(), dout.data_ptr(), stats.data_ptr(), dqkv.data_ptr(), dtable.data_ptr(),
                                  ws.data_ptr(), ws.numel(), B, pH, pW, C, heads, Wh, Ww, sh, sw, int(robust), _st()),
          dqkv, dtable, ws[:nbytes].view(torch.float32))          # every partial of every (head, entry, chunk) is written
    return dqkv, dtable


@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("case", R.WINDOW_CASES)
def test_window_attn_every_element_statistic_and_table_entry(case, robust):
    lib = _lib.load()
    B, pH, pW, C, heads, (Wh, Ww), (sh, sw) = case
    i = R.window_inputs(case)
    qkv, table, dout = (i[n].to(dev) for n in ("qkv", "table", "dout"))
    tok = B * pH * pW
    o, stats = _nan(tok, C, dtype=bf), _nan(tok, heads, 8 if robust else 1)
    _done(lib.nrv_window_attn_fwd(qkv.data_ptr(), table.data_ptr(), o.data_ptr(), stats.data_ptr(), B, pH, pW, C, heads, Wh, Ww, sh, sw,
                                  int(robust), _st()), o, stats)
    dqkv, dtable = _window_bwd(lib, qkv, table, dout, stats, case, robust)
    ref = R.window_ref(i["qkv"], i["table"], i["dout"], *case, robust)
    _inside(R.check_window(ref, o, stats, dqkv, dtable), (case, robust))
    again = _window_bwd(lib, qkv, table, dout, stats, case, robust)
    assert torch.equal(dqkv, again[0]) and torch.equal(dtable, again[1])


# ---- offset-biased attention ----------------------------------------------------------------------------------------------------
def _bias_ops(case, qbuf, kvbuf):
    """The nine operand arguments of the ABI: (pointer, row stride, head stride) of q, k, v."""
    hs = R.bias_layout(case)["hs"]
    return [a for t, h in zip(R.bias_views(case, qbuf, kvbuf), hs) for a in (t.data_ptr(), t.stride(0), h)]


def _bias_bwd(lib, case, robust, qbuf, kvbuf, table, index, o, dact, stats):
    B, H, Nq, Nk, kd, d, T = case[:7]
    L = R.bias_layout(case)
    dqb = None if L["qshape"] is None else _sentinel(L["qshape"])
    dkvb = _sentinel(L["kvshape"])
    dtable = _nan(H, T)
    nbytes = lib.nrv_bias_attn_bwd_workspace(B, H, T)
    assert nbytes == B * H * T * 4
    ws = _ws(nbytes)
    dq, dk, dv = R.bias_views(case, dqb, dkvb)
    rc = lib.nrv_bias_attn_bwd(*_bias_ops(case, qbuf, kvbuf), table.data_ptr(), index.idx.data_ptr(), index.inv_ptr.data_ptr(),
                               index.inv_pos.data_ptr(), o.data_ptr(), dact.data_ptr(), stats.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                               dv.data_ptr(), dtable.data_ptr(), ws.data_ptr(), ws.numel(), B, H, Nq, Nk, kd, d, T, int(robust), _st())
    _done(rc, dtable, ws[:nbytes].view(torch.float32))
    for buf, written in zip((dqb, dkvb), R.bias_written(case)):
        if buf is not None:
            w = written.to(dev)
            assert not bool(torch.isnan(buf[w]).any()), "a gradient element was never written"
            assert bool((buf.view(torch.int16)[~w] == SENTINEL).all()), "a gap column was written"
    return dqb, dkvb, dtable


@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("case", R.BIAS_CASES)
def test_bias_attn_every_element_statistic_and_table_entry(case, robust):
    lib = _lib.load()
    B, H, Nq, Nk, kd, d, T = case[:7]
    i = R.bias_inputs(case)
    qbuf = None if i["qbuf"] is None else i["qbuf"].to(dev)
    kvbuf, table, dact = i["kvbuf"].to(dev), i["table"].to(dev), i["dact"].to(dev)
    index = K.bias_index(i["idx"], T, dev)
    SZ = lib.nrv_bias_attn_stats_size(Nq, Nk, int(robust))
    assert SZ == (5 * Nq + 3 * Nk if robust else Nq)
    o, ao, stats = _nan(B * Nq, H * d, dtype=bf), _nan(B * Nq, H * d, dtype=bf), _nan(B * H, SZ)
    _done(lib.nrv_bias_attn_fwd(*_bias_ops(case, qbuf, kvbuf), table.data_ptr(), index.idx.data_ptr(), o.data_ptr(), ao.data_ptr(),
                                stats.data_ptr(), B, H, Nq, Nk, kd, d, T, int(robust), _st()), o, ao, stats)
    dqb, dkvb, dtable = _bias_bwd(lib, case, robust, qbuf, kvbuf, table, index, o, dact, stats)
    hs = i["hs"]
    q, k, v = R.bias_views(case, i["qbuf"], i["kvbuf"])
    ref = R.bias_ref(q, k, v, hs, i["table"], i["idx"], i["dact"], o.cpu(), B, H, Nq, Nk, kd, d, robust)
    dq, dk, dv = R.bias_views(case, None if dqb is None else dqb.cpu(), dkvb.cpu())
    got = {"dq": R.bias_heads(dq, B, Nq, H, hs[0], kd), "dk": R.bias_heads(dk, B, Nk, H, hs[1], kd), "dv": R.bias_heads(dv, B, Nk, H, hs[2], d)}
    _inside(R.check_bias(ref, Nq, Nk, o, ao, stats, dtable=dtable, **got), (case, robust))
    if case[9] == "holes":
        assert bool((dtable[:, R.HOLE_UNUSED] == 0).all())                          # an empty list: exactly 0
    a_q, a_kv, a_t = _bias_bwd(lib, case, robust, qbuf, kvbuf, table, index, o, dact, stats)
    assert torch.equal(dkvb.view(torch.int16), a_kv.view(torch.int16)) and torch.equal(dtable, a_t)
    assert dqb is None or torch.equal(dqb.view(torch.int16), a_q.view(torch.int16))


@pytest.mark.parametrize("B,H,Nq,Nk,kd,d,T", R.BIAS_REFUSED)
def test_bias_attn_refuses_one_row_past_the_lds_limit(B, H, Nq, Nk, kd, d, T):
    """154 x 256 and 199 x 199 need more than 160 KiB of LDS: NRV_ERR_SHAPE from both directions, and nothing written."""
    lib = _lib.load()
    case = (B, H, Nq, Nk, kd, d, T, "sep", (0, 0), "rand")
    L = R.bias_layout(case)
    qbuf, kvbuf = torch.zeros(L["qshape"], dtype=bf, device=dev), torch.zeros(L["kvshape"], dtype=bf, device=dev)
    table = torch.zeros(H, T, device=dev)
    index = K.bias_index(torch.zeros(Nq, Nk, dtype=torch.int64), T, dev)
    for robust in (0, 1):
        SZ = lib.nrv_bias_attn_stats_size(Nq, Nk, robust)
        o, ao, stats = _nan(B * Nq, H * d, dtype=bf), _nan(B * Nq, H * d, dtype=bf), _nan(B * H, SZ)
        rc = lib.nrv_bias_attn_fwd(*_bias_ops(case, qbuf, kvbuf), table.data_ptr(), index.idx.data_ptr(), o.data_ptr(), ao.data_ptr(),
                                   stats.data_ptr(), B, H, Nq, Nk, kd, d, T, robust, _st())
        assert rc == NRV_ERR_SHAPE
        dqb, dkvb, dtable = _sentinel(L["qshape"]), _sentinel(L["kvshape"]), _nan(H, T)
        ws = _ws(lib.nrv_bias_attn_bwd_workspace(B, H, T))
        dq, dk, dv = R.bias_views(case, dqb, dkvb)
        zo, zs = torch.zeros_like(o), torch.zeros_like(stats)
        rc = lib.nrv_bias_attn_bwd(*_bias_ops(case, qbuf, kvbuf), table.data_ptr(), index.idx.data_ptr(), index.inv_ptr.data_ptr(),
                                   index.inv_pos.data_ptr(), zo.data_ptr(), zo.data_ptr(), zs.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                                   dv.data_ptr(), dtable.data_ptr(), ws.data_ptr(), ws.numel(), B, H, Nq, Nk, kd, d, T, robust, _st())
        assert rc == NRV_ERR_SHAPE
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in (o, ao, stats, dtable)) and bool((ws == 0xFF).all())
        assert bool((dqb.view(torch.int16) == SENTINEL).all()) and bool((dkvb.view(torch.int16) == SENTINEL).all())
