"""GPU: the PatchConvNet kernels (csrc/nrv_pcn.hip, ABI 17) per element, per channel and per key row against the fp64 restatements of
pcn_ref.py, at the smallest shapes that reach their tiling edges (the case lists and what each reaches are in pcn_ref.py).

Every entry point is called through the C ABI with its outputs pre-filled with NaN: an element the kernel does not write fails
the bound, and gap columns of strided operands must still hold the sentinel afterwards.  The bounds are those of pcn_ref.py, each
one shown by tests/test_pcn_ref_host.py to hold for an fp32 emulation of the kernel's arithmetic on these same inputs."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import pcn_ref as PR
from noise_robust_vit_amd import _lib
from noise_robust_vit_amd import kernels as K

pytestmark = pytest.mark.gpu
dev = "cuda"
bf = torch.bfloat16
NAN16 = 0x7FC0          # torch.full(nan, bf16)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _ws(nbytes):
    return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device=dev)          # 0xFFFFFFFF is a NaN too


def _st():
    return torch.cuda.current_stream().cuda_stream


def _done(rc, *outs):
    assert rc == 0, rc
    torch.cuda.synchronize()
    for o in outs:
        if o is not None:
            assert not bool(torch.isnan(o).any()), "an output element was never written"
    return outs


def _d(i, *names):
    return [None if i[n] is None else i[n].to(dev) for n in names]


def _inside(r, what):
    print(what, {k: f"{v:.3f}" for k, v in r.items()})
    assert max(r.values()) <= 1.0, (what, r)


# ---- depthwise 3x3 --------------------------------------------------------------------------------------------------------------
def _dw_bwd(lib, t, gs, gdt, B, H, W, C):
    a, w, bias, dg, s, dmean = t
    da, dw, db = _nan(B * H * W, C, dtype=bf), _nan(C, 9), _nan(C)
    ws = _ws(lib.nrv_dwconv3x3_bwd_workspace(B, H, W, C))
    return _done(lib.nrv_dwconv3x3_bwd(a.data_ptr(), w.data_ptr(), bias.data_ptr(), dg.data_ptr(), s.data_ptr(), dmean.data_ptr(),
                                       K._ptr(gs), gdt, da.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(),
                                       B, H, W, C, _st()), da, dw, db)


@pytest.mark.parametrize("B,H,W,C", PR.DW_CASES + PR.DW_Q8_ONLY)
def test_dwconv_every_token_channel_and_tap(B, H, W, C):
    lib = _lib.load()
    i = PR.dw_inputs(B, H, W, C)
    t = _d(i, "a", "w", "bias", "dg", "s", "dmean")
    n = B * H * W
    d, sq = _nan(n, C, dtype=bf), _nan(B, C)
    _done(lib.nrv_dwconv3x3_fwd(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), d.data_ptr(), sq.data_ptr(), B, H, W, C, _st()), d, sq)
    _inside(PR.check_dw_fwd(PR.dwconv_fwd(i["a"], i["w"], i["bias"], B, H, W), d, sq), ("fwd", B, H, W, C))
    ref = PR.dwconv_bwd(i["a"], i["w"], i["bias"], i["dg"], i["s"], i["dmean"], B, H, W)
    streams = [("none", None, _lib.NRV_BF16, None), ("bf16", i["g16"].to(dev), _lib.NRV_BF16, i["g16"].double())]
    if C % 64 == 0:
        assert i["g8"].numel() == (n + 1) // 2 * 2 * C
        streams.append(("q8", i["g8"].to(dev), _lib.NRV_U8, PR.q8_unpack(i["g8"], n, C)))
    for name, gs, gdt, factor in streams:
        out = _dw_bwd(lib, t, gs, gdt, B, H, W, C)
        _inside(PR.check_dw_bwd(ref, factor, *out), (name, B, H, W, C))
    again = _dw_bwd(lib, t, streams[-1][1], streams[-1][2], B, H, W, C)
    assert all(torch.equal(x, y) for x, y in zip(out, again))


# ---- squeeze-and-excitation -----------------------------------------------------------------------------------------------------
def _se_bwd(lib, t, s, hid, B, C, rd, HW):
    dg, d, sq, wr, we = t
    outs = _nan(B, C), _nan(rd, C), _nan(rd), _nan(C, rd), _nan(C)
    ws = _ws(lib.nrv_se_bwd_workspace(B, C, rd))
    _done(lib.nrv_se_bwd(dg.data_ptr(), d.data_ptr(), sq.data_ptr(), HW, s.data_ptr(), hid.data_ptr(), wr.data_ptr(), we.data_ptr(),
                         *(o.data_ptr() for o in outs), ws.data_ptr(), ws.numel(), B, C, rd, _st()), *outs)
    return outs, ws


@pytest.mark.parametrize("B,C,rd,HW", PR.SE_CASES)
def test_se_every_entry(B, C, rd, HW):
    lib = _lib.load()
    i = PR.se_inputs(B, C, rd, HW)
    pre = i["ref"]["pre"]
    assert float(pre.abs().min()) >= PR.SE_MIN_PRE and bool((pre > 0).any()) and bool((pre < 0).any())      # the relu mask is unambiguous
    sq, wr, br, we, be, d, dg, s32, hid32 = _d(i, "sq", "wr", "br", "we", "be", "d", "dg", "s32", "hid32")
    hid, s = _nan(B, rd), _nan(B, C)
    _done(lib.nrv_se_fwd(sq.data_ptr(), HW, wr.data_ptr(), br.data_ptr(), we.data_ptr(), be.data_ptr(), hid.data_ptr(), s.data_ptr(),
                         B, C, rd, _st()), hid, s)
    _inside(PR.check_se_fwd(i["ref"], s, hid), ("se_fwd", B, C, rd, HW))
    g = _nan(B * HW, C, dtype=bf)
    _done(lib.nrv_se_apply(d.data_ptr(), s.data_ptr(), g.data_ptr(), B, HW, C, _st()), g)
    assert torch.equal(g, PR.se_apply_bits(d, s, HW))                                # one fp32 product: bit for bit
    # the backward on the reference's own s and hid (rounded to fp32), so that its bounds do not inherit the forward's error
    ref = PR.se_bwd(i["dg"], i["d"], i["sq"], HW, i["s32"], i["hid32"], i["wr"], i["we"])
    outs, ws = _se_bwd(lib, (dg, d, sq, wr, we), s32, hid32, B, C, rd, HW)
    _inside(PR.check_se_bwd(ref, *outs), ("se_bwd", B, C, rd, HW))
    work = ws[:(2 * B * C + B * rd) * 4].view(torch.float32)                          # ds | dz | dp (nrv_pcn.hip)
    assert not bool(torch.isnan(work).any())
    dp = work[2 * B * C:].reshape(B, rd)
    assert bool((hid32 == 0).any()) and bool((dp[hid32 == 0] == 0).all()) and bool((dp[hid32 > 0] != 0).all())
    dead = (hid32 == 0).all(0)
    assert bool((outs[2][dead] == 0).all()) and bool((outs[1][dead] == 0).all())      # db_r and the dW_r rows of units no sample fires
    again, _ = _se_bwd(lib, (dg, d, sq, wr, we), s32, hid32, B, C, rd, HW)
    assert all(torch.equal(x, y) for x, y in zip(outs, again))


# ---- LayerScale -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C,rps", PR.LS_CASES)
def test_layerscale_rows_partials_and_keep(rows, C, rps):
    lib = _lib.load()
    i = PR.ls_inputs(rows, C, rps)
    x, y, gamma, dy = _d(i, "x", "y", "gamma", "dy")
    for keep, surv in [(None, 1.0)] + [(k, sv) for k in i["keeps"] for sv in (0.8, 1.0)]:
        kd = None if keep is None else keep.to(dev)
        per = rps if keep is not None else 1
        ref = PR.ls_add(i["x"], i["y"], i["gamma"], keep, surv, rps)
        out, inplace = _nan(rows, C), x.clone()
        for o, xin in ((out, x), (inplace, inplace)):
            _done(lib.nrv_ls_add_f32(xin.data_ptr(), y.data_ptr(), gamma.data_ptr(), K._ptr(kd), surv, o.data_ptr(), rows, per, C, _st()), o)
            assert PR.excess(o, ref["out"], ref["tol"]) <= 1.0
        assert torch.equal(out, inplace)
        refb = PR.ls_bwd(i["dy"], i["y"], i["gamma"], keep, surv, rps)
        res = []
        for _ in range(2):
            dz, dgamma = _nan(rows, C, dtype=bf), _nan(C)
            ws = _ws(lib.nrv_ls_bwd_workspace(rows, C))
            _done(lib.nrv_ls_bwd(dy.data_ptr(), y.data_ptr(), gamma.data_ptr(), K._ptr(kd), surv, dz.data_ptr(), dgamma.data_ptr(),
                                 ws.data_ptr(), ws.numel(), rows, per, C, _st()), dz, dgamma)
            res.append((dz, dgamma))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        assert torch.equal(dz, PR.ls_dz_bits(dy, gamma, kd, surv, rps))              # IEEE fp32 products: bit for bit
        r = PR.excess(dgamma, refb["dgamma"], refb["dgamma_tol"])
        print((rows, C, rps), "keep", None if keep is None else keep.tolist(), surv, f"dgamma {r:.3f}")
        assert r <= 1.0


# ---- dgelu_rows -----------------------------------------------------------------------------------------------------------------
def _dgelu(lib, dx, gs, gdt, rows, C):
    out = _nan(rows, C, dtype=bf)
    return _done(lib.nrv_dgelu_rows(dx.data_ptr(), gs.data_ptr(), gdt, out.data_ptr(), rows, C, _st()), out)[0]


@pytest.mark.parametrize("rows,C", [(1, 8), (37, 72)])
def test_dgelu_rows_bf16_stream_bit_for_bit(rows, C):
    dx = PR._randn((rows, C), 1).to(dev)
    g16 = (torch.rand(rows, C, generator=PR._gen(2)) * 1.258 - 0.129).to(bf).to(dev)
    assert torch.equal(_dgelu(_lib.load(), dx, g16, _lib.NRV_BF16, rows, C), PR.dgelu_bits(dx, g16))


@pytest.mark.parametrize("rows,C", [(1, 64), (37, 128), (6, 192)])
def test_dgelu_rows_packed_8bit_stream(rows, C):
    """The stream is pcn_ref.q8_pack of a known matrix: the factor is q8_unpack of the same bytes and one bf16 ulp is all that is left
    (plus the decode's one fma, 2 EPS 1.4 |dx|)."""
    dx = PR._randn((rows, C), 3)
    g8 = PR.q8_pack(torch.rand(rows, C, generator=PR._gen(4), dtype=PR.D) * 1.258 - 0.129)
    out = _dgelu(_lib.load(), dx.to(dev), g8.to(dev), _lib.NRV_U8, rows, C)
    want = dx.double() * PR.q8_unpack(g8, rows, C)
    assert PR.excess(out, want, PR.bf16_tol(want, 2 * PR.EPS * want.abs() + 2.8 * PR.EPS * dx.double().abs())) <= 1.0


def test_dgelu_rows_stream_of_the_real_epilogue():
    """Bytes written by NRV_EPI_BIAS_GELU_Q8 itself: 1 / 404 plus the pre-activation's bf16-MFMA error, bounded as
    test_pcn_kernels_gpu.test_dgelu_rows_both_streams bounds it."""
    rows, C = 37, 128
    xn, w = PR._randn((rows, C), 1, dtype=bf).to(dev), PR._randn((C, C), 2, 0.1, dtype=bf).to(dev)
    bias, dx = PR._randn((C,), 3, 0.1).to(dev), PR._randn((rows, C), 4).to(dev)
    u8 = torch.empty(rows + 1, C, dtype=torch.uint8, device=dev)
    K.gemm_nt(xn, w, epilogue=_lib.EPI_BIAS_GELU_Q8, bias=bias, aux_out=u8)
    want = dx.double() * PR.dgelu(xn.double() @ w.double().t() + bias.double())
    out = _dgelu(_lib.load(), dx, u8, _lib.NRV_U8, rows, C)
    assert float((out.double() - want).norm() / want.norm()) < 1e-2


# ---- class attention ------------------------------------------------------------------------------------------------------------
def _gap_untouched(t, cols):
    return bool((t[:, cols:].contiguous().view(torch.int16) == NAN16).all())


def _ca(lib, i, B, H, Np, dh, strided=False):
    """Forward, then the backward from the forward's lse, through the C ABI.  strided: q / kc / vc are column slices of one
    [B, 3C + 8] tensor, kp / vp of one [B Np, 2C + 16] tensor, out / dout have ld C + 8; the gradients go to NaN-filled buffers of
    the same strides, whose gap columns (and spare tail rows) must still be NaN afterwards."""
    C = H * dh
    q, kc, kp, vc, vp, dout = _d(i, "q", "kc", "kp", "vc", "vp", "dout")
    if strided:
        T = torch.full((B, 3 * C + 8), 3.0, dtype=bf, device=dev)
        U = torch.full((B * Np, 2 * C + 16), 3.0, dtype=bf, device=dev)
        T[:, :C], T[:, C:2 * C], T[:, 2 * C:3 * C], U[:, :C], U[:, C:2 * C] = q, kc, vc, kp, vp
        q, kc, vc, kp, vp = T[:, :C], T[:, C:2 * C], T[:, 2 * C:3 * C], U[:, :C], U[:, C:2 * C]
        Do = torch.full((B, C + 8), 3.0, dtype=bf, device=dev)
        Do[:, :C] = dout
        dout = Do[:, :C]
        O, dT = _nan(B, C + 8, dtype=bf), _nan(B, 3 * C + 8, dtype=bf)
        spare = -(-B * Np * T.stride(0) // U.stride(0)) + 1                     # rows that any class-row stride could reach
        dU = _nan(spare, 2 * C + 16, dtype=bf)
        o, dq, dkc, dvc, dkp, dvp = O[:, :C], dT[:, :C], dT[:, C:2 * C], dT[:, 2 * C:3 * C], dU[:B * Np, :C], dU[:B * Np, C:2 * C]
    else:
        o, dq, dkc, dvc = (_nan(B, C, dtype=bf) for _ in range(4))
        dkp, dvp = (_nan(B * Np, C, dtype=bf), _nan(B * Np, C, dtype=bf)) if Np else (None, None)
    lse = _nan(B * H)
    ld = lambda t: 0 if t is None else t.stride(0)
    ops = (q.data_ptr(), ld(q), kc.data_ptr(), ld(kc), K._ptr(kp), ld(kp), vc.data_ptr(), ld(vc), K._ptr(vp), ld(vp))
    sc = ctypes.c_float(i["scale"])
    _done(lib.nrv_cls_attn_fwd(*ops, o.data_ptr(), ld(o), lse.data_ptr(), B, H, Np, dh, sc, _st()), o, lse)
    _done(lib.nrv_cls_attn_bwd(*ops, dout.data_ptr(), ld(dout), lse.data_ptr(), dq.data_ptr(), dkc.data_ptr(), K._ptr(dkp), dvc.data_ptr(),
                               K._ptr(dvp), B, H, Np, dh, sc, _st()), dq, dkc, dkp, dvc, dvp)
    if strided:
        assert _gap_untouched(O, C) and _gap_untouched(dT, 3 * C) and _gap_untouched(dU, 2 * C) and _gap_untouched(dU[B * Np:], 0)
        assert bool((T[:, 3 * C:] == 3.0).all()) and bool((U[:, 2 * C:] == 3.0).all())
    return {"o": o, "lse": lse, "dq": dq, "dkc": dkc, "dkp": dkp, "dvc": dvc, "dvp": dvp}


def _ca_check(i, r, B, H, Np, dh, what):
    args = (i["q"], i["kc"], i["kp"], i["vc"], i["vp"])
    res = PR.check_ca_fwd(PR.cls_attn_fwd(*args, B, H, Np, dh, i["scale"]), r["o"], r["lse"])          # every (b, h) of lse
    ref = PR.cls_attn_bwd(*args, i["dout"], B, H, Np, dh, i["scale"])
    dk, dv = PR.ca_rows(r["dkc"], r["dkp"], B, Np, H, dh), PR.ca_rows(r["dvc"], r["dvp"], B, Np, H, dh)
    res.update(PR.check_ca_bwd(ref, r["dq"], dk, dv))
    print(what, {k: f"{v:.3f}" for k, v in res.items()})
    return res, ref, dk


@pytest.mark.parametrize("dh,Np,H,B", PR.CA_CASES)
def test_cls_attn_every_key_row(dh, Np, H, B):
    lib = _lib.load()
    i = PR.ca_inputs(dh, Np, H, B)
    r = _ca(lib, i, B, H, Np, dh)
    res, _, _ = _ca_check(i, r, B, H, Np, dh, (dh, Np, H, B))
    assert max(res.values()) <= 1.0, res
    again = _ca(lib, i, B, H, Np, dh)
    assert all(torch.equal(r[k], again[k]) for k in r)


@pytest.mark.parametrize("dh,Np,H,B", PR.CA_STRIDED)
def test_cls_attn_strided_operands_equal_the_contiguous_run(dh, Np, H, B):
    lib = _lib.load()
    i = PR.ca_inputs(dh, Np, H, B)
    r = _ca(lib, i, B, H, Np, dh, strided=True)
    res, _, _ = _ca_check(i, r, B, H, Np, dh, ("strided", dh, Np, H, B))
    assert max(res.values()) <= 1.0, res
    c = _ca(lib, i, B, H, Np, dh)
    assert all(torch.equal(r[k], c[k]) for k in r), [k for k in r if not torch.equal(r[k], c[k])]


@pytest.mark.parametrize("dh,H,B", PR.CA_NP0)
def test_cls_attn_without_patch_keys(dh, H, B):
    """Np = 0, kp = vp = NULL: P = 1, so out is vc and dvc is dout bit for bit, lse is the one score, and dkc / dq are zero up to
    |P - 1| <= 4 EPS max(1, |lse|) (exp of the rounding of scale s - lse) times scale |dP| |q| and scale |dP| |kc|."""
    i = PR.ca_inputs(dh, 0, H, B)
    r = _ca(_lib.load(), i, B, H, 0, dh)
    assert r["dkp"] is None and r["dvp"] is None
    assert torch.equal(r["o"].cpu(), i["vc"]) and torch.equal(r["dvc"].cpu(), i["dout"])
    q, kc = i["q"].double().reshape(B, H, dh), i["kc"].double().reshape(B, H, dh)
    s = i["scale"] * (q * kc).sum(-1)
    assert PR.excess(r["lse"].reshape(B, H), s, PR.acc(dh + 1, i["scale"] * (q * kc).abs().sum(-1))) <= 1.0
    dP = (i["dout"].double() * i["vc"].double()).reshape(B, H, dh).sum(-1).abs()
    lim = 2 * 4 * PR.EPS * s.abs().clamp_min(1.0) * i["scale"] * dP                                  # [B, H]
    assert PR.excess(r["dkc"].reshape(B, H, dh), torch.zeros(B, H, dh, dtype=PR.D), lim[..., None] * q.abs().max()) <= 1.0
    assert PR.excess(r["dq"].reshape(B, H, dh), torch.zeros(B, H, dh, dtype=PR.D), lim[..., None] * kc.abs().max()) <= 1.0


@pytest.mark.parametrize("peak_key", [6, 0])
def test_cls_attn_bwd_peaked(peak_key):
    """One key 20 nats above the other 196 (a patch key; the class key).  dv per key row within 2e-2 of the largest row and per
    element within a bf16 ulp.  dk and dq cancel to the size of the fp32 lse's rounding (pcn_ref.PEAKED_EMU): the fp32 emulation's
    worst row is 15.7 / 13.5 times the largest reference row (test_pcn_ref_host.py), so their rows are held to twice 16 instead of
    2e-2, and every element to the absolute bound of pcn_ref.check_ca_peaked_abs."""
    dh, Np, H, B = (PR.PEAKED[k] for k in ("dh", "Np", "H", "B"))
    i = PR.ca_peaked_inputs(peak_key)
    r = _ca(_lib.load(), i, B, H, Np, dh)
    res, ref, dk = _ca_check(i, r, B, H, Np, dh, ("peaked", peak_key))
    assert torch.isfinite(dk).all() and torch.isfinite(r["dq"].float()).all()
    assert max(res[k] for k in ("o", "lse", "dv", "dv_elem")) <= 1.0, res
    assert max(res["dk"], res["dq"]) * PR.ROW_REL <= 2 * PR.PEAKED_EMU, res
    a = PR.check_ca_peaked_abs(ref, r["dq"], dk, i["q"], torch.cat((i["kc"], i["kp"])))
    print(a)
    assert max(a.values()) <= 1.0, a
