"""Host: what the bounds of test_pcn_edges_gpu.py rest on.

(1) every hand-written backward of pcn_ref.py equals fp64 torch.autograd of its forward (F.conv2d(groups=C), F.gelu, linear,
sigmoid, softmax); (2) the 8-bit stream layout round-trips and its offset map is a bijection; (3) for every bound the GPU test
applies, an fp32 torch emulation of the kernel's arithmetic (same bf16 operands, fp32 math, the Abramowitz-Stegun erf, bf16
rounding of the outputs) is inside it ON THE GPU TEST'S OWN INPUTS.  A bound the emulation breaks is wrong and is fixed here."""
import math

import pytest
import torch
import torch.nn.functional as F

import pcn_ref as PR

D = torch.float64
bf = torch.bfloat16


def _close(a, b, tol=1e-11):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ---- (1) the restatements against autograd --------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C", [(2, 3, 5, 8), (3, 5, 3, 72), (2, 1, 7, 64), (1, 1, 1, 8)])
def test_dwconv_restatement_is_autograd_of_conv2d(B, H, W, C):
    i = PR.dw_inputs(B, H, W, C)
    a = i["a"].double().reshape(B, H, W, C).permute(0, 3, 1, 2).requires_grad_(True)
    w = i["w"].double().reshape(C, 1, 3, 3).requires_grad_(True)
    b = i["bias"].double().requires_grad_(True)
    d = F.gelu(F.conv2d(a, w, b, padding=1, groups=C))
    f = PR.dwconv_fwd(i["a"], i["w"], i["bias"], B, H, W)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C)
    assert _close(f["d"], rows(d.detach())) and _close(f["sq"], d.detach().sum((2, 3)))
    dg = i["dg"].double().reshape(B, H, W, C).permute(0, 3, 1, 2)
    L = (d * dg * i["s"].double()[:, :, None, None]).sum() + (d.mean((2, 3)) * i["dmean"].double()).sum()
    ga, gw, gb = torch.autograd.grad(L, (a, w, b))
    r = PR.dwconv_bwd(i["a"], i["w"], i["bias"], i["dg"], i["s"], i["dmean"], B, H, W)
    assert _close(r["da"], rows(ga)) and _close(r["dw"], gw.reshape(C, 9)) and _close(r["db"], gb)


@pytest.mark.parametrize("B,C,rd,HW", PR.SE_CASES[:5])
def test_se_restatement_is_autograd(B, C, rd, HW):
    i = PR.se_inputs(B, C, rd, HW)
    P = [t.double().requires_grad_(True) for t in (i["sq"], i["wr"], i["br"], i["we"], i["be"])]
    h = F.relu(F.linear(P[0] / HW, P[1], P[2]))
    s = torch.sigmoid(F.linear(h, P[3], P[4]))
    assert _close(i["ref"]["s"], s.detach()) and _close(i["ref"]["hid"], h.detach())
    L = ((i["dg"].double() * i["d"].double()).reshape(B, HW, C).sum(1) * s).sum()
    g = torch.autograd.grad(L, P)
    r = PR.se_bwd(i["dg"], i["d"], i["sq"], HW, s.detach(), h.detach(), i["wr"], i["we"])
    assert _close(r["dmean"], g[0] * HW)
    for k, want in zip(("dwr", "dbr", "dwe", "dbe"), g[1:]):
        assert _close(r[k], want), k


@pytest.mark.parametrize("rows,C,rps", PR.LS_CASES[2:5])
def test_ls_restatement_is_autograd(rows, C, rps):
    i = PR.ls_inputs(rows, C, rps)
    keep = i["keeps"][0]
    y, g = i["y"].double().requires_grad_(True), i["gamma"].double().requires_grad_(True)
    f = (keep.double() / float(torch.tensor(0.8))).repeat_interleave(rps)[:, None]
    out = i["x"].double() + f * g * y
    assert _close(PR.ls_add(i["x"], i["y"], i["gamma"], keep, 0.8, rps)["out"], out.detach())
    gy, gg = torch.autograd.grad((out * i["dy"].double()).sum(), (y, g))
    r = PR.ls_bwd(i["dy"], i["y"], i["gamma"], keep, 0.8, rps)
    assert _close(r["dz"], gy) and _close(r["dgamma"], gg)


@pytest.mark.parametrize("dh,Np,H,B", [(8, 1, 1, 2), (40, 3, 3, 2), (72, 5, 2, 3), (64, 255, 2, 1), (8, 0, 2, 2)])
def test_cls_attn_restatement_is_autograd_of_softmax(dh, Np, H, B):
    i = PR.ca_inputs(dh, Np, H, B)
    C, sc = H * dh, i["scale"]
    T = [None if t is None else t.double().requires_grad_(True) for t in (i["q"], i["kc"], i["kp"], i["vc"], i["vp"])]
    cat = lambda c, p: (c[:, None] if p is None else torch.cat((c[:, None], p.reshape(B, Np, C)), 1)).reshape(B, Np + 1, H, dh).transpose(1, 2)
    k, v = cat(T[1], T[2]), cat(T[3], T[4])
    S = torch.einsum("bhd,bhjd->bhj", T[0].reshape(B, H, dh), k) * sc
    o = torch.einsum("bhj,bhjd->bhd", torch.softmax(S, -1), v).reshape(B, C)
    f = PR.cls_attn_fwd(i["q"], i["kc"], i["kp"], i["vc"], i["vp"], B, H, Np, dh, sc)
    assert _close(f["o"], o.detach()) and _close(f["lse"], torch.logsumexp(S.detach(), -1))
    g = torch.autograd.grad((o * i["dout"].double()).sum(), [t for t in T if t is not None])
    if Np == 0:
        g = (g[0], g[1], None, g[2], None)
    r = PR.cls_attn_bwd(i["q"], i["kc"], i["kp"], i["vc"], i["vp"], i["dout"], B, H, Np, dh, sc)
    assert _close(r["dq"].reshape(B, C), g[0])
    assert _close(r["dk"], PR.ca_rows(g[1], g[2], B, Np, H, dh)) and _close(r["dv"], PR.ca_rows(g[3], g[4], B, Np, H, dh))


def test_ca_rows_takes_strided_operands():
    i = PR.ca_inputs(40, 3, 3, 2)
    C = 120
    T = torch.zeros(2, 3 * C + 8, dtype=bf)
    U = torch.zeros(6, 2 * C + 16, dtype=bf)
    T[:, C:2 * C], U[:, :C] = i["kc"], i["kp"]
    assert torch.equal(PR.ca_rows(T[:, C:2 * C], U[:, :C], 2, 3, 3, 40), PR.ca_rows(i["kc"], i["kp"], 2, 3, 3, 40))


# ---- (2) the 8-bit stream -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(1, 64), (37, 128), (6, 192), (15, 64), (27, 64)])
def test_q8_round_trip_and_bijection(M, N):
    g = torch.rand(M, N, generator=torch.Generator().manual_seed(M), dtype=D) * 1.258 - 0.129
    buf = PR.q8_pack(g)
    Me = (M + 1) // 2 * 2
    assert buf.numel() == Me * N
    assert float((PR.q8_unpack(buf, M, N) - g).abs().max()) <= 1.0 / 404 + 1e-12          # half the 1 / 202 step (include/nrv.h)
    off = PR.q8_offsets(Me, N, N).reshape(-1)
    assert torch.equal(off.sort().values, torch.arange(Me * N))                           # a bijection onto [0, rows_even * ld)
    # the two rows of a pair share one 128-byte line per 64 columns; a wider ld leaves the gap bytes alone
    assert int(PR.q8_offsets(2, 64, 64)[1, 0]) == 64 and int(PR.q8_offsets(3, 128, 128)[2, 64]) == 2 * 128 + 128
    wide = PR.q8_pack(g, ld=N + 16, fill=7)
    assert torch.equal(PR.q8_unpack(wide, M, N, N + 16), PR.q8_unpack(buf, M, N))
    assert int((wide == 7).sum()) >= wide.numel() - Me * N


# ---- (3) fp32 emulations of the kernels' arithmetic against the GPU test's bounds -----------------------------------------------
def _gelu_parts32(u):
    """nrv_common.hpp gelu_parts in torch fp32."""
    x = u.abs() * 0.70710678118654752
    t = 1.0 / (0.3275911 * x + 1.0)
    e = torch.exp2(u * u * -0.72134752044448170)
    p = 1.061405429 * t - 1.453152027
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = p * t + c
    half = 0.5 * (p * t * e)
    return torch.where(u >= 0, 1.0 - half, half), e * 0.39894228040143268


def _emu_dw(i, B, H, W, C):
    a = i["a"].float().reshape(B, H, W, C)
    taps = [PR._shift(a, t // 3 - 1, t % 3 - 1) for t in range(9)]
    u = i["bias"].clone().expand(B, H, W, C)
    for t in range(9):
        u = i["w"][:, t] * taps[t] + u
    Phi, phi = _gelu_parts32(u)
    d32 = u * Phi
    dd = (i["dg"].float().reshape(B, H, W, C) * i["s"][:, None, None] + (i["dmean"] * torch.tensor(1.0 / (H * W)))[:, None, None]) * (u * phi + Phi)
    dw = torch.stack([(dd * taps[t]).sum((0, 1, 2)) for t in range(9)], 1)
    da = torch.zeros_like(dd)
    for t in range(9):
        da = i["w"][:, t] * PR._shift(dd, -(t // 3 - 1), -(t % 3 - 1)) + da
    return d32.reshape(-1, C).to(bf), d32.sum((1, 2)), da.reshape(-1, C), dw, dd.sum((0, 1, 2))


@pytest.mark.parametrize("B,H,W,C", PR.DW_CASES + PR.DW_Q8_ONLY)
def test_dwconv_emulation_is_inside_the_bounds(B, H, W, C):
    i = PR.dw_inputs(B, H, W, C)
    d, sq, da, dw, db = _emu_dw(i, B, H, W, C)
    r = PR.check_dw_fwd(PR.dwconv_fwd(i["a"], i["w"], i["bias"], B, H, W), d, sq)
    ref = PR.dwconv_bwd(i["a"], i["w"], i["bias"], i["dg"], i["s"], i["dmean"], B, H, W)
    r.update({"none " + k: v for k, v in PR.check_dw_bwd(ref, None, da.to(bf), dw, db).items()})
    r.update({"bf16 " + k: v for k, v in PR.check_dw_bwd(ref, i["g16"].double(), (da * i["g16"].float()).to(bf), dw, db).items()})
    if C % 64 == 0:
        g8 = PR.q8_unpack(i["g8"], B * H * W, C)
        dec = torch.addcmul(torch.tensor(-26.0 / 202.0), (g8 * 202 + 26).round().float(), torch.tensor(1.0 / 202.0))      # the kernel's decode
        r.update({"q8 " + k: v for k, v in PR.check_dw_bwd(ref, g8, (da * dec).to(bf), dw, db).items()})
    print((B, H, W, C), {k: f"{v:.3f}" for k, v in r.items()})
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("B,C,rd,HW", PR.SE_CASES)
def test_se_inputs_and_emulation(B, C, rd, HW):
    i = PR.se_inputs(B, C, rd, HW)
    pre = i["ref"]["pre"]
    assert float(pre.abs().min()) >= PR.SE_MIN_PRE and bool((pre > 0).any()) and bool((pre < 0).any())
    hid = F.relu(F.linear(i["sq"] * torch.tensor(1.0 / HW), i["wr"], i["br"]))
    s = 1.0 / (1.0 + torch.exp(-F.linear(hid, i["we"], i["be"])))
    r = PR.check_se_fwd(i["ref"], s, hid)
    s, hid = i["s32"], i["hid32"]
    ds = (i["dg"].float() * i["d"].float()).reshape(B, HW, C).sum(1)
    dz = ds * s * (1.0 - s)
    dp = (dz @ i["we"]) * (hid > 0)
    mean = i["sq"] * torch.tensor(1.0 / HW)
    ref = PR.se_bwd(i["dg"], i["d"], i["sq"], HW, s, hid, i["wr"], i["we"])
    r.update(PR.check_se_bwd(ref, dp @ i["wr"], dp.t() @ mean, dp.sum(0), dz.t() @ hid, dz.sum(0)))
    print((B, C, rd, HW), {k: f"{v:.3f}" for k, v in r.items()}, "min |pre|", float(pre.abs().min()))
    assert max(r.values()) <= 1.0, r
    g = PR.se_apply_bits(i["d"], s, HW)                    # one product: one bf16 ulp of fp64 at most
    want = i["d"].double() * s.double().repeat_interleave(HW, 0)
    assert PR.excess(g, want, PR.bf16_tol(want, 2 * PR.EPS * want.abs())) <= 1.0


@pytest.mark.parametrize("rows,C,rps", PR.LS_CASES)
def test_ls_emulation_is_inside_the_bounds(rows, C, rps):
    i = PR.ls_inputs(rows, C, rps)
    assert all(k.numel() == rows // rps for k in i["keeps"]) and {float(v) for k in i["keeps"] for v in k} == {0.0, 1.0}
    for keep, surv in [(None, 1.0)] + [(k, sv) for k in i["keeps"] for sv in (0.8, 1.0)]:
        f = 1.0 if keep is None else (keep * (torch.tensor(1.0) / torch.tensor(surv))).repeat_interleave(rps)[:, None]
        a = PR.ls_add(i["x"], i["y"], i["gamma"], keep, surv, rps)
        assert PR.excess((f * i["gamma"]) * i["y"] + i["x"], a["out"], a["tol"]) <= 1.0
        b = PR.ls_bwd(i["dy"], i["y"], i["gamma"], keep, surv, rps)
        assert PR.excess(((i["dy"] * f) * i["y"]).sum(0), b["dgamma"], b["dgamma_tol"]) <= 1.0
        dz = PR.ls_dz_bits(i["dy"], i["gamma"], keep, surv, rps)
        assert PR.excess(dz, b["dz"], PR.bf16_tol(b["dz"], 4 * PR.EPS * b["dz"].abs())) <= 1.0


def _emu_ca(i, B, H, Np, dh, lse=None):
    """fp32: scores, lse = m + log(sum exp), P = exp(S - lse), o; the backward recomputes P from the (given) lse as the kernel does."""
    f32 = lambda t: None if t is None else t.float()
    Q = i["q"].float().reshape(B, H, dh)
    K = PR.ca_rows(i["kc"], i["kp"], B, Np, H, dh).float()
    V = PR.ca_rows(i["vc"], i["vp"], B, Np, H, dh).float()
    S = torch.einsum("bhd,bhjd->bhj", Q, K) * torch.tensor(i["scale"])
    m = S.max(-1, keepdim=True).values
    L = (m + torch.log(torch.exp(S - m).sum(-1, keepdim=True))) if lse is None else lse[..., None]
    P = torch.exp(S - L)
    o = torch.einsum("bhj,bhjd->bhd", P, V).reshape(B, H * dh).to(bf)
    do = i["dout"].float().reshape(B, H, dh)
    dP = torch.einsum("bhd,bhjd->bhj", do, V)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    sc = torch.tensor(i["scale"])
    dq = (torch.einsum("bhj,bhjd->bhd", dS, K) * sc).to(bf)
    dk = ((dS * sc)[..., None] * Q[:, :, None]).to(bf)
    dv = (P[..., None] * do[:, :, None]).to(bf)
    return o, L[..., 0], dq.reshape(B, H * dh), dk, dv


@pytest.mark.parametrize("dh,Np,H,B", PR.CA_CASES)
def test_cls_attn_emulation_is_inside_the_bounds(dh, Np, H, B):
    i = PR.ca_inputs(dh, Np, H, B)
    o, lse, dq, dk, dv = _emu_ca(i, B, H, Np, dh)
    args = (i["q"], i["kc"], i["kp"], i["vc"], i["vp"])
    r = PR.check_ca_fwd(PR.cls_attn_fwd(*args, B, H, Np, dh, i["scale"]), o, lse)
    r.update(PR.check_ca_bwd(PR.cls_attn_bwd(*args, i["dout"], B, H, Np, dh, i["scale"]), dq, dk, dv))
    print((dh, Np, H, B), {k: f"{v:.3f}" for k, v in r.items()})
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("peak_key", [6, 0])
def test_cls_attn_peaked_emulation(peak_key):
    """dv keeps ROW_REL; dk and dq cancel to the size of lse's rounding (pcn_ref.PEAKED_EMU): measured here with lse at its fp32
    value and at both neighbours."""
    dh, Np, H, B = (PR.PEAKED[k] for k in ("dh", "Np", "H", "B"))
    i = PR.ca_peaked_inputs(peak_key)
    args = (i["q"], i["kc"], i["kp"], i["vc"], i["vp"])
    ref = PR.cls_attn_bwd(*args, i["dout"], B, H, Np, dh, i["scale"])
    others = torch.ones(Np + 1, dtype=torch.bool)
    others[peak_key] = False
    gap = ref["P"][..., peak_key].log()[..., None] - ref["P"][..., others].log()
    assert 19.0 < float(gap.min()) and float(gap.max()) < 21.0                            # 20 nats above every other key
    L = ref["lse"].float()
    worst = {"dq": 0.0, "dk": 0.0, "dv": 0.0, "dv_elem": 0.0}
    for nb in (L, torch.nextafter(L, L + 1), torch.nextafter(L, L - 1)):
        _, _, dq, dk, dv = _emu_ca(i, B, H, Np, dh, lse=nb)
        for k, v in PR.check_ca_bwd(ref, dq, dk, dv).items():
            worst[k] = max(worst[k], v * (PR.ROW_REL if k in ("dq", "dk") else 1.0))
    print("peak key", peak_key, worst)
    assert worst["dv"] <= 1.0 and worst["dv_elem"] <= 1.0
    assert worst["dk"] <= PR.PEAKED_EMU and worst["dq"] <= PR.PEAKED_EMU


def test_np0_is_the_identity():
    for dh, H, B in PR.CA_NP0:
        i = PR.ca_inputs(dh, 0, H, B)
        r = PR.cls_attn_bwd(i["q"], i["kc"], None, i["vc"], None, i["dout"], B, H, 0, dh, i["scale"])
        f = PR.cls_attn_fwd(i["q"], i["kc"], None, i["vc"], None, B, H, 0, dh, i["scale"])
        assert torch.equal(f["o"], i["vc"].double()) and torch.equal(r["dv"][:, :, 0].reshape(B, -1), i["dout"].double())
        assert float(r["dk"].abs().max()) == 0.0 and float(r["dq"].abs().max()) == 0.0
        assert _close(f["lse"], i["scale"] * (i["q"].double() * i["kc"].double()).reshape(B, H, dh).sum(-1))
