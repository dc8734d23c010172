"""CPU: the fp32 restatement tests/twins_ref.py reproduces the reference fixture (logits, loss, every gradient; the vanishing
set is exactly the to_q.weight of the single-key global attentions); the bounds of tests/twins_ref.py hold for the emulation of
each Twins kernel's rounding points on the very inputs tests/test_twins_kernels_gpu.py uses (ratio error / bound <= 1, printed);
and wrong kernels exceed them: a dropped key, two swapped query tiles, the scale omitted, one chunk's partial left out, the
PEG input gradient through unflipped taps."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import twins_fixture as TF  # noqa: E402
import twins_ref as R  # noqa: E402

from noise_robust_vit_amd import twins_svt as V  # noqa: E402

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "twins_small.npz")
SUB_CASES = [(H, dh, Nq, Nk) for H in R.SUB_HEADS for dh in R.SUB_DH for (Nq, Nk) in R.SUB_SHAPES]
CHUNK = 512                      # nrv_subattn_plan's chunk (tests/test_twins_host.py checks it against the library)


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


def _rel(a, b):
    a, b = a.detach().float().reshape(-1), b.detach().float().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def vanishing(model, size):
    """The parameters whose gradient is an exact zero at a `size` px image: to_q.weight of a global attention with a single
    key (softmax over one key is the constant 1)."""
    out, g = set(), size
    for si in range(4):
        embed, t1, _, t2 = model.layers[si]
        g //= embed.patch_size
        for ti, t in ((1, t1), (3, t2)):
            for li, layer in enumerate(t.layers):
                if g // layer[2].fn.fn.k == 1:
                    out.add(f"layers.{si}.{ti}.layers.{li}.2.fn.fn.to_q.weight")
    return out


@pytest.mark.parametrize("case", list(TF.CASES))
def test_restatement_reproduces_the_reference(fx, case):
    m = TF.build(V, case)
    m.load_state_dict(TF.weights(m, 3), strict=True)
    img, y = TF.inputs(case)
    logits, loss, grads = R.twins_loss_and_grads(m, img, y)
    ref = TF.unpack(fx, case + ".logits")
    err = float((logits - ref).abs().max() / ref.abs().max())
    print(case, "logits max-abs err / max-abs", err)
    assert err <= 2e-3
    assert abs(loss.item() - float(fx[case + ".loss"])) <= 2e-3 * max(1.0, abs(float(fx[case + ".loss"])))
    if m.training:
        rg = TF.unpack_grads(fx, case)
        assert set(rg) == set(grads)
        gmax = dict(zip((str(n) for n in fx[case + ".gnames"]), fx[case + ".gmax"]))
        zero = vanishing(m, img.shape[-1])
        assert {k for k, v in gmax.items() if v < 1e-4} == zero, case
        for k, g in grads.items():
            if k in zero:
                assert gmax[k] == 0.0 and float(g.abs().max()) < 1e-6, k
                continue
            assert _rel(TF.grad_sample(k, g), rg[k]) <= 5e-3, k
        if case == "s_train":
            assert zero == {"layers.2.1.layers.0.2.fn.fn.to_q.weight", "layers.2.3.layers.0.2.fn.fn.to_q.weight",
                            "layers.2.3.layers.1.2.fn.fn.to_q.weight"}
            assert min(v for k, v in gmax.items() if k not in zero) >= 1e-2     # two orders above the vanishing threshold


def test_robust_restatement_differs_and_is_doubly_normalised():
    m = TF.build(V, "r_train", robust=True)
    m.load_state_dict(TF.weights(m, 3), strict=True)
    img, y = TF.inputs("r_train")
    lr, _, gr = R.twins_loss_and_grads(m, img, y)
    m2 = TF.build(V, "s_train")
    m2.load_state_dict(TF.weights(m2, 3), strict=True)
    ls, _, _ = R.twins_loss_and_grads(m2, img, y)
    assert torch.isfinite(lr).all() and all(torch.isfinite(g).all() for g in gr.values()) and _rel(lr, ls) > 1e-3
    p = R.sinkhorn(torch.softmax(torch.randn(3, 49, 16, generator=R._gen("sk")), dim=-1))
    assert torch.allclose(p.sum(-1), torch.ones(3, 49), atol=1e-5)


@pytest.mark.parametrize("H,dh,Nq,Nk", SUB_CASES)
@pytest.mark.parametrize("kind", R.SUB_KINDS)
def test_subattn_bounds_hold_for_the_emulation(H, dh, Nq, Nk, kind):
    q, k, v, dout = R.sub_inputs(H, dh, Nq, Nk, kind)
    scale = dh ** -0.5
    ref = R.sub_ref(q, k, v, dout, H, dh, Nq, Nk, scale)
    out, lse = R.sub_fwd_emul(q, k, v, H, dh, Nq, Nk, scale)
    dq, dk, dv = R.sub_bwd_emul(q, k, v, dout, lse, H, dh, Nq, Nk, scale, CHUNK)         # the forward's own lse, as the model passes it
    rs = {n: R.ratio(t, ref[n], ref[n + "_bound"]) for n, t in (("out", out), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv))}
    print("subattn", (H, dh, Nq, Nk, kind), "error / bound:", rs)
    assert all(r <= 1.0 for r in rs.values()), rs
    if Nk == 1:
        assert float(dq.float().abs().max()) == 0.0 and float(dk.float().abs().max()) == 0.0
    if kind == "peaked" and Nk > 1:
        s = scale * R._heads(q, Nq, H, dh) @ R._heads(k, Nk, H, dh).transpose(-1, -2)
        top = s.topk(2, dim=-1).values
        low = (-s).topk(2, dim=-1).values
        gap = torch.maximum(top[..., 0] - top[..., 1], low[..., 0] - low[..., 1]) if Nk > 2 else top[..., 0] - top[..., 1]
        assert float(gap.amax(-1).amin()) >= 6.0 and float(gap.max()) >= 100.0     # every (sample, head) has its peak


def test_the_chunked_shape_is_bounded_too():
    """two chunks and 17 rows: the partial sums of dk / dv in chunk order"""
    H, dh, Nq, Nk = 1, 32, 2 * CHUNK + 17, 17
    q, k, v, dout = R.sub_inputs(H, dh, Nq, Nk)
    scale = dh ** -0.5
    ref = R.sub_ref(q, k, v, dout, H, dh, Nq, Nk, scale)
    dq, dk, dv = R.sub_bwd_emul(q, k, v, dout, ref["lse"].float(), H, dh, Nq, Nk, scale, CHUNK)
    assert all(R.ratio(t, ref[n], ref[n + "_bound"]) <= 1.0 for n, t in (("dq", dq), ("dk", dk), ("dv", dv)))
    for c in range(3):                                                    # one chunk's partial left out
        _, dk2, dv2 = R.sub_bwd_emul(q, k, v, dout, ref["lse"].float(), H, dh, Nq, Nk, scale, CHUNK, skip_chunk=c)
        assert R.ratio(dk2, ref["dk"], ref["dk_bound"]) > 1.0 and R.ratio(dv2, ref["dv"], ref["dv_bound"]) > 1.0, c


@pytest.mark.parametrize("wrong", [dict(drop_key=True), dict(swap_tiles=True), dict(no_scale=True)])
@pytest.mark.parametrize("kind", ["random", "peaked"])
def test_a_wrong_forward_exceeds_the_bound(wrong, kind):
    H, dh, Nq, Nk = 3, 64, 64, 17
    q, k, v, dout = R.sub_inputs(H, dh, Nq, Nk, kind)
    scale = dh ** -0.5
    ref = R.sub_ref(q, k, v, dout, H, dh, Nq, Nk, scale)
    assert R.ratio(R.sub_fwd_emul(q, k, v, H, dh, Nq, Nk, scale)[0], ref["out"], ref["out_bound"]) <= 1.0
    out, lse = R.sub_fwd_emul(q, k, v, H, dh, Nq, Nk, scale, **wrong)
    assert R.ratio(out, ref["out"], ref["out_bound"]) > 1.0
    if "swap_tiles" not in wrong:
        assert R.ratio(lse, ref["lse"], ref["lse_bound"]) > 1.0


def test_a_backward_without_the_scale_exceeds_the_bound():
    H, dh, Nq, Nk = 3, 64, 64, 17
    q, k, v, dout = R.sub_inputs(H, dh, Nq, Nk)
    scale = dh ** -0.5
    ref = R.sub_ref(q, k, v, dout, H, dh, Nq, Nk, scale)
    dq, dk, dv = R.sub_bwd_emul(q, k, v, dout, ref["lse"].float(), H, dh, Nq, Nk, scale, CHUNK, no_scale=True)
    assert R.ratio(dq, ref["dq"], ref["dq_bound"]) > 1.0 and R.ratio(dk, ref["dk"], ref["dk_bound"]) > 1.0
    assert R.ratio(dv, ref["dv"], ref["dv_bound"]) > 1.0


def test_the_fp64_attention_reference_is_autograd():
    H, dh, Nq, Nk = 3, 32, 33, 65
    q, k, v, dout = R.sub_inputs(H, dh, Nq, Nk)
    scale = dh ** -0.5
    ref = R.sub_ref(q, k, v, dout, H, dh, Nq, Nk, scale)
    Q, Kk, Vv = (R._heads(t, n, H, dh).clone().requires_grad_(True) for t, n in ((q, Nq), (k, Nk), (v, Nk)))
    o = torch.softmax(scale * Q @ Kk.transpose(-1, -2), dim=-1) @ Vv
    o.backward(R._heads(dout, Nq, H, dh))
    for n, t in (("out", o.detach()), ("dq", Q.grad), ("dk", Kk.grad), ("dv", Vv.grad)):
        assert torch.allclose(R._rows(t), ref[n], rtol=0, atol=1e-11), n


PEG_CASES = [(H, W, C, ks) for (H, W) in R.PEG_PLANES for C in R.PEG_C for ks in R.PEG_KS]


@pytest.mark.parametrize("H,W,C,ks", PEG_CASES)
def test_peg_bounds_hold_for_the_emulation(H, W, C, ks):
    x, w, bias, dy = R.peg_inputs(H, W, C, ks)
    ref = R.peg_ref(x, w, bias, dy, H, W, ks)
    ew, eb = R.peg_dw_emul(x, dy, H, W, ks)
    rs = {"out": R.ratio(R.peg_conv_emul(x, w, bias, H, W, ks), ref["out"], ref["out_bound"]),
          "dx": R.ratio(R.peg_conv_emul(dy, w, None, H, W, ks, flip=True), ref["dx"], ref["dx_bound"]),
          "dw": R.ratio(ew, ref["dw"], ref["dw_bound"]), "dbias": R.ratio(eb, ref["dbias"], ref["dbias_bound"])}
    print("peg", (H, W, C, ks), "error / bound:", rs)
    assert all(r <= 1.0 for r in rs.values()), rs


def test_the_fp64_peg_reference_is_the_reference_module():
    H, W, C, ks = 3, 5, 8, 5
    x, w, bias, dy = R.peg_inputs(H, W, C, ks)
    conv = torch.nn.Conv2d(C, C, ks, padding=ks // 2, groups=C).double()
    with torch.no_grad():
        conv.weight.copy_(w.double().reshape(C, 1, ks, ks))
        conv.bias.copy_(bias.double())
    p = R._planes(x, H, W).clone().requires_grad_(True)
    y = conv(p) + p
    y.backward(R._planes(dy, H, W))
    ref = R.peg_ref(x, w, bias, dy, H, W, ks)
    assert torch.allclose(R._prows(y.detach()), ref["out"], rtol=0, atol=1e-12) and torch.allclose(R._prows(p.grad), ref["dx"], rtol=0, atol=1e-12)
    assert torch.allclose(conv.weight.grad.reshape(C, ks * ks), ref["dw"], rtol=0, atol=1e-12)
    assert torch.allclose(conv.bias.grad, ref["dbias"], rtol=0, atol=1e-12)


def test_a_wrong_peg_kernel_exceeds_the_bound():
    H, W, C, ks = 14, 14, 8, 3
    x, w, bias, dy = R.peg_inputs(H, W, C, ks)
    ref = R.peg_ref(x, w, bias, dy, H, W, ks)
    assert R.ratio(R.peg_conv_emul(dy, w, None, H, W, ks, flip=False), ref["dx"], ref["dx_bound"]) > 1.0      # unflipped taps
    assert R.ratio(R.peg_conv_emul(x, w, None, H, W, ks), ref["out"], ref["out_bound"]) > 1.0                 # the bias left out
