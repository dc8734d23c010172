"""GPU: the Twins-SVT kernels (csrc/nrv_twins.hip) per element against the fp64 references and derived bounds of
tests/twins_ref.py, on the inputs tests/test_twins_ref_host.py proves the bounds on.  Method of test_pit_kernels_gpu.py: outputs
are pre-filled with NaN, every input lives inside a NaN-moated storage (a read outside it poisons the result), every element is
compared as error / bound <= 1, and every call runs twice with bit-identical results.  q is a column block of a wider buffer, k
and v are the two halves of one buffer, as the model passes them; the gradients are written into views of the same layout and
everything around those views stays NaN."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import twins_ref as R  # noqa: E402
from parity_tools import _moated  # noqa: E402        (the NaN-moated input, shared with test_optim_edges_gpu.py)

from noise_robust_vit_amd import kernels as K  # noqa: E402

pytestmark = pytest.mark.gpu
SUB_CASES = [(H, dh, Nq, Nk) for H in R.SUB_HEADS for dh in R.SUB_DH for (Nq, Nk) in R.SUB_SHAPES]
PEG_CASES = [(H, W, C, ks) for (H, W) in R.PEG_PLANES for C in R.PEG_C for ks in R.PEG_KS]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def _nan(shape, dtype, dev):
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device=dev)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _sub_device(q, k, v, dout, H, dh, dev):
    """q as columns [8, 8 + H*dh) of a NaN buffer SUB_QPAD wider, k | v as the halves of one buffer, all moated"""
    inner = H * dh
    qbuf = torch.full((q.shape[0], inner + R.SUB_QPAD), float("nan"), dtype=torch.bfloat16)
    qbuf[:, 8:8 + inner] = q
    qd = _moated(qbuf, dev)[:, 8:8 + inner]
    kvd = _moated(torch.cat((k, v), dim=1), dev)
    return qd, kvd[:, :inner], kvd[:, inner:], _moated(dout, dev)


def _sub_run(H, dh, Nq, Nk, kind, dev):
    q, k, v, dout = R.sub_inputs(H, dh, Nq, Nk, kind)
    scale = dh ** -0.5
    B, inner = R.SUB_B, H * dh
    ref = R.sub_ref(q, k, v, dout, H, dh, Nq, Nk, scale)
    qd, kd, vd, dd = _sub_device(q, k, v, dout, H, dh, dev)
    fwd = [K.subattn_fwd(qd, kd, vd, B, H, Nq, Nk, dh, scale, out=_nan((B * Nq, inner), torch.bfloat16, dev),
                         lse=_nan((B, H, Nq), torch.float32, dev)) for _ in range(2)]
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*fwd))
    out, lse = fwd[0]
    bwd = []
    for _ in range(2):
        dqb = _nan((B * Nq, inner + R.SUB_QPAD), torch.bfloat16, dev)
        dkvb = _nan((B * Nk, 2 * inner), torch.bfloat16, dev)
        K.subattn_bwd(qd, kd, vd, dd, lse, B, H, Nq, Nk, dh, scale, dq=dqb[:, 8:8 + inner], dk=dkvb[:, :inner], dv=dkvb[:, inner:])
        bwd.append((dqb, dkvb))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*bwd))
    dqb, dkvb = bwd[0]
    assert bool(torch.isnan(dqb[:, :8]).all()) and bool(torch.isnan(dqb[:, 8 + inner:]).all())      # nothing outside the view
    dq, dk, dv = dqb[:, 8:8 + inner], dkvb[:, :inner], dkvb[:, inner:]
    rs = {n: R.ratio(t, ref[n], ref[n + "_bound"]) for n, t in (("out", out), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv))}
    print("subattn", (H, dh, Nq, Nk, kind), "error / bound:", rs)
    assert all(r <= 1.0 for r in rs.values()), rs
    return dq, dk


@pytest.mark.parametrize("H,dh,Nq,Nk", SUB_CASES)
@pytest.mark.parametrize("kind", R.SUB_KINDS)
def test_subattn(dev, H, dh, Nq, Nk, kind):
    dq, dk = _sub_run(H, dh, Nq, Nk, kind, dev)
    if Nk == 1:                                                           # softmax over one key is the constant 1
        assert float(dq.float().abs().max()) == 0.0 and float(dk.float().abs().max()) == 0.0


@pytest.mark.parametrize("dh,Nk", [(32, 17), (64, 65)])
def test_subattn_over_several_chunks(dev, dh, Nk):
    """two chunks of the plan's length and 17 rows: three partials per head, added in index order"""
    plan = K.subattn_plan(1, Nk, dh)
    Nq = 2 * plan["chunk"] + 17
    assert K.subattn_plan(Nq, Nk, dh)["chunks"] == 3
    _sub_run(1, dh, Nq, Nk, "random", dev)


def test_subattn_takes_contiguous_tensors_and_allocates(dev):
    """the plain call: contiguous q / k / v, fresh outputs; equal bits to the call on views"""
    H, dh, Nq, Nk = 3, 64, 64, 17
    q, k, v, dout = R.sub_inputs(H, dh, Nq, Nk)
    scale = dh ** -0.5
    qd, kd, vd, dd = _sub_device(q, k, v, dout, H, dh, dev)
    o1, l1 = K.subattn_fwd(qd, kd, vd, R.SUB_B, H, Nq, Nk, dh, scale)
    o2, l2 = K.subattn_fwd(q.to(dev), k.to(dev), v.to(dev), R.SUB_B, H, Nq, Nk, dh, scale)
    assert torch.equal(_bits(o1), _bits(o2)) and torch.equal(l1, l2)
    g2 = K.subattn_bwd(q.to(dev), k.to(dev), v.to(dev), dd, l2, R.SUB_B, H, Nq, Nk, dh, scale)
    assert [tuple(t.shape) for t in g2] == [(R.SUB_B * Nq, H * dh), (R.SUB_B * Nk, H * dh), (R.SUB_B * Nk, H * dh)]
    assert all(bool(torch.isfinite(t.float()).all()) for t in g2)


@pytest.mark.parametrize("H,W,C,ks", PEG_CASES)
def test_peg(dev, H, W, C, ks):
    x, w, bias, dy = R.peg_inputs(H, W, C, ks)
    B = R.PEG_B
    ref = R.peg_ref(x, w, bias, dy, H, W, ks)
    xd, wd, bd, dd = (_moated(t, dev) for t in (x, w, bias, dy))
    outs = [K.peg_fwd(xd, wd, bd, B, H, W, out=_nan(x.shape, torch.float32, dev)) for _ in range(2)]
    assert torch.equal(outs[0], outs[1])
    runs = [K.peg_bwd(xd, wd, dd, B, H, W, dx=_nan(x.shape, torch.float32, dev), dw=_nan((C, ks * ks), torch.float32, dev),
                      dbias=_nan((C,), torch.float32, dev)) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    rs = {"out": R.ratio(outs[0], ref["out"], ref["out_bound"]), "dx": R.ratio(runs[0][0], ref["dx"], ref["dx_bound"]),
          "dw": R.ratio(runs[0][1], ref["dw"], ref["dw_bound"]), "dbias": R.ratio(runs[0][2], ref["dbias"], ref["dbias_bound"])}
    print("peg", (H, W, C, ks), "error / bound:", rs)
    assert all(r <= 1.0 for r in rs.values()), rs


def test_peg_takes_the_conv2d_weight_shape(dev):
    """w [C, 1, ks, ks] as the module holds it; dw comes back in that shape"""
    H, W, C, ks = 3, 5, 8, 5
    x, w, bias, dy = R.peg_inputs(H, W, C, ks)
    w4 = w.reshape(C, 1, ks, ks).to(dev)
    out = K.peg_fwd(x.to(dev), w4, bias.to(dev), R.PEG_B, H, W)
    assert torch.equal(out, K.peg_fwd(x.to(dev), w.to(dev), bias.to(dev), R.PEG_B, H, W))
    _, dw, db = K.peg_bwd(x.to(dev), w4, dy.to(dev), R.PEG_B, H, W)
    assert dw.shape == w4.shape and db.shape == (C,)
