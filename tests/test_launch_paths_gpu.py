"""GPU: every row / elementwise kernel of tests/launch_paths.py at a shape that makes it walk its grid-stride loop for two
full passes and a partial third -- the path every batch-256 training step takes and the small-shape kernel tests never reach.

Copies and one-rounding kernels are compared with their definition bit for bit (integer-valued data where sums are involved,
so any order is exact); a mismatch reports the first bad flat index, the pass it lies in (item // threshold) and the number
of bad elements, so a broken continuation reads differently from a broken tail.

AdamW, bn_apply: the references and bounds of test_optim_gpu.py / test_bn_rows_gpu.py.

LayerNorm, layernorm_pad: float64 F.layer_norm and its autograd.  The whole-tensor bounds of test_kernels_gpu.py's
test_layernorm_fwd_bwd, and per row (outputs) / per column (dgamma, dbeta) the rule of test_talking_heads_gpu.py, which is
not tuned on the kernels: the kernel's error against float64 may be at most 4 x the error of torch's own fp32 evaluation of
the same formula, with a floor of 8 * 2^-23, plus 2^-8 where the kernel stores bf16.  Per row the error is the relative L2
error of the row; per column it is |sum - ref| / |ref|, and dy is drawn with a mean and a component along x^ so that no
column sum cancels (a column whose true sum is near zero has no meaningful relative error).  Both errors are printed."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import launch_paths as LP  # noqa: E402
from noise_robust_vit_amd import kernels as K  # noqa: E402

pytestmark = pytest.mark.gpu

FLOOR = 8 * 2.0 ** -23
BF16 = 2.0 ** -8
EPS = 1e-5


def gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def randn(shape, dev, seed, scale=1.0, shift=0.0, dtype=torch.float32):
    return torch.randn(*shape, generator=gen(dev, seed), device=dev).mul_(scale).add_(shift).to(dtype)


def randint(shape, dev, seed, lo=-8, hi=9):
    return torch.randint(lo, hi, shape, generator=gen(dev, seed), device=dev).float()


# ---------------------------------------------------------------------------------------------- failure reports
def where_bad(bad, rec, per_item, item_of=None):
    """`bad`: bool tensor over the output.  First bad flat index, its work item and pass, the number of bad elements."""
    flat = bad.reshape(-1)
    count = int(flat.sum())
    first = int(flat.nonzero()[0])
    item = first // per_item
    if item_of is not None:
        item = int(item_of[item])
    where = f"pass {item // rec.threshold} (item {item}, threshold {rec.threshold})" if item >= 0 else "written by no item"
    return f"{rec.name}: first bad flat index {first} in {where}; {count} of {flat.numel()} elements bad"


def assert_same(got, ref, rec, per_item=None, item_of=None, what=""):
    """torch.equal(got, ref).  per_item: output elements per work item of the kernel's loop (a row kernel: the row width)."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (rec.name, what, got.shape, ref.shape, got.dtype, ref.dtype)
    if torch.equal(got, ref):
        return
    bad = (got != ref) | (got.isnan() if got.is_floating_point() else torch.zeros_like(got, dtype=torch.bool))
    raise AssertionError(what + " " + where_bad(bad, rec, per_item or rec.per_item, item_of))


def assert_within(err, bound, rec, per_item=None, what=""):
    """err <= bound elementwise (bound a tensor or a number); NaN is bad."""
    bad = ~(err <= bound)
    if bool(bad.any()):
        worst = float(err.reshape(-1)[bad.reshape(-1)].max())
        raise AssertionError(f"{what} worst error {worst:.3e}; " + where_bad(bad, rec, per_item or rec.per_item))


def test_reports_tell_a_broken_continuation_from_a_broken_tail(dev):
    rec = LP.get("cast_bf16")
    ref = torch.zeros(rec.wrapped["n"], device=dev)
    got = ref.clone()
    got[rec.threshold_elements + 5:rec.threshold_elements + 9] = 1.0
    with pytest.raises(AssertionError, match=r"first bad flat index 4194309 in pass 1 .*; 4 of 9937187 elements bad"):
        assert_same(got, ref, rec)
    got = ref.clone()
    got[-1] = float("nan")
    with pytest.raises(AssertionError, match=r"first bad flat index 9937186 in pass 2 .*; 1 of"):
        assert_same(got, ref, rec)


# ---------------------------------------------------------------------------------------------- copies, one rounding
def test_cast_wrapped(dev):
    rec = LP.get("cast_bf16")
    n = rec.wrapped["n"]
    assert n % 4 == 3                                                # scalar tail behind the last vector
    x = randn((n,), dev, 1)
    assert_same(K.cast_bf16(x), x.to(torch.bfloat16), rec)


def _keep(n, dev, seed):
    keep = (torch.rand(n, generator=gen(dev, seed), device=dev) >= 0.3).to(torch.uint8)
    keep[::7] *= 5                                                   # any non-zero byte keeps
    return keep


def test_dropout_add_wrapped_and_in_place(dev):
    rec = LP.get("dropout_add")
    n = rec.wrapped["n"]
    x, y, keep = randn((n,), dev, 2), randn((n,), dev, 3), _keep(n, dev, 4)
    scale = 1.0 / 0.7
    ref = x + torch.where(keep != 0, y * torch.tensor(scale, dtype=torch.float32, device=dev), torch.zeros_like(y))
    assert_same(K.dropout_add(x, y, keep, scale), ref, rec)
    yy = y.clone()
    assert K.dropout_add(x, yy, keep, scale, out=yy) is yy           # out aliases the branch
    assert_same(yy, ref, rec, what="out=y")


def test_mask_mul_wrapped_and_in_place(dev):
    rec = LP.get("mask_mul")
    n = rec.wrapped["n"]
    a, keep = randn((n,), dev, 5, dtype=torch.bfloat16), _keep(n, dev, 6)
    scale = 1.0 / 0.7
    ref = torch.where(keep != 0, a.float() * torch.tensor(scale, dtype=torch.float32, device=dev), torch.zeros(n, device=dev)).bfloat16()
    assert_same(K.mask_mul(a, keep, scale), ref, rec)
    aa = a.clone()
    K.mask_mul(aa, keep, scale, out=aa)
    assert_same(aa, ref, rec, what="out=a")


def test_mask_mul_f32_wrapped_and_in_place(dev):
    rec = LP.get("mask_mul_f32")
    n = rec.wrapped["n"]
    assert n % 8                                                     # any element count
    a, keep = randn((n,), dev, 7), _keep(n, dev, 8)
    scale = 1.0 / 0.9
    ref = torch.where(keep != 0, a * torch.tensor(scale, dtype=torch.float32, device=dev), torch.zeros_like(a))
    assert_same(K.mask_mul_f32(a, keep, scale), ref, rec)
    aa = a.clone()
    K.mask_mul_f32(aa, keep, scale, out=aa)
    assert_same(aa, ref, rec, what="out=a")


def _indices(rec, dev):
    """A partial permutation of the source rows with out-of-range entries (negative, == rows_src, 2^40) in the second and
    third pass of the row loop."""
    rows, rows_src = rec.wrapped["rows"], rec.wrapped["rows_src"]
    idx = torch.randperm(rows_src, generator=gen(dev, 9), device=dev)[:rows].contiguous()
    t = rec.threshold
    assert rows > 2 * t + 100
    for base in (t, 2 * t):
        idx[base + 1] = -1
        idx[base + 5] = rows_src
        idx[base + 64] = 2 ** 40
        idx[base + 99] = -(2 ** 40)
    idx[rows - 1] = rows_src + 7                                     # the last row of the partial pass
    ok = (idx >= 0) & (idx < rows_src)
    return idx, ok


def test_gather_rows_wrapped_with_out_of_range_indices_in_later_passes(dev):
    rec = LP.get("gather_rows")
    dim = rec.wrapped["dim"]
    src = randn((rec.wrapped["rows_src"], dim), dev, 10)
    idx, ok = _indices(rec, dev)
    ref = torch.zeros(idx.numel(), dim, device=dev)
    ref[ok] = src[idx[ok]]
    assert_same(K.gather_rows(src, idx), ref, rec, per_item=dim)


def test_scatter_rows_wrapped_with_out_of_range_indices_in_later_passes(dev):
    rec = LP.get("scatter_rows")
    dim, rows_src = rec.wrapped["dim"], rec.wrapped["rows_src"]
    idx, ok = _indices(rec, dev)
    d = randn((idx.numel(), dim), dev, 11)
    ref = torch.zeros(rows_src, dim, device=dev)
    ref[idx[ok]] = d[ok]
    writer = torch.full((rows_src,), -1, dtype=torch.int64, device=dev)       # destination row -> the loop's row
    writer[idx[ok]] = torch.arange(idx.numel(), device=dev)[ok]
    assert_same(K.scatter_rows(d, idx, rows_src), ref, rec, per_item=dim, item_of=writer)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_patch_unfold_wrapped(dev, layout, dt):
    rec = LP.get("patch_unfold")
    s = rec.wrapped
    B, C, H, W, p = s["B"], s["C"], s["H"], s["W"], s["p"]
    img = randn((B, C, H, W), dev, 12, dtype=dt)
    t = img.reshape(B, C, H // p, p, W // p, p)
    ref = t.permute(0, 2, 4, 3, 5, 1) if layout == 0 else t.permute(0, 2, 4, 1, 3, 5)
    ref = ref.reshape(B * (H // p) * (W // p), C * p * p).to(torch.bfloat16)
    assert_same(K.patch_unfold(img, p, layout), ref, rec)


# ---------------------------------------------------------------------------------------------- unfold / fold
def unfold_tap_major(x, ks, stride, pad):
    """F.unfold of an NCHW image, features reordered (c, ky, kx) -> (ky, kx, c): [B * L, ks * ks * C]."""
    B, C = x.shape[:2]
    u = F.unfold(x, ks, padding=pad, stride=stride)
    return u.reshape(B, C, ks * ks, -1).permute(0, 3, 2, 1).reshape(-1, ks * ks * C)


def check_conv_unfold(dev, rec, s, kind, seed):
    """kind: 'nchw_f32' (rounded once), 'nchw_bf16', 'nhwc_bf16' (copies).  Rounding commutes with the copy."""
    B, C, H, W, ks, stride, pad = (s[k] for k in ("B", "C", "H", "W", "ks", "stride", "pad"))
    x = randn((B, C, H, W), dev, seed)
    xb = x.to(torch.bfloat16)
    ref = unfold_tap_major(xb.float(), ks, stride, pad).to(torch.bfloat16)
    if kind == "nchw_f32":
        cols = K.conv_unfold(x, B, C, H, W, ks, stride, pad, nhwc=False)
    elif kind == "nchw_bf16":
        cols = K.conv_unfold(xb, B, C, H, W, ks, stride, pad, nhwc=False)
    else:
        cols = K.conv_unfold(xb.permute(0, 2, 3, 1).contiguous(), B, C, H, W, ks, stride, pad, nhwc=True)
    Fd, KP = ks * ks * C, LP.pad8(ks * ks * C)
    full = torch.zeros(ref.shape[0], KP, dtype=torch.bfloat16, device=dev)     # pad columns are zero
    full[:, :Fd] = ref
    assert_same(cols, full, rec, what=f"{kind} {s}")


def check_conv_fold(dev, rec, s, seed):
    B, C, H, W, ks, stride, pad = (s[k] for k in ("B", "C", "H", "W", "ks", "stride", "pad"))
    Ho, Wo = LP.conv_out(H, ks, stride, pad), LP.conv_out(W, ks, stride, pad)
    Fd, KP = ks * ks * C, LP.pad8(ks * ks * C)
    d = randint((B * Ho * Wo, KP), dev, seed)                        # integer-valued: the fp32 sums are exact in any order
    dcols = d[:, :Fd].reshape(B, Ho * Wo, ks, ks, C).permute(0, 4, 2, 3, 1).reshape(B, Fd, Ho * Wo)
    ref = F.fold(dcols, (H, W), ks, padding=pad, stride=stride).permute(0, 2, 3, 1).reshape(B * H * W, C)
    assert_same(K.conv_fold(d.to(torch.bfloat16), B, C, H, W, ks, stride, pad), ref.contiguous(), rec, what=str(s))


@pytest.mark.parametrize("case", [("nhwc_bf16", 0), ("nchw_f32", 1), ("nchw_bf16", 2)])
def test_conv_unfold_wrapped(dev, case):
    """C = 8 token rows: the 16-byte tap path; C = 3 fp32 image: KP padded 27 -> 32; C = 20 bf16 image: the generic path."""
    rec = LP.get("conv_unfold")
    kind, which = case
    check_conv_unfold(dev, rec, LP.shapes_of(rec)[which], kind, 20 + which)


def test_conv_fold_wrapped(dev):
    rec = LP.get("conv_fold")
    check_conv_fold(dev, rec, rec.wrapped, 23)


GEOMS = [(3, 2, 1), (3, 1, 1), (5, 2, 2), (7, 4, 3), (4, 3, 1)]      # (ks, stride, pad): the entry points take any ks <= 7


@pytest.mark.parametrize("ks,stride,pad", GEOMS)
def test_conv_unfold_and_fold_geometries(dev, ks, stride, pad):
    """Tiny shapes (one pass): every geometry x C in {3, 8, 20} (padded KP, the 16-byte tap path, the generic path) x the three
    source kinds; H != W and neither is a multiple of the stride."""
    for C in (3, 8, 20):
        s = {"B": 2, "C": C, "H": 13, "W": 10, "ks": ks, "stride": stride, "pad": pad}
        for j, kind in enumerate(("nchw_f32", "nchw_bf16", "nhwc_bf16")):
            check_conv_unfold(dev, LP.get("conv_unfold"), s, kind, 30 + C + j)
        check_conv_fold(dev, LP.get("conv_fold"), s, 40 + C)


@pytest.mark.parametrize("kind", ["nchw_f32", "nchw_bf16", "rows_bf16"])
def test_soft_split_fwd_wrapped(dev, kind):
    rec = LP.get("soft_split_fwd")
    s = rec.wrapped
    B, C, H, W, ks, stride, pad = (s[k] for k in ("B", "C", "H", "W", "ks", "stride", "pad"))
    x = randn((B, C, H, W), dev, 50)
    xb = x.to(torch.bfloat16)
    Fd, KP = ks * ks * C, LP.pad8(ks * ks * C)
    L = LP.conv_out(H, ks, stride, pad) * LP.conv_out(W, ks, stride, pad)
    full = torch.zeros(B * L, KP, dtype=torch.bfloat16, device=dev)                         # pad columns are zero
    for b in range(B):                                                                      # nn.Unfold's (c, ky, kx) order
        full[b * L:(b + 1) * L, :Fd] = F.unfold(xb[b:b + 1].float(), ks, padding=pad, stride=stride)[0].t()
    if kind == "rows_bf16":
        rows = torch.full((B * H * W, LP.pad8(C)), 77.0, dtype=torch.bfloat16, device=dev)  # pad columns are never read
        rows[:, :C] = xb.permute(0, 2, 3, 1).reshape(-1, C)
        cols = K.soft_split_fwd(rows, B, C, H, W, ks, stride, pad, rows=True)
    else:
        cols = K.soft_split_fwd(x if kind == "nchw_f32" else xb, B, C, H, W, ks, stride, pad, rows=False)
    assert_same(cols, full, rec, what=kind)


def test_soft_split_bwd_wrapped(dev):
    rec = LP.get("soft_split_bwd")
    s = rec.wrapped
    B, C, H, W, ks, stride, pad, ld = (s[k] for k in ("B", "C", "H", "W", "ks", "stride", "pad", "ld"))
    Ho, Wo = LP.conv_out(H, ks, stride, pad), LP.conv_out(W, ks, stride, pad)
    Fd, KP = ks * ks * C, LP.pad8(ks * ks * C)
    d = randint((B * Ho * Wo, KP), dev, 51)
    img = F.fold(d[:, :Fd].reshape(B, Ho * Wo, Fd).transpose(1, 2).contiguous(), (H, W), ks, padding=pad, stride=stride)
    ref = torch.zeros(B * H * W, ld, device=dev)                     # columns C .. ld - 1 are written as zeros
    ref[:, :C] = img.permute(0, 2, 3, 1).reshape(-1, C)
    assert_same(K.soft_split_bwd(d.to(torch.bfloat16), B, C, H, W, ks, stride, pad, ld=ld), ref, rec)


# ---------------------------------------------------------------------------------------------- stochastic depth
def _sd_shape(rec):
    s = rec.wrapped
    return s["samples"], s["rows_per_sample"], s["dim"]


def test_sd_add_wrapped(dev):
    rec = LP.get("sd_add")
    nb, per, dim = _sd_shape(rec)
    # multiples of 1/8 and factors keep / 0.5 in {0, 0.5, 1, 2, 3}: product and sum are exact in fp32, fused or not
    x, y = randint((nb * per, dim), dev, 60, -64, 65) / 8, randint((nb * per, dim), dev, 61, -64, 65) / 8
    keep = torch.tensor([0.0, 0.25, 0.5, 1.0, 1.5], device=dev)[torch.arange(nb, device=dev) % 5].contiguous()
    ref = x + y * (keep / 0.5).repeat_interleave(per)[:, None]
    assert_same(K.sd_add(x, y, keep, 0.5), ref, rec)
    # any data: the bound of test_window_attn_gpu.py (the compiler may fuse the multiplication into the addition)
    x, y = randn((nb * per, dim), dev, 62), randn((nb * per, dim), dev, 63)
    keep = (torch.arange(nb, device=dev) % 3 != 0).float()
    ref = x + y * (keep / 0.8).repeat_interleave(per)[:, None]
    assert_within((K.sd_add(x, y, keep, 0.8) - ref).abs(), 1e-6 + 1e-6 * ref.abs(), rec)


def test_sd_scale_wrapped(dev):
    rec = LP.get("sd_scale_bf16")
    nb, per, dim = _sd_shape(rec)
    dy = randn((nb * per, dim), dev, 64)
    keep = (torch.arange(nb, device=dev) % 3 != 0).float()
    ref = (dy * (keep / 0.8).repeat_interleave(per)[:, None]).to(torch.bfloat16)
    assert_same(K.sd_scale_bf16(dy, keep, 0.8), ref, rec)


# ---------------------------------------------------------------------------------------------- AdamW, batch norm
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_adamw_wrapped(dev, gdt):
    """clip_grad_norm_ + torch.optim.AdamW, three steps, 2e-6 of the largest value (test_optim_gpu.py), per element."""
    rec = LP.get("adamw_flat")
    n = rec.wrapped["n"]
    assert n % 4 == 3
    p = randn((n,), dev, 70)
    ref_p = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([ref_p], lr=3e-3, weight_decay=0.05, eps=1e-8, betas=(0.9, 0.999))
    m, v, gn = torch.zeros_like(p), torch.zeros_like(p), torch.zeros(1, device=dev)
    ws = torch.empty(max(K.sumsq_workspace(n) // 4, 4), device=dev)
    for step in range(1, 4):
        g = randn((n,), dev, 70 + step, 0.1).to(gdt)
        ref_p.grad = g.float().clone()                               # clip_grad_norm_ scales it in place
        total = torch.nn.utils.clip_grad_norm_([ref_p], 1.0)
        opt.step()
        K.sumsq(g, gn, ws)
        assert abs(gn.sqrt().item() - total.item()) <= 2e-6 * total.item()
        K.adamw_flat(p, g, m, v, 3e-3, 0.9, 0.999, 1e-8, 0.05, step, gn, 1.0)
        r = ref_p.data
        assert_within((p - r).abs(), 2e-6 * r.abs().max().item(), rec, what=f"p after step {step}")
    st = opt.state[ref_p]
    for got, ref, what in ((m, st["exp_avg"], "m"), (v, st["exp_avg_sq"], "v")):
        assert_within((got - ref).abs(), 2e-6 * ref.abs().max().item(), rec, what=what)


def test_bn_apply_wrapped(dev):
    """F.batch_norm in float64, 2e-4 of the largest value (test_bn_rows_gpu.py): fp32 and bf16 outputs, Hardswish, residual
    + per-sample keep."""
    rec = LP.get("bn_apply")
    T, C = rec.wrapped["T"], rec.wrapped["C"]
    assert T % 8 == 0
    y = randn((T, C), dev, 80) * (0.5 + torch.rand(C, generator=gen(dev, 81), device=dev)) + randn((C,), dev, 82)
    gamma, beta = 1 + randn((C,), dev, 83, 0.2), randn((C,), dev, 84, 0.2)
    mean, invstd, _ = K.bn_stats(y, EPS, 0.1)
    ref = F.batch_norm(y.double(), None, None, gamma.double(), beta.double(), True, 0.1, EPS)
    tol = 2e-4 * ref.abs().max().item()
    z32, z16 = K.bn_apply(y, mean, invstd, gamma, beta, want_f32=True)
    assert_within((z32.double() - ref).abs(), tol, rec, what="fp32")
    assert_same(z16, z32.to(torch.bfloat16), rec, what="bf16")
    h32, h16 = K.bn_apply(y, mean, invstd, gamma, beta, act=True, want_f32=True)
    assert_within((h32.double() - F.hardswish(ref)).abs(), tol, rec, what="hardswish fp32")
    assert_same(h16, h32.to(torch.bfloat16), rec, what="hardswish bf16")
    del h32, h16, z32, z16
    res = randn((T, C), dev, 85)
    keep = (torch.arange(8, device=dev) % 3 != 0).float()
    o32, o16 = K.bn_apply(y, mean, invstd, gamma, beta, residual=res, keep=keep, survival=0.9, want_f32=True)
    want = res.double() + ref * (keep / 0.9).repeat_interleave(T // 8)[:, None].double()
    assert_within((o32.double() - want).abs(), tol, rec, what="residual + keep fp32")
    assert_same(o16, o32.to(torch.bfloat16), rec, what="residual + keep bf16")


# ---------------------------------------------------------------------------------------------- LayerNorm
def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def row_err(got, ref64):
    """Relative L2 error of every row against float64."""
    return (got.double() - ref64).norm(dim=1) / ref64.norm(dim=1).clamp_min(1e-300)


def check_rule(what, e_kernel, e_torch, rec, bf16=False):
    """e_kernel, e_torch: one error per row (or per column).  The largest kernel error against max(4 x the largest fp32-torch
    error, 8 * 2^-23) [+ 2^-8]; prints both."""
    ek, et = float(e_kernel.max()), float(e_torch.max())
    bound = max(4 * et, FLOOR) + (BF16 if bf16 else 0.0)
    print(f"{what}: kernel {ek:.3e}  torch fp32 {et:.3e}  bound {bound:.3e}")
    if not ek <= bound:
        bad = ~(e_kernel <= bound)
        raise AssertionError(f"{what}: kernel {ek:.3e} > bound {bound:.3e} (torch fp32 {et:.3e}); " + where_bad(bad, rec, 1))


def ln_inputs(rows, dim, xdt, dev):
    x = randn((rows, dim), dev, 3, 2.0, 0.5).to(xdt)
    gamma = randn((dim,), dev, 4, 0.5, 1.0)
    beta = randn((dim,), dev, 5, 0.5)
    return x, gamma, beta


def ln_backward_inputs(x, dev, dres_dt):
    """dy with a mean and a component along x^ (no column sum of dy or dy * x^ cancels), the residual-stream gradient."""
    xh = F.layer_norm(x.float(), (x.shape[1],), None, None, EPS)
    dy = (randn(tuple(x.shape), dev, 6, 0.5, 0.75) + 0.5 * xh).to(torch.bfloat16)
    dres = None if dres_dt is None else randn(tuple(x.shape), dev, 7).to(dres_dt)
    return dy, dres


def ln_forward_check(name, rec, x, gamma, beta, y, mean, rstd, chunk=4096):
    """y / mean / rstd of a kernel against F.layer_norm in float64 (and torch's fp32 evaluation of it), in row chunks."""
    rows, dim = x.shape
    ek, et, em, er, ert = [], [], [], [], []
    for r0 in range(0, rows, chunk):
        xc = x[r0:r0 + chunk]
        x64 = xc.double()
        y64 = F.layer_norm(x64, (dim,), gamma.double(), beta.double(), EPS)
        y32 = F.layer_norm(xc.float(), (dim,), gamma, beta, EPS)
        yk = y[r0:r0 + chunk]
        # fp32 math, one bf16 rounding on store: |err| <= 2^-8 relative per element (test_layernorm_fwd_bwd)
        bad = ~((yk.double() - y64).abs() <= y64.abs() * 2 ** -8 + 1e-6)
        if bool(bad.any()):
            bad_all = torch.zeros(rows, dim, dtype=torch.bool, device=x.device)
            bad_all[r0:r0 + chunk] = bad
            raise AssertionError(f"{name} y elementwise: " + where_bad(bad_all, rec, dim))
        ek.append(row_err(yk, y64)); et.append(row_err(y32, y64))
        m64 = x64.mean(1)
        rs64 = (x64.var(1, unbiased=False) + EPS).rsqrt()
        em.append((mean[r0:r0 + chunk].double() - m64).abs().max() / m64.abs().max())
        er.append((rstd[r0:r0 + chunk].double() - rs64).abs() / rs64)
        x32 = xc.float()
        ert.append(((x32.var(1, unbiased=False) + EPS).rsqrt().double() - rs64).abs() / rs64)
    assert float(torch.stack(em).max()) < 1e-5, (name, "mean")
    check_rule(f"{name} y per row", torch.cat(ek), torch.cat(et), rec, bf16=True)
    check_rule(f"{name} rstd per row", torch.cat(er), torch.cat(ert), rec)


def ln_backward_ref(x, gamma, beta, dy, dres, dtype, chunk):
    """dx [+ dres], dgamma, dbeta by autograd of F.layer_norm in `dtype`; in row chunks (the column sums accumulate)."""
    rows, dim = x.shape
    g = gamma.to(dtype).requires_grad_(True)
    b = beta.to(dtype).requires_grad_(True)
    dx = torch.empty(rows, dim, dtype=dtype, device=x.device)
    for r0 in range(0, rows, chunk):
        xc = x[r0:r0 + chunk].to(dtype).requires_grad_(True)
        F.layer_norm(xc, (dim,), g, b, EPS).backward(dy[r0:r0 + chunk].to(dtype))
        dx[r0:r0 + chunk] = xc.grad if dres is None else xc.grad + dres[r0:r0 + chunk].to(dtype)
    return dx, g.grad, b.grad


def ln_backward_check(name, rec, rows, got, ref64, ref32):
    dx32, dx16, dg, db = got
    rdx, rdg, rdb = ref64
    tdx, tdg, tdb = ref32
    # the whole-tensor bounds of test_layernorm_fwd_bwd
    assert rel_err(dx32, rdx) < 2e-5, (name, rel_err(dx32, rdx))
    assert rel_err(dx16, rdx) < 2 ** -7, (name, rel_err(dx16, rdx))
    assert rel_err(dg, rdg) < 2e-5 * math.sqrt(rows), (name, rel_err(dg, rdg))
    assert rel_err(db, rdb) < 2e-5 * math.sqrt(rows), (name, rel_err(db, rdb))
    et = row_err(tdx, rdx)
    check_rule(f"{name} dx fp32 per row", row_err(dx32, rdx), et, rec)
    check_rule(f"{name} dx bf16 per row", row_err(dx16, rdx), et, rec, bf16=True)
    for what, k, t, r in (("dgamma", dg, tdg, rdg), ("dbeta", db, tdb, rdb)):
        check_rule(f"{name} {what} per column", (k.double() - r).abs() / r.abs(), (t.double() - r).abs() / r.abs(), rec)


def _ln_rec(kind, dim):
    return LP.get(f"layernorm_{kind}" + ("_half_wave" if LP.LN_DIMS[dim][0] == 32 else ""))


@pytest.mark.parametrize("xdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dim", sorted(LP.LN_DIMS))
def test_layernorm_fwd_wrapped(dev, dim, xdt):
    rec = _ln_rec("fwd", dim)
    rows = rec.wrapped["rows"]
    x, gamma, beta = ln_inputs(rows, dim, xdt, dev)
    y, mean, rstd = K.layernorm_fwd(x, gamma, beta, EPS)
    ln_forward_check(f"ln_fwd [{rows} x {dim}] {str(xdt)[6:]}", rec, x, gamma, beta, y, mean, rstd)


@pytest.mark.parametrize("dres_dt", [None, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("xdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dim", sorted(LP.LN_DIMS))
def test_layernorm_bwd_wrapped(dev, dim, xdt, dres_dt):
    """Every wave carries its dgamma / dbeta column partials over the two or three rows (pairs of rows) it walks."""
    rec = _ln_rec("bwd", dim)
    rows = rec.wrapped["rows"]
    x, gamma, beta = ln_inputs(rows, dim, xdt, dev)
    dy, dres = ln_backward_inputs(x, dev, dres_dt)
    _, mean, rstd = K.layernorm_fwd(x, gamma, beta, EPS)
    got = K.layernorm_bwd(dy, x, gamma, mean, rstd, dres=dres, want_f32=True, want_bf16=True)
    ref64 = ln_backward_ref(x, gamma, beta, dy, dres, torch.float64, 2048)
    ref32 = ln_backward_ref(x, gamma, beta, dy, dres, torch.float32, rows)
    name = f"ln_bwd [{rows} x {dim}] x {str(xdt)[6:]} dres {str(dres_dt)[6:] if dres_dt else 'none'}"
    ln_backward_check(name, rec, rows, got, ref64, ref32)
    if dres_dt is None and xdt == torch.float32:
        # accumulate=True adds the (bit-reproducible) column sums to the gradients already there
        dg, db = got[2], got[3]
        _, _, dg2, db2 = K.layernorm_bwd(dy, x, gamma, mean, rstd, dgamma=dg.clone(), dbeta=db.clone(), accumulate=True)
        assert rel_err(dg2, 2 * ref64[1]) < 1e-4 and rel_err(db2, 2 * ref64[2]) < 1e-4
        assert torch.equal(dg2, 2 * dg) and torch.equal(db2, 2 * db)


@pytest.mark.parametrize("dres_dt", [None, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("xdt", [torch.float32, torch.bfloat16])
def test_layernorm_pad_wrapped(dev, xdt, dres_dt):
    """n = 147 true columns of ld = 152: the third 64-lane step of a row is partial, the pad columns come out as zeros."""
    rec = LP.get("layernorm_pad_fwd")
    assert LP.get("layernorm_pad_bwd").wrapped == rec.wrapped and LP.get("layernorm_pad_bwd").threshold == rec.threshold
    rows, n = rec.wrapped["rows"], rec.wrapped["n"]
    ld = LP.pad8(n)
    assert n % 64 and n % 4
    xt, gamma, beta = ln_inputs(rows, n, xdt, dev)
    dyt, drest = ln_backward_inputs(xt, dev, dres_dt)
    x = torch.zeros(rows, ld, dtype=xdt, device=dev)
    x[:, :n] = xt
    y, mean, rstd = K.layernorm_pad_fwd(x, n, gamma, beta, EPS)
    name = f"ln_pad [{rows} x {n} of {ld}] x {str(xdt)[6:]} dres {str(dres_dt)[6:] if dres_dt else 'none'}"
    assert_same(y[:, n:], torch.zeros_like(y[:, n:]), rec, per_item=ld - n, what="pad columns of y")
    ln_forward_check(name, rec, xt, gamma, beta, y[:, :n], mean, rstd, chunk=rows)
    dy = torch.zeros(rows, ld, dtype=torch.bfloat16, device=dev)
    dy[:, :n] = dyt
    dres = None
    if drest is not None:
        dres = torch.zeros(rows, ld, dtype=dres_dt, device=dev)
        dres[:, :n] = drest
    dx32, dx16, dg, db = K.layernorm_pad_bwd(dy, x, n, gamma, mean, rstd, dres=dres, want_f32=True, want_bf16=True)
    for t, what in ((dx32, "dx fp32"), (dx16, "dx bf16")):
        assert_same(t[:, n:], torch.zeros_like(t[:, n:]), rec, per_item=ld - n, what="pad columns of " + what)
    ref64 = ln_backward_ref(xt, gamma, beta, dyt, drest, torch.float64, rows)
    ref32 = ln_backward_ref(xt, gamma, beta, dyt, drest, torch.float32, rows)
    ln_backward_check(name, LP.get("layernorm_pad_bwd"), rows, (dx32[:, :n], dx16[:, :n], dg, db), ref64, ref32)
