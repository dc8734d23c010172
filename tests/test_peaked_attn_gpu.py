"""GPU: the ViT attention kernels on PEAKED inputs, per key, against the float64 definition (tests/peaked_ref.py).

Every query scores chosen keys 12 - 20 nats below the rest.  Softmax gives such a key weights e^-15 .. e^-29; the Sinkhorn column
steps rescale its column back to sum 1, so under robust=True it ends with O(1/N) weights and dK / dV rows as large as any other
key's.  A kernel that loses the small P0 entries (a narrow resident copy, a flush, a mask) is wrong on exactly those keys, and a
whole-tensor norm on randn input (tests/test_kernels_gpu.py) cannot see it: one key is 1/N of that norm.

Bounds (conditions, none of them tuned on a kernel):
  dq / dk / dv of the Sinkhorn paths   relative L2 of EVERY (batch, head, token) row <= 3e-2 against fp64 -- the per-key figure of
                                       test_bias_attn_gpu.py / test_window_attn_gpu.py.  tests/test_peaked_ref_host.py shows that
                                       rounding P, dS and the outputs to bf16 alone costs <= 1e-2 per row on these inputs (measured
                                       5.1e-3), and that torch fp32 is within 1e-5: a 3 x margin over what the format costs.
  o                                    max error of every query row <= 2^-6 of the tensor's max (P and o are bf16)
  lse                                  1e-4 max(1, |lse|_max), the figure of the existing streaming / composed tests (fp32 from bf16 operands)
  saved scalings                       relative, element-wise, <= 1e-3 (b3 of a -20 nat key is ~1e9; fp32 sums of N exponentials over
                                       7 compounding steps; the figure of the fused-vs-composed test)
  sinkhorn_fwd / bwd (fp32 on fp32)    test_talking_heads_gpu.py's rule per row AND per column: kernel error vs fp64 <= 4 x the
                                       worst row (column) of a torch fp32 evaluation of the same definition, floor 8 * 2^-23
  softmax controls                     dq per row as above; dk / dv rows as |got - ref| <= 3e-2 x the LARGEST row norm of the tensor:
                                       a weak key's rows are genuinely tiny there, so they are not compared relative to themselves
No row is skipped: a reference row of norm zero is asserted not to exist.

Measured on an MI355X (relative L2 per row against fp64; fused Sinkhorn pair):

  shape (B,N,H,dh)   at 60009cf (P0 resident as fp16)            at the commit that made it bf16
                     worst dq row | weak keys' dq rows           worst row dq / dk / dv | weak keys, max over dq dk dv
  (2,197,2,64)       1.84 | 0.39 0.37                            4.8e-3 / 5.3e-3 / 5.3e-3 | 3.5e-3
  (1,256,2,64)       1.76 | 0.33 0.32                            7.3e-3 / 5.6e-3 / 4.6e-3 | 3.6e-3
  (2,49,2,64)        1.26 | 0.65 0.29                            5.3e-3 / 5.1e-3 / 4.8e-3 | 3.7e-3
  (2,196,1,64)       1.09 | 0.31 0.019                           6.0e-3 / 4.8e-3 / 4.2e-3 | 3.5e-3
  (1,65,1,64)        0.99 | 0.61 0.53 0.045                      5.9e-3 / 4.4e-3 / 4.9e-3 | 4.4e-3
  (45,197,6,64)      1.40 | 0.91 1.11                            8.8e-3 / 7.7e-3 / 6.2e-3 | 5.4e-3
  composed, 4 shapes + keep / bias (both commits)                worst row <= 5.7e-3, weak keys <= 3.5e-3
  softmax controls (both commits)                                dq <= 4.0e-3; dk / dv <= 3.2e-3 of the largest row, weak keys <= 1.4e-8
  sinkhorn_fwd / bwd, 60-nat column: P 2.2e-6, dS 2.6e-6 per column (bound 4.6e-6 / 4.9e-6)
  saved bvec at (4,197,197) / (2,577,577) / (3,50,81), bounds 1.4e-6 / 9.5e-7 / 9.5e-7:
      with __expf 1.4e-6 / 9.3e-7 / 2.8e-6 (two over);  with the two-float exponent 3.4e-7 / 2.5e-7 / 6.6e-7
  a key 120 nats down (treated as absent), fused and composed: worst row of dq / dk / dv <= 6.0e-3 against the definition without it
(at 60009cf the run stopped at dq, so dk / dv were not printed; the whole-tensor randn check passed on both.)
"""
import pytest
import torch

import peaked_ref as PR
from noise_robust_vit_amd import kernels as K

pytestmark = pytest.mark.gpu

FLOOR = 8 * 2.0 ** -23


def _dout(B, N, H, dh, dev, seed=11):
    return torch.randn(B * N, H * dh, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).to(dev)


def _rows(tag, name, err, weak, bound, defer=None):
    """Print and assert the worst row and the weak keys' rows (err: [B, H, N])."""
    assert bool(torch.isfinite(err).all()), (tag, name, "a reference row of norm zero or a non-finite kernel row")
    worst = err.max().item()
    at = tuple(int(i) for i in torch.nonzero(err == err.max())[0])
    wk = {j: err[..., j].max().item() for j, _ in weak}
    print(f"{tag} {name}: worst row {worst:.3e} at (b, h, token) {at}   weak keys " + "  ".join(f"{j}: {e:.3e}" for j, e in wk.items()))
    bad = [(tag, name, f"weak key {j}", e) for j, e in wk.items() if not e <= bound]
    if not worst <= bound:
        bad.append((tag, name, f"worst row {at}", worst))
    if defer is not None:                                   # the caller prints every tensor's figures before it asserts
        defer.extend(bad)
    else:
        assert not bad, bad


def _check_forward(tag, ref, out, lse, B, N, H, dh, weak):
    o = PR.heads(out.cpu().double(), B, N, H, dh)[0]
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse).all()), tag
    err = (o - ref["o"]).abs().amax(dim=-1) / ref["o"].abs().max()
    _rows(tag, "o (max err / tensor max)", err, weak, 2.0 ** -6)
    e_lse = (lse.cpu().double().reshape(B, H, N) - ref["lse"]).abs().max().item()
    print(f"{tag} lse: {e_lse:.3e}")
    assert e_lse <= 1e-4 * max(1.0, ref["lse"].abs().max().item()), (tag, e_lse)


def _check_scalings(tag, qkv, scal, B, N, H, dh, scale, weak):
    q, k, _ = PR.heads(qkv.cpu().double(), B, N, H, dh)
    av, bv = PR.sinkhorn_scalings(q @ k.transpose(-1, -2) * scale)
    ref = torch.empty(B, H, 7, N, dtype=torch.float64)
    ref[:, :, 0::2], ref[:, :, 1::2] = av, bv
    rel = (scal.cpu().double() - ref).abs() / ref.abs()
    print(f"{tag} scalings: worst relative {rel.max().item():.3e}   b3 of the weak keys " +
          "  ".join(f"{j}: {ref[:, :, 5, j].max().item():.2e} (rel {rel[:, :, :, j].max().item():.2e})" for j, _ in weak))
    assert rel.max().item() <= 1e-3, (tag, rel.max().item())


def _check_grads(tag, ref, dqkv, B, N, H, dh, weak, bound=PR.PER_ROW_BOUND, softmax_control=False):
    got = PR.heads(dqkv.cpu().double(), B, N, H, dh)
    bad = []
    for i, name in enumerate(("dq", "dk", "dv")):
        assert bool((ref[name].norm(dim=-1) > 0).all()), (tag, name, "zero reference row for a real token")
        if softmax_control and name != "dq":
            _rows(tag, name + " (|err| / largest row)", PR.per_row_abs_vs_largest(got[i], ref[name]), weak, bound, bad)
        else:
            _rows(tag, name, PR.per_row_rel(got[i], ref[name]), weak, bound, bad)
    assert not bad, bad


def _sinkhorn_case(dev, B, N, H, dh, weak, tag, saved=None, seed=2, between=None):
    scale = dh ** -0.5
    qkv = PR.peaked_qkv(B, N, H, dh, weak, seed=seed).to(dev)
    dout = _dout(B, N, H, dh, dev)
    if saved is None:
        out, lse, scal = K.attn_sinkhorn_fwd(qkv, B, N, H, dh, scale)
        dqkv = K.attn_sinkhorn_bwd(qkv, dout, lse, scal, B, N, H, dh, scale)
    else:                                                   # as encoder.attn_half_fwd / attn_half_bwd call the pair
        out, lse, scal = K.attn_sinkhorn_fwd(qkv, B, N, H, dh, scale, saved=saved)
        if between is not None:
            between()
        dqkv = K.attn_sinkhorn_bwd(qkv, dout, lse, scal, B, N, H, dh, scale, saved=saved)
    ref = PR.attention_reference(qkv, dout, B, N, H, dh, scale)
    _check_forward(tag, ref, out, lse, B, N, H, dh, weak)
    _check_scalings(tag, qkv, scal, B, N, H, dh, scale, weak)
    _check_grads(tag, ref, dqkv, B, N, H, dh, weak)


# ------------------------------------------------------------------ fused Sinkhorn kernels (csrc/nrv_sinkhorn.hip)
@pytest.mark.parametrize("B,N,H,dh,weak", PR.FUSED_CASES)
def test_fused_sinkhorn_peaked_keys(dev, B, N, H, dh, weak):
    assert K._sinkhorn_fused_shape(N, dh)
    _sinkhorn_case(dev, B, N, H, dh, weak, f"fused {(B, N, H, dh)}")


def test_fused_sinkhorn_peaked_keys_over_many_heads(dev):
    """270 heads on 256 CUs: the persistent walk's prefetch slots see the peaked operands (every head, every key)."""
    B, N, H, dh, weak = PR.MANY_HEADS_CASE
    _sinkhorn_case(dev, B, N, H, dh, weak, f"fused persistent {(B, N, H, dh)}")


@pytest.mark.parametrize("B,N,H,dh", [(2, 197, 2, 64), (2, 257, 2, 80)])
def test_sinkhorn_peaked_keys_with_the_saved_dict(dev, B, N, H, dh):
    """The pair as the encoder calls it: one dict handed to the forward and to the backward.  The composed path leaves its P7 image
    in it (asserted between the two calls) and the backward consumes it; the fused kernels never touch it."""
    weak = PR.std_weak(N)
    saved = {}
    fused = K._sinkhorn_fused_shape(N, dh)

    def between():
        if fused:
            assert saved == {}
        else:
            assert tuple(saved["P7"].shape) == (B, H, N, N) and saved["P7"].dtype == torch.float32

    _sinkhorn_case(dev, B, N, H, dh, weak, f"saved dict {(B, N, H, dh)}", saved=saved, between=between)
    assert saved == {}                                    # consumed (composed) or never written (fused)


@pytest.mark.parametrize("B,N,H,dh,j", [(2, 197, 2, 64, 77), (1, 256, 1, 64, 255), (2, 257, 2, 80, 100)])
def test_sinkhorn_attention_key_that_underflows_completely_gives_zeros(dev, B, N, H, dh, j):
    """The deliberate deviation of DESIGN.md section 4 on the attention pairs (fused and composed): key j is 120 nats below the rest
    for every query, its fp32 softmax weights are exactly zero, and the definition divides 0 by 0 in the first column step.  The
    kernels treat the key as absent: finite results, zero dk / dv rows for it, everything else as the definition without that key."""
    weak = ((5, 12.0), (j, 120.0))
    scale = dh ** -0.5
    tag = f"underflowed key {(B, N, H, dh)}"
    qkv = PR.peaked_qkv(B, N, H, dh, weak, seed=16).to(dev)
    dout = _dout(B, N, H, dh, dev)
    out, lse, scal = K.attn_sinkhorn_fwd(qkv, B, N, H, dh, scale)
    dqkv = K.attn_sinkhorn_bwd(qkv, dout, lse, scal, B, N, H, dh, scale)
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(scal).all()) and bool(torch.isfinite(dqkv.float()).all()), tag
    ref = PR.attention_reference(qkv, dout, B, N, H, dh, scale, drop_keys=(j,))
    _check_forward(tag, ref, out, lse, B, N, H, dh, weak[:1])
    got = PR.heads(dqkv.cpu().double(), B, N, H, dh)
    bad = []
    for i, name in enumerate(("dq", "dk", "dv")):
        if name != "dq":
            assert bool((got[i][:, :, j] == 0).all()) and bool((ref[name][:, :, j] == 0).all()), (tag, name, "the absent key's row")
        err = PR.per_row_rel(got[i], ref[name])           # 0 where both rows are zero, inf where only the reference's is
        nonzero = ref[name].norm(dim=-1) > 0
        assert int((~nonzero).sum()) == (0 if name == "dq" else B * H), (tag, name)
        _rows(tag, name, err, weak[:1], PR.PER_ROW_BOUND, bad)
    assert not bad, bad


def test_fused_sinkhorn_peaked_keys_rerun_is_bit_identical(dev):
    B, N, H, dh = 2, 197, 3, 64
    scale = dh ** -0.5
    qkv = PR.peaked_qkv(B, N, H, dh, PR.std_weak(N), seed=5).to(dev)
    dout = _dout(B, N, H, dh, dev)
    runs = []
    for _ in range(2):
        out, lse, scal = K.attn_sinkhorn_fwd(qkv, B, N, H, dh, scale)
        runs.append((out, lse, scal, K.attn_sinkhorn_bwd(qkv, dout, lse, scal, B, N, H, dh, scale)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_fused_against_composed_on_peaked_keys_per_key(dev):
    """Same rounding points (P7 and dS enter their products in bf16), other summation orders: each side's rounding costs <= 1e-2 per
    row (tests/test_peaked_ref_host.py), so two such evaluations differ by <= 2e-2 in every row."""
    B, N, H, dh = 2, 197, 3, 64
    weak = PR.std_weak(N)
    scale = dh ** -0.5
    qkv = PR.peaked_qkv(B, N, H, dh, weak, seed=6).to(dev)
    dout = _dout(B, N, H, dh, dev)
    o1, lse1, scal1 = K.attn_sinkhorn_fwd(qkv, B, N, H, dh, scale)
    d1 = K.attn_sinkhorn_bwd(qkv, dout, lse1, scal1, B, N, H, dh, scale)
    o2, lse2, scal2 = K._attn_sinkhorn_fwd_composed(qkv, B, N, H, dh, scale)
    d2 = K._attn_sinkhorn_bwd_composed(qkv, dout, lse2, scal2, B, N, H, dh, scale)
    assert (lse1 - lse2).abs().max().item() < 1e-4
    assert ((scal1 - scal2).abs() / scal2.abs()).max().item() < 1e-3
    eo = (o1.float() - o2.float()).abs().reshape(B, N, H, dh).amax(dim=-1) / o2.float().abs().max()
    assert eo.max().item() <= 2.0 ** -6, eo.max().item()
    g1, g2 = PR.heads(d1.cpu().double(), B, N, H, dh), PR.heads(d2.cpu().double(), B, N, H, dh)
    for i, name in enumerate(("dq", "dk", "dv")):
        _rows("fused vs composed", name, PR.per_row_rel(g1[i], g2[i]), weak, 2e-2)


# ------------------------------------------------------------------ composed Sinkhorn (nrv_bgemm + csrc/nrv_sinknorm.hip)
@pytest.mark.parametrize("B,N,H,dh,weak", PR.COMPOSED_CASES)
def test_composed_sinkhorn_peaked_keys(dev, B, N, H, dh, weak):
    assert not K._sinkhorn_fused_shape(N, dh)
    _sinkhorn_case(dev, B, N, H, dh, weak, f"composed {(B, N, H, dh)}")


@pytest.mark.parametrize("iters", [0, 3])
@pytest.mark.parametrize("variant", ["keep", "bias", "keep+bias"])
def test_composed_with_dropout_mask_and_score_bias_peaked_keys(dev, iters, variant):
    """attn_composed_fwd / bwd: a keep mask on the weights, and a score bias that ITSELF carries the -12 / -20 (the operands are
    plain randn with the u component of q and k removed, so the bias is the only thing that makes keys 5 and 77 weak)."""
    B, N, H, dh = 2, 197, 2, 64
    weak = PR.std_weak(N)
    scale = dh ** -0.5
    g = torch.Generator().manual_seed(40 + iters)
    bias = keep = None
    pscale = 1.0
    if "bias" in variant:
        qkv = PR.peaked_qkv(B, N, H, dh, (), seed=7).to(dev)
        bias = 0.5 * torch.randn(1, H, N, N, generator=g)
        for j, nats in weak:
            bias[..., j] -= nats
    else:
        qkv = PR.peaked_qkv(B, N, H, dh, weak, seed=7).to(dev)
    if "keep" in variant:
        keep = (torch.rand(B, H, N, N, generator=g) >= 0.2).to(torch.uint8)
        pscale = 1.0 / 0.8
    dout = _dout(B, N, H, dh, dev)
    tag = f"composed {variant} iters={iters}"
    out, cs = K.attn_composed_fwd(qkv, B, N, H, dh, scale, iters, keep=None if keep is None else keep.to(dev), pscale=pscale,
                                  bias=None if bias is None else bias.to(dev))
    lse = cs.lse.reshape(B, H, N)
    dqkv = K.attn_composed_bwd(qkv, dout, cs, B, N, H, dh, scale)
    ref = PR.attention_reference(qkv, dout, B, N, H, dh, scale, iters=iters, bias=bias, keep=keep, pscale=pscale)
    _check_forward(tag, ref, out, lse, B, N, H, dh, weak)
    _check_grads(tag, ref, dqkv, B, N, H, dh, weak, softmax_control=iters == 0)


# ------------------------------------------------------------------ SinkhornAttention on materialised scores (CaiT's robust path)
def _four_x_rule(tag, name, got, f32, f64, weak):
    """Per row and per column: the kernel's relative L2 against fp64 may be at most 4 x the worst row (column) of torch's own fp32
    evaluation (another summation order), floor 8 * 2^-23."""
    for dim, what in ((-1, "row"), (-2, "column")):
        g, a, r = (t.detach().cpu().double().transpose(-1, dim) if dim == -2 else t.detach().cpu().double() for t in (got, f32, f64))
        e_k, e_t = PR.per_row_rel(g, r), PR.per_row_rel(a, r)
        assert bool(torch.isfinite(e_k).all()), (tag, name, what)
        bound = max(4 * e_t.max().item(), FLOOR)
        msg = f"{tag} {name} per {what}: kernel {e_k.max().item():.3e}  torch fp32 {e_t.max().item():.3e}  bound {bound:.3e}"
        if what == "column":
            msg += "   weak columns " + "  ".join(f"{j} (-{n:g}): {e_k[..., j].max().item():.3e}" for j, n in weak)
            for j, _ in weak:
                assert e_k[..., j].max().item() <= bound, (tag, name, f"weak column {j}", e_k[..., j].max().item(), bound)
        print(msg)
        assert e_k.max().item() <= bound, (tag, name, what, e_k.max().item(), bound)


@pytest.mark.parametrize("shape,weak", [((4, 197, 197), ((5, 12.0), (77, 20.0), (130, 60.0))),
                                        ((2, 577, 577), ((5, 12.0), (77, 20.0), (576, 60.0))),
                                        ((3, 50, 81), ((5, 12.0), (77, 20.0), (80, 60.0))),
                                        ((1, 1, 1025), ((5, 12.0), (77, 20.0), (1024, 60.0)))])
def test_sinkhorn_module_on_peaked_scores(dev, shape, weak):
    """sinkhorn_fwd / sinkhorn_bwd on fp32 scores with columns down by 12, 20 and 60 nats (fp32 softmax still represents e^-65).  One
    query (1 x 1025): the column step makes every entry 1, the row step makes the row uniform, whatever the scores."""
    tag = f"module {shape}"
    S = PR.peaked_scores(shape, weak, seed=8)
    W = torch.randn(shape, generator=torch.Generator().manual_seed(9))
    P, lse, avec, bvec = K.sinkhorn_fwd(S.to(dev), iters=3)
    dS = K.sinkhorn_bwd(S.to(dev), W.to(dev), lse, avec, bvec, iters=3)
    res = {}
    for dt in (torch.float32, torch.float64):
        s = S.clone().to(dt).requires_grad_(True)
        p = PR.sinkhorn_definition(s, 3)
        (p * W.to(dt)).sum().backward()
        av, bv = PR.sinkhorn_scalings(s.detach(), 3)
        res[dt] = (p.detach(), s.grad, av, bv)
    P32, dS32, a32, b32 = res[torch.float32]
    P64, dS64, a64, b64 = res[torch.float64]
    assert bool(torch.isfinite(P).all()) and bool(torch.isfinite(dS).all())
    if shape[-2] == 1:
        assert (P.cpu().double() - 1.0 / shape[-1]).abs().max().item() <= FLOOR / shape[-1]
    _four_x_rule(tag, "P", P, P32, P64, weak)
    if shape[-2] > 1:                                      # one query: dS is exactly zero in the definition (P does not depend on S)
        _four_x_rule(tag, "dS", dS, dS32, dS64, weak)
    else:                                                  # 8 fp32 sums over C terms, each with ~ sqrt(C) 2^-24 of round-off, on values ~ |W| / C
        e = dS.abs().max().item()
        print(f"{tag} dS (exactly zero in the definition): {e:.3e}")
        assert e <= 8 * shape[-1] ** 0.5 * 2.0 ** -24 * W.abs().max().item() / shape[-1]
    G = S.numel() // (shape[-2] * shape[-1])
    for name, got, f32, f64 in (("avec", avec.reshape(a64.shape), a32, a64), ("bvec", bvec.reshape(b64.shape), b32, b64)):
        e_k = ((got.cpu().double() - f64).abs() / f64.abs()).max().item()
        e_t = ((f32.double() - f64).abs() / f64.abs()).max().item()
        bound = max(4 * e_t, FLOOR)
        print(f"{tag} {name} (element-wise relative, G = {G}): kernel {e_k:.3e}  torch fp32 {e_t:.3e}  bound {bound:.3e}  largest {f64.max().item():.2e}")
        assert e_k <= bound, (tag, name, e_k, bound)


def test_sinkhorn_module_column_that_underflows_completely_gives_zeros(dev):
    """A deliberate deviation: a column at -inf (or >= 110 nats down) has P0 = 0 for every query, the definition divides
    0 by 0 there and is NaN everywhere after the next row step; the kernels return that column as zeros (inv_or_zero) and every
    other column as the definition evaluated without it."""
    shape, j = (3, 50, 81), 33
    S = PR.peaked_scores(shape, ((5, 12.0),), seed=10)
    S[..., j] = float("-inf")
    W = torch.randn(shape, generator=torch.Generator().manual_seed(15))
    P, lse, avec, bvec = K.sinkhorn_fwd(S.to(dev), iters=3)
    dS = K.sinkhorn_bwd(S.to(dev), W.to(dev), lse, avec, bvec, iters=3).cpu()
    P = P.cpu()
    assert bool(torch.isfinite(P).all()) and bool((P[..., j] == 0).all())
    assert bool(torch.isfinite(dS).all()) and bool((dS[..., j] == 0).all())
    others = [c for c in range(shape[-1]) if c != j]
    res = {}
    for dt in (torch.float32, torch.float64):
        s = S[..., others].to(dt).requires_grad_(True)
        p = PR.sinkhorn_definition(s, 3)
        (p * W[..., others].to(dt)).sum().backward()
        res[dt] = (p.detach(), s.grad)
    _four_x_rule("module -inf column", "P without it", P[..., others], res[torch.float32][0], res[torch.float64][0], ((5, 12.0),))
    _four_x_rule("module -inf column", "dS without it", dS[..., others], res[torch.float32][1], res[torch.float64][1], ((5, 12.0),))


# ------------------------------------------------------------------ softmax controls: same builder, same per-row metric
def _softmax_control(dev, tag, fwd, bwd, B, N, H, dh, weak):
    scale = dh ** -0.5
    qkv = PR.peaked_qkv(B, N, H, dh, weak, seed=12).to(dev)
    dout = _dout(B, N, H, dh, dev)
    out, lse = fwd(qkv, B, N, H, dh, scale)
    dqkv = bwd(qkv, out, dout, lse, B, N, H, dh, scale)
    ref = PR.attention_reference(qkv, dout, B, N, H, dh, scale, iters=0)
    _check_forward(tag, ref, out, lse, B, N, H, dh, weak)
    _check_grads(tag, ref, dqkv, B, N, H, dh, weak, softmax_control=True)


def test_softmax_control_resident(dev):
    _softmax_control(dev, "softmax (2,197,2,64)", K.attn_fwd, K.attn_bwd, 2, 197, 2, 64, PR.std_weak(197))


def test_softmax_control_streaming(dev):
    _softmax_control(dev, "softmax streaming (1,577,2,80)", K.attn_fwd, K.attn_bwd, 1, 577, 2, 80, ((5, 12.0), (77, 20.0), (576, 16.0)))


def test_softmax_control_wide_heads(dev):
    assert K.attn_wide_shape(160)
    _softmax_control(dev, "softmax wide (2,197,1,160)", K.attn_wide_fwd, K.attn_wide_bwd, 2, 197, 1, 160, PR.std_weak(197))


def test_softmax_control_memory_keys(dev):
    """attn_mem_fwd / bwd with M = 70 memory keys behind the token keys (70 straddles a 64-key tile); the weak keys are token keys."""
    B, N, M, H, dh = 2, 197, 70, 2, 64
    weak = PR.std_weak(N)
    scale = dh ** -0.5
    qkv = PR.peaked_qkv(B, N, H, dh, weak, seed=13).to(dev)
    mkv = torch.randn(M, 2 * H * dh, generator=torch.Generator().manual_seed(14)).to(torch.bfloat16).to(dev)
    dout = _dout(B, N, H, dh, dev)
    out, lse = K.attn_mem_fwd(qkv, mkv, B, N, M, H, dh, scale)
    dqkv, dmem = K.attn_mem_bwd(qkv, out, dout, lse, mkv, B, N, M, H, dh, scale)
    x = qkv.cpu().double().requires_grad_(True)
    m = mkv.cpu().double().requires_grad_(True)
    q, k, v = PR.heads(x, B, N, H, dh)
    mk, mv = m.reshape(1, M, 2, H, dh).permute(2, 0, 3, 1, 4)
    s = q @ torch.cat([k, mk.expand(B, -1, -1, -1)], dim=2).transpose(-1, -2) * scale
    o = torch.softmax(s, dim=-1) @ torch.cat([v, mv.expand(B, -1, -1, -1)], dim=2)
    o.backward(PR.heads(dout.cpu().double(), B, N, H, dh)[0])
    ref = {"o": o.detach(), "lse": torch.logsumexp(s.detach(), dim=-1)}
    ref["dq"], ref["dk"], ref["dv"] = PR.heads(x.grad, B, N, H, dh)
    tag = "softmax + memory (2,197+70,2,64)"
    _check_forward(tag, ref, out, lse, B, N, H, dh, weak)
    _check_grads(tag, ref, dqkv, B, N, H, dh, weak, softmax_control=True)
    rm = m.grad.reshape(M, 2, H, dh)                       # shared memories: summed over the batch
    gm = dmem.cpu().double().reshape(M, 2, H, dh)
    for i, name in enumerate(("dmem_k", "dmem_v")):
        e = PR.per_row_abs_vs_largest(gm[:, i].transpose(0, 1), rm[:, i].transpose(0, 1))
        print(f"{tag} {name}: worst row {e.max().item():.3e}")
        assert e.max().item() <= PR.PER_ROW_BOUND, (name, e.max().item())
