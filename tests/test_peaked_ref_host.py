"""Host: the peaked-input builder and the references the GPU bounds of test_peaked_attn_gpu.py rest on.

Two facts per shape: (1) the problem is well conditioned -- torch fp32 evaluates the definition within 1e-5 per row of fp64;
(2) rounding P, dS and the outputs to bf16 (the kernels' documented rounding points, nothing else) stays within 1e-2 per row,
a 3 x margin under the 3e-2 per-row bound the kernels are held to.  If a shape added later breaks (2), change the shape."""
import pytest
import torch

import peaked_ref as PR

CASES = PR.FUSED_CASES + PR.COMPOSED_CASES + (PR.MANY_HEADS_CASE,)


def _dout(B, N, H, dh, seed):
    return torch.randn(B * N, H * dh, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16)


@pytest.mark.parametrize("B,N,H,dh,weak", CASES)
def test_builder_puts_the_weak_keys_where_it_says(B, N, H, dh, weak):
    B = min(B, 2)
    scale = dh ** -0.5
    q, k, _ = PR.heads(PR.peaked_qkv(B, N, H, dh, weak, seed=1).double(), B, N, H, dh)
    q0, k0, _ = PR.heads(PR.peaked_qkv(B, N, H, dh, (), seed=1).double(), B, N, H, dh)
    drop = (q0 @ k0.transpose(-1, -2) - q @ k.transpose(-1, -2)) * scale          # same draw without the weak keys
    wk = dict(weak)
    for j in range(N):
        want = wk.get(j, 0.0)
        # bf16 operands: the u component of q (4) and of the key (up to 40) carry 2^-9 relative rounding each
        assert (drop[..., j] - want).abs().max().item() <= 2 ** -6 * max(want, 1.0), (j, want)
    P0 = PR.sinkhorn_definition(q @ k.transpose(-1, -2) * scale, iters=0)
    P7 = PR.sinkhorn_definition(q @ k.transpose(-1, -2) * scale, iters=3)
    for j, nats in weak:
        assert P0[..., j].log().max().item() < -nats + 6.0            # below the rest for EVERY query
        assert abs(P7[..., j].sum(dim=-1).mean().item() - 1.0) < 0.2   # and rescaled to an ordinary key by the column steps


@pytest.mark.parametrize("B,N,H,dh,weak", CASES)
def test_references_fp32_and_bf16_emulation_against_fp64(B, N, H, dh, weak):
    B = min(B, 4)                                        # the many-heads case: 24 heads are enough on the host
    scale = dh ** -0.5
    qkv = PR.peaked_qkv(B, N, H, dh, weak, seed=2)
    dout = _dout(B, N, H, dh, 3)
    r64 = PR.attention_reference(qkv, dout, B, N, H, dh, scale)
    r32 = PR.attention_reference(qkv, dout, B, N, H, dh, scale, dtype=torch.float32)
    emu = PR.attention_reference(qkv, dout, B, N, H, dh, scale, emulate_bf16=True)
    for name in ("dq", "dk", "dv"):
        assert bool((r64[name].norm(dim=-1) > 0).all()), name
        e32 = PR.per_row_rel(r32[name], r64[name]).max().item()
        eem = PR.per_row_rel(emu[name], r64[name])
        weak_rows = {j: eem[..., j].max().item() for j, _ in weak}
        print(f"{(B, N, H, dh)} {name}: fp32 worst row {e32:.2e}  bf16 emulation worst row {eem.max().item():.2e}  weak keys {weak_rows}")
        assert e32 < 1e-5, (name, e32)
        assert eem.max().item() <= PR.EMULATION_BOUND, (name, eem.max().item())
    # the weak keys' gradient rows are as large as an ordinary key's: that is what makes them worth a per-key check
    for name in ("dk", "dv"):
        norms = r64[name].norm(dim=-1)
        for j, _ in weak:
            assert (norms[..., j] / norms.median(dim=-1).values).min().item() > 0.2, (name, j)


@pytest.mark.parametrize("shape", [(4, 197, 197), (2, 577, 577), (3, 50, 81)])
def test_peaked_scores_and_scalings(shape):
    weak = ((5, 12.0), (33, 20.0), (47, 60.0))
    S = PR.peaked_scores(shape, weak, seed=4)
    S0 = PR.peaked_scores(shape, (), seed=4)
    for j, nats in weak:
        assert torch.allclose(S0[..., j] - S[..., j], torch.full_like(S[..., j], nats), atol=1e-4)
    P = PR.sinkhorn_definition(S.double())
    av, bv = PR.sinkhorn_scalings(S.double())
    P7 = av[..., -1, :, None] * torch.softmax(S.double(), dim=-1) * bv[..., -1, None, :]
    assert (P7 - P).abs().max().item() < 1e-12
    assert bool(torch.isfinite(P).all()) and bv[..., -1, 47].min().item() > 1e20      # e^-60 columns: b3 is huge, P is ordinary


def test_per_row_metrics():
    ref = torch.tensor([[3.0, 4.0], [0.0, 0.0], [0.0, 1.0]])
    got = torch.tensor([[3.0, 4.5], [0.0, 0.0], [0.0, 1.0]])
    assert torch.allclose(PR.per_row_rel(got, ref), torch.tensor([0.1, 0.0, 0.0], dtype=torch.float64))
    assert PR.per_row_rel(torch.ones(1, 2), torch.zeros(1, 2)).item() == float("inf")
    assert torch.allclose(PR.per_row_abs_vs_largest(got, ref), torch.tensor([0.1, 0.0, 0.0], dtype=torch.float64))


def test_weak_key_vit_case_makes_two_tokens_weak_in_every_head():
    """The model-level case of tests/test_model_gpu.py at a small geometry: both tokens are below -12 for every query of every head
    before the normalisation, and the Sinkhorn steps give them ordinary weight (column sums of the normalised matrix near 1)."""
    from oracle import vit_oracle as V
    cfg = dict(image_size=64, patch_size=8, num_layers=1, num_heads=3, hidden_dim=192, mlp_dim=384, num_classes=5)
    sd = V.vit_init_state_dict(seed=1, **cfg)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    sd, x, logw = PR.weak_key_vit_case(sd, x, patch_size=8, num_heads=3, tokens=(5, 40))
    assert logw.shape == (2, 3, 65, 2) and logw.max().item() < -12.0
    assert bool(torch.isfinite(V.vit_forward(sd, x, patch_size=8, num_heads=3, robust=True)).all())
