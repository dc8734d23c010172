"""nrv_attn_mem_* (memory keys + bit-packed score mask, learnable_memory_vit.py:64-86) against fp32 torch on the same bf16
operands: output, LSE, token dq / dk / dv and memory dk / dv, over token counts, memory counts (70 straddles a 64-key tile),
head dims, mask kinds and shared / per-sample memories."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

NEG = -torch.finfo(torch.float32).max


def _k():
    from noise_robust_vit_amd import kernels
    return kernels


def rnd(shape, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).to(dev)


def make_mask(kind, B, H, Nq, Nk, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if kind == "none":
        return None
    if kind == "adapter":                        # Adapter pattern: row 0 sees all, rows 1.. see keys 1 .. Nq-1
        m = torch.zeros(Nq, Nk, dtype=torch.bool)
        m[0] = True
        m[1:, 1:Nq] = True
    elif kind == "random":                       # per (batch, head), broadcast-free
        m = torch.rand(B, H, Nq, Nk, generator=g) > 0.4
    elif kind == "fullrow":                      # one fully masked query row: uniform weights
        m = torch.rand(Nq, Nk, generator=g) > 0.3
        m[Nq // 2] = False
    elif kind == "ones":
        m = torch.ones(Nq, Nk, dtype=torch.bool)
    else:
        raise ValueError(kind)
    return m.to(dev)


def reference(qkv, mkv, B, Nq, M, H, dh, scale, shared, mask):
    """fp32 attention with autograd leaves q, k, v (token) and km, vm (memory)."""
    t = qkv.float().reshape(B, Nq, 3, H, dh).permute(2, 0, 3, 1, 4)
    q, k, v = [x.clone().requires_grad_(True) for x in t]
    mk = mv = None
    ks, vs = k, v
    if M > 0:
        m = mkv.float().reshape(-1, M, 2, H, dh).permute(2, 0, 3, 1, 4)
        mk, mv = [x.clone().requires_grad_(True) for x in m]
        ks = torch.cat([k, mk.expand(B, -1, -1, -1)], dim=2)
        vs = torch.cat([v, mv.expand(B, -1, -1, -1)], dim=2)
    s = q @ ks.transpose(-1, -2) * scale
    if mask is not None:
        s = s.masked_fill(~mask, NEG)
    lse = torch.logsumexp(s, dim=-1)
    o = torch.softmax(s, dim=-1) @ vs
    return o, lse, (q, k, v, mk, mv)


def run(dev, B, Nq, M, H, dh, shared, kind, seed=0):
    K = _k()
    scale = dh ** -0.5
    Nk = Nq + M
    qkv = rnd((B * Nq, 3 * H * dh), dev, seed + 1)
    mkv = rnd(((1 if shared else B) * M, 2 * H * dh), dev, seed + 2) if M > 0 else None
    maskb = make_mask(kind, B, H, Nq, Nk, dev, seed + 3)
    bits = K.mask_pack(maskb, B, H, Nq, Nk) if maskb is not None else None
    out, lse = K.attn_mem_fwd(qkv, mkv, B, Nq, M, H, dh, scale, shared, bits)
    dout = rnd((B * Nq, H * dh), dev, seed + 4)
    dqkv, dmem = K.attn_mem_bwd(qkv, out, dout, lse, mkv, B, Nq, M, H, dh, scale, shared, bits)
    ro, rlse, leaves = reference(qkv, mkv, B, Nq, M, H, dh, scale, shared, maskb)
    ro.backward(dout.float().reshape(B, Nq, H, dh).transpose(1, 2))
    return dict(out=out, lse=lse, dqkv=dqkv, dmem=dmem, ro=ro, rlse=rlse, leaves=leaves, mask=maskb, qkv=qkv, mkv=mkv, dout=dout,
                bits=bits)


def check(r, B, Nq, M, H, dh, shared):
    o = r["out"].float().reshape(B, Nq, H, dh).transpose(1, 2)
    ro = r["ro"].detach()
    # P enters P.V in bf16 and the output is stored in bf16
    assert (o - ro).abs().max().item() < 2 ** -7 * ro.abs().max().item() + 1e-3, (o - ro).abs().max().item()
    rl, kl = r["rlse"].detach(), r["lse"]
    full = rl <= NEG / 2
    assert torch.equal(kl[full], torch.full_like(kl[full], NEG))            # fully masked rows: lse = -FLT_MAX
    assert (kl[~full] - rl[~full]).abs().max().item() < 1e-4 if (~full).any() else True
    q, k, v, mk, mv = r["leaves"]
    dq = r["dqkv"].float().reshape(B, Nq, 3, H, dh).permute(2, 0, 3, 1, 4)
    got = [dq[0], dq[1], dq[2]]
    want = [q.grad, k.grad, v.grad]
    if M > 0:
        dm = r["dmem"].reshape(-1, M, 2, H, dh).permute(2, 0, 3, 1, 4)
        assert dm.shape[1] == (1 if shared else B)
        got += [dm[0], dm[1]]
        want += [mk.grad, mv.grad]
    for name, a, b in zip(("dq", "dk", "dv", "dk_mem", "dv_mem"), got, want):
        den = b.abs().max().item()
        if den == 0.0:
            assert a.abs().max().item() == 0.0, name
            continue
        err = (a - b).abs().max().item() / den
        assert err < 2e-2, (name, err)


KINDS = ["none", "adapter", "random", "fullrow"]
GRID = list(itertools.product([17, 198, 257, 577], [0, 1, 10, 70], [32, 64, 80, 128]))


@pytest.mark.parametrize("Nq,M,dh", GRID)
def test_attn_mem_grid(dev, Nq, M, dh):
    i = GRID.index((Nq, M, dh))
    kind, shared = KINDS[i % 4], (i // 4) % 2 == 0
    B, H = 2, 2
    r = run(dev, B, Nq, M, H, dh, shared, kind, seed=i)
    check(r, B, Nq, M, H, dh, shared)


@pytest.mark.parametrize("kind,shared", list(itertools.product(KINDS, [True, False])))
def test_attn_mem_masks_and_sharing(dev, kind, shared):
    B, Nq, M, H, dh = 3, 70, 10, 3, 64
    r = run(dev, B, Nq, M, H, dh, shared, kind, seed=100)
    check(r, B, Nq, M, H, dh, shared)


def test_fully_masked_row_is_uniform(dev):
    B, Nq, M, H, dh = 2, 40, 5, 2, 64
    r = run(dev, B, Nq, M, H, dh, False, "fullrow", seed=7)
    o = r["out"].float().reshape(B, Nq, H, dh)[:, Nq // 2]                  # [B, H, dh]
    v = r["qkv"].float().reshape(B, Nq, 3, H, dh)[:, :, 2]                  # [B, Nq, H, dh]
    vm = r["mkv"].float().reshape(B, M, 2, H, dh)[:, :, 1]
    mean = torch.cat([v, vm], dim=1).mean(dim=1)
    assert (o - mean).abs().max().item() < 2 ** -7 * mean.abs().max().item() + 1e-3


@pytest.mark.parametrize("Nq,M,dh", [(17, 0, 64), (198, 10, 64), (257, 70, 80), (65, 3, 128)])
def test_all_true_mask_is_bit_identical_to_no_mask(dev, Nq, M, dh):
    K = _k()
    B, H = 2, 3
    scale = dh ** -0.5
    qkv = rnd((B * Nq, 3 * H * dh), dev, 31)
    mkv = rnd((M, 2 * H * dh), dev, 32) if M > 0 else None
    dout = rnd((B * Nq, H * dh), dev, 33)
    bits = K.mask_pack(torch.ones(Nq, Nq + M, dtype=torch.bool, device=dev), B, H, Nq, Nq + M)
    o0, l0 = K.attn_mem_fwd(qkv, mkv, B, Nq, M, H, dh, scale, True, None)
    o1, l1 = K.attn_mem_fwd(qkv, mkv, B, Nq, M, H, dh, scale, True, bits)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    d0 = K.attn_mem_bwd(qkv, o0, dout, l0, mkv, B, Nq, M, H, dh, scale, True, None)
    d1 = K.attn_mem_bwd(qkv, o1, dout, l1, mkv, B, Nq, M, H, dh, scale, True, bits)
    assert torch.equal(d0[0], d1[0])
    if M > 0:
        assert torch.equal(d0[1], d1[1])


@pytest.mark.parametrize("shared", [True, False])
def test_backward_is_deterministic(dev, shared):
    K = _k()
    B, Nq, M, H, dh = 4, 198, 10, 2, 64
    scale = dh ** -0.5
    qkv = rnd((B * Nq, 3 * H * dh), dev, 41)
    mkv = rnd(((1 if shared else B) * M, 2 * H * dh), dev, 42)
    dout = rnd((B * Nq, H * dh), dev, 43)
    bits = K.mask_pack(make_mask("random", B, H, Nq, Nq + M, dev, 44), B, H, Nq, Nq + M)
    o, l = K.attn_mem_fwd(qkv, mkv, B, Nq, M, H, dh, scale, shared, bits)
    a = K.attn_mem_bwd(qkv, o, dout, l, mkv, B, Nq, M, H, dh, scale, shared, bits)
    b = K.attn_mem_bwd(qkv, o, dout, l, mkv, B, Nq, M, H, dh, scale, shared, bits)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_mask_pack_bits(dev):
    K = _k()
    g = torch.Generator().manual_seed(5)
    m = torch.rand(2, 3, 7, 70, generator=g) > 0.5
    mb = K.mask_pack(m.to(dev), 2, 3, 7, 70)
    assert mb.bstride == 3 * 7 * 3 and mb.hstride == 7 * 3
    words = mb.bits.cpu().view(torch.int32).numpy().astype("uint32").reshape(2 * 3 * 7, 3)
    flat = m.reshape(-1, 70)
    for r in range(flat.shape[0]):
        for c in range(70):
            assert bool((int(words[r, c // 32]) >> (c % 32)) & 1) == bool(flat[r, c])
    shared = K.mask_pack(m[0, 0].to(dev), 2, 3, 7, 70)
    assert shared.bstride == 0 and shared.hstride == 0
