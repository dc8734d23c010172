"""GPU: a 2-layer encoder stack (D = 128) whose backward hands the weight gradients' reductions to the dX launches.

Planned for 8 CUs, 54 x 65 = 3510 token rows make the [3510 x 128] dX launches of fc1 (K = 512) and of the qkv projection (K = 384)
ten 384 x 128 tiles on 8 workgroups: 6 late workgroups, and the library admits both jobs (asserted with the plan queries); the dU
and dO launches have K = 128 < 192 (plain kernel: the job runs as a launch of its own in front of them).  Gradients with
`encoder.WGRAD_DEFER` on and off must be bit-equal, without and with a gradient sink; a backward that raises while a token is
pending must leave nothing behind that the next step could pick up."""
import pytest
import torch

from noise_robust_vit_amd import encoder as E
from noise_robust_vit_amd import kernels as K

pytestmark = pytest.mark.gpu

D, H, F, DEPTH, B, N = 128, 2, 512, 2, 54, 65
PLANNED = 8


@pytest.fixture()
def planned8(dev):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    prev = K.set_reserved_cus(cus - PLANNED)
    try:
        assert prev == 0, f"reservation was {prev}, not 0"
        yield
    finally:
        K.set_reserved_cus(0)


def make_params(dev):
    g = torch.Generator(device="cpu").manual_seed(11)
    r = lambda *s, scale=0.05: (torch.randn(*s, generator=g) * scale).to(dev).requires_grad_(True)
    out = []
    for _ in range(DEPTH):
        out += [(1.0 + r(D)).detach().requires_grad_(True), r(D), r(3 * D, D), r(3 * D), r(D, D), r(D),
                (1.0 + r(D)).detach().requires_grad_(True), r(D), r(F, D), r(F), r(D, F), r(D)]
    return out


def make_input(dev):
    g = torch.Generator(device="cpu").manual_seed(12)
    return torch.randn(B, N, D, generator=g).to(dev), torch.randn(B, N, D, generator=g).to(dev)


class Sink:
    """A gradient sink as the data-parallel runtime attaches it: one persistent fp32 buffer per parameter, accumulated into."""

    def __init__(self, params):
        self.buf = {id(p): torch.full_like(p, 0.25) for p in params}
        self.done = []

    def target(self, p):
        return self.buf[id(p)], 1.0

    def layer_done(self, i, params):
        self.done.append(i)


def step(params, x, dy, sink=None):
    meta = E.BlockMeta(heads=H, dim_head=D // H, eps=1e-5, sink=sink)
    xin = x.clone().requires_grad_(True)
    y = E.EncoderStackFn.apply(xin, meta, *params)
    grads = torch.autograd.grad(y, [xin] + params, dy, allow_unused=True)
    torch.cuda.synchronize()
    if sink is not None:
        return [grads[0]] + [sink.buf[id(p)].clone() for p in params]
    return list(grads)


def spy_fused(monkeypatch):
    """Record what every `gemm_nt(..., side=token)` of the backward did with its token."""
    seen = []
    real = K.gemm_nt

    def spy(*a, side=None, **kw):
        pending = side is not None and side.pending
        out = real(*a, side=side, **kw)
        if pending:
            seen.append(side.fused)
        return out

    monkeypatch.setattr(K, "gemm_nt", spy)
    return seen


def test_plans_of_the_stack(dev, planned8):
    T = B * N
    for (Mw, Kk) in ((F, F), (3 * D, 3 * D)):                   # dW1 in front of dXn2 (K = 512), dWqkv in front of dXn (K = 384)
        tn = K.gemm_tn_plan(Mw, D, T, dbias=True)
        sp = K.gemm_nt_side_plan(T, D, Kk, 0, False, tn["splits"] * Mw * D * 4)
        assert K.gemm_nt_plan(T, D, Kk, 0) == {"tile_m": 384, "tile_n": 128, "phased": True, "tiles": 10, "grid": 8}
        assert tn["splits"] == 4 and sp["late"] == 6 and sp["admitted"]
    assert not K.gemm_nt_plan(T, F, D, 6)["phased"] and not K.gemm_nt_plan(T, D, D, 0)["phased"]


@pytest.mark.parametrize("with_sink", [False, True], ids=["autograd", "sink"])
def test_gradients_bit_equal_with_and_without_deferral(dev, planned8, monkeypatch, with_sink):
    monkeypatch.setattr(E, "WGRAD_STREAM", False)               # weight gradients on the main stream: the deferring schedule
    params, (x, dy) = make_params(dev), make_input(dev)
    monkeypatch.setattr(E, "WGRAD_DEFER", False)
    ref = step(params, x, dy, Sink(params) if with_sink else None)
    monkeypatch.setattr(E, "WGRAD_DEFER", True)
    seen = spy_fused(monkeypatch)
    sink = Sink(params) if with_sink else None
    got = step(params, x, dy, sink)
    # per layer: dU and dO take their job as a launch of its own, dXn2 and dXn inside the GEMM launch
    assert seen == [False, True, False, True] * DEPTH
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)
    if with_sink:
        assert sink.done == [1, 0]


def test_token_of_a_backward_that_raised_is_not_applied(dev, planned8, monkeypatch):
    monkeypatch.setattr(E, "WGRAD_STREAM", False)
    params, (x, dy) = make_params(dev), make_input(dev)
    sink_ref = Sink(params)
    ref = step(params, x, dy, sink_ref)
    real = K.gemm_nt
    calls = {"n": 0}

    def raising(*a, side=None, **kw):
        if side is not None and side.pending:
            calls["n"] += 1
            if calls["n"] == 2:                                 # the second weight gradient of the last layer: its token is pending
                raise RuntimeError("injected")
        return real(*a, side=side, **kw)

    sink = Sink(params)
    monkeypatch.setattr(K, "gemm_nt", raising)
    with pytest.raises(RuntimeError, match="injected"):
        step(params, x, dy, sink)
    monkeypatch.setattr(K, "gemm_nt", real)
    torch.cuda.synchronize()
    # what the failed backward completed (dW2, db2 of the last layer) is in the sink; its pending dW1 is not, and stays out
    untouched = torch.full_like(params[-4], 0.25)
    assert torch.equal(sink.buf[id(params[-4])], untouched)
    fresh = Sink(params)
    got = step(params, x, dy, fresh)
    torch.cuda.synchronize()
    assert torch.equal(sink.buf[id(params[-4])], untouched)     # the next step ran no left-over job
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
