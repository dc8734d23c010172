"""Host: what the bounds of test_biased_attn_edges_gpu.py rest on.

(1) the hand-written backward of biased_attn_ref.dense_core equals fp64 torch.autograd of its own forward, and the two wrappers
equal autograd of the definitions (swin_ref.window_core; softmax / Sinkhorn by repeated division for LeViT) on every case;
(2) the fp32 emulation of the kernels' arithmetic is inside every bound on every case, and its worst Sinkhorn-path gradient error
is the SINK_MEASURED that C_SINK is derived from; (3) the emulation with one deliberate mistake at a time -- the mistakes an
index-heavy kernel can make -- falls outside the bounds, at a named output of a named case."""
import functools

import pytest
import torch

import biased_attn_ref as R
import swin_ref

D = torch.float64
WIN = [(ci, rb) for ci in range(len(R.WINDOW_CASES)) for rb in (False, True)]
BIAS = [(ci, rb) for ci in range(len(R.BIAS_CASES)) for rb in (False, True)]


def _close(a, b, tol=1e-10):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@functools.lru_cache(maxsize=None)
def _win(ci, robust):
    case = R.WINDOW_CASES[ci]
    i = R.window_inputs(case)
    return i, R.window_ref(i["qkv"], i["table"], i["dout"], *case, robust)


def _win_emu(ci, robust, bug=None):
    i, ref = _win(ci, robust)
    e = R.emu_window(i["qkv"], i["table"], i["dout"], *R.WINDOW_CASES[ci], robust, bug)
    return ref, e, R.check_window(ref, e["o"], e["stats"], e["dqkv"], e["dtable"])


@functools.lru_cache(maxsize=None)
def _bias_in(ci):
    case = R.BIAS_CASES[ci]
    i = R.bias_inputs(case)
    return i, R.bias_views(case, i["qbuf"], i["kvbuf"])


def _bias_emu(ci, robust, bug=None):
    """The emulation's forward first: the restatement takes Hardswish' on ITS bf16 o, as it takes the kernel's on the GPU."""
    case = R.BIAS_CASES[ci]
    B, H, Nq, Nk, kd, d = case[:6]
    i, (q, k, v) = _bias_in(ci)
    e = R.emu_bias(q, k, v, i["hs"], i["table"], i["idx"], i["dact"], B, H, Nq, Nk, kd, d, robust, bug)
    ref = R.bias_ref(q, k, v, i["hs"], i["table"], i["idx"], i["dact"], e["o"], B, H, Nq, Nk, kd, d, robust)
    return ref, e, R.check_bias(ref, Nq, Nk, e["o"], e["ao"], e["stats"], e["dq"], e["dk"], e["dv"], e["dtable"])


# ---- (1) the restatement against autograd ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("Nq,Nk", [(1, 1), (1, 9), (5, 7), (6, 6)])
def test_core_backward_is_autograd_of_its_forward(Nq, Nk, robust):
    g = torch.Generator().manual_seed(Nq * 16 + Nk)
    T = [torch.randn(2, 3, n, w, generator=g, dtype=D).requires_grad_(True) for n, w in ((Nq, 4), (Nk, 4), (Nk, 5), (Nq, Nk))]
    do = torch.randn(2, 3, Nq, 5, generator=g, dtype=D)
    r = R.dense_core(*T, robust, do)
    grads = torch.autograd.grad((r["o"] * do).sum(), T)
    for n, want in zip(("dq", "dk", "dv", "dS"), grads):
        assert _close(r[n].detach(), want), n
    assert _close(r["lse"].detach(), torch.logsumexp(r["S"].detach(), -1))
    if robust:
        P = r["P"].detach()
        assert _close(P.sum(-1), torch.ones_like(P[..., 0]))                       # the last step normalises the rows


@pytest.mark.parametrize("ci,robust", WIN)
def test_window_wrapper_is_autograd_of_window_core(ci, robust):
    B, pH, pW, C, heads, window, shift = R.WINDOW_CASES[ci]
    i, ref = _win(ci, robust)
    x = i["qkv"].double().reshape(B, pH, pW, 3 * C).requires_grad_(True)
    t = i["table"].double().requires_grad_(True)
    o = swin_ref.window_core(x, t, heads, window, shift, robust)
    gx, gt = torch.autograd.grad((o * i["dout"].double().reshape(B, pH, pW, C)).sum(), (x, t))
    # the restatement scales q by the kernels' fp32 1 / sqrt(dh), window_core by the exact one: they differ by 3e-8 at dh 32
    tol = 1e-10 if R.f32_scale(C // heads) == (C // heads) ** -0.5 else 3e-7
    assert _close(ref["o"], o.detach().reshape(-1, C), tol)
    gx = gx.reshape(-1, 3 * C)
    for n, want in zip(("dq", "dk", "dv"), gx.split(C, 1)):
        assert _close(ref[n], want, tol), n
    assert _close(ref["dtable"], gt, tol)
    assert all(bool(torch.isfinite(v).all()) for k, v in ref.items() if k != "blocks")


@pytest.mark.parametrize("ci,robust", BIAS)
def test_bias_wrapper_is_autograd_of_the_definition(ci, robust):
    case = R.BIAS_CASES[ci]
    B, H, Nq, Nk, kd, d, T = case[:7]
    i, (q, k, v) = _bias_in(ci)
    o_saved = R.emu_bias(q, k, v, i["hs"], i["table"], i["idx"], None, B, H, Nq, Nk, kd, d, robust)["o"]
    ref = R.bias_ref(q, k, v, i["hs"], i["table"], i["idx"], i["dact"], o_saved, B, H, Nq, Nk, kd, d, robust)
    qf, kf, vf = (R.bias_heads(t, B, n, H, s, w).double().requires_grad_(True)
                  for t, n, s, w in ((q, Nq, i["hs"][0], kd), (k, Nk, i["hs"][1], kd), (v, Nk, i["hs"][2], d)))
    tf = i["table"].double().requires_grad_(True)
    p = torch.softmax(qf @ kf.mT * R.f32_scale(kd) + tf[:, i["idx"]], -1)
    if robust:
        for _ in range(3):
            p = p / p.sum(-1, keepdim=True)
            p = p / p.sum(-2, keepdim=True)
        p = p / p.sum(-1, keepdim=True)
    o = p @ vf
    do = R.bias_heads(i["dact"].double() * R.hardswish_grad(o_saved.double()), B, Nq, H, d, d)
    g = torch.autograd.grad((o * do).sum(), (qf, kf, vf, tf))
    flat = o.detach().permute(0, 2, 1, 3).reshape(B * Nq, H * d)
    assert _close(ref["o"], flat) and _close(ref["ao"], torch.nn.functional.hardswish(flat))
    for n, want in zip(("dq", "dk", "dv", "dtable"), g):
        assert _close(ref[n], want), n
    assert all(bool(torch.isfinite(v).all()) for k, v in ref.items() if k != "blocks")
    if case[9] == "holes":
        cnt = torch.bincount(i["idx"].reshape(-1), minlength=T)
        assert int(cnt[R.HOLE_UNUSED]) == 0 and int(cnt[R.HOLE_ONCE]) == 1
        assert float(ref["dtable"][:, R.HOLE_UNUSED].abs().max()) == 0.0 and float(ref["dtable_tol"][:, R.HOLE_UNUSED].max()) == 0.0
    if case[9] == "perm":
        assert bool((torch.bincount(i["idx"].reshape(-1), minlength=T) == 1).all())


def test_case_lists_reach_what_they_claim():
    """The geometry facts the case comments state."""
    N = [c[5][0] * c[5][1] for c in R.WINDOW_CASES]
    T = [(2 * c[5][0] - 1) * (2 * c[5][1] - 1) for c in R.WINDOW_CASES]
    nwin = [c[0] * (c[1] // c[5][0]) * (c[2] // c[5][1]) for c in R.WINDOW_CASES]
    assert N == [4, 6, 56, 56, 64, 64, 49] and T == [9, 15, 195, 195, 127, 225, 169] and nwin == [1, 9, 4, 4, 4, 12, 30]
    lds = lambda Nq, Nk: (Nq * (Nk + 1) + 6 * 256) * 4
    assert lds(153, 256) <= 160 * 1024 < lds(154, 256) and lds(198, 198) <= 160 * 1024 < lds(199, 199)
    # window (7, 8), shift (3, 4) on a 7-row map: some table entries collect only masked pairs -- the underflow floor's reason
    _, ref = _win(2, False)
    small = ref["dtable"].abs() < R.TINY
    assert bool(small.any()) and bool((ref["dtable_tol"][small] >= R.TINY).all())


# ---- (2) the fp32 emulation is inside every bound; the constant of the Sinkhorn-path gradients ----------------------------------
@pytest.mark.parametrize("ci,robust", WIN)
def test_window_emulation_is_inside_the_bounds(ci, robust):
    ref, e, r = _win_emu(ci, robust)
    print(R.WINDOW_CASES[ci], robust, {k: f"{v:.3f}" for k, v in r.items()}, "block error", R.block_error(ref["blocks"], e["blocks"]))
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("ci,robust", BIAS)
def test_bias_emulation_is_inside_the_bounds(ci, robust):
    ref, e, r = _bias_emu(ci, robust)
    print(R.BIAS_CASES[ci], robust, {k: f"{v:.3f}" for k, v in r.items()}, "block error", R.block_error(ref["blocks"], e["blocks"]))
    assert max(r.values()) <= 1.0, r


def test_sinkhorn_constant_is_four_times_the_measured_error():
    worst = 0.0
    for ci in range(len(R.WINDOW_CASES)):
        ref, e, _ = _win_emu(ci, True)
        worst = max(worst, R.block_error(ref["blocks"], e["blocks"]))
    for ci in range(len(R.BIAS_CASES)):
        ref, e, _ = _bias_emu(ci, True)
        worst = max(worst, R.block_error(ref["blocks"], e["blocks"]))
    print("worst Sinkhorn-path block error of the fp32 emulation", worst, "C_SINK", R.C_SINK)
    assert worst <= R.SINK_MEASURED and 4 * worst <= R.C_SINK <= R.ROW_REL
    assert worst >= R.SINK_MEASURED / 2                                            # the recorded figure is the measured one, not a ceiling


# ---- (3) one deliberate mistake at a time: the bounds catch it ------------------------------------------------------------------
# (mistake, family, case index, robust, the output that must leave its bound)
BROKEN = [
    ("region_off_by_one", "window", 5, False, "o"),           # one row / column of slots changes region: -100 on the wrong pairs
    ("region_off_by_one", "window", 2, True, "b1"),
    ("tw_from_wh", "window", 1, False, "o"),                  # (2, 3): tw = 3 instead of 5 reads other table rows
    ("tw_from_wh", "window", 3, True, "dtable"),
    ("decode_swapped", "window", 1, False, "dtable"),
    ("decode_swapped", "window", 4, True, "dtable"),
    ("skip_tail_window", "window", 0, False, "dtable"),       # the single window IS the tail: dtable stays 0
    ("skip_tail_window", "window", 6, True, "dtable"),        # 1 of 30 windows missing
    ("b2_for_b3", "bias", 4, True, "dv"),                     # 63 x 65: successive column scalings differ by ~65 / 63
    ("b2_for_b3", "bias", 5, True, "dv"),
    ("drop_last_key", "window", 0, False, "dq"),
    ("drop_last_key", "bias", 2, True, "dk"),                 # 1 key of 256
    ("roll_neg", "window", 6, False, "o"),
    ("roll_neg", "window", 5, True, "dv"),
    ("table_stride_1", "window", 1, False, "o"),              # heads 3
    ("table_stride_1", "window", 3, True, "lse"),             # heads 2
    ("unused_entry_kept", "bias", 4, False, "dtable"),
    ("unused_entry_kept", "bias", 4, True, "dtable"),
]


@pytest.mark.parametrize("bug,family,ci,robust,output", BROKEN)
def test_a_broken_emulation_leaves_the_bounds(bug, family, ci, robust, output):
    _, _, good = (_win_emu if family == "window" else _bias_emu)(ci, robust)
    _, _, bad = (_win_emu if family == "window" else _bias_emu)(ci, robust, bug)
    print(bug, family, ci, robust, {k: f"{v:.3g}" for k, v in bad.items() if v > 1.0})
    assert good[output] <= 1.0 < bad[output], (bug, output, good[output], bad[output])


def test_every_mistake_of_the_list_is_tried():
    assert {b[0] for b in BROKEN} == {"region_off_by_one", "tw_from_wh", "decode_swapped", "skip_tail_window", "b2_for_b3", "drop_last_key",
                                      "roll_neg", "table_stride_1", "unused_entry_kept"}
