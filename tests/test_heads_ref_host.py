"""CPU: the bounds of tests/heads_ref.py hold for the emulation of every talking-heads and re-attention kernel on the very cases and
input kinds tests/test_heads_edges_gpu.py uses (ratio error / bound <= 1, the worst ratio per output printed), and wrong kernels
exceed them: the last key dropped from the softmax sum, an untransposed gradient mix, non-zero pad positions in front of th_pairs,
an idle th_pairs split counted twice, the one-pass variance, dgamma without the last wave, and the smallest entry of an H x H
gradient zeroed (what a max-norm comparison cannot see).  The case lists are checked against the edges they are named after."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_ref as R  # noqa: E402

ROW_CASES = R.FUSED_CASES + R.ROW_WALK_CASES
TILE_CASES = R.FLAT_CASES + R.TILE_WALK_CASES
WORST = {}                        # entry point -> output -> worst ratio over the cases run so far


def _note(entry, rs):
    w = WORST.setdefault(entry, {})
    for n, r in rs.items():
        w[n] = max(w.get(n, 0.0), r)
    assert all(r <= 1.0 for r in rs.values()), (entry, rs)


def _ratios(ref, got):
    return {n: R.ratio(t, ref[n], ref[n + "_bound"]) for n, t in got.items()}


def th_ratios(case, kind):
    i = R.inputs(*case, kind)
    P, A = R.th_fwd_emul(i["S"], i["W1"], i["W2"])
    f = R.th_fwd_ref(i["S"], i["W1"], i["W2"], P)
    fb = R.th_fwd_ref(i["S"], i["W1"], i["W2"], P, bf=True)
    fwd = dict(_ratios(f, {"P": P, "A": A}), A_bf16=R.ratio(R.bf16(A), fb["A"], fb["A_bound"]))
    dS, dW1, dW2 = R.th_bwd_emul(i["dA"], P, i["S"], i["W1"], i["W2"])
    return fwd, _ratios(R.th_bwd_ref(i["dA"], P, i["S"], i["W1"], i["W2"]), {"dS": dS, "dW1": dW1, "dW2": dW2}), (P, dS)


def ra_ratios(case, kind):
    i = R.inputs(*case, kind)
    P, A = R.ra_fwd_emul(i["S"], i["W"], i["gamma"], i["beta"])
    f = R.ra_norm_fwd_ref(P, i["W"], i["gamma"], i["beta"])
    fb = R.ra_norm_fwd_ref(P, i["W"], i["gamma"], i["beta"], bf=True)
    s = R.ra_softmax_ref(i["S"])
    fwd = {"P": R.ratio(P, s["P"], s["P_bound"]), "A": R.ratio(A, f["A"], f["A_bound"]), "A_bf16": R.ratio(R.bf16(A), fb["A"], fb["A_bound"])}
    dS, dW, dg, db = R.ra_bwd_emul(i["dA"], P, i["W"], i["gamma"])
    bwd = _ratios(R.ra_bwd_ref(i["dA"], P, i["W"], i["gamma"]), {"dS": dS, "dW": dW, "dgamma": dg, "dbeta": db})
    return fwd, bwd, (i, P, A, dS, dW, dg)


@pytest.mark.parametrize("case", ROW_CASES, ids=str)
@pytest.mark.parametrize("kind", R.KINDS)
def test_th_softmax_bounds_hold_for_the_emulation(case, kind):
    fwd, bwd, (P, dS) = th_ratios(case, kind)
    print("th_softmax", case, kind, "error / bound:", fwd, bwd)
    _note("nrv_th_softmax_fwd", fwd)
    _note("nrv_th_softmax_bwd", bwd)
    if case[3] == 1:                                                      # softmax over one key is the constant 1
        assert bool((P == 1).all()) and not dS.any()


@pytest.mark.parametrize("case", ROW_CASES, ids=str)
@pytest.mark.parametrize("kind", R.KINDS)
def test_reattn_softmax_bounds_hold_for_the_emulation(case, kind):
    fwd, bwd, (i, P, A, dS, dW, dg) = ra_ratios(case, kind)
    print("reattn_softmax", case, kind, "error / bound:", fwd, bwd)
    _note("nrv_reattn_softmax_fwd", fwd)
    _note("nrv_reattn_softmax_bwd", bwd)
    if case[3] == 1:
        assert bool((P == 1).all()) and not dS.any()
    if case[1] == 1:                                                      # the LayerNorm over one head leaves beta
        assert torch.equal(A, i["beta"].view(1, 1, 1, 1).expand_as(A)) and not dS.any() and not dW.any() and not dg.any()


@pytest.mark.parametrize("case", TILE_CASES, ids=str)
@pytest.mark.parametrize("kind", R.KINDS)
def test_flat_bounds_hold_for_the_emulation(case, kind):
    i = R.inputs(*case, kind)
    out = R.mix_fwd_emul(i["S"], i["W1"])
    f, fb = R.mix_fwd_ref(i["S"], i["W1"]), R.mix_fwd_ref(i["S"], i["W1"], bf=True)
    fwd = {"out": R.ratio(out, f["out"], f["out_bound"]), "out_bf16": R.ratio(R.bf16(out), fb["out"], fb["out_bound"])}
    din, dW = R.mix_bwd_emul(i["dA"], i["S"], i["W1"])
    bwd = _ratios(R.mix_bwd_ref(i["dA"], i["S"], i["W1"]), {"din": din, "dW": dW})
    print("head_mix", case, kind, "error / bound:", fwd, bwd)
    _note("nrv_head_mix_fwd", fwd)
    _note("nrv_head_mix_bwd", bwd)
    P = torch.softmax(i["S"], -1)
    A = R.ra_norm_fwd_emul(P, i["W"], i["gamma"], i["beta"])
    a, ab = R.ra_norm_fwd_ref(P, i["W"], i["gamma"], i["beta"]), R.ra_norm_fwd_ref(P, i["W"], i["gamma"], i["beta"], bf=True)
    fwd = {"A": R.ratio(A, a["A"], a["A_bound"]), "A_bf16": R.ratio(R.bf16(A), ab["A"], ab["A_bound"])}
    dP, dW, dg, db = R.ra_norm_bwd_emul(i["dA"], P, i["W"], i["gamma"])
    bwd = _ratios(R.ra_bwd_ref(i["dA"], P, i["W"], i["gamma"], softmax=False), {"dP": dP, "dW": dW, "dgamma": dg, "dbeta": db})
    print("reattn_norm", case, kind, "error / bound:", fwd, bwd)
    _note("nrv_reattn_norm_fwd", fwd)
    _note("nrv_reattn_norm_bwd", bwd)
    if case[1] == 1:
        assert torch.equal(A, i["beta"].view(1, 1, 1, 1).expand_as(A)) and not dP.any() and not dW.any() and not dg.any()


def test_print_the_worst_ratios():
    """runs after the three tests above (file order): the record of how tight the bounds are on the emulation"""
    for entry in sorted(WORST):
        print(entry, {n: round(r, 4) for n, r in WORST[entry].items()})
    if WORST:
        assert all(r <= 1.0 for w in WORST.values() for r in w.values())


# ---- wrong kernels ---------------------------------------------------------------------------------
def test_a_key_dropped_from_the_row_sum_exceeds_the_bound():
    for case in ((2, 3, 2, 255), (1, 16, 1, 1021)):
        i = R.inputs(*case)
        P, _ = R.th_fwd_emul(i["S"], i["W1"], i["W2"], drop_last=True)
        f = R.th_fwd_ref(i["S"], i["W1"], i["W2"])
        assert R.ratio(P, f["P"], f["P_bound"]) > 1.0
        P, _ = R.ra_fwd_emul(i["S"], i["W"], i["gamma"], i["beta"], drop_last=True)
        s = R.ra_softmax_ref(i["S"])
        assert R.ratio(P, s["P"], s["P_bound"]) > 1.0


def test_an_untransposed_gradient_mix_exceeds_the_bound():
    case = (2, 7, 1, 64)
    i = R.inputs(*case)
    P, _ = R.th_fwd_emul(i["S"], i["W1"], i["W2"])
    ref = R.th_bwd_ref(i["dA"], P, i["S"], i["W1"], i["W2"])
    dS, _, _ = R.th_bwd_emul(i["dA"], P, i["S"], i["W1"], i["W2"], untransposed=True)
    assert R.ratio(dS, ref["dS"], ref["dS_bound"]) > 1.0
    P, _ = R.ra_fwd_emul(i["S"], i["W"], i["gamma"], i["beta"])
    ref = R.ra_bwd_ref(i["dA"], P, i["W"], i["gamma"])
    assert R.ratio(R.ra_bwd_emul(i["dA"], P, i["W"], i["gamma"], untransposed=True)[0], ref["dS"], ref["dS_bound"]) > 1.0
    flat = (2, 8, 7, 73)
    i = R.inputs(*flat)
    ref = R.mix_bwd_ref(i["dA"], i["S"], i["W1"])
    assert R.ratio(R.mix_bwd_emul(i["dA"], i["S"], i["W1"], untransposed=True)[0], ref["din"], ref["din_bound"]) > 1.0
    P = torch.softmax(i["S"], -1)
    ref = R.ra_bwd_ref(i["dA"], P, i["W"], i["gamma"], softmax=False)
    assert R.ratio(R.ra_norm_bwd_emul(i["dA"], P, i["W"], i["gamma"], untransposed=True)[0], ref["dP"], ref["dP_bound"]) > 1.0


def test_pad_positions_left_in_front_of_th_pairs_exceed_the_bound():
    """the scalar path's images: positions Nk .. round-up-to-4 must be zero when S . dT is summed"""
    case = (2, 11, 2, 5)
    assert R.vec(case[3]) == 1
    i = R.inputs(*case)
    P, _ = R.th_fwd_emul(i["S"], i["W1"], i["W2"])
    ref = R.th_bwd_ref(i["dA"], P, i["S"], i["W1"], i["W2"])
    _, dW1, _ = R.th_bwd_emul(i["dA"], P, i["S"], i["W1"], i["W2"], pad_garbage=1.0)
    assert R.ratio(dW1, ref["dW1"], ref["dW1_bound"]) > 1.0


def test_an_idle_split_counted_twice_exceeds_the_bound():
    """H = 3: 28 splits of 9 pairs use 252 threads; threads 252 .. 255 must return 0"""
    case = (2, 3, 2, 255)
    i = R.inputs(*case)
    P, _ = R.th_fwd_emul(i["S"], i["W1"], i["W2"])
    ref = R.th_bwd_ref(i["dA"], P, i["S"], i["W1"], i["W2"])
    _, _, dW2 = R.th_bwd_emul(i["dA"], P, i["S"], i["W1"], i["W2"], idle_twice=True)
    assert R.ratio(dW2, ref["dW2"], ref["dW2_bound"]) > 1.0


def test_the_one_pass_variance_exceeds_the_bound():
    """peaked: at the peak all heads of M agree to a fraction of a per cent, E[M^2] - E[M]^2 cancels"""
    worst = 0.0
    for case in R.FUSED_ALL_KINDS:
        i = R.inputs(*case, "peaked")
        P, A = R.ra_fwd_emul(i["S"], i["W"], i["gamma"], i["beta"], one_pass=True)
        ref = R.ra_norm_fwd_ref(P, i["W"], i["gamma"], i["beta"])
        r = R.ratio(A, ref["A"], ref["A_bound"])
        print("one-pass variance", case, "A error / bound:", r)
        worst = max(worst, r)
    assert worst > 1.0


def test_dgamma_without_the_last_wave_exceeds_the_bound():
    for case, fused in (((1, 5, 2, 257), True), ((2, 3, 7, 73), False)):
        i = R.inputs(*case)
        P = torch.softmax(i["S"], -1)
        ref = R.ra_bwd_ref(i["dA"], P, i["W"], i["gamma"], softmax=fused)
        emul = R.ra_bwd_emul if fused else R.ra_norm_bwd_emul
        assert R.ratio(emul(i["dA"], P, i["W"], i["gamma"])[2], ref["dgamma"], ref["dgamma_bound"]) <= 1.0
        assert R.ratio(emul(i["dA"], P, i["W"], i["gamma"], skip_last_wave=True)[2], ref["dgamma"], ref["dgamma_bound"]) > 1.0


def test_the_smallest_entry_of_a_gradient_matrix_is_pinned():
    """the hole of a max-norm comparison: the entry of smallest magnitude replaced by zero passes it and fails here"""
    case = (2, 11, 2, 5)
    i = R.inputs(*case)
    P, _ = R.th_fwd_emul(i["S"], i["W1"], i["W2"])
    ref = R.th_bwd_ref(i["dA"], P, i["S"], i["W1"], i["W2"])
    _, dW1, dW2 = R.th_bwd_emul(i["dA"], P, i["S"], i["W1"], i["W2"])
    flat = R.inputs(2, 8, 7, 73)
    fref = R.mix_bwd_ref(flat["dA"], flat["S"], flat["W1"])
    for got, r, b in ((dW1, ref["dW1"], ref["dW1_bound"]), (dW2, ref["dW2"], ref["dW2_bound"]),
                      (R.mix_bwd_emul(flat["dA"], flat["S"], flat["W1"])[1], fref["dW"], fref["dW_bound"])):
        assert R.ratio(got, r, b) <= 1.0
        bad = got.clone()
        bad.view(-1)[r.abs().view(-1).argmin()] = 0.0
        assert float((bad.double() - r).abs().max() / r.abs().max()) < 0.05          # small in the max norm
        assert R.ratio(bad, r, b) > 1.0


def test_the_fp64_references_are_autograd():
    B, H, Nq, Nk = 2, 5, 3, 7
    i = R.inputs(B, H, Nq, Nk)
    S, W1, W2, W, ga, be = (i[k].double().clone().requires_grad_(True) for k in ("S", "W1", "W2", "W", "gamma", "beta"))
    P = torch.softmax(torch.einsum("bhij,hg->bgij", S, W1), -1)
    A = torch.einsum("bhij,hg->bgij", P, W2)
    A.backward(i["dA"].double())
    ref = R.th_bwd_ref(i["dA"], P.detach(), i["S"], i["W1"], i["W2"])
    for n, t in (("dS", S.grad), ("dW1", W1.grad), ("dW2", W2.grad)):
        assert torch.allclose(t, ref[n], rtol=0, atol=1e-12), n
    S.grad = None
    P = torch.softmax(S, -1)
    M = torch.einsum("bhij,hg->bgij", P, W)
    A = torch.nn.functional.layer_norm(M.permute(0, 2, 3, 1), (H,), ga, be, R.EPS).permute(0, 3, 1, 2)
    assert torch.allclose(A.detach(), R.ra_norm_fwd_ref(P.detach(), i["W"], i["gamma"], i["beta"])["A"], rtol=0, atol=1e-12)
    A.backward(i["dA"].double())
    ref = R.ra_bwd_ref(i["dA"], P.detach(), i["W"], i["gamma"])
    for n, t in (("dS", S.grad), ("dW", W.grad), ("dgamma", ga.grad), ("dbeta", be.grad)):
        assert torch.allclose(t, ref[n], rtol=0, atol=1e-11), n


# ---- the case lists ----------------------------------------------------------------------------------
def test_the_case_lists_reach_the_edges_they_name():
    assert all(1 <= H <= R.TH_MAXH and 1 <= Nk <= R.TH_MAXNK and B in (1, 2) and Nq in (1, 2, 3) for B, H, Nq, Nk in R.FUSED_CASES)
    nks = {c[3] for c in R.FUSED_CASES}
    assert nks >= {1, 2, 3, 4, 5, 57, 60, 63, 64, 65, 255, 256, 257, 1017, 1020, 1021, 1024, 1025}
    for name, values in R.BUMP_CASES.items():
        for Nk in values:
            assert Nk in nks and R.th_ld(Nk) == ((Nk + 3) & ~3) + 8 and R.th_ld(Nk) % 64 == 4, (name, Nk)      # really bumps
            assert (R.vec(Nk) == 4) == (name == "bump vector") and (Nk % 4 == 0) == (name == "bump vector")
    for Nk in sorted(nks - {57, 58, 59, 60, 1017, 1018, 1019, 1020}):
        assert R.th_ld(Nk) == ((Nk + 3) & ~3) + 4 and R.th_ld(Nk) % 64 != 0
    assert all(R.th_ld(n) % 4 == 0 and R.th_ld(n) % 64 != 0 and R.th_ld(n) >= ((n + 3) & ~3) + 4 for n in range(1, R.TH_MAXNK + 1))
    for H in (1, 2, 3, 5, 7, 11, 12, 15, 16):
        vs = {R.vec(c[3]) for c in R.FUSED_CASES if c[1] == H}
        assert vs == {1, 4}, H
    assert (2, 16, 1, 1025) in R.FUSED_CASES
    assert (2 * 16 * R.th_ld(1025) + 2 * R.TH_THREADS) * 4 == 134144      # the backward's LDS at the maximum: TH_LDS_MAX
    used = {H: (R.TH_THREADS // (H * H)) * H * H for H in (3, 11, 12, 15)}
    assert used == {3: 252, 11: 242, 12: 144, 15: 225}
    assert all(c in R.FUSED_CASES for c in R.FUSED_ALL_KINDS) and all(c in R.FLAT_CASES for c in R.FLAT_ALL_KINDS)
    rows = [B * Nq for B, _, Nq, _ in R.ROW_WALK_CASES]
    assert rows == [1035, 2051] and [R.vec(c[3]) for c in R.ROW_WALK_CASES] == [1, 4]
    assert [r - R.TH_PARTS for r in rows] == [11, 1027]                    # 11 workgroups own two rows; 1024 two and 3 three
    assert {c[2] * c[3] for c in R.FLAT_CASES} == set(R.FLAT_M) and all(c[0] == 2 for c in R.FLAT_CASES)
    for H in (1, 3, 8, 11, 16):
        assert {R.vec(c[2] * c[3]) for c in R.FLAT_CASES if c[1] == H} == {1, 4}, H
    assert {c[1] for c in R.FLAT_CASES} == {1, 3, 8, 11, 16}
    tiles = [B * -(-(Nq * Nk) // R.TH_TILE) for B, _, Nq, Nk in R.TILE_WALK_CASES]
    assert tiles == [1066, 1025] and [R.vec(c[2] * c[3]) for c in R.TILE_WALK_CASES] == [4, 1] and (25 * 501) % R.TH_TILE != 0
    for (B, H, Nq, Nk), V in zip(R.GRID_CAP_CASES, (1, 4)):
        assert R.vec(Nq * Nk) == V and B * (Nq * Nk // V) > 65536 * R.TH_THREADS and H == 1
    assert [B * (Nq * Nk // R.vec(Nq * Nk)) for B, _, Nq, Nk in R.GRID_CAP_CASES] == [16795650, 16778240]
