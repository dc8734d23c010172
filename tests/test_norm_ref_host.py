"""CPU: the case tables, references and bounds of tests/norm_ref.py, before any kernel runs (tests/test_norm_edges_gpu.py uses them).

  * the dispatch restated in norm_ref.py is what csrc/nrv_norm.hip states (LN_THREADS, the 512 split, the `steps` list, the switch), and
    the LayerNorm table reaches all 60 backward and all 20 forward instantiations;
  * the fp64 references are torch's layer_norm / batch_norm + Hardswish in fp64 through autograd;
  * the Hardswish-kink cap holds for every batch-norm case;
  * the fp32 emulation in each kernel's own summation order stays within HALF of every bound on every case, taken on the fp32 values
    before a bf16 store, and within the bound after the store.  (A store is one rounding to nearest with unit round-off 2^-8, which the
    bottom of a binade attains: the store term of the bounds is that 2^-8, so a stored output can use all of it.  The factor of two is
    for another order of the sums, and a store has no order.)
  * each of the 19 wrong kernels of the issue, written as a variant of the emulation, is over the bound on a named case; the one that
    changes nothing is asserted to change nothing, with the reason.

Worst emulation error / bound per family (before the store | after it), as test_emulation_stays_within_half_of_every_bound prints them:
  LayerNorm          0.237 (dx fp32, width 8)           | 0.995 (y, width 512)
  padded LayerNorm   0.299 (dx fp32, n 65, 129 rows)    | 0.996 (dx bf16, n 1323)
  batch norm         0.456 (running mean, T 512)        | 0.992 (z bf16, T 1000)
  column sums        0.035 (T 129, N 1536, beta 1)      | the output is fp32
The wrong kernels exceed a bound by factors from 7 (mean(dz) over the padded rows, T = 513) to infinity (a NaN pad reached a sum).
"""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_ref as R  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "noise_robust_vit_amd", "csrc")


def _worst(r):
    return max(r.values())


def _find(cases, pred):
    return next(c for c in cases if pred(c))


# ---------------------------------------------------------------------------------------------------------------------------------
# dispatch and coverage
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_restated_dispatch_is_the_sources():
    d = R.read_dispatch(CSRC)
    assert d["threads"] == R.LN_THREADS and d["split"] == R.LN_SPLIT and d["steps"] == R.LN_STEPS
    assert d["switch"] == R.LN_STEPS, "every dispatched chunk count has its case in NRV_DISPATCH_MAXJ"


def test_the_layernorm_table_reaches_every_instantiation():
    reach = R.ln_reachable()
    assert sorted(reach) == sorted([(1, 32), (2, 32), (3, 32), (4, 32), (3, 64), (4, 64), (5, 64), (6, 64), (8, 64), (16, 64)])
    bwd = {(c.xbf, c.dres) + R.ln_inst(c.dim) for c in R.LN_CASES}
    fwd = {(c.xbf,) + R.ln_inst(c.dim) for c in R.LN_CASES}
    assert bwd == {(x, d) + i for x, d, i in itertools.product((0, 1), (0, 1, 2), reach)} and len(bwd) == 60
    assert fwd == {(x,) + i for x, i in itertools.product((0, 1), reach)} and len(fwd) == 20


def test_the_layernorm_table_holds_what_the_issue_lists():
    dims = {c.dim for c in R.LN_CASES}
    assert dims >= {520, 776, 1288, 1536, 1544, 1800, 2048, 2056, 4088, 4096, 8, 64, 136, 392, 504, 512}
    # partial, full and idle last chunks
    for lpr, want in ((32, R.LN_DIMS_32), (64, R.LN_DIMS_64)):
        kinds = set()
        for dim in want:
            J, L = R.ln_inst(dim)
            assert L == lpr
            chunks = dim // 4
            kinds.add("idle" if -(-chunks // L) < J else ("full" if chunks % L == 0 else "partial"))
        # the half-wave form dispatches every count 1..4, so no chunk of it is ever idle; the 64-lane form rounds 7 up to 8 and 9..15 to 16
        assert kinds == ({"idle", "full", "partial"} if lpr == 64 else {"full", "partial"}), (lpr, kinds)
    assert all(c.rows == 9 for c in R.LN_CASES[:-4]) and sorted((c.dim, c.rows) for c in R.LN_CASES[-4:]) == [(136, 1), (136, 2), (1800, 1), (1800, 2)]
    for form in (lambda c: c.dim <= 512, lambda c: c.dim > 512):
        cs = [c for c in R.LN_CASES if form(c)]
        assert {c.eps for c in cs} == {1e-5, 1e-6} and {c.out for c in cs} == set(R.OUTS)
        assert {(c.acc, c.dres > 0) for c in cs} == {(0, False), (0, True), (1, False), (1, True)}
        assert {(c.out, c.dres) for c in cs} >= {("bf16", 1), ("bf16", 2), ("f32", 2)}
    i = R.ln_inputs(_find(R.LN_CASES, lambda c: c.dim == 64 and not c.xbf))
    assert (i["gamma"] == 0).any() and (i["gamma"] < 0).any()
    x, dy = i["x"].astype(np.float64), i["dy"]
    assert len(R.LN_ROW_KINDS) == R.LN_ROWS == x.shape[0]
    assert abs(x[1].mean()) > 500 * x[1].std() and x[2].std() == 0 and x[3].std() < 2e-4 and x[4].std() > 500 and x[5].max() == 1e4
    assert not dy[6].any() and np.count_nonzero(dy[7]) == 1 and np.count_nonzero(dy[8]) > 32
    y = R.bn_inputs(_find(R.BN_CASES, lambda c: c.T == 1000 and c.C == 20))["y"].astype(np.float64)
    assert len(R.BN_COL_KINDS) == 5 and abs(y[:, 1].mean()) > 500 * y[:, 1].std() and y[:, 2].std() == 0 and y[:, 3].max() == 1e4 and y[:, 4].std() < 2e-4
    X = R.cs_inputs(R.CS_CASES[-1])["X"].astype(np.float64)
    assert len(R.CS_COL_KINDS) == 4 and X[:, 1].std() == 0 and np.abs(X[:, 2]).min() > 200 and abs(X[:, 2].sum()) < 300 and np.count_nonzero(X[:, 3]) == 1
    assert R.ln_inst(R.LN_GUARDED.dim) == (8, 64) and R.LN_GUARDED.acc and R.LN_GUARDED.dres == 2


def test_the_other_tables_hold_what_the_issue_lists():
    assert {(c.n, c.ld) for c in R.PAD_CASES} == set(R.PAD_SHAPES) and {c.rows for c in R.PAD_CASES} == {1, 9, 127, 129}
    assert {(c.xbf, c.dres, c.acc) for c in R.PAD_CASES} == set(itertools.product((0, 1), (0, 1, 2), (0, 1)))
    assert R.lnp_slabs(127) == 1 and R.lnp_slabs(129) == 2 and -(-129 // 2) == 65
    for c in R.PAD_CASES:
        i = R.ln_inputs(c)
        for k in ("x", "dy", "dres"):
            if i[k] is not None and c.ld > c.n:
                assert np.isnan(i[k][:, c.n:]).all() and np.isfinite(i[k][:, :c.n]).all()
    bn = R.BN_CASES
    assert {c.T for c in bn} == {1, 2, 3, 5, 512, 513, 1000, 32769} and {c.C for c in bn} == {4, 20, 64, 68, 132}
    assert [c.C for c in bn if c.T == 32769] == [4] and -(-32769 // R.BN_CHUNK) == 65
    assert all(c.per == 0 or c.T % c.per == 0 for c in bn)
    assert {(c.dzbf, c.act) for c in bn} == set(itertools.product((0, 1), (0, 1)))
    assert any(c.act and c.per for c in bn) and any(c.act and not c.training for c in bn) and any(c.per > 1 for c in bn)
    assert {c.mom for c in bn if c.training} == {0.0, 0.1, 1.0} and {c.out for c in bn} == set(R.OUTS)
    assert any(c.res for c in bn) and any(c.res and c.per for c in bn) and any(c.T == 1 and c.training for c in bn)
    assert {(c.T, c.N, c.ld) for c in R.CS_CASES} == set(R.CS_SHAPES) and {c.beta for c in R.CS_CASES} == {0.0, 1.0, -0.5}
    assert R.colsum_split(5) == (4, 2) and R.colsum_split(2) == (4, 1) and R.colsum_split(129) == (4, 33)
    i = R.cs_inputs(R.CsCase(5, 520, 1032, 1.0))
    assert np.isnan(i["back"][:, 520:]).all() and np.isnan(i["back"][5:]).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the references are the definitions
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_layernorm_reference_is_torchs_in_fp64():
    c = R.LnCase(136, 9, 0, 1, 1e-6, "f32", 1)
    i = R.ln_inputs(c)
    ref = R.ln_ref(c, i)
    x = torch.from_numpy(i["x"]).double().requires_grad_(True)
    g, b = (torch.from_numpy(i[k]).double().requires_grad_(True) for k in ("gamma", "beta"))
    y = torch.nn.functional.layer_norm(x, (c.dim,), g, b, c.eps)
    y.backward(torch.from_numpy(i["dy"]).double())
    assert np.allclose(y.detach().numpy(), ref["y"], rtol=1e-12, atol=1e-12)
    assert np.allclose(x.grad.numpy(), ref["core"], rtol=1e-9, atol=1e-12)
    assert np.allclose(g.grad.numpy() + i["dgamma0"], ref["dgamma"], rtol=1e-10, atol=1e-12)
    assert np.allclose(b.grad.numpy() + i["dbeta0"], ref["dbeta"], rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("training", [1, 0])
def test_the_batchnorm_reference_is_torchs_in_fp64(training):
    c = R.BnCase(5, 20, 0, 1, 1, training, 0.1, "f32", 1)
    i = R.bn_inputs(c)
    ref = R.bn_ref(c, i)
    y = torch.from_numpy(i["y"]).double().requires_grad_(True)
    g, b = (torch.from_numpy(i[k]).double().requires_grad_(True) for k in ("gamma", "beta"))
    rm, rv = torch.from_numpy(i["run_mean"]).double().clone(), torch.from_numpy(i["run_var"]).double().clone()
    z = torch.nn.functional.batch_norm(y, rm, rv, g, b, bool(training), c.mom, R.BN_EPS)
    f = torch.from_numpy(i["keep"]).double()[:, None] / R.BN_SURVIVAL
    out = torch.nn.functional.hardswish(z) * f + torch.from_numpy(i["res"]).double()
    out.backward(torch.from_numpy(i["dz"]).double())
    assert np.allclose(out.detach().numpy(), ref["z"], rtol=1e-10, atol=1e-10)
    assert np.allclose(y.grad.numpy(), ref["dy"], rtol=1e-8, atol=1e-10)
    assert np.allclose(g.grad.numpy(), ref["dgamma"], rtol=1e-9, atol=1e-10) and np.allclose(b.grad.numpy(), ref["dbeta"], rtol=1e-9, atol=1e-10)
    if training:
        assert np.allclose(rm.numpy(), ref["run_mean"], rtol=1e-12) and np.allclose(rv.numpy(), ref["run_var"], rtol=1e-12)


def test_one_row_batchnorm_is_the_definition_written_out():
    """torch refuses training-mode batch norm at T = 1; the reference is var = 0 and a running variance updated with the biased value"""
    c = _find(R.BN_CASES, lambda c: c.T == 1 and c.training and c.mom > 0)
    i = R.bn_inputs(c)
    ref = R.bn_ref(c, i)
    assert (ref["m2"] == 0).all() and np.allclose(ref["invstd"], R.BN_EPS ** -0.5) and (ref["xh"] == 0).all()
    assert np.allclose(ref["run_var"], (1 - c.mom) * i["run_var"]) and np.allclose(ref["mean"], i["y"][0])


def test_the_kink_cap_holds_for_every_batchnorm_case():
    seen = 0
    for c in R.BN_CASES:
        k = R.bn_ref(c, R.bn_inputs(c))["kink"]
        seen += int(k.sum())
        assert R.kink_cap_ok(c, k), (R.case_id(c), int(k.sum()), int(k.sum(0).max()))
        assert c.act or not k.any()
    assert seen > 0 and R.RESEEDED == {}, "no case needed another draw"


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulation fits, the wrong kernels do not
# ---------------------------------------------------------------------------------------------------------------------------------
def _emul_ratios(c, store):
    if isinstance(c, R.BnCase):
        i = R.bn_inputs(c)
        return R.bn_check(c, i, R.bn_emul(c, i, store=store))
    if isinstance(c, R.CsCase):
        i = R.cs_inputs(c)
        return R.cs_check(c, i, R.cs_emul(c, i))
    i = R.ln_inputs(c)
    return R.ln_check(c, i, R.ln_emul(c, i, store=store))


def test_emulation_stays_within_half_of_every_bound():
    for name, cases in (("LayerNorm", R.LN_CASES + (R.LN_GUARDED,)), ("padded LayerNorm", R.PAD_CASES), ("batch norm", R.BN_CASES),
                        ("column sums", R.CS_CASES)):
        worst = {False: (0.0, None, None), True: (0.0, None, None)}
        for c in cases:
            for store in (False, True):
                r = _emul_ratios(c, store)
                k = max(r, key=r.get)
                if r[k] > worst[store][0]:
                    worst[store] = (r[k], k, R.case_id(c))
                assert r[k] <= (1.0 if store else 0.5), (R.case_id(c), store, r)
        print(f"{name}: worst emulation error / bound before the store {worst[False][0]:.3f} ({worst[False][1]}, {worst[False][2]}), "
              f"after it {worst[True][0]:.3f} ({worst[True][1]}, {worst[True][2]})")


LN_WRONG = [
    ("E[x^2] - mean^2", lambda c: c.dim == 520 and not c.xbf),                              # 1: the row whose mean is 1e3 x its spread
    ("partial chunk dropped", lambda c: c.dim == 520 and not c.xbf),                        # 2: chunks 128, 129 of 130 are the third j
    ("pair shares the mean", lambda c: c.dim == 136),                                       # 3: row 1 (mean 1e3) with row 0's mean
    ("c1 c2 from dy", lambda c: c.dim == 1544),                                             # 4: gamma has a zero and a negative entry
    ("bf16 drops dres", lambda c: c.out == "bf16" and c.dres == 1),                         # 5
    ("last workgroup lost", lambda c: c.dim == 2056),                                       # 6: row 8 is alone in the third workgroup
]
PAD_WRONG = [
    ("sums to ld", lambda c: (c.n, c.ld, c.rows) == (147, 168, 9)),                         # 7: the NaN pads reach the sums
    ("pads carry dres", lambda c: (c.n, c.ld) == (147, 152) and c.dres),                    # 8
    ("slab rounded down", lambda c: c.rows == 129 and c.n == 65),                           # 9: row 128 is lost to dbeta
]
BN_WRONG = [
    ("sum and sum of squares", lambda c: c.T == 1000 and c.training and c.C >= 20),         # 10: the columns at 1e3 +- 1
    ("no skip in the chunk merge", lambda c: c.T == 2 and c.training),                      # 11: 0 / 0 in the lanes that hold no chunk
    ("keep by row", lambda c: c.T == 512 and c.per == 128),                                 # 12
    ("hs' at x^", lambda c: c.act and c.T == 513),                                          # 13
    ("mean over the padded rows", lambda c: c.T == 513 and c.training),                     # 14: 1024 instead of 513
    ("bf16 dz read as fp32", lambda c: c.dzbf and c.T == 1000),                             # 15
    ("biased running variance", lambda c: c.T == 3 and c.training and c.mom > 0),           # 16
]
CS_WRONG = [
    ("ld ignored", lambda c: (c.T, c.N, c.ld) == (5, 520, 1032)),                           # 17
    ("past T", lambda c: (c.T, c.N, c.ld) == (5, 520, 520)),                                # 18: the second chunk is row 4 alone
    ("beta per partial", lambda c: c.T == 129 and c.beta == 1.0),                           # 19: 33 partial rows
]


@pytest.mark.parametrize("wrong,pred,cases", [w + (t,) for ws, t in ((LN_WRONG, R.LN_CASES), (PAD_WRONG, R.PAD_CASES), (BN_WRONG, R.BN_CASES),
                                                                        (CS_WRONG, R.CS_CASES)) for w in ws], ids=lambda v: v if isinstance(v, str) else "")
def test_a_wrong_kernel_is_over_the_bound_on_a_named_case(wrong, pred, cases):
    c = _find(cases, pred)
    if isinstance(c, R.BnCase):
        i = R.bn_inputs(c)
        good, bad = R.bn_check(c, i, R.bn_emul(c, i)), R.bn_check(c, i, R.bn_emul(c, i, wrong))
    elif isinstance(c, R.CsCase):
        i = R.cs_inputs(c)
        good, bad = R.cs_check(c, i, R.cs_emul(c, i)), R.cs_check(c, i, R.cs_emul(c, i, wrong))
    else:
        i = R.ln_inputs(c)
        good, bad = R.ln_check(c, i, R.ln_emul(c, i)), R.ln_check(c, i, R.ln_emul(c, i, wrong))
    print(wrong, R.case_id(c), "worst error / bound", {k: f"{v:.3g}" for k, v in bad.items() if v > 1.0})
    assert _worst(good) <= 1.0 and _worst(bad) > 1.0, (R.case_id(c), bad)


def test_merging_an_empty_row_group_without_the_skip_changes_nothing():
    """Mistake 11 in bn_stats_partial_kernel alone.  Group 0 of a chunk is never empty (it holds the chunk's first row), so an empty
    group k is merged into n >= 1: nn = n, nb / nn = 0 and n nb / nn = 0, the mean and M2 move by d * 0 and d d * 0 with a finite d.
    The skip matters in bn_stats_final_kernel, where lanes without a chunk merge (0, 0, 0) into (0, 0, 0) and 0 / 0 follows."""
    for c in R.BN_CASES:
        if c.training:
            i = R.bn_inputs(c)
            a, b = R.bn_stats_emul(c, i), R.bn_stats_emul(c, i, "no skip in the group merge")
            assert all(np.array_equal(a[k], b[k]) for k in a), R.case_id(c)
            if c.T <= 63 * R.BN_CHUNK:                       # from 64 chunks on every lane holds one and nothing empty is merged
                assert np.isnan(R.bn_stats_emul(c, i, "no skip in the chunk merge")["mean"]).all()
