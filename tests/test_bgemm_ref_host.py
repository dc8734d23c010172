"""CPU: the batched-GEMM case table of tests/bgemm_ref.py against the real dispatch (kernels.bgemm_plan, the function nrv_bgemm
itself decides with), the table's coverage of every staging / store path and edge, the derived bound on the fp32 emulation of
the kernel's arithmetic, seeded mutations the table must catch, and the refusals through the plan query."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bgemm_ref as R  # noqa: E402

from noise_robust_vit_amd import _lib, kernels as K  # noqa: E402

NAMES = [c.name for c in R.TABLE]


def _plan(case):
    ops = []
    for side in ("a", "b", "c"):
        op = getattr(case, side)
        ops += [(R.fake_address(case, side), op.torch_dtype), op.strides]
    return K.bgemm_plan(*ops, case.G1, case.G2, case.M, case.N, case.K)


@pytest.mark.parametrize("name", NAMES)
def test_record_gets_the_plan_it_names(name):
    case = R.BY_NAME[name]
    pl = _plan(case)
    got = (pl["a_vec"], pl["b_vec"], pl["c_vec"], pl["tiles_m"], pl["tiles_n"])
    assert got == case.plan, (name, got, case.plan)
    assert pl["blocks"] == case.G1 * case.G2 * case.plan[3] * case.plan[4]
    # the label of every operand is what its strides are
    assert R.layout_holds(case, "a") and R.layout_holds(case, "b") and R.cform_holds(case), name
    assert case.edge


def test_table_covers_every_path_and_edge():
    assert R.coverage_gaps(R.TABLE) == []
    assert 25 <= len(R.TABLE) <= 35
    for c in R.TABLE:
        assert max(c.M, c.N, c.K) <= 200 and c.G1 * c.G2 <= 6, c.name
        if c.real is None and c.name != "grid_3x2_batched":
            assert c.M in R.DIMS_MN and c.N in R.DIMS_MN and c.K in R.DIMS_K, c.name


@pytest.mark.parametrize("name", NAMES)
def test_no_record_is_spare(name):
    """Without this record some path or edge is no longer covered; the message names it."""
    rest = tuple(c for c in R.TABLE if c.name != name)
    gaps = R.coverage_gaps(rest)
    assert gaps, f"{name} carries nothing the other records do not"
    print(name, "alone carries:", gaps)


def test_real_records_restate_the_model_calls():
    """The strides of the real records come from the model code's own helpers, at the smallest sizes that keep the calls' edges:
    N = 67 is odd, so the rows of the fp32 [N, N] matrices are only dword-aligned, and dh = 40 leaves dh % 32 == 8, one whole bf16
    vector behind a full K-step; CaiT's class attention has one query row and 1 + 16 keys, a bf16 matrix with an odd row stride."""
    from noise_robust_vit_amd import cait
    B, H, N, dh = R.REAL_B, R.REAL_H, R.REAL_N, R.REAL_DH
    assert (B, H, N, dh) == (2, 2, 67, 40) and (R.CAIT_N, R.CAIT_NK) == (1, 17)
    hq, hqT, ho, mat, matT = K._composed_strides(N, H, dh)
    c = R.BY_NAME["composed_dK"]                           # bgemm((dS, 0), matT, (qkv, 0), hq, (dqkv, H * dh), hq, B, H, N, dh, N, scale)
    assert (c.a.strides, c.b.strides, c.c.strides, c.c.off) == (matT, hq, hq, H * dh) and (c.M, c.N, c.K) == (N, dh, N)
    sq, skv, skvT, cm, cmT = cait._strides(1, 17, H, dh)
    c = R.BY_NAME["cait_O"]                                # K.bgemm((A, 0), mat, (kv, inner), skv, (o, 0), sq, B, H, n, dh, Nk, 1.0)
    assert (c.a.strides, c.b.strides, c.c.strides, c.b.off) == (cm, skv, sq, H * dh) and (c.M, c.N, c.K) == (1, dh, 17)
    assert c.a.dtype == "bf16" and c.plan[:2] == (False, True)
    for fam in ("composed", "cait"):
        for c in R.TABLE:
            if c.real and c.real.startswith(fam):
                assert (c.G1, c.G2) == (B, H)


@pytest.mark.parametrize("name", NAMES)
def test_record_is_a_valid_call(name):
    """What kernels.bgemm checks (last < numel, no negative stride), and C's addressed elements are distinct."""
    case = R.BY_NAME[name]
    inp = R.inputs(name, "random")
    for side, store in (("a", inp.a), ("b", inp.b), ("c", R.sentinel_storage(case))):
        op = getattr(case, side)
        rows, cols = case.dims(side)
        st = op.strides
        last = op.off + (rows - 1) * st[0] + (cols - 1) * st[1] + (case.G1 - 1) * st[2] + (case.G2 - 1) * st[3]
        assert op.off >= 0 and min(st) >= 0 and last < store.numel()
        assert last + R.TAIL_PAD < store.numel() + 1           # a NaN moat behind the last element
    ic = inp.ic.reshape(-1)
    assert ic.unique().numel() == ic.numel(), "C's addressed sets overlap"
    # every operand storage has NaN outside its addressed set, finite values inside, magnitudes in [2^-6, 4] or zero
    for store, ix in ((inp.a, inp.ia), (inp.b, inp.ib)):
        mask = torch.zeros(store.numel(), dtype=torch.bool)
        mask[ix.reshape(-1)] = True
        assert bool(torch.isnan(store[~mask]).all()) and int((~mask).sum()) >= R.TAIL_PAD
        v = store[mask].float().abs()
        assert bool(((v >= 2.0 ** -6) & (v <= 4.0)).all())
    for kind, side in (("select_a", "a"), ("select_b", "b")):
        s = R.inputs(name, kind)
        v = (s.a[s.ia] if side == "a" else s.b[s.ib]).float()
        assert bool(((v == 0) | (v == 1)).all()) and bool((v.sum(dim=-1 if side == "a" else -2) == 1).all())


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_emulation_stays_inside_the_bound(name, kind):
    inp = R.inputs(name, kind)
    case = inp.case
    store = R.emulate(inp)
    got = store[inp.ic]
    assert not bool(torch.isnan(got).any())
    assert bool((R.unwritten(case, store, inp.ic) == R.sentinel_bits(case)).all())
    r = R.ratio(got, inp.ref, inp.bound)
    assert r <= 1.0, (name, kind, r)
    if kind != "random":
        assert torch.equal(got, inp.exact)
        # and that exact result is the other operand's selected value, halved
        other = (inp.b[inp.ib] if kind == "select_a" else inp.a[inp.ia]).to(torch.bfloat16).double()
        rows = case.M if kind == "select_a" else case.N
        sel = (5 * torch.arange(rows) + 3) % case.K
        want = other[:, :, sel, :] if kind == "select_a" else other[:, :, :, sel]
        assert torch.equal(got.double(), 0.5 * want)


def _caught(inp, mutate):
    store = R.emulate(inp, mutate)
    got = store[inp.ic]
    if inp.kind != "random":
        return not torch.equal(got, inp.exact)
    return R.ratio(got, inp.ref, inp.bound) > 1.0


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_table_catches_a_wrong_kernel(mutate):
    caught = [(n, k) for n in NAMES for k in R.KINDS if _caught(R.inputs(n, k), mutate)]
    print(mutate, "caught by", len(caught), "of", len(NAMES) * len(R.KINDS))
    assert caught, mutate
    names = {n for n, _ in caught}
    if mutate == "drop_last_k":                        # every record, in its random kind; in a select kind wherever some row selects K - 1
        assert all((n, "random") in caught for n in NAMES)
        for n in NAMES:
            c = R.BY_NAME[n]
            for kind, side in (("select_a", "a"), ("select_b", "b")):
                hits = any((5 * r + 3) % c.K == c.K - 1 for r in range(c.rows(side)))
                assert ((n, kind) in caught) == hits, (n, kind)
    if mutate == "zero_row_tail":                      # every record with a row-fast vector operand whose rows end inside a vector
        want = {c.name for c in R.TABLE for s in ("a", "b")
                if getattr(c, s).layout in R.VECTOR_KINDS and "a row tail shorter than the vector" in R._edges(c, s)}
        assert want and names == want
    if mutate == "swap_tiles":
        assert "grid_3x2_batched" in names and names == {c.name for c in R.TABLE if c.plan[3] != c.plan[4]}
    if mutate == "moat":                               # NaN times a staged zero: every record with a K tail and a gap behind row 0
        gapped = {c.name for c in R.TABLE if c.K % R.KSTEP and c.real is None and c.a.layout != "L11"}
        assert gapped and gapped <= names <= {c.name for c in R.TABLE if c.K % R.KSTEP}


def _raw_args(G1=1, G2=1, M=8, N=8, K=8, dt=(1, 1, 0)):
    a = [0x1000, dt[0], K, 1, 0, 0, 0x2000, dt[1], N, 1, 0, 0, 0x3000, dt[2], N, 1, 0, 0, G1, G2, M, N, K]
    return a


NRV_ERR_SHAPE, NRV_ERR_DTYPE = -2, -3              # include/nrv.h


def test_error_codes_are_the_header_s():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nrv.h")).read()
    err = {n: int(v) for n, v in re.findall(r"#define (NRV_ERR_[A-Z]+)\s+\((-\d+)\)", hdr)}
    assert (err["NRV_ERR_SHAPE"], err["NRV_ERR_DTYPE"]) == (NRV_ERR_SHAPE, NRV_ERR_DTYPE)


@pytest.mark.parametrize("what,kw,code", [
    ("G1 = 0", dict(G1=0), NRV_ERR_SHAPE),
    ("M = 0", dict(M=0), NRV_ERR_SHAPE),
    ("a bad dtype code", dict(dt=(1, 7, 0)), NRV_ERR_DTYPE),
    ("more than 2^31 - 1 workgroups", dict(G1=2 ** 16, G2=2 ** 15, M=65, N=8), NRV_ERR_SHAPE),
])
def test_refusals_through_the_plan_query(what, kw, code):
    """The query gives the code include/nrv.h documents for nrv_bgemm, which refuses through the same bg_plan().  Only the query
    is called: it launches nothing, so the made-up addresses are never dereferenced."""
    args = _raw_args(**kw)
    pl = _lib.BgemmPlan()
    assert _lib.load().nrv_bgemm_plan(*args, ctypes.addressof(pl)) == code, what
    if what != "a bad dtype code":                       # the wrapper turns the code into an NrvError (a bad dtype never gets past it)
        dts = {0: torch.float32, 1: torch.bfloat16}
        with pytest.raises(_lib.NrvError, match=f"code {code}"):
            K.bgemm_plan((args[0], dts[args[1]]), args[2:6], (args[6], dts[args[7]]), args[8:12], (args[12], dts[args[13]]),
                         args[14:18], *args[18:])
    else:
        with pytest.raises(_lib.NrvError):
            K.bgemm_plan((args[0], torch.float16), args[2:6], (args[6], torch.bfloat16), args[8:12], (args[12], torch.float32),
                         args[14:18], *args[18:])


def test_plan_query_null_arguments_and_the_largest_accepted_grid():
    lib = _lib.load()
    args = _raw_args()
    assert lib.nrv_bgemm_plan(*args, None) == -1
    pl = _lib.BgemmPlan()
    assert lib.nrv_bgemm_plan(None, *args[1:], ctypes.addressof(pl)) == -1
    args = _raw_args(G1=2 ** 16, G2=2 ** 15 - 1, M=8, N=8)             # one tile x (2^31 - 2^16) batches: still a valid grid
    assert lib.nrv_bgemm_plan(*args, ctypes.addressof(pl)) == 0 and pl.blocks == 2 ** 16 * (2 ** 15 - 1) and pl.tiles_m == 1
