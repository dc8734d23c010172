"""CPU: tests/gemm_paths.py against the library's own launch planning (nrv_gemm_nt_plan / nrv_gemm_tn_plan, include/nrv.h).
Every record gets the plan it names at the CU count it names, the table covers all ten NT (tile, kernel) pairs and every TN and
grouped-TN branch, and at the device's own CU count the workload shapes plan as they did before the launch and the query shared
one planning function.  No GPU: the library plans for 256 CUs without one."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_paths as GP  # noqa: E402

CUS = 256            # what the library plans for without a device (csrc/nrv_gemm.hip physical_cus)


@pytest.fixture(scope="module")
def k():
    from noise_robust_vit_amd import kernels
    return kernels


class planned_for:
    """Reserve all but `cus` of the 256 CUs for the block; the previous value must be 0 and 0 is restored."""

    def __init__(self, k, cus):
        self.k, self.cus = k, cus

    def __enter__(self):
        prev = self.k.set_reserved_cus(CUS - self.cus)
        if prev != 0:
            self.k.set_reserved_cus(0)
            raise AssertionError(f"reservation was {prev}, not 0")

    def __exit__(self, *exc):
        self.k.set_reserved_cus(0)


def grouped_slots(rec):
    from noise_robust_vit_amd import _lib
    arr = (_lib.TnProblem * len(rec.problems))()
    for i, (M, N, _) in enumerate(rec.problems):
        arr[i] = _lib.TnProblem(None, M, None, N, None, N, M, N, 0.0, None, 0.0)       # the plan reads the shapes only
    nbytes = int(_lib.load().nrv_gemm_tn_grouped_workspace(ctypes.addressof(arr), len(rec.problems), rec.T))
    assert nbytes % GP.SLOT_BYTES == 0
    return nbytes // GP.SLOT_BYTES


@pytest.mark.parametrize("name", [r.name for r in GP.NT_TABLE])
def test_nt_record_gets_its_plan(k, name):
    rec = GP.nt(name)
    from noise_robust_vit_amd import _lib
    epis = [_lib.EPI_NONE, _lib.EPI_BIAS, _lib.EPI_BIAS_GELU, _lib.EPI_BIAS_RESIDUAL, _lib.EPI_DGELU]
    if rec.q8:
        epis += [_lib.EPI_BIAS_GELU_Q8, _lib.EPI_DGELU_Q8]
    with planned_for(k, rec.cus):
        for epi in epis:
            assert k.gemm_nt_plan(rec.M, rec.N, rec.K, epi) == rec.plan, (name, epi)
    # the conditions gemm_paths.py states for every record
    assert rec.M % rec.tile_m != 0 and rec.N % rec.tile_n != 0 and rec.N % 8 == 0
    assert max(rec.M * rec.K * 2, rec.N * rec.K * 2, rec.M * rec.N * 4) < 10e6          # every operand under ~10 MB
    if rec.phased:
        assert rec.K % 64 == 0 and rec.K >= 192
        assert rec.tiles > rec.grid and rec.tiles % rec.grid != 0 and rec.grid == rec.cus
        if name in GP.SHORT_WALK:
            assert rec.passes == GP.SHORT_WALK[name] < GP.MIN_PASSES
        else:
            assert rec.passes >= GP.MIN_PASSES, (name, rec.passes)
    else:
        assert rec.K < 192 and (rec.K == 128 or rec.K % 64 != 0)
        assert rec.grid == rec.tiles
    if rec.q8 and rec.tile_n == 128:
        assert rec.N % 128 == 64                    # the last 128-column tile holds one 64-column block of the byte stream


def test_cfg128_takes_no_longer_walk_on_the_phased_kernel(k):
    """What gemm_paths.SHORT_WALK claims: over M <= 4096 and the table's widths no shape planned for 8, 16 or 24 CUs runs the
    128-row tile on the persistent kernel over more than 1.875 tiles per CU with an unequal walk."""
    best = 0.0
    for cus in (8, 16, 24):
        with planned_for(k, cus):
            for N in (264, 520, 576):
                for M in range(129, 4097, 8):
                    p = k.gemm_nt_plan(M, N, 192)
                    if p["tile_m"] == 128 and p["tiles"] > p["grid"] and p["tiles"] % p["grid"]:
                        best = max(best, p["tiles"] / cus)
    assert best == 1.875


def test_nt_table_covers_every_tile_on_both_kernels():
    for tile in GP.NT_TILES:
        for phased in (False, True):
            recs = [r for r in GP.NT_TABLE if (r.tile_m, r.tile_n) == tile and r.phased == phased]
            assert any(r.q8 for r in recs) and any(not r.q8 for r in recs), (tile, phased)
            ks = {r.K for r in recs}
            if phased:
                assert 192 in ks and any(x > 192 for x in ks), (tile, ks)
            else:
                assert 128 in ks and ks & {72, 136}, (tile, ks)
    assert {(r.tile_m, r.tile_n) for r in GP.NT_TABLE} == set(GP.NT_TILES)
    assert len({r.name for r in GP.NT_TABLE}) == len(GP.NT_TABLE)


@pytest.mark.parametrize("name", [r.name for r in GP.TN_TABLE])
def test_tn_record_gets_its_plan(k, name):
    rec = GP.tn(name)
    with planned_for(k, rec.cus):
        assert k.gemm_tn_plan(rec.M, rec.N, rec.T, rec.a_group > 0, rec.beta, rec.dbias) == rec.plan
        from noise_robust_vit_amd import _lib
        assert _lib.load().nrv_gemm_tn_workspace(rec.M, rec.N, rec.T) == rec.splits * rec.M * (rec.N + 1) * 4
    assert rec.T % 64 != 0 and rec.kt_q * rec.splits + rec.kt_r == -(-rec.T // 64)


def test_tn_table_covers_every_branch():
    for what, has in GP.TN_BRANCHES.items():
        assert any(has(r) for r in GP.TN_TABLE), what
    direct = GP.tn("phased_direct")
    assert direct.tiles >= 5 and direct.T >= 3 * 64


def test_grouped_records_are_taken_and_refused(k):
    taken, refused = GP.TNG_TABLE
    for rec in GP.TNG_TABLE:
        assert sum(-(-M // 256) * -(-N // 256) for M, N, _ in rec.problems) == rec.tiles
        with planned_for(k, rec.cus):
            assert grouped_slots(rec) == rec.slots, rec.name
    # one cohort (F <= 8 // 6) of one workgroup per tile, so further slots are the remainder workgroups' (Wr > 0)
    assert taken.tiles <= taken.cus < 2 * taken.tiles and taken.slots > taken.tiles
    assert -(-taken.tiles * -(-taken.T // 64) // taken.cus) >= 8                        # Lc >= 8
    assert refused.slots == 0 and refused.tiles > refused.cus


@pytest.mark.parametrize("key", sorted(GP.WORKLOAD_NT))
def test_workload_plans_are_the_recorded_ones(k, key):
    reserved, M, N, K, epi, remap = key
    with planned_for(k, CUS - reserved):
        p = k.gemm_nt_plan(M, N, K, epi, remap)
    assert (p["tile_m"], p["tile_n"], p["phased"], p["tiles"], p["grid"]) == GP.WORKLOAD_NT[key]


def test_workload_weight_gradient_keeps_seven_splits(k):
    from noise_robust_vit_amd import _lib
    assert _lib.load().nrv_gemm_tn_workspace(3072, 768, 50432) == 7 * 3072 * 768 * 4 + 7 * 3072 * 4
    assert k.gemm_tn_plan(3072, 768, 50432) == {"tiles": 36, "splits": 7, "kt_q": 112, "kt_r": 4, "phased": True,
                                                "direct": False, "reduce": True}


def test_queries_refuse_what_the_launches_refuse(k):
    from noise_robust_vit_amd import _lib
    lib = _lib.load()
    pl = _lib.NtPlan()
    at = ctypes.addressof(pl)
    assert lib.nrv_gemm_nt_plan(8, 8, 8, 0, 0, None) == -1
    assert lib.nrv_gemm_nt_plan(8, 12, 8, 0, 0, at) == -2                # N % 8
    assert lib.nrv_gemm_nt_plan(8, 8, 8, 7, 0, at) == -6                 # unknown epilogue
    assert lib.nrv_gemm_nt_plan(8, 8, 8, _lib.EPI_BIAS, 1, at) == -6     # the remap rides on the residual epilogue
    assert lib.nrv_gemm_nt_plan(8, 72, 8, _lib.EPI_DGELU_Q8, 0, at) == -2
    tp = _lib.TnPlan()
    assert lib.nrv_gemm_tn_plan(8, 8, 8, 0, ctypes.c_float(0.5), 0, ctypes.addressof(tp)) == -2
    assert lib.nrv_gemm_tn_plan(8, 8, 8, 0, ctypes.c_float(0.0), 0, None) == -1
    assert lib.nrv_set_reserved_cus(0) == 0                              # and nothing above left a reservation behind


def test_walk_positions_of_the_report():
    """gemm_paths.tile_of: the launch order goes through xcd_remap, so a tile's walk position is not id // grid."""
    rec = GP.nt("192x256_phased_n520_k192")
    ids = sorted(GP.xcd_remap(t, rec.tiles) for t in range(rec.tiles))
    assert ids == list(range(rec.tiles))
    assert GP.tile_of(rec, 0, 0) == (0, 0, 0, 0)
    # 21 tiles over 8 XCDs: the first five take three ids each; position 8 (second walk of workgroup 0) is tile id 1
    assert GP.xcd_remap(8, 21) == 1 and GP.tile_of(rec, 0, 256) == (0, 1, 8, 1)
    assert GP.tile_of(rec, rec.M - 1, rec.N - 1)[:2] == (6, 2)
