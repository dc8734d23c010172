"""CPU: the side-job plan query (`nrv_gemm_nt_side_plan`) answers the hand-computed records of tests/side_reduce_cases.py, and the
records are what they claim to be.  No launch: the library plans for 256 CUs without a device."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import side_reduce_cases as SC  # noqa: E402

CUS = 256            # what the library plans for without a device (csrc/nrv_gemm.hip physical_cus)


@pytest.fixture(scope="module")
def k():
    from noise_robust_vit_amd import kernels
    return kernels


class planned:
    def __init__(self, k, cus):
        self.k, self.cus = k, cus

    def __enter__(self):
        prev = self.k.set_reserved_cus(CUS - self.cus)
        if prev != 0:
            self.k.set_reserved_cus(0)
            raise AssertionError(f"reservation was {prev}, not 0")

    def __exit__(self, *exc):
        self.k.set_reserved_cus(0)


@pytest.mark.parametrize("rec", SC.PAIRS, ids=lambda r: r.name)
def test_pair_records_are_what_they_claim(k, rec):
    M, N, Kk, epi = rec.nt
    Mw, Nw, T, beta = rec.tn
    with planned(k, rec.cus):
        nt = k.gemm_nt_plan(M, N, Kk, epi)
        tn = k.gemm_tn_plan(Mw, Nw, T, beta=beta, dbias=rec.dbias is not None)
        sp = k.gemm_nt_side_plan(M, N, Kk, epi, False, rec.job_bytes)
    assert nt["phased"] and (nt["tile_m"], nt["tile_n"], nt["tiles"], nt["grid"]) == rec.nt_plan
    assert (tn["splits"], tn["kt_r"], tn["direct"]) == (rec.splits, rec.kt_r, rec.direct)
    assert tn["reduce"] == rec.pending
    # the record's own arithmetic, then the library's answer
    tiles, grid = rec.nt_plan[2], rec.nt_plan[3]
    assert tiles > grid and rec.late == grid - tiles % grid and 0 < rec.late < grid
    assert rec.share == -(-rec.job_bytes // rec.late)
    assert rec.admitted == (rec.share <= SC.BYTES_PER_KSTEP * (Kk // 64) * rec.nt_plan[0] // 256)
    assert sp == {"late": rec.late, "share_bytes": rec.share, "admitted": rec.admitted}


def test_records_cover_the_edges():
    P = SC.PAIRS
    assert any(r.late == 1 for r in P) and any(r.late == r.nt_plan[3] - 1 for r in P)
    assert {1, 2, 5, 8} <= {r.splits for r in P if not r.direct} and any(r.splits >= 17 for r in P)
    assert any(r.splits == 1 and r.tn[3] == 1.0 and not r.direct for r in P)
    assert any(r.kt_r != 0 for r in P)
    chunks = lambda r: r.tn[0] * r.tn[1] // 4
    per = lambda r: -(-chunks(r) // r.late)
    assert any(chunks(r) % 64 != 0 for r in P)
    assert any(not r.direct and chunks(r) % r.late != 0 and (r.late - 1) * per(r) < chunks(r) for r in P)      # a short last share
    assert any(not r.direct and (r.late - 1) * per(r) >= chunks(r) for r in P)                                  # an empty one
    assert any(r.dbias is not None and (r.late - 1) * -(-r.tn[0] // r.late) >= r.tn[0] for r in P)              # ... of bias rows
    assert {0.0, 1.0} <= {r.tn[3] for r in P if r.ldc_pad > 0}
    assert {None, 0.0, 1.0} <= {r.dbias for r in P}
    assert any(r.direct and r.dbias is not None for r in P) and any(not r.pending for r in P)
    assert {(256, 0), (320, 0), (384, 0), (256, 6)} <= {(r.nt_plan[0], r.nt[3]) for r in P}
    assert any(not r.admitted for r in P)


@pytest.mark.parametrize("cus,M,N,Kk,epi,remap,why", SC.NO_LATE, ids=[c[-1] for c in SC.NO_LATE])
def test_launches_without_late_workgroups(k, cus, M, N, Kk, epi, remap, why):
    with planned(k, cus):
        nt = k.gemm_nt_plan(M, N, Kk, epi, remap)
        sp = k.gemm_nt_side_plan(M, N, Kk, epi, remap, 4096)
    if why.startswith("plain") or why.startswith("row remap"):
        assert not nt["phased"]
    elif why.startswith("tiles <="):
        assert nt["phased"] and nt["tiles"] <= nt["grid"]
    else:
        assert nt["phased"] and nt["tiles"] > nt["grid"] and nt["tiles"] % nt["grid"] == 0
    assert sp == {"late": 0, "share_bytes": 0, "admitted": False}


def test_workload_pairs(k):
    """ViT-B/16 at batch 256: the late workgroups and shares of the four backward pairs at the device's own CU count."""
    want = {  # NT (M, N, K, epilogue), weight gradient (M, N) -> late, splits
        "dW2 -> dU": ((50432, 3072, 768, 6), (768, 3072), 196, 7),
        "dW1 -> dXn2": ((50432, 768, 3072, 0), (3072, 768), 38, 7),
        "dWo -> dO": ((50432, 768, 768, 0), (768, 768), 38, 28),
        "dWqkv -> dXn": ((50432, 768, 2304, 0), (2304, 768), 38, 9),
    }
    for name, (nt, (Mw, Nw), late, splits) in want.items():
        tn = k.gemm_tn_plan(Mw, Nw, 50432, dbias=True)
        assert tn["splits"] == splits, name
        job = splits * Mw * Nw * 4
        sp = k.gemm_nt_side_plan(*nt, False, job)
        assert sp["late"] == late and sp["share_bytes"] == -(-job // late), name
        tile_m = k.gemm_nt_plan(*nt)["tile_m"]
        assert sp["admitted"] == (sp["share_bytes"] <= SC.BYTES_PER_KSTEP * (nt[2] // 64) * tile_m // 256), name


def test_side_plan_argument_errors(k):
    from noise_robust_vit_amd import _lib
    lib = _lib.load()
    pl = _lib.NtSidePlan()
    assert lib.nrv_gemm_nt_side_plan(1601, 520, 192, 0, 0, 0, None) != 0
    assert lib.nrv_gemm_nt_side_plan(1601, 520, 192, 0, 0, -1, ctypes.addressof(pl)) != 0
    assert lib.nrv_gemm_nt_side_plan(1601, 520, 192, 0, 1, 0, ctypes.addressof(pl)) != 0      # remap without its epilogue
    job = _lib.ReduceJob()
    fused = ctypes.c_int(7)
    assert lib.nrv_splitk_reduce(None, None) != 0
    assert lib.nrv_splitk_reduce(ctypes.addressof(job), None) == 0                             # nothing pending: no launch
    # a NULL job or a NULL `fused` is refused before any launch
    assert lib.nrv_gemm_nt_bf16_side(None, 8, None, 8, None, 1, 8, 8, 8, 8, 0, None, None, 0, 0, 0, None, 0, 0, 0, 0,
                                     None, ctypes.addressof(fused), None) != 0
    assert lib.nrv_gemm_nt_bf16_side(None, 8, None, 8, None, 1, 8, 8, 8, 8, 0, None, None, 0, 0, 0, None, 0, 0, 0, 0,
                                     ctypes.addressof(job), None, None) != 0
