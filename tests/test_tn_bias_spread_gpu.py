"""The bias gradient of the TN (weight-gradient) GEMM, per column: the phased kernel deals the 16 blocks of 16 A-columns of a row
tile out over the row tile's column tiles (block b -> column tile b % tiles_n) and, inside a workgroup, over the waves of a
wave row; the split's bias row is then written by several workgroups in disjoint 16-float ranges.

Shapes M x N x T: tiles_n = 1, 2, 3, 5 and 6, partial last row tiles (M % 256 != 0), partial column tiles and partial last
K-steps (T % 64 != 0).  The planned-CU control (`K.set_reserved_cus`, as tests/test_gemm_paths_gpu.py) picks the split count;
the plan query says which kernel runs.  With at least 8 planned CUs the two smallest shapes only reach the plain kernel (fewer
than three K-steps per split), which keeps its first-column-tile bias; shapes of the same tiles_n with more rows are added so
that the phased kernel runs tiles_n = 1 and 2 as well, at one split and at three or more.

Reference: column sums of the bf16 operand in fp64.  Bound per column c: 1e-5 sqrt(T) sum_t |A[t, c]| -- the factor of
test_gemm_tn's check; an fp32 chain of T exact bf16 terms is off by at most (T - 1) 2^-24 sum|a| = 6e-8 T sum|a|, below the
bound for every T < 27 000.  The operand is positive, so a column that misses a block (or counts one twice) is off by its
whole sum; the bias slots are also pre-set to NaN, which a block nobody wrote would hand to the reduce.
"""
import math

import pytest
import torch

from noise_robust_vit_amd import _lib
from noise_robust_vit_amd import kernels as K

pytestmark = pytest.mark.gpu

GUARD = 64                       # sentinel floats on either side of the workspace and of db
SENT = 12345.0

# (M, N, T, planned CUs, splits expected, phased expected)
CASES = [
    (40, 24, 200, 8, 4, False),              # tiles_n 1; one split is out of reach of the control (8 CUs / 1 tile, 4 K-steps)
    (256, 512, 448, 8, 4, False),            # tiles_n 2
    (256, 512, 448, 256, 7, False),
    (304, 768, 704, 8, 1, True),             # tiles_n 3, last row tile of 48 rows (300 rows: the C ABI takes M % 8 == 0 only)
    (304, 768, 704, 18, 3, True),
    (528, 1288, 1000, 18, 1, True),          # tiles_n 6, last column tile of 8 columns, T % 64 = 40
    (528, 1288, 1000, 54, 3, True),
    (528, 1272, 1000, 15, 1, True),          # tiles_n 5
    (528, 1272, 1000, 60, 4, True),
    (1288, 200, 832, 8, 1, True),            # tiles_n 1 in the phased kernel: all 16 blocks in one workgroup
    (1288, 200, 832, 24, 4, True),
    (520, 264, 832, 8, 1, True),             # tiles_n 2 in the phased kernel
    (520, 264, 832, 24, 4, True),
]


@pytest.fixture(scope="module")
def operands(dev):
    """A (positive, bf16) and B per (M, N, T), with the fp64 column sums of A and of |A|: computed once."""
    cache = {}

    def get(M, N, T):
        if (M, N, T) not in cache:
            g = torch.Generator(device="cpu").manual_seed(1000 * M + N + T)
            A = (torch.rand(T, M, generator=g) + 0.25).to(torch.bfloat16).to(dev)
            B = torch.randn(T, N, generator=g).to(torch.bfloat16).to(dev)
            cache[(M, N, T)] = (A, B, A.double().sum(0), A.double().abs().sum(0))
        return cache[(M, N, T)]
    return get


def launch(A, B, C, db, db_beta, plan, dev):
    """nrv_gemm_tn_bf16 with a workspace of this test: guard | slabs and bias slots (NaN) | guard.  Returns the workspace."""
    T, M = A.shape
    N = B.shape[1]
    lib = _lib.load()
    size = lib.nrv_gemm_tn_workspace(M, N, T)
    slab = 0 if plan["direct"] else plan["splits"] * M * N * 4
    need = slab + plan["splits"] * M * 4
    assert need <= size and size % 4 == 0
    ws = torch.full((2 * GUARD + size // 4,), SENT, dtype=torch.float32, device=dev)
    ws[GUARD + slab // 4: GUARD + need // 4] = float("nan")
    rc = lib.nrv_gemm_tn_bf16(A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), C.data_ptr(), C.stride(0), M, N, T, 0.0,
                              0, 0, 0, db.data_ptr(), float(db_beta), ws.data_ptr() + GUARD * 4, size,
                              K._stream())
    assert rc == 0, rc
    return ws, need // 4


@pytest.mark.parametrize("db_beta", [0.0, 1.0])
@pytest.mark.parametrize("M,N,T,planned,splits,phased", CASES)
def test_tn_bias_per_column(dev, operands, M, N, T, planned, splits, phased, db_beta):
    A, B, colsum, abssum = operands(M, N, T)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert cus >= planned
    prev = K.set_reserved_cus(cus - planned)
    try:
        assert prev == 0
        plan = K.gemm_tn_plan(M, N, T, dbias=True)
        assert plan["splits"] == splits and plan["phased"] == phased, plan
        g = torch.Generator(device="cpu").manual_seed(7)
        db0 = torch.randn(M, generator=g).to(dev)
        runs = []
        for _ in range(2):
            C = torch.empty(M, N, dtype=torch.float32, device=dev)
            dbuf = torch.full((M + 2 * GUARD,), SENT, dtype=torch.float32, device=dev)
            db = dbuf[GUARD:GUARD + M]
            db.copy_(db0)
            ws, used = launch(A, B, C, db, db_beta, plan, dev)
            runs.append((C, dbuf, ws, used))
    finally:
        K.set_reserved_cus(0)
    C, dbuf, ws, used = runs[0]
    db = dbuf[GUARD:GUARD + M]
    # sentinels around db, around the workspace, and in the part of the workspace the plan does not use
    assert torch.all(dbuf[:GUARD] == SENT) and torch.all(dbuf[GUARD + M:] == SENT)
    assert torch.all(ws[:GUARD] == SENT) and torch.all(ws[GUARD + used:] == SENT)
    # every bias slot was written, by somebody
    slots = ws[GUARD + used - plan["splits"] * M: GUARD + used]
    assert not torch.isnan(slots).any()
    # per column against fp64
    got = db.double() - (db0.double() if db_beta else 0.0)
    bound = 1e-5 * math.sqrt(T) * abssum + (2.0 ** -23) * (db0.double().abs() + colsum.abs()) * (1 if db_beta else 0)
    err = (got - colsum).abs()
    worst = int(torch.argmax(err / bound))
    print(f"worst column {worst} (block {worst % 256 // 16}): err {err[worst].item():.3e}, bound {bound[worst].item():.3e}")
    assert torch.all(err <= bound), (worst, err[worst].item(), bound[worst].item())
    rel = ((got - colsum).abs().max() / colsum.abs().max()).item()
    assert rel < 1e-5 * math.sqrt(T) + (2.0 ** -22 if db_beta else 0.0), rel
    # the same bits again, and the weight gradient itself
    assert torch.equal(C, runs[1][0]) and torch.equal(dbuf, runs[1][1])
    ref = A.float().t() @ B.float()
    assert ((C - ref).abs().max() / ref.abs().max()).item() < 2e-5 * math.sqrt(T)


@pytest.mark.parametrize("M,N,T,planned", [(304, 768, 1000, 24), (528, 1272, 1000, 60), (520, 264, 832, 24)])
def test_tn_bias_does_not_depend_on_the_column_tiles(dev, operands, M, N, T, planned):
    """One accumulator chain per column over the K-steps of a split, whoever runs it: the bias gradient of the same A with a
    one-tile-wide B (all 16 blocks in one workgroup) has the same bits, and so has K.gemm_tn's accumulation (beta 1)."""
    A, B, _, _ = operands(M, N, T)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    tiles_m = (M + 255) // 256
    prev = K.set_reserved_cus(cus - planned)
    try:
        assert prev == 0
        plan = K.gemm_tn_plan(M, N, T, dbias=True)
        _, db = K.gemm_tn(A, B, want_dbias=True)
        _, db2 = K.gemm_tn(A, B, dbias=db.clone(), dbias_beta=1.0)
    finally:
        K.set_reserved_cus(0)
    # same split count with one column tile: planned CUs = splits * tiles_m (>= 8 by the choice of cases)
    narrow = plan["splits"] * tiles_m
    assert narrow >= 8
    prev = K.set_reserved_cus(cus - narrow)
    try:
        plan1 = K.gemm_tn_plan(M, 64, T, dbias=True)
        assert (plan1["splits"], plan1["kt_q"], plan1["kt_r"], plan1["phased"]) == (plan["splits"], plan["kt_q"], plan["kt_r"], True)
        _, db1 = K.gemm_tn(A, B[:, :64].contiguous(), want_dbias=True)
    finally:
        K.set_reserved_cus(0)
    assert torch.equal(db, db1)
    assert torch.equal(db2, db + db)
