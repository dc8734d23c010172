"""GPU: nrv_bgemm per element on every staging, K-loop and store path, over the case table of tests/bgemm_ref.py (the plans, the
coverage and the bound are pinned on the host by tests/test_bgemm_ref_host.py).  For every record and input kind: the plan the
record names is the one the dispatch gives for the real device addresses; two launches leave bit-identical C storages; every
addressed element is finite (operand storages are NaN outside their addressed sets, so a stray read poisons a result) and
within the derived bound of the fp64 reference (`random`) or equal to the selected value of the other operand (`select_*`);
every element of C's storage that the product does not address still holds the sentinel bit pattern."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bgemm_ref as R  # noqa: E402

from noise_robust_vit_amd import kernels as K  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", [c.name for c in R.TABLE])
def test_bgemm_record(dev, name, kind):
    inp = R.inputs(name, kind)
    case = inp.case
    a, b = inp.a.to(dev), inp.b.to(dev)
    fresh = R.sentinel_storage(case)
    runs = []
    for _ in range(2):
        c = fresh.to(dev)
        ops = ((a, case.a.off), case.a.strides, (b, case.b.off), case.b.strides, (c, case.c.off), case.c.strides)
        pl = K.bgemm_plan(*ops, case.G1, case.G2, case.M, case.N, case.K)
        assert (pl["a_vec"], pl["b_vec"], pl["c_vec"], pl["tiles_m"], pl["tiles_n"]) == case.plan, (name, pl)
        K.bgemm(*ops, case.G1, case.G2, case.M, case.N, case.K, inp.alpha)
        runs.append(c)
    torch.cuda.synchronize()
    assert torch.equal(R.bits(runs[0]), R.bits(runs[1])), "two launches differ"
    store = runs[0].cpu()
    got = store[inp.ic]
    assert not bool(torch.isnan(got).any()), "a NaN from outside an operand's addressed set (or an unwritten element)"
    assert bool((R.unwritten(case, store, inp.ic) == R.sentinel_bits(case)).all()), "an element outside C[0:M, 0:N] was written"
    if kind == "random":
        r = R.ratio(got, inp.ref, inp.bound)
        print("bgemm", name, kind, "error / bound", r)
        assert r <= 1.0
    else:
        assert torch.equal(got, inp.exact)
