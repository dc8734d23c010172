"""MI355X: the strided forms the wrappers accept are real.  tests/launch_audit.py classifies, on the CPU and against a stand-in
library, what each wrapper does with a tensor argument given as a column block of a wider buffer: refused, copied, or launched
with its row stride.  For the last two this file runs the wrapper once at the case's tiny shape, with the values in columns
[8, 8 + cols) of a NaN-filled buffer 16 columns wider, and asks for the bits of the call on contiguous tensors; around an output
the NaN must still be there.  The view stays inside its own allocation whichever row stride a kernel uses (the last row ends at
8 + (rows - 1)(cols + 16) + cols <= rows (cols + 16)).  No other mutation of launch_audit.py is ever run here: those are refused
or not, and that is the CPU test's business."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import launch_audit as LA  # noqa: E402
from noise_robust_vit_amd import _lib  # noqa: E402
from noise_robust_vit_amd._lib import NrvError  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().contiguous().view(torch.uint8).cpu()


def _filler(t):
    return float("nan") if t.is_floating_point() else (True if t.dtype == torch.bool else torch.iinfo(t.dtype).max)


def _untouched(buf, cols):
    outside = torch.cat([buf[..., :LA.PAD], buf[..., LA.PAD + cols:]], -1)
    return bool(torch.isnan(outside).all()) if buf.is_floating_point() else bool((outside == _filler(buf)).all())


def _run(case, kwargs):
    """The call's results and the tensors it writes in place, as bytes."""
    result = case.function()(**kwargs)
    torch.cuda.synchronize()
    got = {"result." + ".".join(map(str, p[1:])): _bits(t) for p, t in LA.leaves({"result": result})}
    got.update({name: _bits(kwargs[name]) for name in case.outs if kwargs.get(name) is not None})
    return got


def _accepted(case):
    """The audit of this case, against the stand-in and on CPU tensors; the library is the real one again afterwards."""
    with pytest.MonkeyPatch.context() as mp:
        findings, classes = LA.audit(LA.install(mp), case)
    assert not isinstance(_lib.load(), LA.StandIn)
    assert findings == [], findings                       # a wrapper with a hole is not run on the device at all
    return [path for path, kind in classes.items() if kind in (LA.COPIED, LA.PASSED_ON)], classes


@pytest.mark.parametrize("case", LA.CASES, ids=LA.case_ids())
def test_a_column_block_gives_the_bits_of_the_contiguous_call(case):
    paths, classes = _accepted(case)
    if not paths:
        assert all(kind == LA.REFUSED for kind in classes.values())
        return
    torch.manual_seed(0)
    want = _run(case, case.make("cuda"))
    for path in paths:
        torch.manual_seed(0)
        kwargs = case.make("cuda")
        t = dict(LA.leaves(kwargs))[path]
        view, buf = LA.column_block(t, _filler(t))
        assert view.data_ptr() != buf.data_ptr() and not view.is_contiguous() and torch.equal(view, t)
        try:
            got = _run(case, LA.replaced(kwargs, path, view))
        except NrvError as e:                                 # e.g. the C side's alignment rule
            print(f"{case.name}({path}): {classes[path]} on the host, refused on the device: {e}")
            continue
        assert _untouched(buf, t.shape[-1]), (case.name, path, "wrote outside the view" if path[0] in case.outs else "input changed")
        assert got.keys() == want.keys()
        for k in want:
            assert torch.equal(got[k], want[k]), (case.name, path, classes[path], k)
