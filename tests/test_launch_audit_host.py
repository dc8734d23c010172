"""CPU: tests/launch_audit.py over every wrapper of noise_robust_vit_amd/kernels.py.  No tensor that is too short, of another
dtype, strided otherwise or on the host reaches a launch unnoticed, and no scalar dimension larger than the tensors does.  The
library is a stand-in that records the calls; nothing here touches a device."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import launch_audit as LA  # noqa: E402
from noise_robust_vit_amd import _lib  # noqa: E402
from noise_robust_vit_amd import kernels as K  # noqa: E402
from noise_robust_vit_amd._lib import NrvError  # noqa: E402

ALLOWED_EXEMPT = {"probe", "bgemm", "bgemm_plan", "build_cast_jobs", "run_cast_jobs", "cast_transpose_batched", "gemm_tn_grouped",
                  "flush_reduce"}


def test_every_wrapper_has_a_case_or_a_written_exemption():
    found = LA.wrappers()
    assert len(found) >= 80, found                    # the scan itself: kernels.py has about 85 of them
    cased = {c.name for c in LA.CASES}
    missing = [n for n in found if n not in cased and n not in LA.EXEMPT]
    assert missing == [], missing
    assert set(LA.EXEMPT) <= ALLOWED_EXEMPT and all(len(r) > 20 for r in LA.EXEMPT.values())
    assert not set(LA.EXEMPT) & cased
    for n in ("mask_pack", "bias_index", "adamw_flat", "sumsq", "rotary_fwd", "rotary_bwd"):
        assert n in cased, n
    for c in LA.CASES:                                # a case names arguments its wrapper has
        kw = c.make("cpu")
        assert set(c.outs) <= set(kw) and set(c.dims) <= set(kw), c.name


def test_the_stand_in_launches_nothing_and_forwards_the_host_entries(monkeypatch):
    lib = LA.install(monkeypatch)
    assert lib.nrv_abi_version() == _lib.ABI_VERSION and lib.nrv_layernorm_bwd_workspace(3, 64) > 0
    assert K.sumsq_workspace(64) > 0 and lib.calls == []
    assert lib.nrv_cast_f32_bf16(1, 2, 3, 4) == 0 and lib.calls == [("nrv_cast_f32_bf16", (1, 2, 3, 4))]
    with pytest.raises(AttributeError):
        lib.nrv_no_such_entry
    launching = [n for n in _lib.SIGNATURES if not LA.needs_no_device(n)]
    assert "nrv_probe" in launching and all(_lib.SIGNATURES[n][1][-1] is _lib.c_void_p for n in launching)


@pytest.mark.parametrize("case", LA.CASES, ids=LA.case_ids())
def test_no_changed_tensor_reaches_the_same_launch(case, monkeypatch):
    lib = LA.install(monkeypatch)
    findings, classes = LA.audit(lib, case)
    assert findings == [], "\n" + "\n".join(findings)
    # every tensor of two or more dimensions got its column-block form classified (test_launch_audit_gpu.py runs the accepted ones)
    torch.manual_seed(0)
    wide = {p for p, t in LA.leaves(case.make("cpu")) if t.dim() >= 2}
    assert set(classes) == wide and set(classes.values()) <= {LA.REFUSED, LA.COPIED, LA.PASSED_ON}


# ---- the auditor must be able to fail: two wrappers that are wrong on purpose ---------------------------------------
def _toy_ignores_out(x, out, n):
    """Checks x, never looks at out's size, dtype or device, and believes the caller's n."""
    K._f32(x, "x")
    if not x.is_contiguous():
        raise NrvError("toy: the input must be contiguous")
    _lib.check(_lib.load().nrv_cast_f32_bf16(x.data_ptr(), out.data_ptr(), n, K._stream()), "toy")
    return out


def _toy_passes_strided_pointer(x):
    """Checks dtype, device and size, and launches a strided tensor's own pointer with the contiguous dimensions."""
    K._f32(x, "x")
    if x.dim() != 2:
        raise NrvError("toy: x must be 2-D")
    out = torch.empty(x.shape, dtype=torch.bfloat16)
    _lib.check(_lib.load().nrv_cast_f32_bf16(x.data_ptr(), out.data_ptr(), x.numel(), K._stream()), "toy")
    return out


def test_the_auditor_fires_on_two_broken_wrappers(monkeypatch):
    lib = LA.install(monkeypatch)
    a = LA.Case("toy_out", lambda dev: dict(x=torch.zeros(8, 8), out=torch.zeros(8, 8, dtype=torch.bfloat16), n=64), outs=("out",),
                dims=("n",), fn=_toy_ignores_out)
    found, _ = LA.audit(lib, a)
    for rule in ("toy_out(out) shorter: the same launch", "toy_out(out) dtype float32: reaches the launch",
                 "toy_out(out) strides column block: its own pointer", "toy_out(out) strides transposed: its own pointer",
                 "toy_out(out) strides stride 0: its own pointer", "toy_out(out) host: a host tensor reaches",
                 "toy_out[n x 2]: launches with a dimension", "toy_out(x) strides transposed: the refusal does not name"):
        assert any(f.startswith(rule) for f in found), (rule, found)
    assert not any(f.startswith("toy_out(x) dtype") or f.startswith("toy_out(x) host") for f in found), found   # what it does check

    b = LA.Case("toy_ptr", lambda dev: dict(x=torch.zeros(8, 8)), fn=_toy_passes_strided_pointer)
    found, classes = LA.audit(lib, b)
    assert sorted(f.split(":")[0] for f in found) == ["toy_ptr(x) strides column block", "toy_ptr(x) strides stride 0",
                                                      "toy_ptr(x) strides transposed"], found

    # an exception that is not the wrapper's own refusal is a finding too
    c = LA.Case("toy_crash", lambda dev: dict(x=torch.zeros(8, 8)), fn=lambda x: x.reshape(8, 8).view(64))
    found, _ = LA.audit(lib, c)
    assert any("RuntimeError instead of the wrapper's own refusal" in f for f in found), found


def test_a_silently_copied_output_is_a_finding(monkeypatch):
    lib = LA.install(monkeypatch)

    def copies_out(x, out):
        K._f32(x, "x"); K._bf16(out, "out")
        if not x.is_contiguous() or out.shape != x.shape:
            raise NrvError("toy: x contiguous, out of x's shape")
        o = out.contiguous()
        _lib.check(_lib.load().nrv_cast_f32_bf16(x.data_ptr(), o.data_ptr(), x.numel(), K._stream()), "toy")
    c = LA.Case("toy_copy", lambda dev: dict(x=torch.zeros(8, 8), out=torch.zeros(8, 8, dtype=torch.bfloat16)), outs=("out",), fn=copies_out)
    found, classes = LA.audit(lib, c)
    assert sorted(f.split(":")[0] for f in found) == ["toy_copy(out) strides column block", "toy_copy(out) strides stride 0",
                                                      "toy_copy(out) strides transposed"], found
    assert classes[("out",)] == LA.COPIED
