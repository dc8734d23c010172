"""What the model ports' tests (test_X_gpu.py, test_X_host.py) share: the parity judge, the steps every GPU file repeats and the
host checklist.

The parity bound is the project's definition of "the port is right": the HIP result's rel-L2 to the fp32 restatement may be at
most twice the rel-L2 of the same restatement in low precision (bf16 autocast on the GPU, or bf16-rounded operands on the CPU)
plus 1e-2, per logits tensor and per parameter gradient.  `judge` holds it, touches no device and is tested on the CPU by
test_port_checks_host.py; `compare` runs the HIP step and the two restatements and hands the three results to it.
"""
import ctypes
import os
import re

import torch

from port_fixture import grad_sample, unpack, unpack_grads, unpack_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VANISHED = 1e-4


def rel(a, b):
    a, b = a.detach().float().cpu().reshape(-1), b.detach().float().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---- the judge ------------------------------------------------------------------------------------
def small_in_restatement(k, r):
    """The default vanishing rule: the fp32 restatement's gradient is below VANISHED everywhere."""
    return float(r.abs().max()) < VANISHED


def dropped_layers(prefixes):
    """A `skip` rule: a parameter under one of `prefixes` took no part in the step, its gradient is None or exactly zero."""
    def rule(k, g, r):
        if not k.startswith(tuple(prefixes)):
            return False
        assert g is None or float(g.abs().max()) == 0.0, k
        return True
    return rule


def frozen(suffix):
    """A `skip` rule: a parameter the restatement has no gradient for is called `suffix` and has none on the HIP side either."""
    def rule(k, g, r):
        if r is not None:
            return False
        assert g is None and k.endswith(suffix), k
        return True
    return rule


def judge(hip, r32, r16, vanishes=small_in_restatement, expect_vanished=None, skip=None, fixture_logits=None, fixture_grads=None):
    """`hip`, `r32`, `r16`: (logits, loss, grads) of the HIP model, the fp32 and the low-precision restatement; `hip`'s grads are
    None for an eval-mode step.  Logits and every gradient are held to 2 rel(r16, r32) + 1e-2 against r32, the loss to 2e-2
    (relative above 1), and both sides name the same parameters.

    vanishes(k, r32 gradient): where true, both gradients must stay below VANISHED instead (a relative error of rounding noise
        says nothing); None bounds every gradient.  expect_vanished: the exact set of keys that must have done so.
    skip(k, hip gradient, r32 gradient): true for a key that is left out, after asserting whatever holds for it instead.
    fixture_logits: the reference's logits, held to the logits bound.  fixture_grads: the reference's sampled gradients
        (port_fixture.grad_sample), each held to its parameter's bound + 1e-3 (the float16 storage)."""
    logits, loss, grads = hip
    l32, s32, g32 = r32
    l16, _, g16 = r16
    loss, s32 = float(loss), float(s32)
    bound = 2 * rel(l16, l32) + 1e-2
    r = rel(logits, l32)
    print(f"logits rel {r:.3e} bound {bound:.3e}; loss {loss:.5f} vs {s32:.5f}")
    assert r <= bound, ("logits", r, bound)
    assert abs(loss - s32) <= 2e-2 * max(1.0, abs(s32)), ("loss", loss, s32)
    if fixture_logits is not None:
        assert rel(logits, fixture_logits) <= bound, ("fixture logits", rel(logits, fixture_logits), bound)
    if grads is None:
        return
    assert set(grads) == set(g32), sorted(set(grads) ^ set(g32))
    vanished = set()
    for k, g in grads.items():
        if skip is not None and skip(k, g, g32[k]):
            continue
        assert g is not None, k
        if vanishes is not None and vanishes(k, g32[k]):
            assert float(g.abs().max()) < VANISHED and float(g32[k].abs().max()) < VANISHED, k
            vanished.add(k)
            continue
        b = 2 * rel(g16[k], g32[k]) + 1e-2
        r = rel(g, g32[k])
        print(f"{k}: rel {r:.3e} bound {b:.3e}")
        assert r <= b, (k, r, b)
        if fixture_grads is not None:
            r = rel(grad_sample(k, g.cpu()), fixture_grads[k])
            assert r <= b + 1e-3, (k, "fixture", r, b + 1e-3)
    if expect_vanished is not None:
        assert vanished == set(expect_vanished), sorted(vanished ^ set(expect_vanished))


# ---- the steps every GPU file repeats ---------------------------------------------------------------
def hip_step(model, x, y, pre=None):
    """One forward, cross-entropy and (in training mode) backward: (logits, loss, {name: grad} or None).  `pre(model)` runs
    just before the forward (injected masks, seeds of a draw)."""
    model.zero_grad(set_to_none=True)
    if pre is not None:
        pre(model)
    logits = model(x)
    loss = torch.nn.functional.cross_entropy(logits, y)
    if not model.training:
        return logits.detach(), loss.detach(), None
    loss.backward()
    return logits.detach(), loss.detach(), {k: p.grad for k, p in model.named_parameters()}


def compare(model, x, y, restate, on_cpu=False, pre=None, **rules):
    """hip_step against `restate(model, x, y, low)` at low = False and True, judged with `rules` (judge's keywords).  on_cpu:
    the restatements get the model and the batch on the CPU, and the model goes back afterwards.  Returns the HIP result."""
    hip = hip_step(model, x, y, pre)
    dev = x.device
    if on_cpu:
        model.to("cpu")
        x, y = x.cpu(), y.cpu()
    r32 = restate(model, x, y, False)
    r16 = restate(model, x, y, True)
    if on_cpu:
        model.to(dev)
    judge(hip, r32, r16, **rules)
    return hip


def profiled_step(model, x, y):
    """A warm step, then one under kernels.LaunchProfile: its summary."""
    from noise_robust_vit_amd import kernels as K
    hip_step(model, x, y)
    with K.LaunchProfile() as prof:
        hip_step(model, x, y)
    return prof.summary()


def check_reruns_bit_identical(model, x, y):
    runs = []
    for _ in range(2):
        lg, _, g = hip_step(model, x, y)
        runs.append([lg] + [t.clone() for t in g.values() if t is not None])
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs))


def check_eager_vs_captured(make, x, y, steps=3, falls=20, same_params=True, cuda_seed=None):
    """Two models from `make()`, one Trainer captured and one eager: `steps` losses are bit-equal, then the parameters are, then
    the eager loss falls over `falls` more steps (0: not asked).  cuda_seed: set before the capture and before each series (a
    model that draws on the device).  Returns the eager Trainer."""
    from noise_robust_vit_amd.train import TrainConfig, Trainer
    a, b = make(), make()
    cfg = TrainConfig(lr=1e-3)
    ta, tb = Trainer(a, cfg), Trainer(b, cfg)

    def reseed():
        if cuda_seed is not None:
            torch.cuda.manual_seed(cuda_seed)
    reseed()
    ta.capture(x, y)
    reseed()
    la = [ta.step(x, y) for _ in range(steps)]
    reseed()
    lb = [tb.step(x, y) for _ in range(steps)]
    assert all(torch.equal(u, v) for u, v in zip(la, lb)), (la, lb)
    if same_params:
        for (n, p), q in zip(a.named_parameters(), b.parameters()):
            assert torch.equal(p, q), n
    if falls:
        losses = [lb[-1].item()] + [tb.step(x, y).item() for _ in range(falls)]
        assert losses[-1] < losses[0], losses
    return tb


def check_state_dict_round_trip(a, fresh, x):
    """A reference-shaped state_dict (the fixture's keys and shapes) loads strictly, gives the same logits after a save / load
    cycle into a model from `fresh()`, and the bf16 weight images follow the loaded values.  `a`: a loaded model in eval mode."""
    with torch.no_grad():
        la = a(x)
        sd = {k: v.detach().cpu().clone() for k, v in a.state_dict().items()}
        torch.manual_seed(7)
        b = fresh().to(x.device).eval()
        lb0 = b(x)
        b.load_state_dict(sd, strict=True)
        lb = b(x)
    assert not torch.equal(la, lb0) and torch.equal(la, lb)


# ---- the host checklist ---------------------------------------------------------------------------
class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on the device: the refusals under test come before any kernel."""

    @property
    def is_cuda(self):
        return True


def fake_cuda(t):
    return t.as_subclass(_FakeCuda)


def check_keys_and_sums(model, weights, fx, case, rtol=1e-6):
    """The state_dict's keys and shapes are the reference's, in order; the fixture weights load strictly (a reference-shaped
    dict) and sum to what the reference side saw."""
    tree = unpack_tree(fx, case)
    sd = model.state_dict()
    assert list(sd.keys()) == list(tree.keys())
    for k, (shape, _) in tree.items():
        assert tuple(sd[k].shape) == shape, k
    model.load_state_dict(weights, strict=True)
    for k, (_, s) in tree.items():
        assert abs(float(model.state_dict()[k].double().sum()) - s) <= rtol * max(1.0, abs(s)), k


def check_tree_and_keys(model, weights, fx, case):
    assert [n for n, _ in model.named_modules()] == [str(n) for n in fx[case + ".modules"]]
    check_keys_and_sums(model, weights, fx, case)


def check_seeded_init(model, fx, name, rtol=1e-9, atol=1e-6):
    """`model`, built under torch.manual_seed(0): the reference's keys, shapes, parameter count and per-tensor sums."""
    tree = unpack_tree(fx, name)
    sd = model.state_dict()
    assert list(sd.keys()) == list(tree.keys())
    assert sum(p.numel() for p in model.parameters()) == int(fx[name + ".nparams"])
    for k, (shape, s) in tree.items():
        assert tuple(sd[k].shape) == shape, k
        v = float(sd[k].double().sum())
        assert abs(v - s) <= rtol * max(1.0, abs(s)) + atol, (k, v, s)


def check_restatement(result, fx, case, training, loss_tol=2e-3, grad_tol=5e-3, noise=None):
    """`result`: the fp32 restatement's (logits, loss, grads) on the fixture's weights and inputs, against what the reference
    computed.  noise(k, reference gradient): true where both gradients are rounding noise and must stay below 1e-6."""
    logits, loss, grads = result
    ref = unpack(fx, case + ".logits")
    err = float((logits - ref).abs().max() / ref.abs().max())
    print(case, "logits max-abs err / max-abs", err)
    assert err <= 2e-3
    assert abs(loss.item() - float(fx[case + ".loss"])) <= loss_tol
    if training:
        rg = unpack_grads(fx, case)
        assert set(rg) == {k for k, g in grads.items() if g is not None}
        for k, g in rg.items():
            a = grad_sample(k, grads[k])
            if noise is not None and noise(k, g):
                assert float(a.abs().max()) < 1e-6 and float(g.abs().max()) < 1e-6, k
                continue
            assert rel(a, g) <= grad_tol, k


def check_prototypes(names, abi=None, source=None, wrappers=()):
    """Every name is declared in include/nrv.h (comments aside), bound in _lib.SIGNATURES and exported by the built library;
    header, binding and library agree on the ABI version (`abi`: and it is this one); `source` is among the built sources and
    kernels.py has each of `wrappers`.  Returns the raw ctypes handle."""
    from noise_robust_vit_amd import _lib, build
    from noise_robust_vit_amd import kernels as K
    text = open(os.path.join(ROOT, "include", "nrv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = ctypes.CDLL(build.build())
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(handle, name), name
    assert handle.nrv_abi_version() == _lib.ABI_VERSION
    assert abi is None or abi == _lib.ABI_VERSION
    assert re.search(r"#define\s+NRV_ABI_VERSION\s+%d\b" % _lib.ABI_VERSION, text)
    if source is not None:
        assert source in build.SOURCES
    for name in wrappers:
        assert callable(getattr(K, name)), name
    return handle
