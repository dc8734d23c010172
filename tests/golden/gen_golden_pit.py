#!/usr/bin/env python3
"""Golden fixture for PiT, produced by running the reference's pit.py itself on CPU (development container only; needs einops).
The package's __init__ imports torchvision, so `pit` and `utils` are imported as submodules of a bare package shim, as in
gen_golden_rvt.py.

    python tests/golden/gen_golden_pit.py <path to the reference's vit_pytorch_robust directory>

Weights and inputs are rebuilt from seeds by tests/pit_fixture.py; stored (float16 relative to max-abs):
  <case>.logits / .loss                 for the cases of pit_fixture.CASES
  <case>.gnames / .g / .glen / .gscale  every parameter's gradient (training cases; sampled as in swin_fixture)
  <case>.keys / .shapes / .sums         the module tree and the sums of the fixture weights
  <case>.modules                        named_modules() names of the case's model
  small.* / full.* (+ .nparams)         the SMALL and FULL configurations under torch.manual_seed(0) (seeded init)
"""
import importlib, os, sys, types
import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else "vit_pytorch_robust"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import pit_fixture as PF  # noqa: E402

pkg = types.ModuleType("vit_pytorch_robust"); pkg.__path__ = [REF]
sys.modules["vit_pytorch_robust"] = pkg
pit = importlib.import_module("vit_pytorch_robust.pit")
utils = importlib.import_module("vit_pytorch_robust.utils")

out = {"meta": np.array("reference pit.py, CPU fp32; weights / inputs from tests/pit_fixture.py")}
for case in PF.CASES:
    m = PF.build(pit, case, sinkhorn=utils.SinkhornAttention)
    w = PF.weights(m, seed=3)
    m.load_state_dict(w, strict=True)
    img, y = PF.inputs(case)
    logits = m(img)
    loss = torch.nn.functional.cross_entropy(logits, y)
    PF.pack(out, case + ".logits", logits)
    out[case + ".loss"] = loss.detach().numpy()
    if m.training:
        loss.backward()
        PF.pack_grads(out, case, [(k, p.grad) for k, p in m.named_parameters()])
    PF.pack_tree(out, case, m.state_dict(), {k: w[k].double().sum() for k in w})
    out[case + ".modules"] = np.array([n for n, _ in m.named_modules()])
    print(case, "loss", loss.item())

for name, cfg in (("small", PF.SMALL), ("full", PF.FULL)):
    torch.manual_seed(0)
    t = pit.PiT(**cfg)
    sd = t.state_dict()
    PF.pack_tree(out, name, sd, {k: v.double().sum() for k, v in sd.items()})
    out[name + ".nparams"] = np.int64(sum(p.numel() for p in t.parameters()))
    del t, sd

np.savez_compressed(os.path.join(OUT, "pit_small.npz"), **out)
print("pit_small.npz", os.path.getsize(os.path.join(OUT, "pit_small.npz")))
