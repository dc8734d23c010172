#!/usr/bin/env python3
"""Golden fixture for Twins-SVT, produced by running the reference's twins_svt.py itself on CPU (development container only;
needs einops).  The package's __init__ imports torchvision, so `twins_svt` is imported as a submodule of a bare package shim, as
in gen_golden_pit.py.

    python tests/golden/gen_golden_twins.py <path to the reference's vit_pytorch_robust directory>

Weights and inputs are rebuilt from seeds by tests/twins_fixture.py; stored (float16 relative to max-abs):
  <case>.logits / .loss                 for the cases of twins_fixture.CASES
  <case>.gnames / .g / .glen / .gscale  every parameter's gradient (training cases; sampled as in swin_fixture)
  <case>.gmax                           every parameter's gradient abs max (the vanishing set is read off these)
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
import twins_fixture as TF  # noqa: E402

pkg = types.ModuleType("vit_pytorch_robust"); pkg.__path__ = [REF]
sys.modules["vit_pytorch_robust"] = pkg
twins = importlib.import_module("vit_pytorch_robust.twins_svt")

out = {"meta": np.array("reference twins_svt.py, CPU fp32; weights / inputs from tests/twins_fixture.py")}
for case in TF.CASES:
    m = TF.build(twins, case)
    w = TF.weights(m, seed=3)
    m.load_state_dict(w, strict=True)
    img, y = TF.inputs(case)
    logits = m(img)
    loss = torch.nn.functional.cross_entropy(logits, y)
    TF.pack(out, case + ".logits", logits)
    out[case + ".loss"] = loss.detach().numpy()
    if m.training:
        loss.backward()
        named = [(k, p.grad) for k, p in m.named_parameters()]
        TF.pack_grads(out, case, named)
        out[case + ".gmax"] = np.array([float(g.abs().max()) for _, g in named], dtype=np.float64)
    TF.pack_tree(out, case, m.state_dict(), {k: w[k].double().sum() for k in w})
    out[case + ".modules"] = np.array([n for n, _ in m.named_modules()])
    print(case, "loss", loss.item())

for name, cfg in (("small", TF.SMALL), ("full", TF.FULL)):
    torch.manual_seed(0)
    t = twins.TwinsSVT(**cfg)
    sd = t.state_dict()
    TF.pack_tree(out, name, sd, {k: v.double().sum() for k, v in sd.items()})
    out[name + ".nparams"] = np.int64(sum(p.numel() for p in t.parameters()))
    del t, sd

np.savez_compressed(os.path.join(OUT, "twins_small.npz"), **out)
print("twins_small.npz", os.path.getsize(os.path.join(OUT, "twins_small.npz")))
