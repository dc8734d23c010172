#!/usr/bin/env python3
"""Golden fixture for DeepViT, produced by running the reference's deepvit.py itself on CPU (development container only).  The
module is loaded through a stub package, so that the package's __init__ (and what it imports) is not needed.

    python tests/golden/gen_golden_deepvit.py <path to the reference's vit_pytorch_robust directory>

Weights and inputs are rebuilt from seeds by tests/deepvit_fixture.py; stored (float16 relative to max-abs):
  <case>.logits / .loss                 for the cases of deepvit_fixture.CASES
  <case>.gnames / .g / .glen / .gscale  every parameter's gradient (training cases; sampled as in swin_fixture)
  <case>.keys / .shapes / .sums         the module tree and the sums of the fixture weights
  small.* / full.* (+ .nparams)         the SMALL and FULL configurations under torch.manual_seed(0) (seeded init)
"""
import importlib, os, sys, types
import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else "vit_pytorch_robust"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import deepvit_fixture as DF  # noqa: E402

pkg = types.ModuleType("vit_pytorch_robust"); pkg.__path__ = [REF]
sys.modules["vit_pytorch_robust"] = pkg
deepvit = importlib.import_module("vit_pytorch_robust.deepvit")

out = {"meta": np.array("reference deepvit.py, CPU fp32; weights / inputs from tests/deepvit_fixture.py")}
for case in DF.CASES:
    m = DF.build(deepvit, case)
    w = DF.weights(m, seed=3)
    m.load_state_dict(w, strict=True)
    img, y = DF.inputs(case)
    logits = m(img)
    loss = torch.nn.functional.cross_entropy(logits, y)
    DF.pack(out, case + ".logits", logits)
    out[case + ".loss"] = loss.detach().numpy()
    if m.training:
        loss.backward()
        DF.pack_grads(out, case, [(k, p.grad) for k, p in m.named_parameters()])
    DF.pack_tree(out, case, m.state_dict(), {k: w[k].double().sum() for k in w})
    print(case, "loss", loss.item())

for name, cfg in (("small", DF.SMALL), ("full", DF.FULL)):
    torch.manual_seed(0)
    t = deepvit.DeepViT(**cfg)
    sd = t.state_dict()
    DF.pack_tree(out, name, sd, {k: v.double().sum() for k, v in sd.items()})
    out[name + ".nparams"] = np.int64(sum(p.numel() for p in t.parameters()))
    del t, sd
assert out["small.nparams"] == DF.SMALL_NPARAMS, out["small.nparams"]

np.savez_compressed(os.path.join(OUT, "deepvit_small.npz"), **out)
print("deepvit_small.npz", os.path.getsize(os.path.join(OUT, "deepvit_small.npz")))
