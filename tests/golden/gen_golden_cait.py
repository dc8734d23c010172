#!/usr/bin/env python3
"""Golden fixture for CaiT, produced by running the reference's cait.py itself on CPU (development container only).  cait.py
imports SinkhornAttention from the package's utils.py; the module is loaded through a stub package.

    python tests/golden/gen_golden_cait.py <path to the reference's vit_pytorch_robust directory>

Weights and inputs are rebuilt from seeds by tests/cait_fixture.py; stored (float16 relative to max-abs):
  <case>.logits / .loss                 for the cases of cait_fixture.CASES
  <case>.gnames / .g / .glen / .gscale  every parameter's gradient (training cases; sampled as in swin_fixture)
  <case>.keys / .shapes / .sums         the module tree and the sums of the fixture weights
  small.* / full.* (+ .nparams)         the SMALL and FULL configurations under torch.manual_seed(0) (seeded init)
  draws                                 the kept layer indices of dropout_layers for cait_fixture.DRAWS (-1 padded)
"""
import importlib, os, sys, types
import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else "vit_pytorch_robust"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import cait_fixture as CF  # noqa: E402

pkg = types.ModuleType("vit_pytorch_robust"); pkg.__path__ = [REF]
sys.modules["vit_pytorch_robust"] = pkg
cait = importlib.import_module("vit_pytorch_robust.cait")

out = {"meta": np.array("reference cait.py, CPU fp32; weights / inputs from tests/cait_fixture.py")}
for case in CF.CASES:
    m = CF.build(cait, case)
    w = CF.weights(m, seed=3)
    m.load_state_dict(w, strict=True)
    img, y = CF.inputs(case)
    logits = m(img)
    loss = torch.nn.functional.cross_entropy(logits, y)
    CF.pack(out, case + ".logits", logits)
    out[case + ".loss"] = loss.detach().numpy()
    if m.training:
        loss.backward()
        CF.pack_grads(out, case, [(k, p.grad) for k, p in m.named_parameters()])
    CF.pack_tree(out, case, m.state_dict(), {k: w[k].double().sum() for k in w})
    print(case, "loss", loss.item())

for name, cfg in (("small", CF.SMALL), ("full", CF.FULL)):
    torch.manual_seed(0)
    t = cait.CaiT(**cfg)
    sd = t.state_dict()
    CF.pack_tree(out, name, sd, {k: v.double().sum() for k, v in sd.items()})
    out[name + ".nparams"] = np.int64(sum(p.numel() for p in t.parameters()))
    del t, sd
assert out["small.nparams"] == CF.SMALL_NPARAMS

draws = np.full((len(CF.DRAWS), max(d[2] for d in CF.DRAWS)), -1, dtype=np.int64)
for r, d in enumerate(CF.DRAWS):
    kept = CF.draw(cait, *d)
    draws[r, :len(kept)] = kept
out["draws"] = draws
np.savez_compressed(os.path.join(OUT, "cait_small.npz"), **out)
print("cait_small.npz", os.path.getsize(os.path.join(OUT, "cait_small.npz")))
