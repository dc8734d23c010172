#!/usr/bin/env python3
"""Golden fixture for PatchConvNet, produced by running the reference's patch_convnet.py itself on CPU (development container
only).  patch_convnet.py imports SqueezeExcite, DropPath, to_2tuple and trunc_normal_ from the package's utils.py; the module is
loaded through a stub package.

Weights and inputs are rebuilt from seeds by tests/patchconvnet_fixture.py; stored (float16 relative to max-abs):
  <case>.logits / .loss                 for the cases of patchconvnet_fixture.CASES
  <case>.gnames / .g / .glen / .gscale  every parameter's gradient (training cases; sampled as in swin_fixture)
  <case>.keys / .shapes / .sums         the module tree and the sums of the fixture weights
  <builder>.keys / .shapes / .sums / .nparams   the six builders under torch.manual_seed(0) (seeded init), 100 classes
"""
import importlib, os, sys, types
import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else "vit_pytorch_robust"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import patchconvnet_fixture as PF  # noqa: E402

pkg = types.ModuleType("vit_pytorch_robust"); pkg.__path__ = [REF]
sys.modules["vit_pytorch_robust"] = pkg
pc = importlib.import_module("vit_pytorch_robust.patch_convnet")

out = {"meta": np.array("reference patch_convnet.py, CPU fp32; weights / inputs from tests/patchconvnet_fixture.py")}
for case in PF.CASES:
    m = PF.build(pc, case)
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
    print(case, "loss", loss.item())

for name in PF.BUILDERS:
    torch.manual_seed(0)
    t = getattr(pc, name)(num_classes=100)
    sd = t.state_dict()
    PF.pack_tree(out, name, sd, {k: v.double().sum() for k, v in sd.items()})
    out[name + ".nparams"] = np.int64(sum(p.numel() for p in t.parameters()))
    if name in PF.NPARAMS:
        assert out[name + ".nparams"] == PF.NPARAMS[name], (name, out[name + ".nparams"])
    del t, sd
np.savez_compressed(os.path.join(OUT, "patchconvnet_small.npz"), **out)
print("patchconvnet_small.npz", os.path.getsize(os.path.join(OUT, "patchconvnet_small.npz")))
