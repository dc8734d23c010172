#!/usr/bin/env python3
"""Golden fixture for T2T-ViT, produced by running the reference's t2t.py itself on CPU (development container only; needs
einops).  t2t.py does `from vit_pytorch_robust.vit import Transformer`, which that vit.py does not define: as in
gen_golden_mae.py the module is pre-seeded with learnable_memory_vit's Transformer, the class the file intends.

    python tests/golden/gen_golden_t2t.py <path to the reference's vit_pytorch_robust directory>

Weights and inputs are rebuilt from seeds by tests/t2t_fixture.py; stored (float16 relative to max-abs):
  <case>.logits / .loss                 for the cases of t2t_fixture.CASES
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
import t2t_fixture as TF  # noqa: E402

pkg = types.ModuleType("vit_pytorch_robust"); pkg.__path__ = [REF]
sys.modules["vit_pytorch_robust"] = pkg
lm = importlib.import_module("vit_pytorch_robust.learnable_memory_vit")
shim = types.ModuleType("vit_pytorch_robust.vit"); shim.Transformer = lm.Transformer
sys.modules["vit_pytorch_robust.vit"] = shim
t2t = importlib.import_module("vit_pytorch_robust.t2t")
utils = importlib.import_module("vit_pytorch_robust.utils")

out = {"meta": np.array("reference t2t.py, CPU fp32; weights / inputs from tests/t2t_fixture.py")}
for case in TF.CASES:
    m = TF.build(t2t, case, sinkhorn=utils.SinkhornAttention)
    w = TF.weights(m, seed=3)
    m.load_state_dict(w, strict=True)
    img, y = TF.inputs(case)
    logits = m(img)
    loss = torch.nn.functional.cross_entropy(logits, y)
    TF.pack(out, case + ".logits", logits)
    out[case + ".loss"] = loss.detach().numpy()
    if m.training:
        loss.backward()
        TF.pack_grads(out, case, [(k, p.grad) for k, p in m.named_parameters()])
    TF.pack_tree(out, case, m.state_dict(), {k: w[k].double().sum() for k in w})
    out[case + ".modules"] = np.array([n for n, _ in m.named_modules()])
    print(case, "loss", loss.item())

for name, cfg in (("small", TF.SMALL), ("full", TF.FULL)):
    torch.manual_seed(0)
    t = t2t.T2TViT(**cfg)
    sd = t.state_dict()
    TF.pack_tree(out, name, sd, {k: v.double().sum() for k, v in sd.items()})
    out[name + ".nparams"] = np.int64(sum(p.numel() for p in t.parameters()))
    del t, sd

np.savez_compressed(os.path.join(OUT, "t2t_small.npz"), **out)
print("t2t_small.npz", os.path.getsize(os.path.join(OUT, "t2t_small.npz")))
