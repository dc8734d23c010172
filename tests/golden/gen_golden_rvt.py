#!/usr/bin/env python3
"""Golden fixture for RvT, produced by running the reference's rvt.py itself on CPU (development container only; needs einops).
The package's __init__ imports torchvision, so `rvt` and `utils` are imported as submodules of a bare package shim, as in
gen_golden_t2t.py.

    python tests/golden/gen_golden_rvt.py <path to the reference's vit_pytorch_robust directory>

Weights and inputs are rebuilt from seeds by tests/rvt_fixture.py; stored (float16 relative to max-abs):
  <case>.logits / .loss                 for the cases of rvt_fixture.CASES
  <case>.gnames / .g / .glen / .gscale  every parameter's gradient (training cases; sampled as in swin_fixture)
  <case>.keys / .shapes / .sums         the module tree and the sums of the fixture weights
  <case>.modules                        named_modules() names of the case's model
  small.* / full.* (+ .nparams)         the SMALL and FULL configurations under torch.manual_seed(0) (seeded init)
  rot<i>.sin / .cos / .rot              AxialRotaryEmbedding's tables and rotate_every_two of rvt_fixture.ROTARY_PROBES (float32)
"""
import importlib, os, sys, types
import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else "vit_pytorch_robust"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import rvt_fixture as RF  # noqa: E402

pkg = types.ModuleType("vit_pytorch_robust"); pkg.__path__ = [REF]
sys.modules["vit_pytorch_robust"] = pkg
rvt = importlib.import_module("vit_pytorch_robust.rvt")
utils = importlib.import_module("vit_pytorch_robust.utils")

out = {"meta": np.array("reference rvt.py, CPU fp32; weights / inputs from tests/rvt_fixture.py")}
for case in RF.CASES:
    m = RF.build(rvt, case, sinkhorn=utils.SinkhornAttention)
    w = RF.weights(m, seed=3)
    m.load_state_dict(w, strict=True)
    img, y = RF.inputs(case)
    logits = m(img)
    loss = torch.nn.functional.cross_entropy(logits, y)
    RF.pack(out, case + ".logits", logits)
    out[case + ".loss"] = loss.detach().numpy()
    if m.training:
        loss.backward()
        RF.pack_grads(out, case, [(k, p.grad) for k, p in m.named_parameters()])
    RF.pack_tree(out, case, m.state_dict(), {k: w[k].double().sum() for k in w})
    out[case + ".modules"] = np.array([n for n, _ in m.named_modules()])
    print(case, "loss", loss.item())

for name, cfg in (("small", RF.SMALL), ("full", RF.FULL)):
    torch.manual_seed(0)
    t = rvt.RvT(**cfg)
    sd = t.state_dict()
    RF.pack_tree(out, name, sd, {k: v.double().sum() for k, v in sd.items()})
    out[name + ".nparams"] = np.int64(sum(p.numel() for p in t.parameters()))
    del t, sd

for i, (n, dim, mf) in enumerate(RF.ROTARY_PROBES):
    x = RF.rotary_probe_input(n, dim)
    sin, cos = rvt.AxialRotaryEmbedding(dim, max_freq=mf)(x)
    out[f"rot{i}.sin"] = sin.numpy().astype(np.float32)
    out[f"rot{i}.cos"] = cos.numpy().astype(np.float32)
    out[f"rot{i}.rot"] = rvt.rotate_every_two(x).numpy().astype(np.float32)

np.savez_compressed(os.path.join(OUT, "rvt_small.npz"), **out)
print("rvt_small.npz", os.path.getsize(os.path.join(OUT, "rvt_small.npz")))
