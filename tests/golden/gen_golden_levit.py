#!/usr/bin/env python3
"""Golden fixture for LeViT, produced by running the reference's levit.py itself on CPU (development container only).  levit.py
imports `trunc_normal_` from the package's utils.py; the module is loaded through a stub package.

Weights and inputs are rebuilt from seeds by tests/levit_fixture.py; stored (float16 relative to max-abs, levit_small.npz):
  <case>.logits / .loss                 for the cases of levit_fixture.CASES (train and eval, softmax and Sinkhorn, 224 px)
  <case>.gnames / .g / .glen / .gscale  every parameter's gradient (training cases; sampled as in swin_fixture)
  <case>.bufnames / .buf ...            the running means / variances after the forward (same packing)
  <case>.keys / .shapes / .sums         the module tree and the sums of the fixture weights
  g224.idx.<i>                          every attention_bias_idxs of the 224-px case (int16)
  <builder>.keys / .shapes / .sums / .nparams   the five builders under torch.manual_seed(0) (seeded init), 1000 classes
"""
import importlib, os, sys, types
import numpy as np
import torch

REF = "/root/reference/vit_pytorch_robust"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import levit_fixture as LF  # noqa: E402

pkg = types.ModuleType("vit_pytorch_robust"); pkg.__path__ = [REF]
sys.modules["vit_pytorch_robust"] = pkg
lv = importlib.import_module("vit_pytorch_robust.levit")

out = {"meta": np.array("reference levit.py, CPU fp32; weights / inputs from tests/levit_fixture.py")}
for case in LF.CASES:
    m = LF.build(lv, case)
    w = LF.weights(m, seed=3)
    m.load_state_dict(w, strict=False)
    m.train(LF.CASES[case][2])
    img, y = LF.inputs(case)
    logits = m(img)
    loss = torch.nn.functional.cross_entropy(logits, y, label_smoothing=0.1)
    LF.pack(out, case + ".logits", logits)
    out[case + ".loss"] = loss.detach().numpy()
    if m.training:
        loss.backward()
        LF.pack_grads(out, case, [(k, p.grad) for k, p in m.named_parameters()])
    LF.pack_grads(out, case + ".buf", LF.running_stats(m))
    LF.pack_tree(out, case, m.state_dict(), {k: w[k].double().sum() for k in w})
    if case == "g224":
        idx = [v for k, v in m.state_dict().items() if k.endswith("attention_bias_idxs")]
        for i, t in enumerate(idx):
            out[f"g224.idx.{i}"] = t.numpy().astype(np.int16)
    print(case, "loss", loss.item())

for name in LF.BUILDERS:
    torch.manual_seed(0)
    t = getattr(lv, name)()
    sd = t.state_dict()
    LF.pack_tree(out, name, sd, {k: v.double().sum() for k, v in sd.items()})
    out[name + ".nparams"] = np.int64(sum(p.numel() for p in t.parameters()))
    assert out[name + ".nparams"] == LF.NPARAMS[name], (name, out[name + ".nparams"])
np.savez_compressed(os.path.join(OUT, "levit_small.npz"), **out)
print("levit_small.npz", os.path.getsize(os.path.join(OUT, "levit_small.npz")))
