#!/usr/bin/env python3
"""Golden fixture for the Swin Transformer, produced by running the reference's swin.py itself on CPU (development container
only).  swin.py imports torchvision.ops.misc.{MLP, Permute} and torchvision.ops.stochastic_depth.StochasticDepth; minimal
stand-ins with torchvision's semantics are installed in sys.modules, and the module is loaded through a stub package.

Weights and inputs are rebuilt from seeds by tests/swin_fixture.py; stored (float16 relative to max-abs, swin_small.npz):
  <case>.logits / .loss               for the four cases of swin_fixture.CASES
  <case>.gnames / .g / .glen / .gscale  every parameter's gradient (at swin_fixture.grad_index), packed by pack_grads
  <case>.keys / .shapes / .sums       the module tree and the sums of the seeded weights (pack_tree)
  swin_t.keys / .shapes / .sums / .nparams   swin_t() under torch.manual_seed(0) (the reference's seeded init)
Few arrays, not one per tensor: the zip container's per-entry overhead would otherwise outweigh the data.
"""
import importlib, os, sys, types
import numpy as np
import torch
from torch import nn

REF = "/root/reference/vit_pytorch_robust"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import swin_fixture as SF  # noqa: E402


class Permute(nn.Module):
    def __init__(self, dims):
        super().__init__()
        self.dims = dims

    def forward(self, x):
        return torch.permute(x, self.dims)


class MLP(nn.Sequential):
    def __init__(self, in_channels, hidden_channels, norm_layer=None, activation_layer=nn.ReLU, inplace=None, bias=True, dropout=0.0):
        layers, d = [], in_channels
        for h in hidden_channels[:-1]:
            layers += [nn.Linear(d, h, bias=bias), activation_layer(), nn.Dropout(dropout)]
            d = h
        layers += [nn.Linear(d, hidden_channels[-1], bias=bias), nn.Dropout(dropout)]
        super().__init__(*layers)


class StochasticDepth(nn.Module):
    def __init__(self, p, mode):
        super().__init__()
        self.p, self.mode = p, mode

    def forward(self, x):
        if not self.training or self.p == 0.0:
            return x
        survival = 1.0 - self.p
        noise = torch.empty([x.shape[0]] + [1] * (x.ndim - 1), dtype=x.dtype, device=x.device).bernoulli_(survival)
        if survival > 0.0:
            noise.div_(survival)
        return x * noise


tv = types.ModuleType("torchvision"); ops = types.ModuleType("torchvision.ops")
misc = types.ModuleType("torchvision.ops.misc"); misc.MLP, misc.Permute = MLP, Permute
sdm = types.ModuleType("torchvision.ops.stochastic_depth"); sdm.StochasticDepth = StochasticDepth
tv.ops, ops.misc, ops.stochastic_depth = ops, misc, sdm
sys.modules.update({"torchvision": tv, "torchvision.ops": ops, "torchvision.ops.misc": misc, "torchvision.ops.stochastic_depth": sdm})
pkg = types.ModuleType("vit_pytorch_robust"); pkg.__path__ = [REF]
sys.modules["vit_pytorch_robust"] = pkg
sw = importlib.import_module("vit_pytorch_robust.swin")

out = {"meta": np.array("reference swin.py, CPU fp32; weights / inputs from tests/swin_fixture.py")}
for case in SF.CASES:
    m = sw.SwinTransformer(**SF.model_kwargs(case)).train()
    w = SF.weights(m.state_dict(), seed=3)
    m.load_state_dict(w, strict=False)
    img, y = SF.inputs(case)
    logits = m(img)
    loss = torch.nn.functional.cross_entropy(logits, y)
    loss.backward()
    SF.pack(out, case + ".logits", logits)
    out[case + ".loss"] = loss.detach().numpy()
    SF.pack_tree(out, case, m.state_dict(), {k: w[k].double().sum() for k in w})
    SF.pack_grads(out, case, [(k, p.grad) for k, p in m.named_parameters()])
    print(case, "loss", loss.item())

torch.manual_seed(0)
t = sw.swin_t()
sd = t.state_dict()
SF.pack_tree(out, "swin_t", sd, {k: v.double().sum() for k, v in sd.items()})
out["swin_t.nparams"] = np.int64(sum(p.numel() for p in t.parameters()))
assert out["swin_t.nparams"] == SF.SWIN_T_PARAMS, out["swin_t.nparams"]
np.savez_compressed(os.path.join(OUT, "swin_small.npz"), **out)
print("swin_small.npz", os.path.getsize(os.path.join(OUT, "swin_small.npz")))
