#!/usr/bin/env python3
"""Golden fixture for CCT, produced by running the reference's cct.py itself on CPU (development container only; needs einops).
The package's __init__ imports torchvision, so `cct` and `utils` are imported as submodules of a bare package shim, as in
gen_golden_pit.py.

    python tests/golden/gen_golden_cct.py <path to the reference's vit_pytorch_robust directory>

Weights and inputs are rebuilt from seeds by tests/cct_fixture.py; stored (float16 relative to max-abs):
  <case>.logits / .loss                 for the cases of cct_fixture.CASES
  <case>.gnames / .g / .glen / .gscale  every trainable parameter's gradient (training cases; sampled as in swin_fixture)
  <case>.keys / .shapes / .sums         the module tree and the sums of the fixture weights
  <case>.modules                        named_modules() names of the case's model
  drop.attn_keep.<i> / drop.path_keep.<i>   the keep masks the reference drew (forward hooks on attn_drop and DropPath: output != 0)
  full.* (+ .nparams)                   cct_fixture.FULL under torch.manual_seed(0) (seeded init)
  sine.16x64                            sinusoidal_embedding(16, 64), fp32 as computed
"""
import importlib, os, sys, types
import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else "vit_pytorch_robust"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import cct_fixture as CF  # noqa: E402

pkg = types.ModuleType("vit_pytorch_robust"); pkg.__path__ = [REF]
sys.modules["vit_pytorch_robust"] = pkg
cct = importlib.import_module("vit_pytorch_robust.cct")
utils = importlib.import_module("vit_pytorch_robust.utils")
_sink = utils.SinkhornAttention()


def sinkhorn_forward(self, x):
    """The reference Attention's computation with utils.SinkhornAttention (softmax + normalisation) in the place of softmax."""
    B, N, C = x.shape
    q, k, v = (t.reshape(B, N, self.heads, C // self.heads).transpose(1, 2) for t in self.qkv(x).chunk(3, dim=-1))
    attn = self.attn_drop(_sink((q * self.scale) @ k.transpose(-1, -2)))
    return self.proj_drop(self.proj((attn @ v).transpose(1, 2).reshape(B, N, C)))


out = {"meta": np.array("reference cct.py, CPU fp32; weights / inputs from tests/cct_fixture.py")}
for case, (cfg, robust, train, B, pa) in CF.CASES.items():
    m = CF.build(cct, case, reference=True, sinkhorn_forward=sinkhorn_forward)
    w = CF.weights(m, seed=3)
    m.load_state_dict(w, strict=True)
    x, y = CF.inputs(case)
    blocks = CF.classifier_of(m).blocks
    attn_keep, path_keep, hooks = [], {}, []
    drops = train and (pa > 0 or any(b.drop_path.drop_prob > 0 for b in blocks))
    if drops:
        torch.manual_seed(1)
        for i, blk in enumerate(blocks):
            hooks.append(blk.self_attn.attn_drop.register_forward_hook(lambda mod, inp, o: attn_keep.append((o != 0).clone())))
            if blk.drop_path.drop_prob > 0:
                hooks.append(blk.drop_path.register_forward_hook(
                    lambda mod, inp, o, i=i: path_keep.setdefault(i, []).append((o != 0).flatten(1).any(1))))
    logits = m(x)
    for h in hooks:
        h.remove()
    loss = torch.nn.functional.cross_entropy(logits, y)
    CF.pack(out, case + ".logits", logits)
    out[case + ".loss"] = loss.detach().numpy()
    if train:
        loss.backward()
        CF.pack_grads(out, case, [(k, p.grad) for k, p in m.named_parameters() if p.requires_grad])
    if drops:
        path = {i: torch.stack(v) for i, v in path_keep.items()}
        last = path[len(blocks) - 1]
        assert bool((last == 0).any()) and bool((last == 1).any()), "the recorded layer-2 keep must hold a 0 and a 1: change the seed"
        CF.pack_masks(out, case, attn_keep, path)
    CF.pack_tree(out, case, m.state_dict(), {k: w[k].double().sum() for k in w})
    out[case + ".modules"] = np.array([n for n, _ in m.named_modules()])
    print(case, "loss", loss.item())

torch.manual_seed(0)
t = getattr(cct, CF.FULL_BUILDER)(**CF.FULL)
sd = t.state_dict()
CF.pack_tree(out, "full", sd, {k: v.double().sum() for k, v in sd.items()})
out["full.nparams"] = np.int64(sum(p.numel() for p in t.parameters()))
out["sine.16x64"] = cct.sinusoidal_embedding(16, 64).numpy()

np.savez_compressed(os.path.join(OUT, "cct_small.npz"), **out)
print("cct_small.npz", os.path.getsize(os.path.join(OUT, "cct_small.npz")))
