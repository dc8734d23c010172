"""Weights, inputs and cases of the PatchConvNet fixture (tests/golden/patchconvnet_small.npz), rebuilt from seeds on both sides.

tests/golden/gen_golden_patchconvnet.py loads these into the reference's patch_convnet.py modules and stores what the reference
computes (logits, CE loss, the gradient of every parameter) plus the module trees; the tests load the same tensors into the HIP
modules and into tests/patchconvnet_ref.py.  Seeds, the weight recipe, packing and gradient sampling are port_fixture's.
"""
import torch

from port_fixture import (_gen, grad_index, grad_sample, image_inputs, pack, pack_grads, pack_tree, seeded_weights,  # noqa: F401
                          unpack, unpack_grads, unpack_tree, vit_tokens)

BUILDERS = ("S60", "S120", "B60", "B120", "L60", "L120")
# under torch.manual_seed(0) with 100 classes (the reference's CIFAR-100 script)
NPARAMS = {"S60": 24884596, "B60": 98696836, "L60": 175087076}

SMALL = dict(img_size=64, patch_size=16, embed_dim=64, depth=2, num_heads=1, qkv_bias=True, num_classes=10)
G224 = dict(img_size=224, patch_size=16, embed_dim=64, depth=1, num_heads=1, qkv_bias=True, num_classes=10)
# name -> (model config overrides, train, batch)
CASES = {
    "s_train": (SMALL, True, 4),                                         # 4x4 grid, 17 keys
    "s_eval": (SMALL, False, 4),
    "h2": (dict(SMALL, num_heads=2, qkv_bias=False), True, 3),          # two heads (dh 32), no q / k / v bias
    "g224": (G224, True, 2),                                             # 14x14 grid, 197 keys
}


def build(module, case: str):
    """The case's model from `module` (the reference's patch_convnet or noise_robust_vit_amd.patch_convnet)."""
    from functools import partial
    cfg, train, _ = CASES[case]
    m = module.PatchConvnet(**cfg, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    return m.train(train)


def weights(model, seed: int) -> dict:
    """Rank >= 2 weights ~ N(0, 1/fan_in); LayerNorm weights 1 + 0.1 N(0, 1); gamma_* 0.1 (1 + 0.1 N(0, 1)) (the reference's 1e-4
    would hide every branch in the logits); cls_token 0.5 N(0, 1); biases 0.02 N(0, 1)."""
    def special(name, leaf, t, z):
        return 0.1 * (1.0 + 0.1 * z) if leaf.startswith("gamma_") else vit_tokens(name, leaf, t, z)
    return seeded_weights(model.state_dict(), seed, special)


def inputs(case: str):
    cfg, _, B = CASES[case]
    return image_inputs(case, B, 3, cfg["img_size"], cfg["img_size"], cfg["num_classes"])
