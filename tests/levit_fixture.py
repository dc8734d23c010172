"""Weights, inputs and cases of the LeViT fixture (tests/golden/levit_small.npz), rebuilt from seeds on both sides.

tests/golden/gen_golden_levit.py loads these into the reference's levit.py modules and stores what the reference computes
(logits, CE loss, the gradient of every parameter, the running statistics after the forward) plus the module trees; the tests
load the same tensors into the HIP modules and into tests/levit_ref.py.  Seeds, packing and gradient sampling are
port_fixture's; the weight recipe (batch norms, bias tables, running statistics) is its own.
"""
import torch
from torch import nn

from port_fixture import (_gen, grad_index, grad_sample, image_inputs, pack, pack_grads, pack_tree, unpack, unpack_grads,  # noqa: F401
                          unpack_tree)

BUILDERS = ("LeViT_128S", "LeViT_128", "LeViT_192", "LeViT_256", "LeViT_384")
NPARAMS = {"LeViT_128S": 7391290, "LeViT_128": 8828168, "LeViT_192": 10561301, "LeViT_256": 18379852, "LeViT_384": 38358300}

# small model at 112 px: 7 -> 4 -> 2 tokens per side after the stem (Nq != Nk at odd sizes), kd 16, one block per stage
SMALL = dict(img_size=112, patch_size=16, embed_dim=[64, 96, 128], key_dim=[16, 16, 16], depth=[1, 1, 1], num_heads=[4, 6, 8],
             attn_ratio=[2, 2, 2], mlp_ratio=[2, 2, 2], down_ops=[["Subsample", 16, 4, 4, 2, 2], ["Subsample", 16, 6, 4, 2, 2]],
             num_classes=10, drop_path=0)
# 224 px with small channels: pins the (196, 196), (49, 196), (49, 49), (16, 49), (16, 16) geometries and their bias indices
G224 = dict(img_size=224, patch_size=16, embed_dim=[64, 64, 64], key_dim=[16, 16, 16], depth=[1, 1, 1], num_heads=[2, 2, 2],
            attn_ratio=[2, 2, 2], mlp_ratio=[2, 2, 2], down_ops=[["Subsample", 16, 2, 4, 2, 2], ["Subsample", 16, 2, 4, 2, 2]],
            num_classes=10, drop_path=0)
# name -> (model config, robust, train, batch)
CASES = {
    "s_train": (SMALL, False, True, 4),
    "r_train": (SMALL, True, True, 4),
    "s_eval": (SMALL, False, False, 4),
    "r_eval": (SMALL, True, False, 4),
    "g224": (G224, False, True, 2),
}


def build(module, case: str):
    """The case's model from `module` (the reference's levit or noise_robust_vit_amd.levit)."""
    cfg, robust, train, _ = CASES[case]
    act = nn.Hardswish
    m = module.LeViT(**dict(cfg, down_ops=[list(d) for d in cfg["down_ops"]]), attention_activation=act, mlp_activation=act,
                     hybrid_backbone=module.b16(cfg["embed_dim"][0], activation=act), robust=robust)
    return m.train(train)


def closing_bns(model) -> set:
    """state_dict prefixes of the BNs that close a residual branch (bn_weight_init=0 in the reference, levit.py:227,475)."""
    names = {id(m): n for n, m in model.named_modules()}
    out = set()
    for mod in model.modules():
        if type(mod).__name__ == "Residual":
            inner = mod.m
            last = inner.proj[1] if hasattr(inner, "proj") else inner[2]
            out.add(names[id(last.bn)])
    return out


def weights(model, seed: int) -> dict:
    """Float entries of the state_dict: Linear / Conv2d weights ~ N(0, 1/fan_in); BN weights 1 + 0.1 N(0, 1), away from 0 (0.1 x
    that on the BNs that close a residual branch: at full strength the fp32 model is too badly conditioned to compare a bf16
    implementation against); BN biases and bias tables 0.1 N(0, 1); running means 0.1 N(0, 1), running variances 0.5 + U(0, 1)."""
    closing = closing_bns(model)
    out = {}
    for name, t in model.state_dict().items():
        if not t.is_floating_point():
            continue
        g = _gen(seed, name)
        z = torch.randn(tuple(t.shape), generator=g)
        prefix, leaf = name.rsplit(".", 1)
        if t.dim() >= 2 and "attention_biases" not in name:
            z = z / t[0].numel() ** 0.5
        elif leaf == "weight":
            z = (0.1 if prefix in closing else 1.0) * (1.0 + 0.1 * z)
        elif leaf == "running_var":
            z = 0.5 + torch.rand(tuple(t.shape), generator=g)
        else:
            z = 0.1 * z
        out[name] = z
    return out


def inputs(case: str):
    cfg, _, _, B = CASES[case]
    return image_inputs(case, B, 3, cfg["img_size"], cfg["img_size"], cfg["num_classes"])


def running_stats(model):
    return [(k, v) for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var"))]
