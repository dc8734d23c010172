"""Weights and inputs of the Adapter fixture (tests/golden/adapter_small.npz), rebuilt from seeds on both sides.

The generator (tests/golden/gen_golden_adapter.py) loads these into the reference's modules and stores only what the
reference computes from them (outputs, loss, gradients) plus the module tree; the tests load the same tensors into the HIP
modules.  The per-name generator and the float16 packing are port_fixture's, re-exported here for the generator script.
"""
import torch

from port_fixture import _gen, pack, unpack  # noqa: F401

# Adapter case: lucid ViT(image_size=64, patch_size=16, dim=128, depth=2, heads=2, dim_head=64, mlp_dim=256) + Adapter(M=3, 5 classes)
ADAPTER_VIT = dict(image_size=64, patch_size=16, num_classes=10, dim=128, depth=2, heads=2, dim_head=64, mlp_dim=256)
ADAPTER_M, ADAPTER_CLASSES, ADAPTER_BATCH = 3, 5, 4
# masks-and-memories case: bare Transformer(dim, depth, heads, dim_head, mlp_dim), per-sample memories, one fully masked row
TR_ARGS = (64, 2, 2, 32, 128)
TR_B, TR_NQ, TR_M, TR_FULL_ROW = 3, 21, 5, 4


def weights(state_dict, seed: int) -> dict:
    """Deterministic float entries for a state_dict (non-float buffers such as the Adapter's attn_mask are left out):
    2-D weights ~ N(0, 1/fan_in), 1-D weights (LayerNorm) 1 + 0.1 N(0, 1), biases 0.02 N(0, 1), other tensors (positions,
    class / memory tokens, memories) N(0, 1) as the modules initialise them."""
    out = {}
    for name, t in state_dict.items():
        if not t.is_floating_point():
            continue
        z = torch.randn(tuple(t.shape), generator=_gen(seed, name))
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "weight" and t.dim() >= 2:
            z = z / t[0].numel() ** 0.5
        elif leaf == "weight":
            z = 1.0 + 0.1 * z
        elif leaf == "bias":
            z = 0.02 * z
        out[name] = z
    return out


def adapter_inputs(seed: int = 7):
    g = _gen(seed, "inputs")
    img = torch.randn(ADAPTER_BATCH, 3, ADAPTER_VIT["image_size"], ADAPTER_VIT["image_size"], generator=g)
    y = torch.randint(0, ADAPTER_CLASSES, (ADAPTER_BATCH,), generator=g)
    return img, y


def transformer_inputs(seed: int = 11):
    dim, depth = TR_ARGS[0], TR_ARGS[1]
    g = _gen(seed, "inputs")
    x = torch.randn(TR_B, TR_NQ, dim, generator=g)
    mems = torch.randn(depth, TR_B, TR_M, dim, generator=g)
    mask = torch.rand(TR_NQ, TR_NQ + TR_M, generator=g) > 0.3
    mask[TR_FULL_ROW] = False                      # one fully masked query row: uniform weights
    dy = torch.randn(TR_B, TR_NQ, dim, generator=g)
    return x, mems, mask, dy
