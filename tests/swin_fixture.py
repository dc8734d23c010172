"""Weights, inputs and cases of the Swin fixture (tests/golden/swin_small.npz), rebuilt from seeds on both sides.

tests/golden/gen_golden_swin.py loads these into the reference's swin.py modules and stores what the reference computes
(logits, CE loss, the gradient of every parameter) plus the module tree; the tests load the same tensors into the HIP modules.
Seeds, the weight recipe, packing and gradient sampling are port_fixture's, re-exported here for the generator script.
"""
from port_fixture import (GRAD_SAMPLE, _gen, grad_index, grad_sample, image_inputs, pack, pack_grads, pack_tree,  # noqa: F401
                          seeded_weights, unpack, unpack_grads, unpack_tree)

# small models: embed 32, depths [2, 2], heads [1, 2] (dh 32), window 7, no stochastic depth, 10 classes
MODEL = dict(patch_size=[4, 4], embed_dim=32, depths=[2, 2], num_heads=[1, 2], window_size=[7, 7], stochastic_depth_prob=0.0,
             num_classes=10)
# name -> (robust, image H, image W, batch)
CASES = {
    "s56": (False, 56, 56, 2),     # 14x14 map: shifted stage 1; stage 2 (7x7) has its shift zeroed
    "r56": (True, 56, 56, 2),      # the same with Sinkhorn attention
    "p64": (False, 64, 64, 2),     # 16x16 -> padded 21x21 with shift; 8x8 -> padded 14x14 with shift
    "ns": (False, 28, 56, 3),      # 7x14: the height's shift is zeroed, the width's kept; 4x7 after merging
}
SWIN_T_PARAMS = 28288354


def weights(state_dict, seed: int) -> dict:
    """Float entries of a state_dict (the integer relative_position_index is left out): weights of rank >= 2 (Linear, Conv2d,
    the relative-position table) ~ N(0, 1/fan_in), LayerNorm weights 1 + 0.1 N(0, 1), biases 0.02 N(0, 1)."""
    return seeded_weights(state_dict, seed)


def inputs(case: str):
    _, H, W, B = CASES[case]
    return image_inputs(case, B, 3, H, W, MODEL["num_classes"])


def model_kwargs(case: str) -> dict:
    return dict(MODEL, robust=CASES[case][0])
