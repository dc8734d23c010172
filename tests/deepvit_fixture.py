"""Weights, inputs and cases of the DeepViT fixture (tests/golden/deepvit_small.npz), rebuilt from seeds on both sides.

tests/golden/gen_golden_deepvit.py loads these into the reference's deepvit.py modules and stores what the reference computes
(logits, CE loss, the gradient of every parameter) plus the module trees; the tests load the same tensors into the HIP modules
and into tests/deepvit_ref.py.  Seeds, the weight recipe, packing and gradient sampling are port_fixture's.

Every case has at least 3 heads: with two, the LayerNorm over the heads leaves one degree of freedom per position and the
gradient of reattn_weights is mostly cancellation (bf16 operand rounding alone moves it by 0.1 to 3 rel-L2), so a two-head model
is no parity case.  The reference's DeepViT is softmax only: robust models have no recording and are checked against the
restatement, whose Sinkhorn is pinned to the reference by sinkhorn_unit.npz.
"""
from port_fixture import (_gen, grad_index, grad_sample, image_inputs, pack, pack_grads, pack_tree, seeded_weights,  # noqa: F401
                          unpack, unpack_grads, unpack_tree, vit_tokens)

SMALL = dict(image_size=64, patch_size=16, num_classes=10, dim=64, depth=2, heads=4, mlp_dim=128, dim_head=16)
SMALL_NPARAMS = 117754
# name -> (model config, train, batch)
CASES = {
    "s_train": (SMALL, True, 4),                                          # 4x4 grid + class token: 17 tokens
    "s_eval": (SMALL, False, 4),
    "mean": (dict(SMALL, pool="mean"), True, 4),
    "h3": (dict(SMALL, heads=3, dim_head=24), True, 4),
    "h8": (dict(SMALL, heads=8, dim_head=8), True, 4),
    "g14": (dict(SMALL, image_size=224, depth=1, dim_head=48), True, 2),  # 14x14 grid + class token: 197 tokens
}
# seeded init (torch.manual_seed(0)) of one full-size configuration: DeepViT-S-like at 224 px, 100 classes
FULL = dict(image_size=224, patch_size=16, num_classes=100, dim=384, depth=16, heads=12, mlp_dim=1152, dim_head=32)


def build(module, case: str, **kw):
    """The case's model from `module` (the reference's deepvit or noise_robust_vit_amd.deepvit); `kw` (robust=True) only for
    the latter."""
    cfg, train, _ = CASES[case]
    return module.DeepViT(**cfg, **kw).train(train)


def weights(model, seed: int) -> dict:
    """Linear weights ~ N(0, 1/fan_in); reattn_weights N(0, 1) (the reference's init); LayerNorm weights 1 + 0.1 N(0, 1);
    cls_token 0.5 N(0, 1); pos_embedding 0.2 N(0, 1); biases 0.02 N(0, 1)."""
    def special(name, leaf, t, z):
        return z if leaf == "reattn_weights" else vit_tokens(name, leaf, t, z)
    return seeded_weights(model.state_dict(), seed, special)


def inputs(case: str):
    cfg, _, B = CASES[case]
    return image_inputs(case, B, 3, cfg["image_size"], cfg["image_size"], cfg["num_classes"])
