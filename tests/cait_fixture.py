"""Weights, inputs and cases of the CaiT fixture (tests/golden/cait_small.npz), rebuilt from seeds on both sides.

tests/golden/gen_golden_cait.py loads these into the reference's cait.py modules and stores what the reference computes (logits,
CE loss, the gradient of every parameter) plus the module trees; the tests load the same tensors into the HIP modules and into
tests/cait_ref.py.  Seeds, the weight recipe, packing and gradient sampling are port_fixture's.
"""
import torch

from port_fixture import (_gen, grad_index, grad_sample, image_inputs, pack, pack_grads, pack_tree, seeded_weights,  # noqa: F401
                          unpack, unpack_grads, unpack_tree, vit_tokens)

SMALL = dict(image_size=64, patch_size=16, num_classes=10, dim=64, depth=2, cls_depth=2, heads=2, mlp_dim=128, dim_head=32)
SMALL_NPARAMS = 184746
# name -> (model config, robust, train, batch)
CASES = {
    "s_train": (SMALL, False, True, 4),                                  # 4x4 grid: 16 / 17 keys
    "s_eval": (SMALL, False, False, 4),
    "r_train": (SMALL, True, True, 4),                                   # Sinkhorn in both transformers
    "h4": (dict(SMALL, heads=4, dim_head=48), False, True, 3),           # the paper's head dim
    "g14": (dict(SMALL, image_size=224, depth=1, cls_depth=1), False, True, 2),      # 14x14 grid: 196 / 197 keys
}
# seeded init (torch.manual_seed(0)) of one full-size configuration: XXS24 at 224 px, 100 classes
FULL = dict(image_size=224, patch_size=16, num_classes=100, dim=192, depth=24, cls_depth=2, heads=4, mlp_dim=768, dim_head=48)
# dropout_layers draws: (torch seed, random seed, layers, probability)
DRAWS = ((0, 0, 24, 0.1), (1, 2, 24, 0.5), (3, 4, 2, 0.5), (5, 6, 3, 0.999), (7, 8, 12, 0.9))


def build(module, case: str):
    """The case's model from `module` (the reference's cait or noise_robust_vit_amd.cait).  The reference's CaiT has no `robust`
    argument: there the two transformers are rebuilt through Transformer(robust=True)."""
    cfg, robust, train, _ = CASES[case]
    try:
        m = module.CaiT(**cfg, robust=robust)
    except TypeError:
        m = module.CaiT(**cfg)
        if robust:
            args = (cfg["dim"], cfg["heads"], cfg["dim_head"], cfg["mlp_dim"])
            m.patch_transformer = module.Transformer(args[0], cfg["depth"], *args[1:], robust=True)
            m.cls_transformer = module.Transformer(args[0], cfg["cls_depth"], *args[1:], robust=True)
    return m.train(train)


def weights(model, seed: int) -> dict:
    """Linear weights and the head-mixing matrices ~ N(0, 1/fan_in) (1/H for the [H, H] matrices); LayerNorm weights
    1 + 0.1 N(0, 1); LayerScale 0.1 (1 + 0.1 N(0, 1)) so that no branch is hidden; cls_token 0.5 N(0, 1); pos_embedding
    0.2 N(0, 1); biases 0.02 N(0, 1)."""
    def special(name, leaf, t, z):
        return 0.1 * (1.0 + 0.1 * z) if leaf == "scale" else vit_tokens(name, leaf, t, z)
    return seeded_weights(model.state_dict(), seed, special)


def inputs(case: str):
    cfg, _, _, B = CASES[case]
    return image_inputs(case, B, 3, cfg["image_size"], cfg["image_size"], cfg["num_classes"])


def draw(module, ts: int, rs: int, n: int, p: float):
    """The kept layer indices of one dropout_layers call under the given seeds."""
    import random
    torch.manual_seed(ts)
    random.seed(rs)
    return [int(i) for i in module.dropout_layers(list(range(n)), p)]
