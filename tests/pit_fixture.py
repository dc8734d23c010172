"""Weights, inputs and cases of the PiT fixture (tests/golden/pit_small.npz), rebuilt from seeds on both sides.

tests/golden/gen_golden_pit.py loads these into the reference's pit.py modules and stores what the reference computes (logits,
CE loss, the gradient of every parameter) plus the module trees; the tests load the same tensors into the HIP modules and into
tests/pit_ref.py.  Seeds, the weight recipe, packing and gradient sampling are port_fixture's.
"""
from port_fixture import (_gen, grad_index, grad_sample, image_inputs, pack, pack_grads, pack_tree, seeded_weights,  # noqa: F401
                          unpack, unpack_grads, unpack_tree, vit_tokens)

BASE = dict(image_size=32, patch_size=8, num_classes=10, dim=32, depth=(1, 1, 1), heads=(2, 4, 8), dim_head=32, mlp_dim=64)
TWO = dict(BASE, depth=(1, 1), heads=2)
# name -> (model config, robust, train, batch)
CASES = {
    "s_train": (BASE, False, True, 3),                                    # planes 7 x 7 -> 4 x 4 -> 2 x 2: odd and even pooling
    "s_eval": (BASE, False, False, 3),
    "d21": (dict(BASE, depth=(2, 1), heads=2), False, True, 2),           # two layers in a stage, an int `heads`
    "d1": (dict(BASE, depth=(1,), heads=2), False, True, 2),              # one stage: no Pool
    "p14": (dict(BASE, image_size=42, patch_size=14), False, True, 2),    # 588 features padded to 592; planes 5 -> 3 -> 2
    "dh64": (dict(TWO, dim_head=64), False, True, 2),                     # single-pass attention
    "r_train": (dict(TWO, dim_head=64), True, True, 2),                   # fused Sinkhorn
    "r_comp": (TWO, True, True, 2),                                       # Sinkhorn at head dim 32: the composed path
    "g224": (dict(BASE, image_size=224, patch_size=14), False, True, 1),  # the real grid: 962 -> 257 -> 65 tokens
}
SMALL = BASE
# seeded init (torch.manual_seed(0)) of one full-size configuration: PiT-S-like at 224 px, 100 classes
FULL = dict(image_size=224, patch_size=14, num_classes=100, dim=64, depth=(2, 6, 4), heads=(2, 4, 8), dim_head=32, mlp_dim=256)


def build(module, case: str, sinkhorn=None):
    """The case's model from `module` (the reference's pit or noise_robust_vit_amd.pit).  The reference's PiT has no `robust`
    argument: there `attend` of every Attention is replaced with `sinkhorn()` (utils.SinkhornAttention)."""
    cfg, robust, train, _ = CASES[case]
    try:
        m = module.PiT(**cfg, robust=robust)
    except TypeError:
        m = module.PiT(**cfg)
        if robust:
            for stage in m.layers:
                if isinstance(stage, module.Transformer):
                    for attn, _ in stage.layers:
                        attn.fn.attend = sinkhorn()
    return m.train(train)


def weights(model, seed: int) -> dict:
    """Linear / Conv2d weights ~ N(0, 1/fan_in); LayerNorm weights 1 + 0.1 N(0, 1); cls_token 0.5 N(0, 1); pos_embedding
    0.2 N(0, 1); biases 0.02 N(0, 1)."""
    return seeded_weights(model.state_dict(), seed, vit_tokens)


def inputs(case: str):
    cfg, _, _, B = CASES[case]
    return image_inputs(case, B, cfg.get("channels", 3), cfg["image_size"], cfg["image_size"], cfg["num_classes"])
