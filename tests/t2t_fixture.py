"""Weights, inputs and cases of the T2T-ViT fixture (tests/golden/t2t_small.npz), rebuilt from seeds on both sides.

tests/golden/gen_golden_t2t.py loads these into the reference's t2t.py modules and stores what the reference computes (logits,
CE loss, the gradient of every parameter) plus the module trees; the tests load the same tensors into the HIP modules and into
tests/t2t_ref.py.  Seeds, the weight recipe, packing and gradient sampling are port_fixture's.
"""
from port_fixture import (_gen, grad_index, grad_sample, image_inputs, pack, pack_grads, pack_tree, seeded_weights,  # noqa: F401
                          unpack, unpack_grads, unpack_tree, vit_tokens)

SMALL = dict(image_size=64, num_classes=10, dim=64, depth=2, heads=2, mlp_dim=128, dim_head=32)
# name -> (model config, robust, train, batch)
CASES = {
    "s_train": (SMALL, False, True, 3),                                  # grids 16 / 8 / 4, widths 147 / 1323 / 11907
    "s_eval": (SMALL, False, False, 3),
    # pool="mean" on two splits of a 3-channel image: width 27 stored as 32, the stage runs nrv_attn_fwd's head dim 32 (1024 tokens)
    "s_mean": (dict(SMALL, pool="mean", depth=1, t2t_layers=((3, 2), (3, 2))), False, True, 2),
    "c1": (dict(SMALL, channels=1, depth=1, t2t_layers=((3, 2), (3, 2))), False, True, 3),      # widths 9 / 81: one stage, below 16
    "g224": (dict(SMALL, image_size=224, depth=1), False, True, 1),      # 3136 / 784 / 196 tokens: the real stage-1 shape
    "r_train": (dict(SMALL, depth=1, t2t_layers=((7, 4), (3, 2))), True, True, 3),     # Sinkhorn in the backbone, 65 keys
}
# seeded init (torch.manual_seed(0)) of one full-size configuration: T2T-ViT-14-like at 224 px, 100 classes
FULL = dict(image_size=224, num_classes=100, dim=384, depth=14, heads=6, mlp_dim=1152)


def build(module, case: str, sinkhorn=None):
    """The case's model from `module` (the reference's t2t or noise_robust_vit_amd.t2t).  The reference's T2TViT has no
    `robust` argument: there `attend` of the backbone's Attention layers is replaced with `sinkhorn()` (utils.SinkhornAttention)."""
    cfg, robust, train, _ = CASES[case]
    try:
        m = module.T2TViT(**cfg, robust=robust)
    except TypeError:
        m = module.T2TViT(**cfg)
        if robust:
            for attn, _ in m.transformer.layers:
                attn.attend = sinkhorn()
    return m.train(train)


def weights(model, seed: int) -> dict:
    """Linear weights ~ N(0, 1/fan_in); LayerNorm weights 1 + 0.1 N(0, 1); cls_token 0.5 N(0, 1); pos_embedding 0.2 N(0, 1);
    biases 0.02 N(0, 1)."""
    return seeded_weights(model.state_dict(), seed, vit_tokens)


def inputs(case: str):
    cfg, _, _, B = CASES[case]
    return image_inputs(case, B, cfg.get("channels", 3), cfg["image_size"], cfg["image_size"], cfg["num_classes"])
