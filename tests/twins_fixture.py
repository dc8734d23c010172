"""Weights, inputs and cases of the Twins-SVT fixture (tests/golden/twins_small.npz), rebuilt from seeds on both sides.

tests/golden/gen_golden_twins.py loads these into the reference's twins_svt.py modules and stores what the reference computes
(logits, CE loss, the gradient of every parameter) plus the module trees; the tests load the same tensors into the HIP modules
and into tests/twins_ref.py.  Seeds, packing and gradient sampling are port_fixture's; the weight recipe is its own (the
LayerNorm gains `g` are rank 4 and the rule goes by leaf name, not by rank).

The reference's Twins-SVT has no `attend` module to swap, so the robust cases have no fixture: they are compared against the
restatement only (ROBUST_CASES).
"""
import torch

from port_fixture import (_gen, grad_index, grad_sample, image_inputs, pack, pack_grads, pack_tree, unpack, unpack_grads,  # noqa: F401
                          unpack_tree)

# 56 px: maps 28 / 14 / 7 / 7; global attention 784 x 16, 196 x 49, 49 x 1, 49 x 49 (queries x keys)
BASE = dict(num_classes=10,
            s1_emb_dim=16, s1_patch_size=2, s1_local_patch_size=7, s1_global_k=7, s1_depth=1,
            s2_emb_dim=24, s2_patch_size=2, s2_local_patch_size=7, s2_global_k=2, s2_depth=1,
            s3_emb_dim=32, s3_patch_size=2, s3_local_patch_size=7, s3_global_k=7, s3_depth=2,
            s4_emb_dim=40, s4_patch_size=1, s4_local_patch_size=7, s4_global_k=1, s4_depth=1)
# 224 px with the default patch sizes and k: maps 56 / 28 / 14 / 7; global attention 3136 x 64, 784 x 16, 196 x 4, 49 x 1
G224 = dict(num_classes=10, s1_emb_dim=8, s1_depth=1, s2_emb_dim=8, s2_depth=1, s3_emb_dim=16, s3_depth=1, s4_emb_dim=16, s4_depth=1)
# name -> (model config, image side, train, batch)
CASES = {
    "s_train": (BASE, 56, True, 2),
    "s_eval": (BASE, 56, False, 2),
    "d1": (dict(BASE, s3_depth=1), 56, True, 2),          # one layer per stage behind the PEG
    "g224": (G224, 224, True, 1),                         # the real grid at a tiny width
}
# batch 3: its seeded labels give a loss of 9.7 in the restatement (batch 2 happens to draw a loss of 0.06, which scales every
# gradient down and puts the smallest to_q gradient below the tests' vanishing threshold of 1e-4)
ROBUST_CASES = {"r_train": (BASE, 56, True, 3)}
SMALL = BASE
# seeded init (torch.manual_seed(0)) of the default-argument model
FULL = dict(num_classes=100)


def build(module, case: str, robust: bool = False):
    """The case's model from `module` (the reference's twins_svt or noise_robust_vit_amd.twins_svt)."""
    cfg, _, train, _ = {**CASES, **ROBUST_CASES}[case]
    m = module.TwinsSVT(**cfg, robust=True) if robust else module.TwinsSVT(**cfg)
    return m.train(train)


def weights(model, seed: int) -> dict:
    """Conv2d / Linear weights ~ N(0, 1/fan_in); the LayerNorm gains `g` 1 + 0.1 N(0, 1); `b` and the biases 0.02 N(0, 1)."""
    out = {}
    for name, t in model.state_dict().items():
        z = torch.randn(tuple(t.shape), generator=_gen(seed, name))
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "g":
            z = 1.0 + 0.1 * z
        elif leaf == "weight":
            z = z / t[0].numel() ** 0.5
        else:
            z = 0.02 * z
        out[name] = z
    return out


def inputs(case: str):
    cfg, size, _, B = {**CASES, **ROBUST_CASES}[case]
    return image_inputs(case, B, 3, size, size, cfg["num_classes"])
