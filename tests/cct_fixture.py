"""Weights, inputs and cases of the CCT fixture (tests/golden/cct_small.npz), rebuilt from seeds on both sides.

tests/golden/gen_golden_cct.py loads these into the reference's cct.py modules and stores what the reference computes (logits,
CE loss, the gradient of every parameter), the module trees, a seeded-init record and the keep masks the reference drew in the
dropout case; the tests load the same tensors into the HIP modules and into tests/cct_ref.py.  Seeds, the weight recipe,
packing and gradient sampling are port_fixture's.
"""
import numpy as np
import torch

from port_fixture import (_gen, grad_index, grad_sample, image_inputs, pack, pack_grads, pack_tree, seeded_weights,  # noqa: F401
                          unpack, unpack_grads, unpack_tree)

BASE = dict(img_size=16, embedding_dim=64, n_input_channels=3, n_conv_layers=1, kernel_size=3, stride=1, padding=1, num_layers=2,
            num_heads=2, mlp_ratio=2, num_classes=10, stochastic_depth_rate=0.0)
CLS = dict(seq_pool=False, embedding_dim=64, num_layers=2, num_heads=2, mlp_ratio=2, num_classes=10, dropout_rate=0.0,
           stochastic_depth_rate=0.0, positional_embedding="learnable", sequence_length=12)
# name -> (model config, robust, train, batch, attention dropout); "cls" is a bare TransformerClassifier on given tokens
CASES = {
    "s_eval": (BASE, False, False, 3, 0.0),                                # 16 px, 3 x 3 s1 p1, one conv layer -> 8 x 8 = 64 tokens
    "s_train": (BASE, False, True, 3, 0.0),
    "k7x2": (dict(BASE, img_size=30, kernel_size=7, stride=2, padding=3, n_conv_layers=2), False, True, 2, 0.0),   # planes 30 -> 15 -> 8 -> 4 -> 2
    "rect": (dict(BASE, img_size=(16, 24)), False, True, 2, 0.0),          # 8 x 12 tokens
    "learn": (dict(BASE, positional_embedding="learnable"), False, True, 2, 0.0),
    "nopos": (dict(BASE, positional_embedding="none"), False, True, 2, 0.0),
    "dh64": (dict(BASE, embedding_dim=128), False, True, 2, 0.0),          # head dim 64: single-pass attention
    "r_fused": (dict(BASE, embedding_dim=128), True, True, 2, 0.0),        # fused Sinkhorn
    "r_comp": (BASE, True, True, 2, 0.0),                                  # Sinkhorn at head dim 32: the composed path
    "drop": (dict(BASE, stochastic_depth_rate=0.5), False, True, 4, 0.1),  # drop path (layer 2: p = 0.5) + attention dropout
    "cls": (CLS, False, True, 3, 0.0),
    "g224": (dict(BASE, img_size=224, kernel_size=7, stride=2, padding=3, num_layers=1), False, True, 1, 0.0),   # 56 x 56 = 3136 tokens
}
# seeded init (torch.manual_seed(0)) of one full-size configuration: cct_7 with a 3 x 3 tokenizer at 32 px, 100 classes
FULL = dict(img_size=32, n_conv_layers=1, kernel_size=3, num_classes=100)
FULL_BUILDER = "cct_7"


def build(module, case: str, reference: bool = False, sinkhorn_forward=None):
    """The case's model from `module` (the reference's cct or noise_robust_vit_amd.cct).  The reference has no `robust` and no
    `attention_dropout` argument on CCT: there every Attention gets `attn_drop.p` set, and for the robust cases its forward
    replaced with `sinkhorn_forward` (softmax followed by utils.SinkhornAttention's normalisation)."""
    cfg, robust, train, _, pa = CASES[case]
    if case == "cls":
        m = module.TransformerClassifier(**cfg, attention_dropout=pa) if reference else \
            module.TransformerClassifier(**cfg, attention_dropout=pa, robust=robust)
        blocks = m.blocks
    elif reference:
        m = module.CCT(**cfg)
        blocks = m.classifier.blocks
    else:
        m = module.CCT(**cfg, robust=robust, attention_dropout=pa)
        blocks = m.classifier.blocks
    if reference:
        for blk in blocks:
            blk.self_attn.attn_drop.p = pa
            if robust:
                blk.self_attn.forward = sinkhorn_forward.__get__(blk.self_attn)
    return m.train(train)


def classifier_of(model):
    return getattr(model, "classifier", model)


def weights(model, seed: int) -> dict:
    """Linear / Conv2d weights ~ N(0, 1/fan_in); LayerNorm weights 1 + 0.1 N(0, 1); class_emb 0.5 N(0, 1); a learnable
    positional_emb 0.2 N(0, 1), the frozen sine table as constructed; biases 0.02 N(0, 1)."""
    params = dict(model.named_parameters())

    def special(name, leaf, t, z):
        if leaf == "class_emb":
            return 0.5 * z
        if leaf == "positional_emb":
            return 0.2 * z if params[name].requires_grad else t.detach().clone()
    return seeded_weights(model.state_dict(), seed, special)


def inputs(case: str):
    cfg, _, _, B, _ = CASES[case]
    if case == "cls":                                                       # tokens, not an image
        g = _gen(17, "inputs." + case)
        x = torch.randn(B, cfg["sequence_length"], cfg["embedding_dim"], generator=g)
        return x, torch.randint(0, cfg["num_classes"], (B,), generator=g)
    h, w = cfg["img_size"] if isinstance(cfg["img_size"], tuple) else (cfg["img_size"],) * 2
    return image_inputs(case, B, cfg["n_input_channels"], h, w, cfg["num_classes"])


# ---- the keep masks of the dropout case -----------------------------------------------------------
def pack_masks(out: dict, case: str, attn: list, path: dict) -> None:
    """attn: per layer a bool [B, H, N, N]; path: layer -> bool [calls, B] (layers whose drop path draws)."""
    for i, m in enumerate(attn):
        out[f"{case}.attn_keep.{i}"] = np.packbits(m.numpy().astype(np.uint8).reshape(-1))
        out[f"{case}.attn_keep.{i}.shape"] = np.array(m.shape, dtype=np.int64)
    for i, k in path.items():
        out[f"{case}.path_keep.{i}"] = k.numpy().astype(np.uint8)


def unpack_masks(fx, case: str, layers: int) -> dict:
    """{"attn": [uint8 [B, H, N, N] per layer], "path": {layer: uint8 [calls, B]}}"""
    attn, path = [], {}
    for i in range(layers):
        shape = tuple(int(d) for d in fx[f"{case}.attn_keep.{i}.shape"])
        bits = np.unpackbits(fx[f"{case}.attn_keep.{i}"])[:int(np.prod(shape))]
        attn.append(torch.from_numpy(bits.reshape(shape).copy()))
        if f"{case}.path_keep.{i}" in fx:
            path[i] = torch.from_numpy(fx[f"{case}.path_keep.{i}"].copy())
    return {"attn": attn, "path": path}


def inject_masks(model, masks: dict) -> None:
    """Make the HIP model use the recorded masks: BlockMeta.mask_source for the attention weights (site -(2 + layer)),
    DropPath.keep_source for the drop path (calls in order: attention branch, MLP branch)."""
    for i, blk in enumerate(classifier_of(model).blocks):
        blk._meta.mask_source = lambda site, shape, m=masks["attn"]: m[-site - 2].to(torch.uint8).reshape(shape)
        if i in masks["path"]:
            calls = iter(masks["path"][i].float())
            blk.drop_path.keep_source = lambda batch, device, it=calls: next(it)
