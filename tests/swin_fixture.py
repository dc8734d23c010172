"""Weights, inputs and cases of the Swin fixture (tests/golden/swin_small.npz), rebuilt from seeds on both sides.

tests/golden/gen_golden_swin.py loads these into the reference's swin.py modules and stores what the reference computes
(logits, CE loss, the gradient of every parameter) plus the module tree; the tests load the same tensors into the HIP modules.
Every tensor comes from a CPU generator seeded from the case seed and the tensor's name (adapter_fixture's scheme and packing).

A gradient of more than GRAD_SAMPLE elements is stored at GRAD_SAMPLE fixed positions drawn from a generator seeded by the
parameter's name (`grad_index`), which keeps the fixture small: the rel-L2 of a difference over 1024 uniformly drawn positions
estimates the full tensor's within a few per cent, and every parameter is still checked.
"""
import zlib

import numpy as np
import torch

from adapter_fixture import pack, unpack  # noqa: F401  (float16-relative-to-max-abs storage)

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
GRAD_SAMPLE = 1024


def _gen(seed: int, name: str) -> torch.Generator:
    return torch.Generator().manual_seed(seed * 1_000_003 + zlib.crc32(name.encode()))


def weights(state_dict, seed: int) -> dict:
    """Float entries of a state_dict (the integer relative_position_index is left out): weights of rank >= 2 (Linear, Conv2d,
    the relative-position table) ~ N(0, 1/fan_in), LayerNorm weights 1 + 0.1 N(0, 1), biases 0.02 N(0, 1)."""
    out = {}
    for name, t in state_dict.items():
        if not t.is_floating_point():
            continue
        z = torch.randn(tuple(t.shape), generator=_gen(seed, name))
        leaf = name.rsplit(".", 1)[-1]
        if t.dim() >= 2:
            z = z / t[0].numel() ** 0.5
        elif leaf == "weight":
            z = 1.0 + 0.1 * z
        else:
            z = 0.02 * z
        out[name] = z
    return out


def inputs(case: str):
    _, H, W, B = CASES[case]
    g = _gen(17, "inputs." + case)
    img = torch.randn(B, 3, H, W, generator=g)
    y = torch.randint(0, MODEL["num_classes"], (B,), generator=g)
    return img, y


def model_kwargs(case: str) -> dict:
    return dict(MODEL, robust=CASES[case][0])


def grad_index(name: str, numel: int):
    """Flat positions of a parameter's gradient kept in the fixture (None = all of them)."""
    if numel <= GRAD_SAMPLE:
        return None
    return torch.randperm(numel, generator=_gen(5, "grad." + name))[:GRAD_SAMPLE].sort().values


def grad_sample(name: str, g: torch.Tensor) -> torch.Tensor:
    """The stored part of gradient `g` of parameter `name` (flattened)."""
    flat = g.reshape(-1)
    idx = grad_index(name, flat.numel())
    return flat if idx is None else flat[idx.to(flat.device)]


def pack_tree(out: dict, prefix: str, state_dict, values) -> None:
    """Keys, shapes ([n, 4], -1 padded) and one float64 per key (`values[key]`, NaN where absent) as three arrays."""
    keys = list(state_dict.keys())
    shapes = np.full((len(keys), 4), -1, dtype=np.int64)
    for r, k in enumerate(keys):
        shapes[r, :state_dict[k].dim()] = state_dict[k].shape
    out[prefix + ".keys"] = np.array(keys)
    out[prefix + ".shapes"] = shapes
    out[prefix + ".sums"] = np.array([float(values[k]) if k in values else np.nan for k in keys], dtype=np.float64)


def unpack_tree(fx, prefix: str) -> dict:
    """key -> (shape, value or NaN)"""
    return {k: (tuple(int(d) for d in s if d >= 0), float(v))
            for k, s, v in zip(fx[prefix + ".keys"], fx[prefix + ".shapes"], fx[prefix + ".sums"])}


def pack_grads(out: dict, prefix: str, named_grads) -> None:
    """Every parameter's stored gradient part (grad_sample), each float16 relative to its own max-abs, in one array."""
    names, parts, scales = [], [], []
    for name, g in named_grads:
        a = grad_sample(name, g.detach().float()).numpy()
        sc = float(np.abs(a).max()) or 1.0
        names.append(name); parts.append((a / sc).astype(np.float16)); scales.append(sc)
    out[prefix + ".gnames"] = np.array(names)
    out[prefix + ".g"] = np.concatenate(parts)
    out[prefix + ".glen"] = np.array([len(a) for a in parts], dtype=np.int64)
    out[prefix + ".gscale"] = np.array(scales, dtype=np.float32)


def unpack_grads(fx, prefix: str) -> dict:
    """name -> the stored (flattened, possibly sampled) gradient, fp32"""
    flat, res, off = fx[prefix + ".g"], {}, 0
    for name, n, sc in zip(fx[prefix + ".gnames"], fx[prefix + ".glen"], fx[prefix + ".gscale"]):
        res[str(name)] = torch.from_numpy(flat[off:off + int(n)].astype(np.float32) * sc)
        off += int(n)
    return res
