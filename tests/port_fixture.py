"""What every model port's fixture (tests/X_fixture.py, tests/golden/X_small.npz) shares: the per-tensor seeded generator, the
weight recipe, the image batch, the float16 packing and the gradient sampling.

Every tensor comes from a CPU torch.Generator seeded from the case seed and the tensor's name, so it depends neither on module
construction order nor on which other tensors are drawn: skipping an entry cannot move another one.  Stored outputs are float16
relative to their max-abs (`pack` / `unpack`): 2^-11 relative per element, far below the parity checks, at a quarter of the fp32
bytes.  A gradient of more than GRAD_SAMPLE elements is stored at GRAD_SAMPLE fixed positions drawn from a generator seeded by
the parameter's name (`grad_index`): the rel-L2 of a difference over 1024 uniformly drawn positions estimates the full tensor's
within a few per cent, and every parameter is still checked.
"""
import zlib

import numpy as np
import torch

GRAD_SAMPLE = 1024


def _gen(seed: int, name: str) -> torch.Generator:
    return torch.Generator().manual_seed(seed * 1_000_003 + zlib.crc32(name.encode()))


def seeded_weights(named_tensors, seed: int, special=None) -> dict:
    """One tensor per float entry of `named_tensors` (a state_dict; non-float buffers are left out), from z ~ N(0, 1) drawn for
    that name: rank >= 2 (Linear, Conv2d, tables) z / sqrt(fan_in), a leaf called `weight` (LayerNorm) 1 + 0.1 z, anything else
    (biases) 0.02 z.  `special(name, leaf, t, z)` may return the tensor of one entry instead, or None for the rule."""
    out = {}
    for name, t in named_tensors.items():
        if not t.is_floating_point():
            continue
        z = torch.randn(tuple(t.shape), generator=_gen(seed, name))
        leaf = name.rsplit(".", 1)[-1]
        own = special(name, leaf, t, z) if special is not None else None
        if own is not None:
            z = own
        elif t.dim() >= 2:
            z = z / t[0].numel() ** 0.5
        elif leaf == "weight":
            z = 1.0 + 0.1 * z
        else:
            z = 0.02 * z
        out[name] = z
    return out


def vit_tokens(name, leaf, t, z):
    """The `special` of the ViT-shaped ports, alone or as the last resort of their own: cls_token 0.5 z, pos_embedding 0.2 z."""
    scale = {"cls_token": 0.5, "pos_embedding": 0.2}.get(name)
    return None if scale is None else scale * z


def image_inputs(case: str, B: int, channels: int, H: int, W: int, num_classes: int):
    """The case's image batch and labels, both from the generator of "inputs.<case>"."""
    g = _gen(17, "inputs." + case)
    img = torch.randn(B, channels, H, W, generator=g)
    y = torch.randint(0, num_classes, (B,), generator=g)
    return img, y


def pack(out: dict, key: str, t) -> None:
    a = np.asarray(t.detach().float().numpy() if torch.is_tensor(t) else t, dtype=np.float32)
    s = float(np.abs(a).max()) or 1.0
    out[key] = (a / s).astype(np.float16)
    out[key + ".scale"] = np.float32(s)


def unpack(fx, key: str) -> torch.Tensor:
    return torch.from_numpy(fx[key].astype(np.float32) * fx[key + ".scale"])


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
