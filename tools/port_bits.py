#!/usr/bin/env python3
"""Bit fingerprints of one training step of the model ports, for comparing two trees that run the same libnrv_hip.so (a
host-code refactor against its parent commit).

    python tools/port_bits.py --root <tree> --out bits.json [--only CASE ...] [--runs 2]
    python tools/port_bits.py --diff parent.json new.json

Every case builds a small model (the configurations of tests/*_fixture.py, B = 3, training mode) from the package under --root
with torch.manual_seed(0), moves every parameter off its initial value by seeded noise (0.05 N(0, 1): no zero-initialised
batch-norm weight or 1e-4 layer scale hides a branch), runs forward + cross-entropy + backward `--runs` times and writes sha256,
shape and dtype of the logits and of every parameter gradient of the first run, and whether the reruns gave the same bits.
"""
import argparse
import hashlib
import json
import os
import sys
from functools import partial

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tests"))                     # the fixtures' configurations, from this tree

B = 3


def _cases():
    """name -> (image side, classes, builder); the package is imported inside the builders, after --root is on sys.path."""
    import cait_fixture as CF, cct_fixture as CC, deepvit_fixture as DF, levit_fixture as LF, patchconvnet_fixture as PF  # noqa: E401
    import pit_fixture as PI, rvt_fixture as RF, swin_fixture as SF, t2t_fixture as TF, twins_fixture as TW             # noqa: E401
    from torch import nn

    def levit():
        from noise_robust_vit_amd import levit as M
        cfg = dict(LF.SMALL, down_ops=[list(d) for d in LF.SMALL["down_ops"]])
        return M.LeViT(**cfg, attention_activation=nn.Hardswish, mlp_activation=nn.Hardswish,
                       hybrid_backbone=M.b16(cfg["embed_dim"][0], activation=nn.Hardswish))

    def pcn():
        from noise_robust_vit_amd import patch_convnet as M
        return M.PatchConvnet(**PF.SMALL, norm_layer=partial(nn.LayerNorm, eps=1e-6))

    def cct(**kw):
        from noise_robust_vit_amd import cct as M
        return M.CCT(**dict(CC.BASE, n_conv_layers=2, **kw), attention_dropout=0.0)

    def vit(side, patch):
        from noise_robust_vit_amd.vit import VisionTransformer
        return VisionTransformer(image_size=side, patch_size=patch, num_layers=1, num_heads=2, hidden_dim=64, mlp_dim=128, num_classes=10)

    def port(module, cls, cfg, **kw):
        import importlib
        return getattr(importlib.import_module("noise_robust_vit_amd." + module), cls)(**dict(cfg, **kw))

    return {
        # conv stems
        "levit_small": (112, 10, levit),                                                # four BN convs
        "pcn_embed64": (64, 10, pcn),
        "cct_k7x2": (30, 10, partial(cct, img_size=30, kernel_size=7, stride=2, padding=3)),   # two conv layers: the NHWC unfold and
        "cct_k3x2": (16, 10, partial(cct)),                                             # the fold of layer 1, at kernel 7 and at kernel 3
        # padded_images, both branches in each caller
        "vit_p14": (28, 10, partial(vit, 28, 14)),                                      # 588 -> 592
        "vit_p16": (32, 10, partial(vit, 32, 16)),
        "pit_p14": (42, 10, partial(port, "pit", "PiT", PI.BASE, image_size=42, patch_size=14)),      # stride 7
        "pit_p16": (48, 10, partial(port, "pit", "PiT", PI.BASE, image_size=48, patch_size=16)),      # stride 8
        "twins_p2": (56, 10, partial(port, "twins_svt", "TwinsSVT", TW.BASE)),          # stage 1: 12 -> 16
        "twins_p4": (112, 10, partial(port, "twins_svt", "TwinsSVT", TW.BASE, s1_patch_size=4)),
        # holders, guards and constants
        "cait_softmax": (64, 10, partial(port, "cait", "CaiT", CF.SMALL)),
        "cait_robust": (64, 10, partial(port, "cait", "CaiT", CF.SMALL, robust=True)),
        "deepvit_softmax": (64, 10, partial(port, "deepvit", "DeepViT", DF.SMALL)),
        "deepvit_robust": (64, 10, partial(port, "deepvit", "DeepViT", DF.SMALL, robust=True)),
        "rvt_conv": (48, 10, partial(port, "rvt", "RvT", RF.SMALL)),
        "rvt_noconv": (48, 10, partial(port, "rvt", "RvT", RF.SMALL, use_ds_conv=False)),
        "t2t_small": (64, 10, partial(port, "t2t", "T2TViT", TF.SMALL)),
        "swin_pad64": (64, 10, partial(port, "swin", "SwinTransformer", SF.MODEL)),    # 16 x 16 and 8 x 8 maps, both padded
    }


def _digest(t):
    t = t.detach().contiguous().cpu()
    return [hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest(), list(t.shape), str(t.dtype)]


def run_case(name, side, classes, make, runs):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = make()
    g = torch.Generator().manual_seed(1234)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    x = torch.randn(B, 3, side, side, generator=g).to(dev)
    y = torch.randint(0, classes, (B,), generator=g).to(dev)
    model = model.to(dev).train()
    out = []
    for _ in range(runs):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(1)
        logits = model(x)
        torch.nn.functional.cross_entropy(logits, y).backward()
        torch.cuda.synchronize()
        rec = {"logits": _digest(logits)}
        for k, p in model.named_parameters():
            if p.grad is not None:
                rec["grad." + k] = _digest(p.grad)
        out.append(rec)
    return {"tensors": out[0], "rerun_same": all(r == out[0] for r in out[1:])}


def diff(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    total = bad = 0
    for case in a:
        ta, tb = a[case]["tensors"], b[case]["tensors"]
        assert list(ta) == list(tb), case
        d = sum(ta[k] != tb[k] for k in ta)
        total, bad = total + len(ta), bad + d
        print(f"  {case:18s} {len(ta):4d} tensors {d:4d} different   rerun gave the same bits: "
              f"{'yes' if a[case]['rerun_same'] else 'NO'} / {'yes' if b[case]['rerun_same'] else 'NO'}")
    print(f"  {total} tensors compared, {bad} different")
    return bad == 0 and all(v["rerun_same"] for v in list(a.values()) + list(b.values()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--out")
    ap.add_argument("--only", nargs="+")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--diff", nargs=2)
    a = ap.parse_args()
    if a.diff:
        sys.exit(0 if diff(*a.diff) else 1)
    sys.path.insert(0, os.path.abspath(a.root))
    import noise_robust_vit_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(noise_robust_vit_amd.__file__))) == os.path.abspath(a.root)
    cases = _cases()
    res = {}
    for name in a.only or cases:
        res[name] = run_case(name, *cases[name], a.runs)
        print(name, len(res[name]["tensors"]), "tensors, rerun same:", res[name]["rerun_same"], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
