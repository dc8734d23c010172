"""Swin Transformer on the HIP path: parity with the reference's fixture (logits, loss, every gradient), full swin_t at
224 px against the fp32 restatement (softmax and Sinkhorn), stochastic depth with injected keep vectors, a Trainer step,
and a one-rank RCCL GradReducer step that equals the plain step bit for bit."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import swin_fixture as SF
import swin_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel_l2(a, b):
    a, b = a.detach().float().cpu(), torch.as_tensor(b).detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _rel_max(a, b):
    a, b = a.detach().float().cpu(), torch.as_tensor(b).detach().float().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


def _small(case, dev, **kw):
    from noise_robust_vit_amd.swin import SwinTransformer
    m = SwinTransformer(**dict(SF.model_kwargs(case), **kw))
    m.load_state_dict(SF.weights(m.state_dict(), seed=3), strict=False)
    return m.to(dev).train()


@pytest.mark.parametrize("case", list(SF.CASES))
def test_swin_matches_reference_fixture(dev, golden_dir, case):
    fx = np.load(os.path.join(golden_dir, "swin_small.npz"))
    m = _small(case, dev)
    img, y = SF.inputs(case)
    logits = m(img.to(dev))
    loss = torch.nn.functional.cross_entropy(logits, y.to(dev))
    loss.backward()
    # these models are small (embed 32) and their fixture table is drawn at std 1 / sqrt(heads): peaked windows, where the
    # bf16 rounding of q and k moves the scores most; measured on MI355X: logits up to 1.14e-2 (Sinkhorn)
    assert _rel_max(logits, SF.unpack(fx, case + ".logits")) < 2e-2
    assert abs(loss.item() - float(fx[case + ".loss"])) < 2e-2
    worst, tables = [], []
    ref = SF.unpack_grads(fx, case)
    for k, p in m.named_parameters():
        e = (_rel_l2(SF.grad_sample(k, p.grad), ref[k]), k)
        (tables if k.endswith("relative_position_bias_table") else worst).append(e)
    # measured on MI355X (softmax, 56 px): LayerNorm-weight gradients up to 1.002e-2
    assert max(worst)[0] <= 2e-2, sorted(worst)[-3:]
    # the table gradient sums dS over every window of a relative offset; its rows sum to zero, so the bf16 rounding of q, k, v
    # and dO (which the kernel tests take as exact operands) cancels less there: measured 1.5e-2 (softmax, 56 px)
    assert max(tables)[0] <= 4e-2, sorted(tables)[-3:]


@pytest.mark.parametrize("robust", [False, True])
def test_swin_t_224_against_fp32(dev, robust):
    from noise_robust_vit_amd import swin_t
    torch.manual_seed(0)
    m = swin_t(num_classes=100, robust=robust)
    for mod in m.modules():                    # the reference's swin_t fixes p = 0.2; compare deterministic steps
        if hasattr(mod, "keep_source"):
            mod.p = 0.0
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(11)
    img = torch.randn(8, 3, 224, 224, generator=g)
    y = torch.randint(0, 100, (8,), generator=g)
    m = m.to(dev).train()
    logits = m(img.to(dev))
    loss = torch.nn.functional.cross_entropy(logits, y.to(dev))
    loss.backward()
    cfg = dict(embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=[7, 7], patch_size=[4, 4], robust=robust)
    rl, rloss, rg = swin_ref.loss_and_grads({k: v.to(dev) for k, v in sd.items()}, cfg, img.to(dev), y.to(dev))
    assert _rel_max(logits, rl) < 3e-2
    assert abs(loss.item() - rloss.item()) < 2e-2
    errs = sorted((_rel_l2(p.grad, rg[k]), k) for k, p in m.named_parameters())
    assert errs[-1][0] < 5e-2, errs[-3:]


def test_stochastic_depth_with_injected_keeps(dev):
    case = "p64"
    m = _small(case, dev, stochastic_depth_prob=0.6)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    B = SF.CASES[case][3]
    keeps, probs = {}, {}
    gen = torch.Generator().manual_seed(21)
    for s in (1, 3):
        for i, blk in enumerate(m.features[s]):
            name = f"features.{s}.{i}"
            ks = [(torch.rand(B, generator=gen) > 0.5).float() for _ in range(2)]
            ks[0][0], ks[1][1] = 1.0, 0.0
            keeps[name], probs[name] = ks, blk.stochastic_depth.p
            it = iter(ks)
            blk.stochastic_depth.keep_source = lambda b, d, it=it: next(it)
    img, y = SF.inputs(case)
    logits = m(img.to(dev))
    loss = torch.nn.functional.cross_entropy(logits, y.to(dev))
    loss.backward()
    kw = dict(keeps={k: [t.to(dev) for t in v] for k, v in keeps.items()}, sd_probs={k: v for k, v in probs.items() if v > 0})
    kw["keeps"] = {k: v for k, v in kw["keeps"].items() if k in kw["sd_probs"]}
    rl, rloss, rg = swin_ref.loss_and_grads({k: v.to(dev) for k, v in sd.items()}, SF.model_kwargs(case), img.to(dev), y.to(dev), **kw)
    assert _rel_max(logits, rl) < 2e-2
    errs = sorted((_rel_l2(p.grad, rg[k]), k) for k, p in m.named_parameters()
                  if rg[k].norm() > 0 and not k.endswith("relative_position_bias_table"))
    assert errs[-1][0] < 2e-2, errs[-3:]
    tables = sorted((_rel_l2(p.grad, rg[k]), k) for k, p in m.named_parameters() if k.endswith("relative_position_bias_table"))
    assert tables[-1][0] < 4e-2, tables[-3:]


def test_trainer_step_runs(dev):
    from noise_robust_vit_amd.train import Trainer, TrainConfig
    m = _small("s56", dev, stochastic_depth_prob=0.2)
    tr = Trainer(m, TrainConfig(lr=1e-3, grad_max_norm=1.0))
    img, y = SF.inputs("s56")
    losses = [tr.step(img.to(dev), y.to(dev)).item() for _ in range(3)]
    assert all(np.isfinite(losses))


RCCL_WORKER = r"""
import os, sys, json, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import torch.distributed as dist
import swin_fixture as SF
from noise_robust_vit_amd.swin import SwinTransformer
from noise_robust_vit_amd.parallel import GradReducer
from noise_robust_vit_amd.train import Trainer, TrainConfig
use_rccl = sys.argv[3] == "rccl"
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
if use_rccl:
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
m = SwinTransformer(**SF.model_kwargs("p64"))
m.load_state_dict(SF.weights(m.state_dict(), seed=3), strict=False)
m = m.to(dev).train()
red = GradReducer(m, 1, bucket_mib=0.05, force_collectives=True) if use_rccl else None
tr = Trainer(m, TrainConfig(lr=1e-3, grad_max_norm=5.0), red)
img, y = SF.inputs("p64")
losses = [tr.step(img.to(dev), y.to(dev)).item() for _ in range(2)]
torch.cuda.synchronize()
out = {"loss": losses, "nbuckets": len(red.buckets) if red else 0}
for k, p in m.named_parameters():
    out["w." + k] = p.detach().float().cpu().reshape(-1).tolist()[:256]
json.dump(out, open(sys.argv[2], "w"))
if use_rccl:
    dist.barrier(); dist.destroy_process_group()
"""


def test_rccl_grad_reducer_step_is_bit_equal(dev, tmp_path):
    import json
    script = tmp_path / "swin_rccl_worker.py"
    script.write_text(RCCL_WORKER)
    outs = {}
    for mode in ("plain", "rccl"):
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1",
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        out = tmp_path / f"{mode}.json"
        r = subprocess.run([sys.executable, str(script), ROOT, str(out), mode], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        outs[mode] = json.load(open(out))
    a, b = outs["plain"], outs["rccl"]
    assert b["nbuckets"] >= 1
    assert a["loss"] == b["loss"]
    for k in a:
        if k.startswith("w."):
            assert a[k] == b[k], k
