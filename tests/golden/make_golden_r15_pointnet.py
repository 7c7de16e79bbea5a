#!/usr/bin/env python3
"""Fixture of the PointNet network (tests/golden/reference_cpu_r15_pointnet.npz), produced by running the REFERENCE's own
models/modules/pointnet.py (on its own external_libs/pointnet2_utils/pointnet_utils.py) on CPU in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_r15_pointnet.py

Weights: tests/golden/seeded.py (seed 151), so no weight file is kept; input: two 2 048-point synthetic scans in one batch
(synth.scan_batch(2, 2048, "arch", seed=31), stored as a digest).

  params  the name:shape list of PointFirstModule({})'s floating state_dict entries, in the reference's order.
  eval    fp32 pass of PointFirstModule.eval(): every 2nd point of cls_pred (log-probabilities), and trans_feat; then a float64 pass of
          the same module (likewise), and own = max |fp32 - fp64| / (1 + |fp64|) of cls_pred (own_trans: of trans_feat), so that the
          tests can tell the reference's own fp32 noise from a discrepancy.
  train   PointFirstModule.train() (BatchNorm batch statistics; the network has no dropout) with tooth_class_loss(cls_pred, labels, 17)
          (models/tgn_loss.py:355) on seeded labels: the loss, and per parameter a strided gradient sample plus its norm.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("TGN_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from crop_cases import digest  # noqa: E402
from seeded import seeded_fill  # noqa: E402
from toothgroupnetwork_amd import synth  # noqa: E402

SEED, B, N = 151, 2, 2048


def scans():
    return synth.scan_batch(B, N, "arch", seed=31)


def labels():
    return np.random.default_rng(32).integers(-1, 16, size=(B, 1, N)).astype(np.int64)


def grad_stride(numel):
    return max(1, -(-numel // 64))          # at most 64 values


def err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / (1 + np.abs(b))))


def load():
    for name in [m for m in sys.modules if m == "external_libs" or m.startswith("external_libs.")]:
        del sys.modules[name]               # (this repository's drop-in package of the same name)
    sys.path.insert(0, REFERENCE)
    import models.modules.pointnet as RP
    import models.tgn_loss as TL
    import external_libs.pointnet2_utils.pointnet_utils as RU
    assert os.path.abspath(RU.__file__).startswith(os.path.abspath(REFERENCE)), RU.__file__
    assert RP.PointNetEncoder is RU.PointNetEncoder
    return RP, TL


def main():
    RP, TL = load()
    out = {}
    x = scans()
    out["input_digest"] = np.array(digest(x))
    feats = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1)))
    net = RP.PointFirstModule({})
    out["params"] = np.array(seeded_fill(net, SEED))
    net.eval()
    with torch.no_grad():
        y32, t32 = net.first_sem_model([feats])
        assert torch.equal(net([feats])["cls_pred"], y32)
        y64, t64 = net.double().first_sem_model([feats.double()])
    net.float()
    out["eval_cls_32"] = y32[:, :, ::2].contiguous().numpy()
    out["eval_trans_32"] = t32.numpy()
    out["eval_cls_64"] = y64[:, :, ::2].contiguous().numpy().astype(np.float64)
    out["eval_trans_64"] = t64.numpy().astype(np.float64)
    out["own"] = np.array(err(y32.numpy(), y64.numpy()))
    out["own_trans"] = np.array(err(t32.numpy(), t64.numpy()))
    print(f"eval: |fp32 - fp64| / (1 + |fp64|) = {float(out['own']):.2e} (cls_pred), {float(out['own_trans']):.2e} (trans_feat)")

    net.train()
    gt = torch.from_numpy(labels())
    with torch.enable_grad():
        pred = net([feats, gt])["cls_pred"]
        torch.Tensor.cuda, keep = (lambda self, *a, **k: self), torch.Tensor.cuda
        torch.nn.Module.cuda, keep_m = (lambda self, *a, **k: self), torch.nn.Module.cuda
        try:
            loss = TL.tooth_class_loss(pred, gt, 17)
        finally:
            torch.Tensor.cuda, torch.nn.Module.cuda = keep, keep_m
        loss.backward()
    out["train_loss"] = np.array(float(loss))
    for name, p in net.named_parameters():
        assert p.grad is not None, name
        g = p.grad.reshape(-1)
        out[f"grad::{name}"] = g[::grad_stride(g.numel())].numpy()
        out[f"gradnorm::{name}"] = np.array(float(g.double().norm()))
    print(f"train: loss {float(loss):.6f}, {sum(1 for k in out if k.startswith('grad::'))} gradients")
    path = os.path.join(HERE, "reference_cpu_r15_pointnet.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
