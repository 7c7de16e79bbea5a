#!/usr/bin/env python3
"""Fixture of the DGCNN network (tests/golden/reference_cpu_r8_dgcnn.npz), produced by running the REFERENCE's own
models/modules/dgcnn.py on CPU in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_r8_dgcnn.py

The reference's get_graph_feature builds its index base on torch.device('cuda'); the module is served a torch whose device('cuda')
is the CPU, the way make_golden_r7_grouping.py serves .cuda().  Weights: tests/golden/seeded.py (seed 91); input: two 2 048-point
synthetic scans in one batch (synth.scan_batch(2, 2048, "arch", seed=21), stored as a digest), so that idx_base is exercised.

  eval    fp32 pass of DGCnnModule.eval(): the kNN index SETS of its three levels (crop_cases.pack_sets: sorted, uint16
          differences; the max over the neighbours does not see their order), every 2nd point of cls_pred; then a float64 pass of
          the same module on the SAME indices (cls_pred likewise), so that the tests can tell the reference's own fp32 noise from a
          discrepancy.
  train   DGCnnModule.train() with dp1 in eval (the only random element): the three levels' index sets, the tooth_class_loss term of
          DGCnnModel.get_loss (models/dgcnn_model.py:7-11, models/tgn_loss.py:355) on synthetic labels, and per parameter a strided
          gradient sample (at most 64 values) plus its norm.  The scans have no duplicated points, so the max over the neighbours
          routes its gradient the same way whatever order equal values come in.
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("TGN_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from crop_cases import digest, pack_sets  # noqa: E402
from seeded import seeded_fill  # noqa: E402
from toothgroupnetwork_amd import synth  # noqa: E402

SEED, B, N, K = 91, 2, 2048, 20


def scans():
    return synth.scan_batch(B, N, "arch", seed=21)


def labels():
    return np.random.default_rng(22).integers(-1, 16, size=(B, 1, N)).astype(np.int64)


def grad_stride(numel):
    return max(1, numel // 64)


class _TorchCudaIsCpu(types.ModuleType):
    """torch, except that torch.device('cuda') is the CPU."""

    def __init__(self):
        super().__init__("torch")

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def device(*a, **k):
        if a and isinstance(a[0], str) and a[0].startswith("cuda"):
            return torch.device("cpu")
        return torch.device(*a, **k)


def load():
    sys.path.insert(0, REFERENCE)
    import models.modules.dgcnn as RD
    import models.tgn_loss as TL
    RD.torch = _TorchCudaIsCpu()
    return RD, TL


def main():
    RD, TL = load()
    out = {}
    x = scans()
    out["input_digest"] = np.array(digest(x))
    feats = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1)))
    net = RD.DGCnnModule({})
    names = seeded_fill(net, SEED)
    out["params"] = np.array(names)
    real_knn = RD.knn
    seen = []

    def recording(t, k):
        i = real_knn(t, k)
        seen.append(i)
        return i
    RD.knn = recording
    net.eval()
    with torch.no_grad():
        y32 = net([feats])["cls_pred"]
    eval_idx = list(seen)
    served = iter(eval_idx)
    RD.knn = lambda t, k: next(served)
    with torch.no_grad():
        y64 = net.double()([feats.double()])["cls_pred"]
    net.float()
    for lvl, i in enumerate(eval_idx):
        out[f"eval_idx{lvl}"] = pack_sets(i.reshape(-1, K).numpy())
    out["eval_cls_32"] = y32[:, :, ::2].numpy()
    out["eval_cls_64"] = y64[:, :, ::2].numpy().astype(np.float64)
    err = float(np.max(np.abs(y32.double().numpy() - y64.numpy()) / (1 + np.abs(y64.numpy()))))
    print(f"eval: |fp32 - fp64| / (1 + |fp64|) = {err:.2e}")

    seen.clear()
    RD.knn = recording
    net.train()
    net.dp1.eval()
    gt = torch.from_numpy(labels())
    with torch.enable_grad():
        pred = net([feats, gt])["cls_pred"]
        TL.torch = _TorchCudaIsCpu()
        torch.Tensor.cuda, keep = (lambda self, *a, **k: self), torch.Tensor.cuda
        torch.nn.Module.cuda, keep_m = (lambda self, *a, **k: self), torch.nn.Module.cuda
        try:
            loss = TL.tooth_class_loss(pred, gt, 17)
        finally:
            torch.Tensor.cuda, torch.nn.Module.cuda = keep, keep_m
        loss.backward()
    for lvl, i in enumerate(seen):
        out[f"train_idx{lvl}"] = pack_sets(i.reshape(-1, K).numpy())
    out["train_loss"] = np.array(float(loss))
    for name, p in net.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.reshape(-1)
        out[f"grad::{name}"] = g[::grad_stride(g.numel())].numpy()
        out[f"gradnorm::{name}"] = np.array(float(g.double().norm()))
    print(f"train: loss {float(loss):.6f}, {sum(1 for k in out if k.startswith('grad::'))} gradients")
    path = os.path.join(HERE, "reference_cpu_r8_dgcnn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
