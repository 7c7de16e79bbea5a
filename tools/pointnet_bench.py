#!/usr/bin/env python3
"""PointNet at the inference shape (N = 24 000 points, B = 1 and 8): each of the three fused linear + max-over-points layers of
pointnet.PointFirstModule (stn.conv3 and fstn.conv3: 128 -> 1024, relu; feat.conv3: 256 -> 2048, identity), the same kernel at
DGCNN's conv6 shape (192 -> 1024, leaky 0.2), and the whole eval forward, each against the torch composition on the same GPU
(conv -> bn -> act -> max; for the forward the reference's formulation, pointnet.get_model._forward_train).  Median of --reps
timed calls (CUDA events) after --warmup, the peak of torch's allocator over one call of each, and for the layers the fraction of
the fp32 matrix peak (155 TFLOP/s measured for v_mfma_f32_32x32x2_f32) the fused kernel reaches.  Prints ONE JSON line.

    python tools/pointnet_bench.py [--batches 1 8] [--reps 50] [--warmup 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

from seeded import seeded_fill  # noqa: E402
from toothgroupnetwork_amd import dgcnn, pointnet, synth  # noqa: E402

FP32_MATRIX_PEAK = 155e12


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return float(np.median(ts)), peak / 2 ** 20


def composition(x, conv, bn, act, slope):
    y = bn(conv(x))
    if act == "relu":
        y = F.relu(y)
    elif act == "leaky_relu":
        y = F.leaky_relu(y, slope)
    return torch.max(y, 2)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--n", type=int, default=24000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    net = pointnet.PointFirstModule({})
    seeded_fill(net, 151)
    net = net.to(dev).eval()
    dg = dgcnn.DGCnnModule({})
    seeded_fill(dg, 81)
    dg = dg.to(dev).eval()
    feat = net.first_sem_model.feat
    layers = (("stn.conv3 128->1024 relu", feat.stn.conv3, feat.stn.bn3, "relu", 0.0),
              ("fstn.conv3 128->1024 relu", feat.fstn.conv3, feat.fstn.bn3, "relu", 0.0),
              ("feat.conv3 256->2048 identity", feat.conv3, feat.bn3, "identity", 0.0),
              ("dgcnn conv6 192->1024 leaky 0.2", dg.conv6[0], dg.bn6, "leaky_relu", 0.2))
    rows = []
    with torch.no_grad():
        for B in a.batches:
            for what, conv, bn, act, slope in layers:
                K, C = conv.in_channels, conv.out_channels
                h = torch.randn(B, K, a.n, device=dev)
                ours = timed(lambda: pointnet.linear_act_max(h, conv, bn, act, slope), a.reps, a.warmup)
                ref = timed(lambda: composition(h, conv, bn, act, slope), a.reps, a.warmup)
                floor_ms = 2.0 * B * a.n * K * C / FP32_MATRIX_PEAK * 1e3
                rows.append({"what": what, "B": B, "N": a.n, "fused_ms": round(ours[0], 4), "fused_peak_MiB": round(ours[1], 1),
                             "torch_ms": round(ref[0], 4), "torch_peak_MiB": round(ref[1], 1), "speedup": round(ref[0] / ours[0], 2),
                             "fp32_matrix_floor_ms": round(floor_ms, 4), "fraction_of_fp32_matrix_peak": round(floor_ms / ours[0], 3)})
                del h
                torch.cuda.empty_cache()
            x = torch.from_numpy(np.ascontiguousarray(synth.scan_batch(B, a.n, "arch", seed=1).transpose(0, 2, 1))).to(dev)
            ours = timed(lambda: net([x]), a.reps, a.warmup)
            ref = timed(lambda: net.first_sem_model._forward_train(x), a.reps, a.warmup)
            rows.append({"what": "eval forward", "B": B, "N": a.n, "fused_ms": round(ours[0], 4), "fused_peak_MiB": round(ours[1], 1),
                         "torch_ms": round(ref[0], 4), "torch_peak_MiB": round(ref[1], 1), "speedup": round(ref[0] / ours[0], 2)})
            del x
            torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "rows": rows}
    print(json.dumps(result), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
