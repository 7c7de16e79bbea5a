#!/usr/bin/env python3
"""GPU time of the unlabelled path's clustering (toothgroupnetwork_amd/cluster.py) on a 24 000-point synthetic scan -- dbscan alone,
get_clustering_labels without and with a MeanShift re-split -- and of GroupingNetworkModule's unlabelled forward end to end: its
first stage (seeded weights) plus everything after it, fed the split case's classes and offsets (clustering, crops, second stage), plus sklearn's time for the same clustering when sklearn is importable.  Prints one JSON line; times in ms, medians.

    python tools/cluster_bench.py [--reps 20]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cluster_cases import labelling_cases  # noqa: E402
from toothgroupnetwork_amd import cluster, nets, synth  # noqa: E402

CONFIG = {"model_parameter": {"input_feat": 6, "stride": [1, 4, 4, 4, 4], "nsample": [36, 24, 24, 24, 24], "blocks": [2, 3, 4, 6, 3],
                              "block_num": 5, "planes": [32, 64, 128, 256, 512], "crop_sample_size": 3072}}


class Stub(torch.nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, inputs, **kwargs):
        return self.fn(inputs)


def gpu_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def cpu_ms(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cases = labelling_cases()
    res = {"metric": "cluster_bench", "points": 24000, "device": torch.cuda.get_device_name(0)}
    for tag in ("nosplit", "split"):
        moved, cls = cases[tag]
        m, c = torch.from_numpy(moved).to(dev), torch.from_numpy(cls).to(dev)
        fg = m[c != 0].contiguous()
        res[f"fg_points_{tag}"] = int(fg.shape[0])
        if tag == "nosplit":
            res["dbscan_ms"] = gpu_ms(lambda: cluster.dbscan(fg, 0.03, 30), a.reps)
        res[f"get_clustering_labels_{tag}_ms"] = gpu_ms(lambda: cluster.get_clustering_labels(m, c), a.reps)
    rows, _ = synth.labelled_arch(24000, 14, seed=912)
    feats = torch.from_numpy(np.ascontiguousarray(rows.T))[None].to(dev)
    torch.manual_seed(0)
    net = nets.GroupingNetworkModule(CONFIG).to(dev).eval()
    first = net.first_ins_cent_model
    moved, cls = cases["split"]
    sem_1 = torch.from_numpy(np.eye(10, dtype=np.float32)[cls].T.copy())[None].to(dev)
    offset_1 = torch.from_numpy(np.ascontiguousarray((moved - rows[:, :3]).T))[None].to(dev)
    reps = max(3, a.reps // 4)
    with torch.no_grad():
        # untrained weights give no tooth-shaped classes, so the stages after the first one see the split case's sem_1 / offset_1
        res["first_stage_ms"] = gpu_ms(lambda: first([feats]), reps)
        net.first_ins_cent_model = Stub(lambda inp: (sem_1, offset_1, None, None))
        res["after_first_stage_ms"] = gpu_ms(lambda: net([feats]), reps)
    res["unlabelled_forward_ms"] = res["first_stage_ms"] + res["after_first_stage_ms"]
    try:
        from sklearn.cluster import DBSCAN
        moved, cls = cases["nosplit"]
        res["sklearn_dbscan_ms"] = cpu_ms(lambda: DBSCAN(eps=0.03, min_samples=30).fit(moved[cls != 0]), a.cpu_reps)
    except ImportError:
        res["sklearn_dbscan_ms"] = None
    print(json.dumps(res))


if __name__ == "__main__":
    main()
