#!/usr/bin/env python3
"""tsegnet at the inference shape (one 24 000-point scan): (a) the whole eval forward of nets.TSegNetModule, (b) the join alone --
centroid-module outputs to segmentation-module input: proposal filter, DBSCAN, cluster means, the 8-of-T choice, kNN crops and the
36-channel crop tensor (toothgroupnetwork_amd/tsegnet.py) -- and (c) the label painting.  Device events after --warmup, median of
--reps (at least 20) repetitions; (b) also by the wall clock (it holds two host synchronisations) and with its kernel-launch count.
If sklearn imports, the reference's host formulation of (b) (models/modules/tsegnet.py:57-81 restated: numpy filter, sklearn DBSCAN and
KDTree, python gathers, the copies they need) is timed by the wall clock in the same process, alternating with the GPU path; if it
does not, "host_path" is "not measured".  Seeded weights and a seeded synthetic scan of separated teeth (tests/golden/tsegnet_cases.py);
prints one JSON line.

    python tools/tsegnet_bench.py [--reps 20] [--warmup 3] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

import tsegnet_cases as TC  # noqa: E402
from seeded import seeded_fill  # noqa: E402
from toothgroupnetwork_amd import nets, tsegnet  # noqa: E402
from toothgroupnetwork_amd.pointnet2_utils import square_distance  # noqa: E402


def gpu_join(feats, c, labels):
    moved, counts = tsegnet.centroid_proposals(c[3], c[4], c[5])
    cents = tsegnet.cluster_centers(moved, counts)
    chosen = [x[torch.from_numpy(np.random.permutation(x.shape[0])[:8]).to(x.device)] for x in cents]
    return tsegnet.crop_features(feats, c[0], chosen, tsegnet.CROP_K, labels)


def host_join(feats, c, labels, DBSCAN, KDTree):
    """tsegnet.py:57-81 with ops_utils.get_nearest_neighbor_idx / get_indexed_features and get_ddf written out."""
    l0_points, _, l0_xyz, l3_xyz, offset_result, dist_result = c
    moved_points = (l3_xyz + offset_result).cpu().detach().numpy().T.reshape(-1, 3)
    moved_points = moved_points[dist_result.cpu().detach().numpy().reshape(-1) < 0.3, :]
    db = DBSCAN(eps=0.05, min_samples=3).fit(moved_points, 3)
    center_points = np.array([moved_points[db.labels_ == lab].mean(axis=0) for lab in np.unique(db.labels_) if lab != -1])[None]
    rand_indexes = np.random.permutation(center_points.shape[1])[:8]
    center_points = center_points[:, rand_indexes, :]
    org_xyz = l0_xyz.permute(0, 2, 1).cpu().detach().numpy()
    idx = [KDTree(org_xyz[b], leaf_size=2).query(center_points[b], k=3072, return_distance=False) for b in range(org_xyz.shape[0])]

    def indexed(features):
        return torch.stack([features[b][:, i] for b in range(len(idx)) for i in idx[b]], dim=0)
    cropped_input, cropped_feature, crop_labels = indexed(feats), indexed(l0_points), indexed(labels)
    cent = torch.from_numpy(center_points).to(feats.device)
    ddf = torch.exp(torch.sqrt(square_distance(cropped_input[:, :3, :].permute(0, 2, 1).contiguous(), cent.permute(1, 0, 2).contiguous())) * (-4))
    return torch.cat([cropped_input[:, :3, :], cropped_feature, ddf.permute(0, 2, 1)], dim=1), idx, crop_labels


def events_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def launches(fn):
    """Kernel launches of one call, counted by torch's profiler; None if it records no device activity here."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and not e.name.lower().startswith(("memcpy", "memset")))
        return n or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = max(a.reps, 20)
    dev = torch.device("cuda", 0)
    net = nets.TSegNetModule({"run_tooth_segmentation_module": True})
    seeded_fill(net, 1111)
    net = TC.set_heads(net).to(dev).eval()
    rows, lab = TC.clumped_scan(1121)
    feats = torch.from_numpy(rows)[None].to(dev)
    labels = torch.from_numpy(lab).view(1, 1, -1).to(dev)
    try:
        from sklearn.cluster import DBSCAN
        from sklearn.neighbors import KDTree
    except Exception:
        DBSCAN = KDTree = None
    res = {"what": "tsegnet", "device": torch.cuda.get_device_name(0), "B": 1, "N": feats.shape[2], "reps": reps, "warmup": a.warmup}
    with torch.no_grad():
        c = net.cent_module(feats)
        o = net([feats, labels])
        cropped, idx, _ = gpu_join(feats, c, labels)
        pd_2, id_pred = o["pd_2"], o["id_pred"]
        res["crops"] = int(cropped.shape[0])
        fns = {"forward": lambda: net([feats, labels]), "join": lambda: gpu_join(feats, c, labels),
               "paint": lambda: tsegnet.paint_labels(idx, pd_2, id_pred, feats.shape[2])}
        if DBSCAN is not None:
            fns["host_join"] = lambda: host_join(feats, c, labels, DBSCAN, KDTree)
            np.random.seed(3)
            want, got = host_join(feats, c, labels, DBSCAN, KDTree), None
            np.random.seed(3)
            got = gpu_join(feats, c, labels)
            res["host_join_same_crops"] = bool(torch.equal(want[0][:, :35], got[0][:, :35]) and torch.equal(want[2], got[2]))
        for fn in fns.values():
            for _ in range(a.warmup):
                fn()
        ev = {n: [] for n in fns}
        wall = {n: [] for n in fns}
        for _ in range(reps):                                    # alternating: the paths see the same machine state
            for n, fn in fns.items():
                ev[n].append(events_ms(fn))
            for n in ("join", "host_join"):
                if n in fns:
                    wall[n].append(wall_ms(fns[n]))
        res["forward_ms"] = round(float(np.median(ev["forward"])), 4)
        res["join_ms"] = round(float(np.median(ev["join"])), 4)
        res["join_wall_ms"] = round(float(np.median(wall["join"])), 4)
        res["paint_ms"] = round(float(np.median(ev["paint"])), 4)
        n = launches(fns["join"])
        res["join_launches"] = n if n is not None else "not measured"
        if "host_join" in fns:
            res["host_path"] = {"join_ms": round(float(np.median(ev["host_join"])), 4), "join_wall_ms": round(float(np.median(wall["host_join"])), 4)}
        else:
            res["host_path"] = "not measured"
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
