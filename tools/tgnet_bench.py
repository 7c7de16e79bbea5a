#!/usr/bin/env python3
"""tgnet at the inference shape (one scan of 30 000 vertices, 24 000 sampled points): (a) the stage times of
inference.TgnInferencePipeLine with two randomly initialised nets.GroupingNetworkModule (five-stage and two-stage; random weights give
arbitrary teeth, and a run whose clustering finds fewer than three of them ends in number_teeth's ValueError: the stages up to there are
reported with the error), (b) the join alone on the scripted case of tests/golden/tgnet_cases.py -- boundary_flags, boundary_resample,
kmeans, merge_boundary (toothgroupnetwork_amd/tgnet.py) -- by the wall clock, since each holds host synchronisations, median of --reps
repetitions after --warmup, and (c) the host synchronisations of each, counted from torch's profiler (runtime calls on which the host
waits: *Synchronize and synchronous copies in either direction).  If sklearn imports, the reference's host formulation of (b) (inference_pipeline_tgn.py:289-304,
:268-274, :107-126 as sklearn calls: the two KDTree queries and a direct count of the nearest label, KMeans with k-means++, the KDTree
query and bincount vote per cluster) is timed the same way in the
same process; if it does not, "host_path" is "not measured".  Prints one JSON line.

    python tools/tgnet_bench.py [--reps 10] [--warmup 2] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

import tgnet_cases as TC  # noqa: E402
from toothgroupnetwork_amd import inference, nets, preprocess, resample, synth, tgnet  # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def waits(fn):
    """The runtime calls of one fn() on which the host waits for the device, by name; None if the profiler records none here."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
        names = {}
        for e in prof.events():
            n = e.name
            if "Synchronize" in n or (n.startswith(("hipMemcpy", "cudaMemcpy")) and "Async" not in n):
                names[n] = names.get(n, 0) + 1
        return names or None
    except Exception:
        return None


def host_flags(dense_xyz, sampled_xyz, labels, KDTree):
    tree = KDTree(sampled_xyz, leaf_size=40)
    near = tree.query(dense_xyz, k=40, return_distance=False)
    a = labels[near]
    same = (a == a[:, :1]).sum(axis=1)                   # (cheaper than the reference's np.unique over all n x 40 entries: the host path is flattered)
    return same / 40.0 < 0.7, labels[tree.query(dense_xyz, k=1, return_distance=False)[:, 0]]


def host_merge(first_xyz, first_ins, first_sem, bdl_xyz, bdl_ins, KDTree):
    tree = KDTree(first_xyz, leaf_size=2)
    ins, sem = np.zeros(len(bdl_ins), np.int64), np.zeros(len(bdl_ins), np.int64)
    for c in np.unique(bdl_ins):
        if c == 0:
            continue
        near = tree.query(bdl_xyz[bdl_ins == c], k=1, return_distance=False)
        win = np.argmax(np.bincount(first_ins[near.reshape(-1)]))
        ins[bdl_ins == c], sem[bdl_ins == c] = win, first_sem[first_ins == win][0]
    return ins, sem


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"what": "tgnet", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup}
    nu, nv, seed = TC.MESHES["main"]
    with tempfile.TemporaryDirectory() as root:
        path = os.path.join(root, "scan.obj")
        with open(path, "w") as f:
            f.write(synth.obj_text(nu, nv, seed, "plain", with_tail=False))
        # (a) the pipeline with real modules
        torch.manual_seed(a.seed)
        first = nets.GroupingNetworkModule({"model_parameter": inference.inference_config("tgnet")["fps_model_info"]["model_parameter"]})
        bdl = nets.GroupingNetworkModule({"model_parameter": inference.inference_config("tgnet")["boundary_model_info"]["model_parameter"]})
        pipe = inference.TgnInferencePipeLine(first.to(dev).eval(), bdl.to(dev).eval())
        stages, error = [], None
        for _ in range(a.warmup + a.reps):
            np.random.seed(TC.PERM_SEED)
            try:
                pipe(path)
                stages.append(dict(pipe.times))
            except ValueError as e:
                error = str(e)
                break
        if stages[a.warmup:]:
            res["pipeline_stage_ms"] = {k: round(float(np.median([s[k] for s in stages[a.warmup:]])) * 1e3, 3) for k in pipe.STAGES}
            res["pipeline_ms"] = round(sum(res["pipeline_stage_ms"].values()), 3)
        if error is not None:
            res["pipeline_error"] = error
        # the two modules alone (device events would miss their host synchronisations: wall clock)
        _, mesh = preprocess.read_txt_obj_ls(path, ret_mesh=True)
    dense = np.concatenate([inference.normalise_for_inference(mesh["vertices"]), mesh["vertex_normals"]], axis=1)
    sampled = dense[resample.fps(dense[:, :3], 24000)[:24000]]
    inp = torch.from_numpy(np.ascontiguousarray(sampled.astype("float32"))[None]).to(dev).permute(0, 2, 1).contiguous()
    # (b) the join on the scripted case
    s_first, s_bdl = TC.stand_ins(TC.device_knn)
    with torch.no_grad():
        fi = {k: v.cpu().numpy() for k, v in tgnet.first_instances(inp, s_first([inp])).items()}
        np.random.seed(TC.PERM_SEED)
        feats, lab, only, _ = tgnet.boundary_resample(dense, sampled, fi["ins"])
        binp = torch.from_numpy(np.ascontiguousarray(feats.astype("float32"))[None]).to(dev).permute(0, 2, 1).contiguous()
        blab = torch.from_numpy(tgnet.dense_rank_labels(lab)[None, None]).to(dev)
        bout = s_bdl([binp, blab], test=True)
        second = tgnet.second_instances(binp, blab, bout)
        fg = second["moved"][second["mask"] != 0].contiguous()
        sem, ins = tgnet.number_teeth(fi["xyz"], fi["ins"], fi["sem"])
        nb = only.shape[0]
        bdl_xyz, bdl_ins = second["xyz"][:nb].cpu().numpy(), second["ins"][:nb].cpu().numpy()
        res.update({"dense_rows": int(dense.shape[0]), "boundary_rows": int(nb), "kmeans_points": int(fg.shape[0]), "kmeans_k": int(second["centres"].shape[0])})

        def resample_once():
            np.random.seed(TC.PERM_SEED)
            return tgnet.boundary_resample(dense, sampled, fi["ins"])
        fns = {"first_module": lambda: first([inp]), "boundary_module": lambda: bdl([binp, blab], test=True),
               "boundary_flags": lambda: tgnet.boundary_flags(dense, sampled, fi["ins"]), "boundary_resample": resample_once,
               "kmeans": lambda: tgnet.kmeans(fg, second["centres"] + 0.01), "merge_boundary": lambda: tgnet.merge_boundary(fi["xyz"], ins, sem, bdl_xyz, bdl_ins)}
        try:
            from sklearn.cluster import KMeans
            from sklearn.neighbors import KDTree
            fg_host = fg.cpu().numpy()
            fns.update({"host_boundary_flags": lambda: host_flags(dense[:, :3], sampled[:, :3], fi["ins"], KDTree),
                        "host_kmeans": lambda: KMeans(int(second["centres"].shape[0]), init="k-means++").fit(fg_host),
                        "host_merge_boundary": lambda: host_merge(fi["xyz"].astype(np.float64), ins, sem, bdl_xyz.astype(np.float64), bdl_ins, KDTree)})
            want = host_flags(dense[:, :3], sampled[:, :3], fi["ins"], KDTree)
            got = tgnet.boundary_flags(dense, sampled, fi["ins"])
            res["host_path_same_flags"] = bool(np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]))
        except ImportError:
            res["host_path"] = "not measured"
        wall = {n: [] for n in fns}
        for n, fn in fns.items():
            try:
                for _ in range(a.warmup):
                    fn()
            except ValueError as e:                              # a random module's clustering can find nothing to crop
                wall[n] = str(e)
        for _ in range(a.reps):                                  # alternating: the paths see the same machine state
            for n, fn in fns.items():
                if isinstance(wall[n], list):
                    wall[n].append(wall_ms(fn))
        ms = {n: (round(float(np.median(v)), 3) if isinstance(v, list) else v) for n, v in wall.items()}
        res["join_wall_ms"] = {n: v for n, v in ms.items() if not n.startswith("host_") and not n.endswith("_module")}
        res["module_wall_ms"] = {n: v for n, v in ms.items() if n.endswith("_module")}
        if any(n.startswith("host_") for n in ms):
            res["host_path"] = {n[5:]: v for n, v in ms.items() if n.startswith("host_")}
        res["host_waits"] = {n: (waits(fns[n]) or "not measured") for n in ("boundary_flags", "boundary_resample", "kmeans", "merge_boundary")}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
