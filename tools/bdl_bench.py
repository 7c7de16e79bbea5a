#!/usr/bin/env python3
"""tgnet_bdl's training inputs at the reference's sizes: one synthetic scan of 100 000 vertices, 24 000 points a batch, 24 000 / 20 000
boundary-sampled rows, a randomly initialised five-stage first module (frozen) and two-stage trained module.  Wall-clock medians of
--reps repetitions after --warmup, the timed paths alternating so that they see the same machine state:

  miss_sample      training.BoundarySampler.sample with no cache file: the mesh and label files, the first module, the instance labels,
                   the flags, the resampling, the cache file's write -- and its pieces alone: load_mesh, base_forward, instance_labels
                   (tgnet.second_instances), flags (tgnet.boundary_flags), resample (tgnet.boundary_resample, which holds the flags)
  hit_sample       the same call served from the cache file
  miss_step, hit_step   BdlGroupingNetworkModel.step(.., "train") behind each, the sample included
  host_*           if sklearn imports, the reference's host formulation of the same join in the same process
                   (bdl_grouping_netowrk_model.py:76-107, 146-161): the numpy crop vote, KMeans with k-means++ on the moved foreground,
                   a KDTree over the batch and the 40-neighbour query of every vertex with a direct count of the nearest label

A random first module can vote every point into the background, which the sampler refuses: the seeds --seed, --seed + 1, ... are tried
and the one used is reported.  Prints one JSON line.

    python tools/bdl_bench.py [--reps 7] [--warmup 2] [--out FILE.json]
"""
import argparse
import copy
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from toothgroupnetwork_amd import augment, inference, nets, resample, synth, tgnet, training  # noqa: E402

CHAIN = "aug.Augmentator([aug.Scaling([0.85, 1.15]), aug.Rotation([-30,30], 'fixed'), aug.Translation([-0.2, 0.2])])"
LOSS = {"cbl_loss_1": 1, "cbl_loss_2": 1, "tooth_class_loss_1": 1, "tooth_class_loss_2": 1, "offset_1_loss": 0.03, "offset_1_dir_loss": 0.03,
        "chamf_1_loss": 0.15}
INFO = {"bdl_ratio": 0.7, "num_of_bdl_points": 20000, "num_of_all_points": 24000}
TEETH, BASE_NAME = 14, "BENCH_upper"


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def write_scan(root, n_u, n_v):
    """A labelled synthetic scan: TEETH angular sectors along the arch above the gingiva band, FDI numbers of an upper jaw."""
    folder = os.path.join(root, "BENCH")
    os.makedirs(folder)
    with open(os.path.join(folder, BASE_NAME + ".obj"), "w") as f:
        f.write(synth.obj_text(n_u, n_v, 2020, "plain", with_tail=False))
    u = np.repeat(np.arange(n_u), n_v) / n_u
    v = np.tile(np.arange(n_v), n_u) / n_v
    tooth = np.minimum((u * TEETH).astype(np.int64), TEETH - 1)
    fdi = np.where(v < 0.35, 0, np.where(tooth < 7, 17 - tooth, 21 + tooth - 7))
    with open(os.path.join(folder, BASE_NAME + ".json"), "w") as f:
        json.dump({"id_patient": "BENCH", "jaw": "upper", "labels": fdi.tolist(), "instances": fdi.tolist()}, f)


def host_join(feat, labels, out, dense_xyz, KDTree, KMeans):
    """-> the pieces of the reference's join as functions of no argument"""
    xyz = feat[0, :3].t().cpu().numpy()
    sem_2, idx = out["sem_2"].permute(0, 2, 1).cpu().numpy(), out["nn_crop_indexes"][0].cpu().numpy()
    moved = xyz + out["offset_1"][0].t().cpu().numpy()
    k = len(np.unique(labels.cpu().numpy())) - 1
    state = {}

    def vote():
        sums = np.zeros((xyz.shape[0], 2), np.float32)
        for crop in range(sem_2.shape[0]):
            sums[idx[crop]] += sem_2[crop]
        state["mask"] = np.argmax(sums, axis=1)
    vote()

    def kmeans():
        point_labels = np.full(xyz.shape[0], -1.0)
        point_labels[state["mask"] == 1] = KMeans(k, init="k-means++").fit(moved[state["mask"] == 1]).labels_
        state["labels"] = point_labels
    kmeans()

    def flags():
        near = KDTree(xyz, leaf_size=2).query(dense_xyz, k=40, return_distance=False)
        a = state["labels"][near]
        return (a == a[:, :1]).sum(axis=1) / 40.0 < 0.7      # (cheaper than the reference's np.unique over all n x 40 entries)
    return {"host_vote": vote, "host_kmeans": kmeans, "host_flags": flags}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"what": "tgnet_bdl training inputs", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup}
    tgn = inference.inference_config("tgnet")
    with tempfile.TemporaryDirectory() as root:
        write_scan(root, 400, 250)
        cache = os.path.join(root, "cache")
        cfg = {"tr_set": {"optimizer": {"lr": 1e-2, "NAME": "sgd", "momentum": 0.9, "weight_decay": 1.0e-4},
                          "scheduler": {"sched": "cosine", "warmup_epochs": 0, "full_steps": 40, "schedueler_step": 15000000, "min_lr": 1e-5},
                          "loss": dict(LOSS), "contrastive_boundary": True},
               "checkpoint_path": os.path.join(root, "ckpts", "bdl"), "model_parameter": dict(tgn["boundary_model_info"]["model_parameter"]),
               "boundary_sampling_info": dict(INFO, orginal_data_obj_path=root, orginal_data_json_path=root, bdl_cache_path=cache),
               "fps_model_info": {"model_parameter": dict(tgn["fps_model_info"]["model_parameter"])}}
        probe = training.BoundarySampler(cfg, None)
        mesh, mesh_labels = probe.load_mesh(BASE_NAME)
        pick = resample.fps(mesh[:, :3].astype(np.float64), 24000)[:24000]
        aug = augment.from_config_string(CHAIN)
        np.random.seed(a.seed)
        aug.reload_vals()
        item = {"feat": torch.from_numpy(np.ascontiguousarray(aug.run(mesh[pick].copy()).T))[None], "aug_obj": [copy.deepcopy(aug)],
                "gt_seg_label": torch.from_numpy(np.ascontiguousarray(mesh_labels[pick].astype(np.int64).reshape(1, 1, -1))),
                "mesh_path": [os.path.join(root, BASE_NAME + "_sampled_points.npy")]}
        cache_file = os.path.join(cache, BASE_NAME + ".npy")
        model, errors = None, []
        for seed in range(a.seed, a.seed + 8):
            torch.manual_seed(seed)
            base = nets.GroupingNetworkModule(cfg["fps_model_info"]).cuda()
            candidate = training.BdlGroupingNetworkModel(cfg, base_model=base)
            try:
                np.random.seed(a.seed)
                candidate.sampler.sample(item)
                model, res["base_seed"] = candidate, seed
                break
            except ValueError as e:
                errors.append(f"seed {seed}: {e}")
        if errors:
            res["refused"] = errors
        if model is None:
            print(json.dumps(res), flush=True)
            return 1
        sampler, dev = model.sampler, model.device
        feat, labels = item["feat"].to(dev), item["gt_seg_label"].to(dev)
        with torch.no_grad():
            out = model.base_model([feat, labels])
        ins = tgnet.second_instances(feat, labels, out)["ins"] - 1
        augmented = item["aug_obj"][0].run(mesh.copy())
        xyz = feat[0, :3].t().contiguous()
        boundary, _ = tgnet.boundary_flags(augmented, xyz, ins)
        res.update({"vertices": int(mesh.shape[0]), "batch_points": int(feat.shape[2]), "foreground": int((ins >= 0).sum()),
                    "clusters": int(len(torch.unique(ins[ins >= 0]))), "flagged_vertices": int(boundary.sum())})

        def miss():
            if os.path.exists(cache_file):
                os.remove(cache_file)
            np.random.seed(a.seed)
            return sampler.sample(item)

        def base_forward():
            with torch.no_grad():
                return model.base_model([feat, labels])

        def resample_once():
            np.random.seed(a.seed)
            return tgnet.boundary_resample(augmented, xyz, ins, info=INFO, carry=(mesh_labels, mesh))

        def miss_step():
            if os.path.exists(cache_file):
                os.remove(cache_file)
            np.random.seed(a.seed)
            return model.step(0, item, "train")
        fns = {"miss_sample": miss, "load_mesh": lambda: sampler.load_mesh(BASE_NAME), "base_forward": base_forward,
               "instance_labels": lambda: tgnet.second_instances(feat, labels, out), "flags": lambda: tgnet.boundary_flags(augmented, xyz, ins),
               "resample": resample_once, "miss_step": miss_step}
        # the cache-hit paths run right behind a miss of the same round, so the file is there
        fns["hit_sample"] = lambda: sampler.sample(item)
        fns["hit_step"] = lambda: model.step(0, item, "train")
        try:
            from sklearn.cluster import KMeans
            from sklearn.neighbors import KDTree
            fns.update(host_join(feat, labels, out, augmented[:, :3], KDTree, KMeans))
        except ImportError:
            res["host_path"] = "not measured"
        wall = {n: [] for n in fns}
        for r in range(a.warmup + a.reps):
            for n, fn in fns.items():
                ms = wall_ms(fn)
                if r >= a.warmup:
                    wall[n].append(ms)
        ms = {n: round(float(np.median(v)), 3) for n, v in wall.items()}
        res["sample_wall_ms"] = {n: ms[n] for n in ("miss_sample", "load_mesh", "base_forward", "instance_labels", "flags", "resample", "hit_sample")}
        res["step_wall_ms"] = {"miss_step": ms["miss_step"], "hit_step": ms["hit_step"],
                               "step_without_sample": round(ms["hit_step"] - ms["hit_sample"], 3)}
        if "host_flags" in ms:
            res["host_path"] = {n[5:]: ms[n] for n in ("host_vote", "host_kmeans", "host_flags")}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
