#!/usr/bin/env python3
"""Fixtures of tgnet_fps's two-stage network (tests/golden/reference_cpu_r7_grouping.npz), produced by running the REFERENCE's own
Python on CPU in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_r7_grouping.py [part ...]      (parts: ops module)

  (a) `ops`: the crop step of models/modules/grouping_network_module.py:45-72 on the labelled path -- the centroid lines (:45-56,
      restated verbatim: np.unique over the labels, `xyz[label == t].mean(axis=0)` on the float32 coordinates), then the reference's
      own ops_utils.get_nearest_neighbor_idx (sklearn KDTree, leaf_size=2), get_indexed_features and centering_object -- on
        s24     one 24 000-point scan with 14 teeth, k = 3072;
        ragged  a batch of two 12 000-point scans with 16 and 11 teeth (ragged T), k = 3072;
        k4096   an 8 000-point scan, k = 4096;
        dup     a scan with 600 duplicated vertices plus one copy (label -1, so no centroid moves) of the 3072nd-nearest point of the
                first tooth: a distance tie across the k-th boundary, k = 3072;
        single  a scan in which tooth 15 is a single point, k = 512.
      Stored: a digest of each input (tests/golden/crop_cases.py rebuilds it), the centroids, each crop's KDTree index SET (sorted,
      as uint16 differences: KDTree's order among equal distances is unspecified and the distance sequence follows from the set),
      and every 64th column of the centred crops.
  (b) `module`: the reference's GroupingNetworkModule (tgnet_fps config) in TRAIN mode (BatchNorm batch statistics) on one
      24 000-point scan with seeded weights (tests/golden/seeded.py), called as forward([feat, labels], test=True) -- the labelled-
      centroid path without the contrastive-boundary criterion, no change to the reference -- then the loss terms of
      FpsGroupingNetworkModel.get_loss (models/fps_grouping_network_model.py:8-24 with train_configs/tgnet_fps.py's weights, the cbl
      terms left out) and the backward.  In float32 and in float64 on the SAME indices (FPS / kNN served by the oracle on the float32
      values as in make_golden_r4.py; the float64 pass reuses the float32 pass's crop indices), so that the tests can tell the
      reference's own fp32 noise from a discrepancy.  Stored: strided samples of sem_1, offset_1, sem_2, the index sets of all
      nn_crop_indexes (as above), the loss terms, and per parameter a strided gradient sample plus norms.  The weights are not stored: the parameter
      names and shapes (the reference's state_dict order) are, and seeded_fill rebuilds the values from them.
"""
import os
import sys
import time
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("TGN_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden import load_reference  # noqa: E402
from make_golden_r2_io import _stub_open3d  # noqa: E402
from make_golden_r3 import cpu_as_cuda, rel_err  # noqa: E402
from make_golden_r4 import _serve_pointops  # noqa: E402
from crop_cases import digest, op_cases, pack_sets  # noqa: E402
from seeded import seeded_fill  # noqa: E402
from toothgroupnetwork_amd import synth  # noqa: E402

GRAD_SAMPLES = 16
CROP_STRIDE = 64
LOSS_NAMES = ("tooth_class_loss_1", "tooth_class_loss_2", "offset_1_loss", "offset_1_dir_loss", "chamf_1_loss")


def _reference_modules():
    sys.modules["open3d"] = _stub_open3d([])
    sys.modules.setdefault("trimesh", types.ModuleType("trimesh"))
    if REFERENCE not in sys.path:
        sys.path.append(REFERENCE)
    import gen_utils as gu
    import ops_utils as ou
    assert ou.__file__.startswith(REFERENCE) and gu.__file__.startswith(REFERENCE)
    return gu, ou


def _reference_centroids(gu, feats, labels):
    """grouping_network_module.py:45-56, verbatim on numpy inputs."""
    cluster_centroids = []
    for b_idx in range(feats.shape[0]):
        b_gt_seg_labels = gu.torch_to_numpy(labels[b_idx, :, :].view(-1))
        b_points_coords = gu.torch_to_numpy(feats[b_idx, :3, :]).T
        contained_tooth_num = np.unique(b_gt_seg_labels)
        temp_list = []
        for tooth_num in contained_tooth_num:
            if tooth_num == -1:
                continue
            temp_list.append(b_points_coords[tooth_num == b_gt_seg_labels].mean(axis=0))
        cluster_centroids.append(temp_list)
    return cluster_centroids


def ops(out):
    gu, ou = _reference_modules()
    for tag, (rows, labels, k) in op_cases().items():
        feats = torch.from_numpy(np.ascontiguousarray(rows.transpose(0, 2, 1)))
        lab = torch.from_numpy(labels).view(labels.shape[0], 1, -1)
        cents = _reference_centroids(gu, feats, lab)
        org_xyz = gu.torch_to_numpy(feats[:, :3, :].permute(0, 2, 1))
        idx = ou.get_nearest_neighbor_idx(org_xyz, cents, k)
        cropped = ou.centering_object(ou.get_indexed_features(feats, idx))
        T = [len(c) for c in cents]
        print(f"  {tag}: B={rows.shape[0]} N={rows.shape[1]} k={k} teeth per scan {T}, crops {tuple(cropped.shape)}")
        out[f"op_{tag}_digest"] = np.array([digest(rows, labels)])
        out[f"op_{tag}_k"] = np.array([k])
        out[f"op_{tag}_teeth"] = np.array(T)
        out[f"op_{tag}_cent"] = np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in cents])
        out[f"op_{tag}_idxset"] = pack_sets(np.concatenate(idx))
        out[f"op_{tag}_crop"] = cropped.numpy()[:, :, ::CROP_STRIDE]


def module(out, N=24000):
    gu, ou = _reference_modules()
    import models.modules.grouping_network_module as GM
    import models.modules.cbl_point_transformer.blocks as RB
    import models.fps_grouping_network_model as FM
    sys.path.insert(0, os.path.join(REFERENCE, "train_configs"))
    from tgnet_fps import config
    sys.path.pop(0)
    RP = RB.pointops
    assert GM.__file__.startswith(REFERENCE) and RP.__file__.startswith(REFERENCE)
    rows, labels = synth.labelled_arch(N, 14, seed=707)
    feats = torch.from_numpy(np.ascontiguousarray(rows.T))[None]
    gt = torch.from_numpy(labels).view(1, 1, N)
    keep_nn, keep_mcuda = ou.get_nearest_neighbor_idx, torch.nn.Module.cuda
    keep = _serve_pointops(RP)
    torch.nn.Module.cuda = lambda self, *a, **k: self
    res, crop_idx = {}, None
    try:
        for tag, ftype, dt in (("32", torch.FloatTensor, torch.float32), ("64", torch.DoubleTensor, torch.float64)):
            net = GM.GroupingNetworkModule(config).train()
            names = seeded_fill(net, 71)
            keys = [f"{n}:{'x'.join(map(str, t.shape))}" for n, t in net.state_dict().items()]
            net = net.to(dt)
            if crop_idx is not None:         # the float64 pass crops the points the float32 pass cropped
                ou.get_nearest_neighbor_idx = lambda *a, **k: crop_idx
            t0 = time.time()
            with cpu_as_cuda(ftype):
                x = feats.to(dt)
                o = net([x, gt], test=True)
                crop_idx = o["nn_crop_indexes"]
                clabel = ou.get_indexed_features(gt, crop_idx)                # grouping_network_module.py:74-75
                terms = FM.FpsGroupingNetworkModel.get_loss(
                    types.SimpleNamespace(config=config), o["offset_1"], o["offset_2"], o["sem_1"], o["sem_2"], o["mask_1"], o["mask_2"],
                    gt, clabel, x[:, :3, :], o["cropped_feature_ls"][:, :3, :])
                loss = sum(v * w for v, w in terms.values())
                loss.backward()
            vals = [float(terms[n][0]) for n in LOSS_NAMES]
            print(f"  GroupingNetworkModule fp{tag}: loss {float(loss):.6f} terms {vals} crops {tuple(o['cropped_feature_ls'].shape)} "
                  f"{time.time() - t0:.0f} s")
            res[tag] = dict(terms=[float(loss)] + vals, sem_1=o["sem_1"].detach().numpy(), offset_1=o["offset_1"].detach().numpy(),
                            sem_2=o["sem_2"].detach().numpy(),
                            grads={n: p.grad.detach().numpy().astype(np.float64) for n, p in net.named_parameters() if p.grad is not None},
                            none=[n for n, p in net.named_parameters() if p.grad is None])
    finally:
        RP.furthestsampling, RP.knnquery = keep
        ou.get_nearest_neighbor_idx, torch.nn.Module.cuda = keep_nn, keep_mcuda
    for n_ in ("sem_1", "offset_1", "sem_2"):
        print(f"    {n_:9s} {res['32'][n_].shape}  |fp32 - fp64| / (1 + |fp64|) = {rel_err(res['32'][n_], res['64'][n_]):.2e}")
    out["mod_points"] = np.array([N])
    out["mod_seed"] = np.array([707])
    out["mod_params"] = np.array(names)
    out["mod_state_keys"] = np.array(keys)
    out["mod_digest"] = np.array([digest(rows, labels)])
    out["mod_nn_crop_idxset"] = pack_sets(np.concatenate(crop_idx))
    out["mod_term_names"] = np.array(("loss",) + LOSS_NAMES)
    for tag in ("32", "64"):
        out[f"mod_terms_{tag}"] = np.array(res[tag]["terms"], np.float64)
        out[f"mod_sem_1_{tag}"] = res[tag]["sem_1"][:, :, ::16].astype(np.float32)
        out[f"mod_offset_1_{tag}"] = res[tag]["offset_1"][:, :, ::16].astype(np.float32)
        out[f"mod_sem_2_{tag}"] = res[tag]["sem_2"][:, :, ::16].astype(np.float32)
    gnames = sorted(res["64"]["grads"])
    assert gnames == sorted(res["32"]["grads"])
    out["mod_grad_names"] = np.array(gnames)
    out["mod_grad_none"] = np.array(res["64"]["none"] or [""])
    norms, samples, own = [], [], []
    for n in gnames:
        g64, g32 = res["64"]["grads"][n].reshape(-1), res["32"]["grads"][n].reshape(-1)
        pick = np.linspace(0, g64.size - 1, min(GRAD_SAMPLES, g64.size)).astype(np.int64)
        row64, row32 = np.zeros(GRAD_SAMPLES), np.zeros(GRAD_SAMPLES)
        row64[:pick.size], row32[:pick.size] = g64[pick], g32[pick]
        norms.append([np.linalg.norm(g64), np.linalg.norm(g32), np.linalg.norm(g32 - g64)])
        samples.append(np.stack([row64, row32]))
        own.append(np.linalg.norm(g32 - g64) / max(np.linalg.norm(g64), 1e-30))
    out["mod_grad_norms"] = np.array(norms)
    out["mod_grad_samples"] = np.array(samples)
    own = np.array(own)
    print(f"  {len(gnames)} parameter gradients; reference fp32 vs fp64, relative L2 per parameter: median {np.median(own):.2e}, "
          f"max {own.max():.2e}; without gradient: {len(res['64']['none'])}")


def main():
    torch.set_num_threads(8)
    parts = sys.argv[1:] or ["ops", "module"]
    path = os.path.join(HERE, "reference_cpu_r7_grouping.npz")
    keep = ("op_",) if "ops" not in parts else ("mod_",) if "module" not in parts else ()
    out = {n: v for n, v in np.load(path).items() if n.startswith(keep)} if keep and os.path.exists(path) else {}
    load_reference()
    if "ops" in parts:
        ops(out)
    if "module" in parts:
        torch.set_num_threads(1)        # the CPU backward's threaded scatter-adds are not deterministic: one thread, a reproducible fixture
        module(out)
    np.savez_compressed(path, **out)
    print(f"wrote tests/golden/reference_cpu_r7_grouping.npz ({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
