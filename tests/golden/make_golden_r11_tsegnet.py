#!/usr/bin/env python3
"""Fixtures of tsegnet's two-stage module and inference pipeline (tests/golden/reference_cpu_r11_tsegnet.npz), produced by running the
REFERENCE's own classes on CPU in the build container (open3d / trimesh stubbed, `.cuda()` served, the networks replaced by stubs):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_r11_tsegnet.py

  mod_*   the reference's TSegNetModule.forward([feats, labels]) (models/modules/tsegnet.py:35-88) on tsegnet_cases.module_case(): the
          centroid stage is a stub returning the case's l0_points, l3_xyz, offset and dist, the segmentation stage a stub recording its
          input; np.random.seed(PERM_SEED) in front, so that the 8-of-T choice is reproducible.  Stored: the kept mask, DBSCAN's labels on
          the kept points, all cluster centres' float32 bits, the chosen permutation, the crop index SETS (crop_cases.pack_sets), every
          64th column of the crop tensor and of cluster_gt_seg_label (columns sorted by point index first, so that the order among equal
          distances does not matter), and every 4th column of the distance channel twice: the reference's float32 and the reference's
          get_ddf evaluated on float64 inputs.  Also the reference class's state_dict names and shapes.
  paint_* the painting loop of inference_pipelines/inference_pipeline_tsegnet.py:60-66 (restated verbatim) on the module case's crops,
          with tsegnet_cases.fixed_seg's mask logits and ids and PLANTED written into them: the painted class per scan point.
  pipe_*  the reference's InferencePipeLine.__call__ (tsegnet) on a synthetic OBJ with a TSegNetModule whose two stages are
          tsegnet_cases.fixed_cent / fixed_seg and whose get_ddf is the reference's own: `sem` per vertex.  Asserted as for the module case: at least 12 kept proposals, no
          pair at eps, the k-th and (k+1)-th distances of every crop differ.
The generator asserts, before writing, that the reference alone defines a unique answer (see the asserts)."""
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("TGN_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from sklearn.cluster import DBSCAN  # noqa: E402

import tsegnet_cases as TC  # noqa: E402
import tsegnet_ref  # noqa: E402
from crop_cases import pack_sets  # noqa: E402
from make_golden import load_reference  # noqa: E402
from make_golden_r2_io import _stub_open3d  # noqa: E402
from make_golden_r3 import cpu_as_cuda  # noqa: E402
from make_golden_r9_cluster import _no_boundary_pairs  # noqa: E402
from oracle import cpu as O, meshio as OM  # noqa: E402
from toothgroupnetwork_amd import synth  # noqa: E402

CROP_STRIDE, DDF_STRIDE = 64, 4
CONFIG = {"run_tooth_segmentation_module": True}


def _reference_modules():
    load_reference()          # the reference's external_libs, not this repository's drop-in of the same name
    sys.modules["open3d"] = _stub_open3d([])
    tri = types.ModuleType("trimesh")

    def load_mesh(path, process=False):
        v, f = OM.read_obj(path)
        return types.SimpleNamespace(vertices=v, faces=f - 1)
    tri.load_mesh = load_mesh
    sys.modules["trimesh"] = tri
    if REFERENCE not in sys.path:
        sys.path.append(REFERENCE)
    import gen_utils as gu
    import ops_utils as ou
    import models.modules.tsegnet as TM
    assert all(m.__file__.startswith(REFERENCE) for m in (gu, ou, TM, sys.modules[TM.square_distance.__module__]))
    return gu, ou, TM


def _unique_kth(xyz, cents, k):
    """The k-th and (k+1)-th float64 squared distances of every crop differ: the index SET is unique."""
    x = xyz.astype(np.float64)
    gaps = []
    for c in cents.astype(np.float64):
        d = ((0.0 + (x[:, 0] - c[0]) ** 2) + (x[:, 1] - c[1]) ** 2) + (x[:, 2] - c[2]) ** 2
        s = np.partition(d, (k - 1, k))
        gaps.append(s[k] - s[k - 1])
    assert min(gaps) > 0, "a distance tie across the k-th boundary"
    return min(gaps)


def module_part(out, gu, ou, TM):
    case = TC.module_case()
    t = {n: torch.from_numpy(v) for n, v in case.items()}
    net = TM.TSegNetModule(CONFIG)
    out["mod_state_keys"] = np.array([f"{n}:{'x'.join(map(str, v.shape))}" for n, v in net.state_dict().items()])
    seen = {}
    net.cent_module = TC.Stage(lambda x: (t["l0_points"], None, x[:, :3, :], t["l3_xyz"], t["offset"], t["dist"]))

    def seg(x):
        seen["crops"] = x
        return None, None, None, None
    net.seg_module = TC.Stage(seg)
    keep_nn = ou.get_nearest_neighbor_idx

    def record_nn(*a, **k):
        seen["idx"] = keep_nn(*a, **k)
        return seen["idx"]
    ou.get_nearest_neighbor_idx = record_nn
    try:
        np.random.seed(TC.PERM_SEED)
        with cpu_as_cuda():
            o = net([t["feats"], t["labels"]])
    finally:
        ou.get_nearest_neighbor_idx = keep_nn
    crops, idx = seen["crops"].numpy(), np.asarray(seen["idx"][0])
    centre_out = np.asarray(o["center_points"])
    assert centre_out.dtype == np.float32 and centre_out.shape == (1, TC.MAX_CROPS, 3)
    # tsegnet.py:57-66 restated on the same values, for what the module does not return
    moved = gu.torch_to_numpy(t["l3_xyz"] + t["offset"]).T.reshape(-1, 3)
    kept = gu.torch_to_numpy(t["dist"]).reshape(-1) < 0.3
    moved = moved[kept, :]
    db = DBSCAN(eps=0.05, min_samples=3).fit(moved, 3)
    cents = np.array([moved[db.labels_ == lab].mean(axis=0) for lab in np.unique(db.labels_) if lab != -1])
    np.random.seed(TC.PERM_SEED)
    perm = np.random.permutation(cents.shape[0])[:TC.MAX_CROPS]
    assert np.array_equal(cents[perm].view(np.uint32), centre_out[0].view(np.uint32)), "the restated centres are not the module's"
    f0, f1, fn = TC.FORCED
    assert not kept[f0] and kept[f1] and not kept[fn], "float32(0.3) and NaN are dropped, the float32 below 0.3 is kept"
    assert kept.sum() >= 12, "below 12 points sklearn switches to a brute-force distance form"
    _no_boundary_pairs(moved, 0.05, "module")
    noise, T = int(np.sum(db.labels_ == -1)), cents.shape[0]
    assert noise >= 1 and T >= 9, (noise, T)
    xyz = case["feats"][0, :3].T
    gap = _unique_kth(xyz, centre_out[0], TC.CROP_K)
    assert np.array_equal(crops[:, :3], np.stack([case["feats"][0, :3][:, i] for i in idx]))
    ddf32 = crops[:, 35]
    assert not np.isnan(ddf32).any()
    with cpu_as_cuda():
        ddf64 = net.get_ddf(torch.from_numpy(crops[:, :3]).double().permute(0, 2, 1), centre_out.astype(np.float64)).numpy()[:, 0]
    assert ddf64.dtype == np.float64
    err = np.abs(ddf32 - ddf64)
    multi = np.bincount(idx.reshape(-1), minlength=TC.N_POINTS)
    print(f"  mod: kept {kept.sum()} of {kept.size}, clusters {T}, noise {noise}, chosen {perm.tolist()}, crops {crops.shape}, smallest k-th gap "
          f"{gap:.2e}, ddf fp32 vs fp64 max {err.max():.2e} rms {np.sqrt(np.mean(err ** 2)):.2e}, points in >= 2 crops {np.sum(multi >= 2)}")
    out["mod_digest"] = np.array([TC.case_digest(case)])
    out["mod_kept"] = np.packbits(kept)
    out["mod_db_labels"] = db.labels_.astype(np.int16)
    out["mod_cent_bits"] = cents.astype(np.float32).view(np.uint32)
    out["mod_perm"] = perm.astype(np.int16)
    out["mod_idxset"] = pack_sets(idx)
    out["mod_crop"] = tsegnet_ref.sorted_columns(crops, idx)[:, :35, ::CROP_STRIDE]
    out["mod_crop_labels"] = tsegnet_ref.sorted_columns(o["cluster_gt_seg_label"].numpy(), idx)[:, :, ::CROP_STRIDE].astype(np.int8)
    out["mod_ddf32"] = tsegnet_ref.sorted_columns(ddf32[:, None], idx)[:, 0, ::DDF_STRIDE]
    out["mod_ddf64"] = tsegnet_ref.sorted_columns(ddf64[:, None], idx)[:, 0, ::DDF_STRIDE]
    return crops, idx


def paint_part(out, gu, crops, idx):
    cropped_feature_ls = torch.from_numpy(crops)
    _, _, pd_2, id_pred = TC.fixed_seg(cropped_feature_ls)
    pd_2 = torch.from_numpy(TC.plant(pd_2.numpy(), idx))
    nn_crop_indexes = [idx]
    # inference_pipeline_tsegnet.py:60-66, verbatim
    pred_labels = np.zeros(TC.N_POINTS)
    for i in range(cropped_feature_ls.shape[0]):
        pred_bin_labels = np.zeros(cropped_feature_ls[i].shape[1])
        pred_bin_labels[gu.torch_to_numpy(torch.sigmoid(pd_2[i].reshape(-1))) > 0.5] = 1
        pred_labels[nn_crop_indexes[0][i][pred_bin_labels == 1]] = gu.torch_to_numpy(id_pred.argmax(axis=1))[i]
    mask = torch.sigmoid(pd_2[:, 0]).numpy() > 0.5
    cols = np.argsort(idx[-1], kind="stable")[:len(TC.PLANTED)]
    assert mask[-1, cols].tolist() == [False, False, False, False, True, True], mask[-1, cols]
    ids = id_pred.argmax(axis=1).numpy()
    first = np.zeros(TC.N_POINTS, np.int64)                    # the id of the first crop that paints a point
    clash = np.zeros(TC.N_POINTS, bool)
    for i in range(idx.shape[0]):
        p = idx[i][mask[i]]
        clash[p] |= (first[p] != 0) & (first[p] != ids[i])
        first[p] = np.where(first[p] == 0, ids[i], first[p])
    covered = np.bincount(idx.reshape(-1), minlength=TC.N_POINTS) > 0
    assert clash.sum() >= 100, f"only {clash.sum()} points are painted by two crops with different ids"
    assert np.any(covered & (pred_labels == 0)), "no point lies in a crop and is masked out everywhere"
    print(f"  paint: ids {ids.tolist()}, masked per crop {mask.sum(1).tolist()}, painted {np.sum(pred_labels > 0)}, by two crops with different "
          f"ids {clash.sum()}, in a crop but unpainted {np.sum(covered & (pred_labels == 0))}")
    out["paint_labels"] = pred_labels.astype(np.int8)


def pipeline_part(out, gu, TM):
    gu.fps = lambda xyz, npoint: O.furthestsampling(np.ascontiguousarray(np.asarray(xyz), dtype=np.float32), [len(xyz)], [npoint]).reshape(-1)
    from inference_pipelines.inference_pipeline_tsegnet import InferencePipeLine
    net = TM.TSegNetModule(CONFIG)
    seen = {}

    def cent(x):
        seen["feats"] = x
        return TC.fixed_cent(x)
    net.cent_module, net.seg_module = TC.Stage(cent), TC.Stage(TC.fixed_seg)
    with tempfile.TemporaryDirectory() as root:
        path = os.path.join(root, "scan.obj")
        with open(path, "w") as f:
            f.write(synth.obj_text(TC.MESH[0], TC.MESH[1], TC.MESH[2], "plain", with_tail=False))
        with cpu_as_cuda():
            res = InferencePipeLine(net)(path)
    sem = np.asarray(res["sem"]).reshape(-1)
    assert sem.shape[0] == TC.MESH[0] * TC.MESH[1] and np.array_equal(sem, np.asarray(res["ins"]).reshape(-1))
    # inference_pipeline_tsegnet.py:37-47 restated on the values the centroid stage saw: the answer is unique as in the module case
    _, _, l0_xyz, l3_xyz, offset, dist = TC.fixed_cent(seen["feats"])
    moved = gu.torch_to_numpy(l3_xyz + offset).T.reshape(-1, 3)
    moved = moved[gu.torch_to_numpy(dist).reshape(-1) < 0.3, :]
    assert len(moved) >= 12, "below 12 points sklearn switches to a brute-force distance form"
    _no_boundary_pairs(moved, 0.05, "pipeline")
    db = DBSCAN(eps=0.05, min_samples=3).fit(moved, 3)
    cents = np.array([moved[db.labels_ == lab].mean(axis=0) for lab in np.unique(db.labels_) if lab != -1])
    gap = _unique_kth(l0_xyz[0].numpy().T, cents, TC.CROP_K)
    print(f"  pipe: kept {len(moved)} of {TC.N_COARSE}, clusters {len(cents)}, noise {int(np.sum(db.labels_ == -1))}, smallest k-th gap {gap:.2e}")
    vals, cnt = np.unique(sem, return_counts=True)
    print(f"  pipe: {sem.shape[0]} vertices, labels {dict(zip(vals.astype(int).tolist(), cnt.tolist()))}")
    assert len(vals) >= 4 and vals.min() == 0, "the pipeline case must paint several teeth and leave gingiva"
    out["pipe_sem"] = sem.astype(np.int16)
    out["pipe_mesh"] = np.array(TC.MESH)


def main():
    torch.set_num_threads(8)
    out = {}
    gu, ou, TM = _reference_modules()
    keep = torch.nn.Module.cuda
    torch.nn.Module.cuda = lambda self, *a, **k: self
    try:
        crops, idx = module_part(out, gu, ou, TM)
        paint_part(out, gu, crops, idx)
        pipeline_part(out, gu, TM)
    finally:
        torch.nn.Module.cuda = keep
    path = os.path.join(HERE, "reference_cpu_r11_tsegnet.npz")
    np.savez_compressed(path, **out)
    print(f"wrote tests/golden/reference_cpu_r11_tsegnet.npz ({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
