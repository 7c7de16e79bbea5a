"""The scripted case of the boundary-sampled training inputs (training.BoundarySampler), shared by tests/golden/make_golden_r20_bdl.py
(which runs the REFERENCE's BdlGroupingNetworkModel.load_mesh and get_boundary_sampled_points on it, on the CPU) and the tests (which
run this package's sampler, on the host and on the GPU).

  mesh      tgnet_cases.MESHES["small"], the 15 000-vertex synth.obj_text horseshoe, written as <root>/<PATIENT>/<BASE_NAME>.obj and
            .json.  A vertex's tooth is tgnet_cases.tooth_of of its coordinates in the inference pipeline's frame, decided once, here.
            The json is a lower jaw's: FDI 31..37 for tgnet_cases' teeth 0..6, 41..47 for teeth 7..13, 0 for gingiva, so that
            load_mesh takes its `- 20` path and gives the labels 0..6, 8..14 and -1.
  batch     BATCH_POINTS rows of the normalised mesh (a seeded choice, ascending) with their labels; with a seed, put through the
            default augmentation chain after np.random.seed(seed), the applied object handed on as aug_obj: what
            training.DentalModelGenerator and collate_fn make of one preprocessed scan.
  base      BaseStandIn: a GroupingNetworkModule's call and output dict that gives the same bits on the CPU and on the GPU under any
            augmentation, because it never decides anything from a coordinate: a point's tooth is its LABEL; offset_1 moves every
            tooth point onto centres[label] by one float32 subtraction (blobs one rounding wide: any seeding of k-means finds the one
            partition); the crops are the K_CROP nearest points of the present teeth's centres by the caller's kNN; sem_2 is (1, 0)
            for gingiva and (0, 1) for a tooth's point, as in tgnet_cases.StandIn.  `centres` is the (16, 3) float32 table by label:
            centre_table(vertices, labels, aug_obj) on the host -- the maker stores the tables in the fixture and the tests read them from there.
"""
import copy
import json
import os

import numpy as np
import torch

import tgnet_cases as TC
import training_cases as C
from toothgroupnetwork_amd import augment, preprocess, synth

PATIENT, JAW = "P20", "lower"
BASE_NAME = f"{PATIENT}_{JAW}"
INFO = {"bdl_ratio": 0.7, "num_of_bdl_points": 4096, "num_of_all_points": 6144}
BATCH_POINTS, BATCH_PICK_SEED = 6144, 2001
MISS_SEED, HIT_SEED = 2010, 2011                    # np.random.seed in front of the augmentation draws of the two augmented batches
PERM_SEED = TC.PERM_SEED                            # np.random.seed right behind the k-means: the boundary permutation's state
LABEL_OF_TOOTH = np.array([t if t < 7 else t + 1 for t in range(TC.TEETH)], np.int64)      # load_mesh's label of tgnet_cases' tooth


def _inference_frame(raw):
    """Raw vertices -> the inference pipeline's frame (centred, the mesh's own y range on [-0.8, 1]), in which tgnet_cases' boxes lie."""
    xyz = raw - raw.mean(axis=0)
    lo, hi = xyz[:, 1].min(), xyz[:, 1].max()
    return ((xyz - lo) / (hi - lo) * 1.8 - 0.8).astype(np.float32)


def write_scan(root):
    """Writes the mesh and its labels under root -> (obj path, json path)."""
    nu, nv, seed = TC.MESHES["small"]
    folder = os.path.join(root, PATIENT)
    os.makedirs(folder, exist_ok=True)
    obj_path, json_path = os.path.join(folder, BASE_NAME + ".obj"), os.path.join(folder, BASE_NAME + ".json")
    with open(obj_path, "w") as f:
        f.write(synth.obj_text(nu, nv, seed, "plain", with_tail=False))
    tooth = TC.tooth_of(torch.from_numpy(_inference_frame(preprocess.read_obj(obj_path)[0]))).numpy()
    fdi = np.where(tooth < 0, 0, np.where(tooth < 7, 31 + tooth, 41 + tooth - 7))
    with open(json_path, "w") as f:
        json.dump({"id_patient": PATIENT, "jaw": JAW, "labels": fdi.tolist(), "instances": fdi.tolist()}, f)
    return obj_path, json_path


def config(root, cache="cache"):
    info = dict(INFO, orginal_data_obj_path=root, orginal_data_json_path=root, bdl_cache_path=os.path.join(root, "_" + cache))
    return {"boundary_sampling_info": info}


def batch_rows():
    return np.sort(np.random.default_rng(BATCH_PICK_SEED).choice(TC.MESHES["small"][0] * TC.MESHES["small"][1], BATCH_POINTS, replace=False))


def drawn_augmentation(seed, aug=augment):
    """The default chain with the values np.random.seed(seed) gives it; `aug`: the module the chain's string is evaluated against."""
    obj = eval(C.DEFAULT_CHAIN, {"__builtins__": {}, "aug": aug})  # noqa: S307
    np.random.seed(seed)
    obj.reload_vals()
    return obj


def batch(vertices, labels, root, seed=None, aug=augment):
    """vertices (n, 6) float32, labels (n, 1): load_mesh's -> the collated batch of one scan; seed None: the validation loader's."""
    pick = batch_rows()
    rows = np.ascontiguousarray(vertices[pick], dtype=np.float32)
    aug_obj = None
    if seed is not None:
        aug_obj = drawn_augmentation(seed, aug)
        rows = aug_obj.run(rows)
    return {"feat": torch.from_numpy(np.ascontiguousarray(rows.T))[None], "aug_obj": [copy.deepcopy(aug_obj)],
            "gt_seg_label": torch.from_numpy(np.ascontiguousarray(labels[pick].astype(np.int64).reshape(1, 1, -1))),
            "mesh_path": [os.path.join(root, "preprocessed", BASE_NAME + "_sampled_points.npy")]}


def centre_table(vertices, labels, aug_obj=None):
    """(16, 3) float32: row `label` holds the mean of that label's vertices of the mesh (load_mesh's), augmented; the rows of absent
    labels are zero."""
    present = np.unique(labels[labels >= 0])
    centres = np.stack([vertices[labels.reshape(-1) == label, :3].astype(np.float64).mean(axis=0) for label in present]).astype(np.float32)
    if aug_obj is not None:
        centres = aug_obj.run(centres)
    table = np.zeros((16, 3), np.float32)
    table[present] = centres
    return table


class BaseStandIn:
    """knn(xyz (N, 3) float32 tensor, centres (T, 3) float32 tensor, k) -> (T, k) int64 indices on xyz's device.  `calls` counts."""

    def __init__(self, knn, centres, k=TC.K_CROP):
        self.knn, self.centres, self.k, self.calls = knn, np.asarray(centres, np.float32), k, 0

    def cuda(self):
        return self

    def __call__(self, inputs, test=False):
        self.calls += 1
        feats, labels = inputs[0], inputs[1]
        assert feats.dim() == 3 and feats.shape[0] == 1 and feats.dtype == torch.float32
        dev = feats.device
        xyz = feats[0, :3].t().contiguous()
        label = labels.reshape(-1).to(torch.int64)
        tooth = label >= 0
        table = torch.from_numpy(self.centres).to(dev)
        to_centre = table[label.clamp(min=0)] - xyz
        offset = torch.where(tooth[:, None], to_centre, torch.zeros_like(to_centre))
        present = torch.unique(label[tooth])
        idx = self.knn(xyz, table[present].contiguous(), self.k)
        fg = tooth[idx]
        sem_2 = torch.stack([~fg, fg], dim=1).to(torch.float32)
        return {"sem_1": None, "offset_1": offset.t().contiguous()[None], "mask_1": None, "first_features": None, "sem_2": sem_2,
                "offset_2": None, "mask_2": None, "nn_crop_indexes": [idx]}


def same_partition(a, b):
    """Two labelings of the same points describe one partition: a bijection between their values maps one onto the other."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    pairs = np.unique(np.stack([a, b], axis=1), axis=0)
    return a.shape == b.shape and len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


def rebuild_cache(vertices, labels, rows):
    """The cache file's array from the mesh and the selected rows: (len(rows), 7) float64."""
    return np.concatenate([vertices[rows], labels[rows]], axis=1).astype(np.float64)
