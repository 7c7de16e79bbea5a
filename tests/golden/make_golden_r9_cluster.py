#!/usr/bin/env python3
"""Fixtures of the clustering of tgnet_fps's unlabelled path (tests/golden/reference_cpu_r9_cluster.npz), produced on CPU with sklearn
and the REFERENCE's own Python in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_r9_cluster.py

  db_*   sklearn's DBSCAN(eps, min_samples).fit on every case of cluster_cases.dbscan_cases (per cloud for the ragged batch): labels
         as int16, core flags packed with packbits.
  cl_*   the reference's ops_utils.get_clustering_labels on cluster_cases.labelling_cases (moved points, classes), and sklearn's
         MeanShift(0.07) on the points of the cluster the split case re-splits (labels_, cluster_centers_).
  mod_*  the reference's GroupingNetworkModule.forward([feats]) -- the unlabelled path, grouping_network_module.py:57-69 -- on the
         split case's scan, first_ins_cent_model replaced by a stub returning the case's sem_1 (one-hot classes) and offset_1 (moved -
         xyz), second_ins_cent_model by a stub recording its input: the centroids' float32 bits, the nn_crop_indexes sets
         (crop_cases.pack_sets) and every 64th column of the crops.
Every input is stored as a digest (cluster_cases.py rebuilds it).  The generator asserts that each case exercises its branch and that
no pair's rdist lies within 1e-12 relative of eps^2 (the lattice excepted: it is AT eps on purpose) and no split ratio within 1e-6 of 8.
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
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from sklearn.cluster import DBSCAN, MeanShift  # noqa: E402
from sklearn.decomposition import PCA  # noqa: E402

import cluster_ref  # noqa: E402
from cluster_cases import dbscan_cases, digest, labelling_cases, pack_core, pack_labels  # noqa: E402
from crop_cases import pack_sets  # noqa: E402
from make_golden_r2_io import _stub_open3d  # noqa: E402

CROP_STRIDE = 64
CROP_K = 3072
CONFIG = {"model_parameter": {"input_feat": 6, "stride": [1, 4, 4, 4, 4], "nsample": [36, 24, 24, 24, 24], "blocks": [2, 3, 4, 6, 3],
                              "block_num": 5, "planes": [32, 64, 128, 256, 512], "crop_sample_size": CROP_K}}


def _reference_modules():
    sys.modules["open3d"] = _stub_open3d([])
    sys.modules.setdefault("trimesh", types.ModuleType("trimesh"))
    if REFERENCE not in sys.path:
        sys.path.append(REFERENCE)
    import gen_utils as gu
    import ops_utils as ou
    assert ou.__file__.startswith(REFERENCE) and gu.__file__.startswith(REFERENCE)
    return gu, ou


def _no_boundary_pairs(x, eps, tag):
    x = np.asarray(x, np.float64)
    e2 = eps * eps
    for s in range(0, len(x), 512):
        r = x[s:s + 512]
        d = r[:, None, :] - x[None, :, :]
        rd = ((0.0 + d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert not np.any(np.abs(rd - e2) <= 1e-12 * e2), f"{tag}: a pair at eps within 1e-12"


def dbscan_part(out):
    for tag, (x, eps, ms, offset) in dbscan_cases().items():
        labels, core, lo = [], [], 0
        for hi in offset:
            r = DBSCAN(eps=eps, min_samples=ms).fit(x[lo:hi])
            c = np.zeros(hi - lo, bool)
            c[r.core_sample_indices_] = True
            labels.append(r.labels_)
            core.append(c)
            lo = hi
        labels, core = np.concatenate(labels), np.concatenate(core)
        if tag != "lattice":
            _no_boundary_pairs(x, eps, tag)
        nb = np.sum((labels >= 0) & ~core)
        print(f"  db {tag}: N={len(x)} eps={eps} min_samples={ms} clouds={len(offset)} clusters={labels.max() + 1} core={core.sum()} "
              f"border={nb} noise={np.sum(labels < 0)}")
        if tag == "noise":
            assert labels.max() == -1
        if tag == "ms1":
            assert core.all()
        if tag == "lattice":
            assert core.any() and nb > 0
        if tag == "border":
            mid = np.arange(480, 489)                   # the nine points between the chains
            m = cluster_ref.neighbour_matrix(x, eps, mid)
            two = [len(set(labels[np.flatnonzero(row & core)])) for row in m]
            assert not core[mid].any() and min(two) == 2 and np.all(labels[mid] == 0), "border points must see two clusters"
        if tag == "chain":
            assert labels.max() == 0, "the chain must join the two blobs"
        out[f"db_{tag}_digest"] = np.array([digest(x)])
        out[f"db_{tag}_labels"] = pack_labels(labels)
        out[f"db_{tag}_core"] = pack_core(core)


def _ratios(moved, cls):
    """ops_utils.py:97-128 restated, to see how far the split test's ratios are from 8."""
    fg = moved[cls != 0].astype(np.float64)
    r = DBSCAN(eps=0.03, min_samples=30).fit(moved[cls != 0])
    core = np.zeros(len(fg), bool)
    core[r.core_sample_indices_] = True
    ev = np.array([PCA(3).fit(fg[core & (r.labels_ == k)]).explained_variance_[0] for k in range(r.labels_.max() + 1)])
    s = np.sort(ev)[::-1]
    return s[:3] / s[3:].mean(), r


def labelling_part(out, ou):
    for tag, (moved, cls) in labelling_cases().items():
        ratios, r = _ratios(moved, cls)
        assert np.all(np.abs(ratios - 8) > 1e-6 * 8), f"{tag}: a split ratio within 1e-6 of 8"
        got = ou.get_clustering_labels(moved, cls)
        noise = np.sum(r.labels_ == -1)
        split = int(np.sum(ratios > 8))
        print(f"  cl {tag}: fg={len(got)} clusters={r.labels_.max() + 1} ratios={np.round(ratios, 2)} split={split} votes={noise} "
              f"final labels={len(np.unique(got))}")
        assert noise > 0, "votes must be cast"
        assert split == (1 if tag == "split" else 0)
        out[f"cl_{tag}_digest"] = np.array([digest(moved, cls)])
        out[f"cl_{tag}_labels"] = pack_labels(got)
        if tag == "split":
            fg = moved[cls != 0].astype(np.float64)
            lab = r.labels_
            ev = np.array([PCA(3).fit(fg[np.isin(np.arange(len(fg)), r.core_sample_indices_) & (lab == k)]).explained_variance_[0]
                           for k in range(lab.max() + 1)])
            c = int(np.argmax(ev))
            ms = MeanShift(bandwidth=0.07).fit(fg[lab == c])
            sizes = np.bincount(ms.labels_)
            print(f"    MeanShift on cluster {c} ({np.sum(lab == c)} points): {len(ms.cluster_centers_)} centres, sizes {sizes}")
            assert len(ms.cluster_centers_) >= 2 and len(set(sizes.tolist())) == len(sizes)
            out["ms_cluster"] = np.array([c])
            out["ms_labels"] = pack_labels(ms.labels_)
            out["ms_centers"] = ms.cluster_centers_


class Stub(torch.nn.Module):
    """A stage of GroupingNetworkModule replaced by a function of its input list."""

    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, inputs, **kwargs):
        return self.fn(inputs)


def module_part(out, gu, ou):
    import models.modules.grouping_network_module as GM
    moved, cls = labelling_cases()["split"]
    from toothgroupnetwork_amd import synth
    rows, _ = synth.labelled_arch(24000, 14, seed=912)
    feats = torch.from_numpy(np.ascontiguousarray(rows.T))[None]
    sem_1 = torch.from_numpy(np.eye(10, dtype=np.float32)[cls].T.copy())[None]
    offset_1 = torch.from_numpy(np.ascontiguousarray((moved - rows[:, :3]).T))[None]
    assert np.array_equal((feats[0, :3].numpy().T + offset_1[0].numpy().T), moved), "moved = xyz + offset must be exact in float32"
    keep = torch.nn.Module.cuda
    torch.nn.Module.cuda = lambda self, *a, **k: self
    try:
        net = GM.GroupingNetworkModule(CONFIG)
    finally:
        torch.nn.Module.cuda = keep
    seen = {}
    net.first_ins_cent_model = Stub(lambda inp: (sem_1, offset_1, None, None))

    def second(inp):
        seen["crops"] = inp[0]
        return None, None, None, None
    net.second_ins_cent_model = Stub(second)
    o = net([feats])
    crops = seen["crops"].numpy()
    # the centroids the module computed (grouping_network_module.py:64-68), restated on the same values for the fixture
    fl = ou.get_clustering_labels(moved, cls)
    fg = moved[cls != 0]
    cents = np.array([np.mean(fg[fl == i, :], axis=0) for i in np.unique(fl)], np.float32)
    print(f"  mod: {len(cents)} centroids, crops {crops.shape}")
    out["mod_digest"] = np.array([digest(rows, moved, cls)])
    out["mod_cent_bits"] = cents.view(np.uint32)
    out["mod_idxset"] = pack_sets(np.concatenate(o["nn_crop_indexes"]))
    out["mod_crop"] = crops[:, :, ::CROP_STRIDE]


def main():
    torch.set_num_threads(8)
    out = {}
    gu, ou = _reference_modules()
    dbscan_part(out)
    labelling_part(out, ou)
    module_part(out, gu, ou)
    path = os.path.join(HERE, "reference_cpu_r9_cluster.npz")
    np.savez_compressed(path, **out)
    print(f"wrote tests/golden/reference_cpu_r9_cluster.npz ({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
