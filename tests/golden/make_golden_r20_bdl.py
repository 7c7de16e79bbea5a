#!/usr/bin/env python3
"""Fixture of the boundary-sampled training inputs (tests/golden/reference_cpu_r20_bdl.npz), produced by running the REFERENCE's own
BdlGroupingNetworkModel (models/bdl_grouping_netowrk_model.py) on CPU in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_r20_bdl.py [seeds]

open3d, trimesh and pointops are served as for the r16 fixture (make_golden_r16_tgnet._reference_modules: gu.fps is the CPU oracle's
FPS, `.cuda()` is the identity).  __init__ is bypassed -- it loads a checkpoint and walks directories -- and config, the two path maps,
the two constants and base_model are set by hand; base_model is bdl_cases.BaseStandIn with an sklearn KDTree for its crops.  load_mesh,
get_points_cluster_labels and get_boundary_sampled_points run unmodified, with the reference's own augmentator objects as aug_obj.
ou.clustering_points is wrapped so that np.random.seed(PERM_SEED) runs right after it returns: sklearn's k-means++ draws from numpy's
global generator in front of the boundary permutation, this package's k-means does not, and the wrapper puts both at the same state.

  mesh_*    load_mesh's vertices (bit patterns) and labels
  centres_* bdl_cases.centre_table of the three calls' augmentations: what the stand-in moves the teeth onto
  miss_*    the cache-miss call under the MISS_SEED augmentation: every dense vertex's flag (packed bits), the batch points' instance
            labels, the selected rows as indices into the mesh (boundary rows first), the returned feat (bit patterns) and labels.  The
            cache file is asserted to be bdl_cases.rebuild_cache of those rows, so it is not stored.
  hit_*     the second call for the same scan under the HIT_SEED augmentation, served from that cache file: its returns
  val_*     a cache-miss call with aug_obj None and an un-augmented batch (the validation loader's): flags, selected rows, labels;
            the returned feat is asserted to be the mesh's rows, and the cache file to be rebuild_cache of them

Before anything is written the cache-miss case is run under `seeds` (default 20) other np.random.seed values in front of the k-means;
every run must give the same flag on every vertex, the same partition and, behind the re-seeding, the same selection."""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bdl_cases as BC  # noqa: E402
from make_golden_r16_tgnet import REFERENCE, _reference_modules, kdtree_knn  # noqa: E402
from make_golden_r3 import cpu_as_cuda  # noqa: E402
from toothgroupnetwork_amd import augment, preprocess  # noqa: E402


def _reference_model(ou):
    import augmentator
    import models.bdl_grouping_netowrk_model as M
    assert M.__file__.startswith(REFERENCE) and augmentator.__file__.startswith(REFERENCE)
    assert M.ou is ou
    keep = ou.clustering_points

    def clustering_points(*args, **kwargs):
        try:
            return keep(*args, **kwargs)
        finally:
            np.random.seed(BC.PERM_SEED)
    ou.clustering_points = clustering_points
    return M, augmentator


def _model(M, root, cache, centres):
    model = M.BdlGroupingNetworkModel.__new__(M.BdlGroupingNetworkModel)
    model.config = BC.config(root, cache)
    folder = os.path.join(root, BC.PATIENT)
    model.stl_path_map = {BC.BASE_NAME: os.path.join(folder, BC.BASE_NAME + ".obj")}
    model.json_path_map = {BC.BASE_NAME: os.path.join(folder, BC.BASE_NAME + ".json")}
    model.Y_AXIS_MAX, model.Y_AXIS_MIN = preprocess.Y_AXIS_MAX, preprocess.Y_AXIS_MIN
    model.base_model = BC.BaseStandIn(kdtree_knn, centres)
    return model


def _call(M, model, batch_item, seed):
    """-> (feat, labels, locals of get_boundary_sampled_points when it returned)"""
    seen = {}
    code = M.BdlGroupingNetworkModel.get_boundary_sampled_points.__code__

    def profile(frame, event, arg):
        if event == "return" and frame.f_code is code:
            seen.update(frame.f_locals)
    np.random.seed(seed)
    with cpu_as_cuda():
        sys.setprofile(profile)
        try:
            feat, labels = model.get_boundary_sampled_points(batch_item)
        finally:
            sys.setprofile(None)
    return feat, labels, seen


def _rows_in(mesh, selected):
    """The row of `mesh` every row of `selected` is a copy of (the mesh's rows are distinct)."""
    key = {row.tobytes(): i for i, row in enumerate(np.ascontiguousarray(mesh))}
    assert len(key) == mesh.shape[0], "two vertices with the same six values"
    return np.array([key[row.tobytes()] for row in np.ascontiguousarray(selected)], np.int64)


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def _miss(M, R_aug, root, cache, vertices, labels, aug_seed, kmeans_seed):
    """One cache-miss call -> dict of what it gave."""
    own = BC.drawn_augmentation(aug_seed) if aug_seed is not None else None
    item = BC.batch(vertices, labels, root, aug_seed)
    if aug_seed is not None:
        theirs = BC.drawn_augmentation(aug_seed, R_aug)
        probe = vertices[BC.batch_rows()].copy()
        assert np.array_equal(theirs.run(probe.copy()), own.run(probe.copy())), "the two augmentators disagree on this machine"
        item["aug_obj"] = [theirs]
    centres = BC.centre_table(vertices, labels, own)
    model = _model(M, root, cache, centres)
    cache_path = os.path.join(model.config["boundary_sampling_info"]["bdl_cache_path"], BC.BASE_NAME + ".npy")
    assert not os.path.exists(cache_path)
    feat, lab, loc = _call(M, model, item, kmeans_seed)
    assert model.base_model.calls == 1
    feat, lab = feat.numpy(), lab.numpy()
    n_all = BC.INFO["num_of_all_points"]
    assert feat.shape == (1, 6, n_all) and feat.dtype == np.float32 and lab.shape == (1, 1, n_all)
    rows = _rows_in(vertices, loc["sampled_org_feat_cpu"])
    assert np.array_equal(lab.reshape(-1), labels[rows].reshape(-1))
    cached = np.load(cache_path)
    assert cached.dtype == np.float64 and np.array_equal(cached, BC.rebuild_cache(vertices, labels, rows)), "the cache file's layout"
    flags = np.asarray(loc["bd_labels"]) == 1
    nb = loc["bd_auged_org_feat_cpu"].shape[0]
    assert np.all(flags[rows[:nb]]) and not np.any(flags[rows[nb:]]) and len(np.unique(rows)) == n_all
    return dict(flags=flags, point_labels=np.asarray(loc["points_labels"]).astype(np.int64), rows=rows, nb=nb, feat=feat, labels=lab,
                centres=centres, model=model, cache_path=cache_path, item=item)


def main():
    torch.set_num_threads(8)
    seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    gu, ou, _ = _reference_modules()
    M, R_aug = _reference_model(ou)
    out = {}
    with tempfile.TemporaryDirectory() as root:
        BC.write_scan(root)
        probe = _model(M, root, "probe", np.zeros((16, 3), np.float32))
        vertices, labels = probe.load_mesh(BC.BASE_NAME)
        assert vertices.dtype == np.float32 and vertices.shape == (15000, 6) and labels.shape == (15000, 1)
        print(f"  mesh: {vertices.shape[0]} vertices, labels {np.unique(labels).tolist()}")
        assert np.unique(labels).tolist() == [-1] + BC.LABEL_OF_TOOTH.tolist()
        out["mesh_vertices_bits"], out["mesh_labels"] = _bits(vertices), labels.astype(np.int8)

        miss = _miss(M, R_aug, root, "miss", vertices, labels, BC.MISS_SEED, BC.PERM_SEED)
        n_bd = int(miss["flags"].sum())
        print(f"  miss: {n_bd} of {miss['flags'].shape[0]} vertices flagged, {miss['nb']} kept, "
              f"instances {np.unique(miss['point_labels']).tolist()}")
        assert miss["nb"] == min(n_bd, BC.INFO["num_of_bdl_points"]) and 0 < n_bd
        assert len(np.unique(miss["point_labels"])) == BC.TC.TEETH + 1 and miss["point_labels"].min() == -1
        gt = miss["item"]["gt_seg_label"].numpy().reshape(-1)
        assert BC.same_partition(miss["point_labels"], gt), "the stand-in's blobs are the ground-truth teeth"
        for s in range(seeds):
            other = _miss(M, R_aug, root, f"seed{s}", vertices, labels, BC.MISS_SEED, 1000 + s)
            assert np.array_equal(other["flags"], miss["flags"]), f"np.random.seed({1000 + s}) gives other flags"
            assert BC.same_partition(other["point_labels"], miss["point_labels"]) and np.array_equal(other["rows"], miss["rows"])
            assert np.array_equal(_bits(other["feat"]), _bits(miss["feat"]))
        print(f"  miss: the same flags, partition and selection under {seeds} other np.random.seed values in front of the k-means")
        out["miss_flags"], out["miss_point_labels"] = np.packbits(miss["flags"]), miss["point_labels"].astype(np.int8)
        out["miss_rows"], out["miss_boundary_count"] = miss["rows"].astype(np.int16), np.array([miss["nb"]])
        out["miss_feat_bits"], out["miss_labels"] = _bits(miss["feat"]), miss["labels"].astype(np.int8)
        out["centres_miss"] = miss["centres"]

        # the second call for the same scan: served from the file the first one wrote
        hit_item = BC.batch(vertices, labels, root, BC.HIT_SEED)
        hit_item["aug_obj"] = [BC.drawn_augmentation(BC.HIT_SEED, R_aug)]
        feat, lab, _ = _call(M, miss["model"], hit_item, 7)
        assert miss["model"].base_model.calls == 1, "a cache hit does not run the base model"
        assert feat.dtype == torch.float32 and np.array_equal(lab.numpy(), miss["labels"])
        out["hit_feat_bits"] = _bits(feat.numpy())
        own = BC.drawn_augmentation(BC.HIT_SEED).run(np.load(miss["cache_path"])[:, :6].copy()).astype(np.float32)
        print(f"  hit: max |reference - package augmentation| = {np.abs(own.T[None] - feat.numpy()).max():.3g}")

        # the validation loader's batch: no augmentation
        val = _miss(M, R_aug, root, "val", vertices, labels, None, BC.PERM_SEED)
        assert np.array_equal(_bits(val["feat"][0].T), _bits(vertices[val["rows"]])), "without augmentation the rows are the mesh's"
        print(f"  val: {int(val['flags'].sum())} vertices flagged, {val['nb']} kept")
        out["val_flags"], out["val_rows"] = np.packbits(val["flags"]), val["rows"].astype(np.int16)
        out["val_boundary_count"], out["val_labels"] = np.array([val["nb"]]), val["labels"].astype(np.int8)
        out["centres_val"] = val["centres"]
        assert augment.__file__.startswith(os.path.dirname(os.path.dirname(HERE)))
    path = os.path.join(HERE, "reference_cpu_r20_bdl.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"wrote tests/golden/reference_cpu_r20_bdl.npz ({size / 1e6:.2f} MB, {len(out)} arrays)")
    assert size < 1_000_000


if __name__ == "__main__":
    main()
