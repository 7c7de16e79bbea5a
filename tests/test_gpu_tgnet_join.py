"""GPU: every function of toothgroupnetwork_amd/tgnet.py against the numpy restatement of its contract (tests/tgnet_ref.py) and against
the rows the reference's own pipeline produced on the same case (tests/golden/make_golden_r16_tgnet.py: the locals of its methods)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tgnet_cases as TC  # noqa: E402
import tgnet_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r16_tgnet.npz")))


@pytest.fixture(scope="module")
def main_case(dev, fx, tmp_path_factory):
    """The main mesh as the pipeline sees it up to the first module: dense rows, the 24 000 sampled rows, the module's input."""
    from toothgroupnetwork_amd import inference, preprocess, resample, synth
    path = str(tmp_path_factory.mktemp("tgnet") / "scan.obj")
    nu, nv, seed = TC.MESHES["main"]
    with open(path, "w") as f:
        f.write(synth.obj_text(nu, nv, seed, "plain", with_tail=False))
    _, mesh = preprocess.read_txt_obj_ls(path, ret_mesh=True)
    dense = np.concatenate([inference.normalise_for_inference(mesh["vertices"]), mesh["vertex_normals"]], axis=1)
    sampled = dense[resample.fps(dense[:, :3], 24000)[:24000]]
    assert np.array_equal(sampled[:, :3].astype(np.float32), fx["first_xyz"]), "the sampled points are not the reference run's"
    inp = torch.from_numpy(np.ascontiguousarray(sampled.astype("float32"))[None]).to(dev).permute(0, 2, 1).contiguous()
    return {"dense": dense, "sampled": sampled, "inp": inp}


# ---------------------------------------------------------------------------------------------------------------------------
# crop_vote
# ---------------------------------------------------------------------------------------------------------------------------
def test_crop_vote_adds_crop_after_crop(dev):
    from toothgroupnetwork_amd import tgnet
    rng = np.random.default_rng(11)
    idx = np.stack([rng.permutation(19)[:8] for _ in range(3)]).astype(np.int64)       # 3 crops of 8 over points 0..18; point 19 in none
    sem_2 = rng.normal(size=(3, 2, 8)).astype(np.float32)
    shared = np.intersect1d(idx[0], idx[1])
    assert len(shared) >= 1 and len(np.unique(idx)) < 20
    p = shared[0]                                                                      # a point whose two sums are equal: channel 0
    for t in range(3):
        sem_2[t, 1, idx[t] == p] = sem_2[t, 0, idx[t] == p]
    want_mask, want_sums = R.crop_vote(sem_2, idx, 20)
    mask, sums = tgnet.crop_vote(torch.from_numpy(sem_2).to(dev), [torch.from_numpy(idx).to(dev)], 20)
    assert sums.dtype == torch.float32 and mask.dtype == torch.int64
    assert np.array_equal(sums.cpu().numpy().view(np.uint32), want_sums.view(np.uint32)), "the sums are the loop's, bit for bit"
    assert np.array_equal(mask.cpu().numpy(), want_mask) and mask[p] == 0 and mask[19] == 0 and not sums[19].any()
    assert 0 < int(mask.sum()) < 19
    with pytest.raises(IndexError, match="nn_crop_indexes"):
        tgnet.crop_vote(torch.from_numpy(sem_2).to(dev), torch.from_numpy(idx).to(dev), 18)


def test_crop_vote_gives_the_reference_sums(dev, fx, main_case):
    from toothgroupnetwork_amd import tgnet
    first, _ = TC.stand_ins(TC.device_knn)
    out = first([main_case["inp"]])
    mask, sums = tgnet.crop_vote(out["sem_2"], out["nn_crop_indexes"], 24000)
    assert np.array_equal(sums.cpu().numpy(), fx["vote_sums"].astype(np.float32))
    assert np.array_equal(mask.cpu().numpy(), np.argmax(fx["vote_sums"], axis=1))


def test_first_instances_gives_the_reference_instances(dev, fx, main_case):
    from toothgroupnetwork_amd import tgnet
    first, _ = TC.stand_ins(TC.device_knn)
    got = tgnet.first_instances(main_case["inp"], first([main_case["inp"]]))
    assert np.array_equal(got["xyz"].cpu().numpy(), fx["first_xyz"])
    assert np.array_equal(got["ins"].cpu().numpy(), fx["first_ins"]) and np.array_equal(got["sem"].cpu().numpy(), fx["teeth_full_sem_in"])
    assert np.array_equal(got["ins"].cpu().numpy() == 0, got["mask"].cpu().numpy() == 0)


# ---------------------------------------------------------------------------------------------------------------------------
# boundary_flags
# ---------------------------------------------------------------------------------------------------------------------------
def _stripes(xyz, n=4):
    return np.floor((xyz[:, 0] + 1.0) * n / 2.0).astype(np.int64)


def _flag_cases():
    rng = np.random.default_rng(21)
    sampled = rng.random((600, 3)) * 2 - 1
    dense = rng.random((1500, 3)) * 2 - 1
    few = rng.random((40, 3)) * 2 - 1
    twice = np.concatenate([sampled[:300], sampled[:50]])                              # 50 sampled points are there twice, with equal labels
    return {"k_equals_n": (dense[:100], few, rng.integers(0, 3, 40)),
            "stripes": (dense, sampled, _stripes(sampled)),
            "on_the_samples": (sampled[:200].copy(), sampled, _stripes(sampled)),
            "duplicated_samples": (dense[:400], twice, _stripes(twice))}


@pytest.mark.parametrize("case", ["k_equals_n", "stripes", "on_the_samples", "duplicated_samples"])
def test_boundary_flags_against_the_restatement(dev, case):
    from toothgroupnetwork_amd import tgnet
    dense, sampled, labels = _flag_cases()[case]
    want_flags, want_near = R.boundary_flags(dense, sampled, labels)
    flags, near = tgnet.boundary_flags(dense, sampled, labels)
    assert isinstance(flags, np.ndarray) and flags.dtype == bool and near.dtype == np.int64
    assert np.array_equal(flags, want_flags) and np.array_equal(near, want_near)
    t_flags, t_near = tgnet.boundary_flags(torch.from_numpy(dense).to(dev), torch.from_numpy(sampled).to(dev), torch.from_numpy(labels).to(dev))
    assert t_flags.is_cuda and np.array_equal(t_flags.cpu().numpy(), want_flags) and np.array_equal(t_near.cpu().numpy(), want_near)
    if case == "stripes":
        assert 0 < want_flags.sum() < len(want_flags), "both outcomes occur"
    if case == "on_the_samples":
        assert np.array_equal(near, labels[:200]), "distance 0: the nearest sampled point is the point itself"
    if case == "k_equals_n":
        assert np.array_equal(want_flags, np.array([np.mean(labels == l) for l in want_near]) < 0.7)


def test_boundary_flags_count_the_nearest_label_not_the_most_frequent(dev):
    from toothgroupnetwork_amd import tgnet
    sampled = np.array([[0.01 * (i + 1), 0.0, 0.0] for i in range(40)])
    labels = np.array([7] * 10 + [3] * 30)                                             # the nearest label holds 10 of 40, label 3 holds 30
    flags, near = tgnet.boundary_flags(np.zeros((1, 3)), sampled, labels)
    assert near.tolist() == [7] and flags.tolist() == [True]                           # 10 / 40 < 0.7; the most frequent label's 30 / 40 is not
    with pytest.raises(ValueError, match="k = 40"):
        tgnet.boundary_flags(np.zeros((1, 3)), sampled[:39], labels[:39])


def test_boundary_flags_give_the_reference_rows(dev, fx, main_case):
    from toothgroupnetwork_amd import tgnet
    flags, near = tgnet.boundary_flags(main_case["dense"], main_case["sampled"], fx["first_ins"])
    assert np.array_equal(flags, np.unpackbits(fx["bd_flags"])[:flags.shape[0]].astype(bool)) and np.array_equal(near, fx["bd_nearest"])


# ---------------------------------------------------------------------------------------------------------------------------
# boundary_resample
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def resample_case():
    rng = np.random.default_rng(31)
    dense = np.concatenate([rng.random((3000, 2)) * 2 - 1, np.zeros((3000, 1)), rng.normal(size=(3000, 3))], axis=1)
    sampled = dense[::2][:1200]
    return dense, sampled, _stripes(sampled)


@pytest.mark.parametrize("case,n_bdl", [("truncated", 100), ("fewer", 900), ("none", 100)])
def test_boundary_resample_against_the_restatement(dev, resample_case, case, n_bdl):
    from toothgroupnetwork_amd import resample, tgnet
    dense, sampled, labels = resample_case
    labels = np.zeros_like(labels) if case == "none" else labels
    info = {"bdl_ratio": 0.7, "num_of_bdl_points": n_bdl, "num_of_all_points": 1024}
    flags, near = R.boundary_flags(dense[:, :3], sampled[:, :3], labels)
    assert {"truncated": flags.sum() > n_bdl, "fewer": 0 < flags.sum() < n_bdl, "none": flags.sum() == 0}[case], flags.sum()
    np.random.seed(5)
    bd, rest = R.boundary_rows(flags, n_bdl, 1024, dense[:, :3], resample.fps)
    follow = np.random.random()                                                        # the generator's state after one permutation
    rows = np.concatenate([bd, rest])
    carry = np.arange(3000)
    np.random.seed(5)
    feats, lab, bd_feats, bd_lab, (carried,) = tgnet.boundary_resample(dense, sampled, labels, info, carry=(carry,))
    assert np.random.random() == follow, "exactly one np.random.permutation is drawn from the global generator"
    assert feats.shape == (1024, 6) and lab.shape == (1024, 1) and lab.dtype == np.int64 and bd_feats.shape[0] == len(bd) == min(n_bdl, flags.sum())
    assert np.array_equal(carried, rows) and np.array_equal(feats, dense[rows]) and np.array_equal(lab[:, 0], near[rows])
    assert np.array_equal(bd_feats, dense[bd]) and np.array_equal(bd_lab[:, 0], near[bd])
    assert len(tgnet.boundary_resample(dense, sampled, labels, info)) == 4


def test_boundary_resample_refuses_too_few_other_points(dev, resample_case):
    from toothgroupnetwork_amd import tgnet
    dense, sampled, labels = resample_case
    info = {"bdl_ratio": 0.7, "num_of_bdl_points": 10, "num_of_all_points": 1024}
    flags, _ = R.boundary_flags(dense[:1100, :3], sampled[:, :3], labels)
    assert 1100 - flags.sum() <= 1014
    with pytest.raises(ValueError, match="non-boundary"):
        tgnet.boundary_resample(dense[:1100], sampled, labels, info)


def test_boundary_resample_gives_the_reference_rows(dev, fx, main_case):
    from toothgroupnetwork_amd import tgnet
    np.random.seed(TC.PERM_SEED)
    feats, lab, bd_feats, bd_lab = tgnet.boundary_resample(main_case["dense"], main_case["sampled"], fx["first_ins"])
    assert bd_feats.shape[0] == int(fx["bd_count"][0]) and feats.shape == (24000, 6)
    assert np.array_equal(lab[:, 0], fx["bd_rows_label"]) and np.array_equal(feats[::16, :3], fx["bd_rows_xyz"])
    assert np.array_equal(bd_feats[:, :3].astype(np.float32), fx["merge_bdl_xyz"])


# ---------------------------------------------------------------------------------------------------------------------------
# kmeans
# ---------------------------------------------------------------------------------------------------------------------------
def _blobs():
    rng = np.random.default_rng(41)
    centres = np.array([[0.0, 0.0, 0.0], [1.0, 0.2, 0.0], [0.1, 1.0, 0.3], [-1.0, 0.1, 0.5], [0.3, -1.0, -0.4]])
    pts = np.concatenate([c + rng.normal(size=(64, 3)) * 0.05 for c in centres]).astype(np.float32)
    return pts[rng.permutation(len(pts))], centres


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_kmeans_an_empty_cluster_keeps_its_centre(dev):
    from toothgroupnetwork_amd import tgnet
    pts, centres = _blobs()
    init = np.concatenate([centres + 0.1, [[10.0, 10.0, 10.0]]])
    labels, cent = tgnet.kmeans(pts, init)
    want_labels, want_cent, iters = R.kmeans(pts, init)
    assert labels.dtype == np.int64 and cent.dtype == np.float64 and iters >= 1
    assert np.array_equal(labels, want_labels) and _same_bits(cent, want_cent)
    assert np.array_equal(cent[5], [10.0, 10.0, 10.0]) and 5 not in labels and np.bincount(labels).tolist() == [64] * 5


@pytest.mark.parametrize("max_iter", [0, 1])
def test_kmeans_max_iter(dev, max_iter):
    from toothgroupnetwork_amd import tgnet
    pts, centres = _blobs()
    init = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.2, 0.0, 0.0]])               # three centres inside one of five blobs: 4 iterations
    labels, cent = tgnet.kmeans(torch.from_numpy(pts).to(dev), torch.from_numpy(init).to(dev), max_iter=max_iter)
    want_labels, want_cent, _ = R.kmeans(pts, init, max_iter)
    assert labels.is_cuda and np.array_equal(labels.cpu().numpy(), want_labels) and _same_bits(cent.cpu().numpy(), want_cent)
    if max_iter == 0:
        assert _same_bits(cent.cpu().numpy(), init) and np.array_equal(want_labels, R.nearest_center(pts, init))
    else:
        assert not np.array_equal(R.kmeans(pts, init, 300)[0], want_labels), "one iteration is not enough here"
    with pytest.raises(ValueError, match="max_iter"):
        tgnet.kmeans(pts, init, max_iter=-1)


def test_kmeans_equidistant_point_goes_to_the_lower_centre(dev):
    from toothgroupnetwork_amd import tgnet
    pts = np.array([[0.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.5, 0.0]], np.float32)
    init = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    labels, cent = tgnet.kmeans(pts, init, max_iter=0)
    assert labels.tolist() == [0, 1, 0, 0]
    labels, _ = tgnet.kmeans(pts, init[::-1].copy(), max_iter=0)
    assert labels.tolist() == [0, 0, 1, 0]


def test_kmeans_is_the_restatements_float64_lloyd_bit_for_bit(dev):
    from toothgroupnetwork_amd import tgnet
    rng = np.random.default_rng(43)
    pts = rng.normal(size=(700, 3)).astype(np.float32)                                 # no structure: many iterations, more than 256 points
    init = pts[:7].astype(np.float64) * 0.5
    labels, cent = tgnet.kmeans(pts, init)
    want_labels, want_cent, iters = R.kmeans(pts, init)
    assert iters > 3 and np.array_equal(labels, want_labels) and _same_bits(cent, want_cent)


# ---------------------------------------------------------------------------------------------------------------------------
# merge_boundary
# ---------------------------------------------------------------------------------------------------------------------------
def test_merge_boundary_equal_counts_and_a_majority_of_zero(dev):
    from toothgroupnetwork_amd import tgnet
    first_xyz = np.array([[float(i), 0.0, 0.0] for i in range(8)])
    first_ins = np.array([0, 0, 3, 3, 5, 5, 9, 9])
    first_sem = np.array([0, 0, 12, 12, 4, 4, 7, 7])
    bdl_xyz = np.array([[2.1, 0, 0], [3.1, 0, 0], [4.1, 0, 0], [4.9, 0, 0],            # cluster 1: instances 3, 3, 5, 5 -> 3, the smaller
                        [0.1, 0, 0], [0.9, 0, 0], [6.1, 0, 0],                         # cluster 2: 0, 0, 9 -> 0 wins
                        [6.9, 0, 0],                                                   # second-pass background stays 0 whatever it is near
                        [4.5, 0.0, 0.0], [7.2, 0, 0]])                                 # cluster 4: equidistant from points 4 and 5 (both 5), and 9 -> 5 / 9 tie -> 5
    bdl_ins = np.array([1, 1, 1, 1, 2, 2, 2, 0, 4, 4])
    points, ins, sem = tgnet.merge_boundary(first_xyz, first_ins, first_sem, bdl_xyz, bdl_ins)
    want_ins, want_sem = R.merge_boundary(first_xyz, first_ins, first_sem, bdl_xyz, bdl_ins)
    assert np.array_equal(ins, want_ins) and np.array_equal(sem, want_sem) and np.array_equal(points, np.concatenate([first_xyz, bdl_xyz]))
    assert ins[8:].tolist() == [3, 3, 3, 3, 0, 0, 0, 0, 5, 5] and sem[8:].tolist() == [12, 12, 12, 12, 0, 0, 0, 0, 4, 4]
    points, ins, sem = tgnet.merge_boundary(first_xyz, first_ins, first_sem, np.zeros((0, 3)), np.zeros(0, np.int64))
    assert len(points) == 8 and np.array_equal(ins, first_ins)


def test_merge_boundary_gives_the_reference_rows(dev, fx):
    from toothgroupnetwork_amd import tgnet
    bdl_ins = np.where(fx["merge_bdl_background"], 0, fx["merge_bdl_partition"].astype(np.int64) + 1)
    points, ins, sem = tgnet.merge_boundary(fx["first_xyz"], fx["teeth_full_ins"], fx["teeth_full_sem"], fx["merge_bdl_xyz"], bdl_ins)
    assert np.array_equal(ins[24000:], fx["merge_ins"]) and np.array_equal(sem[24000:], fx["merge_sem"])
    assert np.array_equal(ins[:24000], fx["teeth_full_ins"]) and points.shape == (24000 + len(bdl_ins), 3)


def test_second_instances_find_the_teeth_of_the_boundary_points(dev, fx, main_case):
    """the boundary stand-in moves every tooth's points onto its centre: the k-means partition is the partition by tooth"""
    from toothgroupnetwork_amd import tgnet
    np.random.seed(TC.PERM_SEED)
    feats, lab, _, _ = tgnet.boundary_resample(main_case["dense"], main_case["sampled"], fx["first_ins"])
    inp = torch.from_numpy(np.ascontiguousarray(feats.astype("float32"))[None]).to(dev).permute(0, 2, 1).contiguous()
    labels = torch.from_numpy(tgnet.dense_rank_labels(lab)[None, None]).to(dev)
    _, bdl = TC.stand_ins(TC.device_knn)
    got = tgnet.second_instances(inp, labels, bdl([inp, labels], test=True))
    tooth = TC.tooth_of(got["xyz"]).cpu().numpy()
    ins = got["ins"].cpu().numpy()
    assert got["centres"].shape == (TC.TEETH, 3) and np.array_equal(ins == 0, tooth == -1)
    pairs = np.unique(np.stack([ins[tooth >= 0], tooth[tooth >= 0]]), axis=1)
    assert pairs.shape[1] == TC.TEETH, "one cluster per tooth and one tooth per cluster"
    nb = int(fx["bd_count"][0])
    want = np.where(fx["merge_bdl_background"], -1, fx["merge_bdl_partition"])
    mine = np.where(ins[:nb] == 0, -1, ins[:nb])
    _, a = np.unique(want, return_inverse=True)
    _, b = np.unique(mine, return_inverse=True)
    assert len(np.unique(np.stack([a.reshape(-1), b.reshape(-1)]), axis=1)[0]) == len(np.unique(a)) == len(np.unique(b)), "the reference's partition"
