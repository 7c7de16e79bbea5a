"""On-device tooth crops (toothgroupnetwork_amd/crops.py, csrc/crop.hip) against numpy restatements of the reference's crop step
(models/modules/grouping_network_module.py:45-72) and against the reference's own output on CPU (tests/golden/make_golden_r7_grouping.py:
numpy means, sklearn KDTree, get_indexed_features, centering_object).

  centroids   bit-equal to a sequential float32 sum in point order divided by the count (numpy's xyz[mask].mean(axis=0))
  indices     bit-equal to lexsort((index, float64 squared distance)); against KDTree: the same distance sequence, and the same index
              set wherever the k-th and (k+1)-th distances differ (KDTree's order among equal distances is unspecified)
  crops       labels exact, channels 3.. bit-exact, xyz within 1 ulp of the float64-mean restatement"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
from crop_cases import digest, op_cases, unpack_sets  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden_r7():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r7_grouping.npz")))


def np_centroids(xyz, lab):
    """xyz (N, 3) float32, lab (N,): {t: centroid} for t != -1 in ascending order, sequential float32 sum / count."""
    out = {}
    for t in np.unique(lab):
        if t == -1:
            continue
        pts = xyz[lab == t]
        s = np.zeros(3, np.float32)
        for p in pts:
            s = (s + p).astype(np.float32)
        out[int(t)] = (s / np.float32(pts.shape[0])).astype(np.float32)
    return out


def d64(xyz, c):
    x = xyz.astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    return ((0.0 + (x[:, 0] - c[0]) * (x[:, 0] - c[0])) + (x[:, 1] - c[1]) * (x[:, 1] - c[1])) + (x[:, 2] - c[2]) * (x[:, 2] - c[2])


def np_knn(xyz, c, k):
    d = d64(xyz, c)
    return np.lexsort((np.arange(d.size), d))[:k]


def np_crop(rows_cf, idx):
    """rows_cf (C, N) float32 -> (C, k): gathered, xyz minus the float64 mean rounded once to float32."""
    g = rows_cf[:, idx].copy()
    m = (g[:3].astype(np.float64).sum(1) / idx.size).astype(np.float32)
    g[:3] = (g[:3] - m[:, None]).astype(np.float32)
    return g


def _run(dev, rows, labels, k, stream=None):
    from toothgroupnetwork_amd import crops
    feats = torch.from_numpy(np.ascontiguousarray(rows.transpose(0, 2, 1))).to(dev)
    lab = torch.from_numpy(labels.astype(np.int64)).to(dev)
    if stream is None:
        return crops.tooth_crops(feats, lab, k=k), feats
    with torch.cuda.stream(stream):
        r = crops.tooth_crops(feats, lab, k=k)
    stream.synchronize()
    return r, feats


def _check_against_restatement(r, rows, labels, k):
    B = rows.shape[0]
    crops_np, lab_np, t0 = [], [], 0
    assert len(r.nn_crop_indexes) == len(r.centroids) == B
    for b in range(B):
        want_c = np_centroids(rows[b, :, :3], labels[b])
        got_c = r.centroids[b].cpu().numpy()
        assert got_c.shape == (len(want_c), 3)
        assert np.array_equal(got_c.view(np.uint32), np.stack(list(want_c.values())).view(np.uint32)), "centroids not bit-equal"
        got_i = r.nn_crop_indexes[b].cpu().numpy()
        assert got_i.dtype == np.int64 and got_i.shape == (len(want_c), k)
        for j, c in enumerate(want_c.values()):
            want_i = np_knn(rows[b, :, :3], c, k)
            assert np.array_equal(got_i[j], want_i), (b, j)
            crops_np.append(np_crop(rows[b].T, want_i))
            lab_np.append(np.where(labels[b][want_i] >= 0, 0, labels[b][want_i]))
        t0 += len(want_c)
    want = np.stack(crops_np)
    got = r.cropped.cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(got[:, 3:], want[:, 3:]), "feature channels not bit-exact"
    ulp = np.spacing(np.maximum(np.abs(want[:, :3]), np.abs(got[:, :3])).astype(np.float32))
    assert np.all(np.abs(got[:, :3].astype(np.float64) - want[:, :3]) <= ulp), "xyz beyond 1 ulp"
    assert np.array_equal(r.cluster_gt_seg_label.cpu().numpy(), np.stack(lab_np)[:, None, :])


def _random_case(n, teeth, seed, dup=0):
    rng = np.random.default_rng(seed)
    rows = rng.random((n, 6), dtype=np.float32) * 2 - 1
    if dup:
        rows[rng.integers(0, n, dup)] = rows[rng.integers(0, n, dup)]
    lab = rng.integers(-1, teeth, n).astype(np.int64)
    return rows[None], lab[None]


@pytest.mark.parametrize("kind,n,k,dup", [
    ("arch", 24000, 3072, 0), ("arch", 24000, 4096, 0), ("arch", 24000, 1, 0), ("arch", 24000, 3072, 2000),
    ("arch", 3072, 3072, 0), ("arch", 4099, 4096, 300), ("arch", 100000, 3072, 0), ("arch", 100000, 4096, 5000),
    ("random", 24001, 3072, 0), ("random", 9999, 4096, 3000), ("random", 3072, 3072, 500), ("random", 777, 777, 100),
])
def test_crops_equal_the_numpy_restatement(dev, kind, n, k, dup):
    from toothgroupnetwork_amd import synth
    if kind == "arch":
        rows, lab = synth.labelled_arch(n, 14, seed=n + k + dup, dup=dup)
        rows, lab = rows[None], lab[None]
    else:
        rows, lab = _random_case(n, 16, seed=n + k, dup=dup)
    r, _ = _run(dev, rows, lab, k)
    _check_against_restatement(r, rows, lab, k)


def test_crops_on_a_ragged_batch_with_int32_labels_of_shape_b1n(dev):
    from toothgroupnetwork_amd import crops, synth
    (f1, l1), (f2, l2) = synth.labelled_arch(12000, 16, seed=11), synth.labelled_arch(12000, 5, seed=12, dup=700)
    rows, lab = np.stack([f1, f2]), np.stack([l1, l2])
    feats = torch.from_numpy(np.ascontiguousarray(rows.transpose(0, 2, 1))).to(dev)
    r = crops.tooth_crops(feats, torch.from_numpy(lab.astype(np.int32)).view(2, 1, -1).to(dev), k=2048)
    assert [t.shape[0] for t in r.nn_crop_indexes] == [16, 5]
    _check_against_restatement(r, rows, lab, 2048)


def test_crops_run_on_a_non_default_stream(dev):
    from toothgroupnetwork_amd import synth
    rows, lab = synth.labelled_arch(24000, 14, seed=21, dup=300)
    s = torch.cuda.Stream()
    r, _ = _run(dev, rows[None], lab[None], 3072, stream=s)
    _check_against_restatement(r, rows[None], lab[None], 3072)


def test_given_centroids_replace_the_label_centroids(dev):
    from toothgroupnetwork_amd import crops, synth
    rows, lab = synth.labelled_arch(6000, 6, seed=31)
    cent = [np.array([[0.1, 0.2, 0.0], [-0.3, 0.1, 0.05]], np.float32)]
    feats = torch.from_numpy(np.ascontiguousarray(rows.T))[None].to(dev)
    r = crops.tooth_crops(feats, centroids=cent, k=1000)
    assert r.cluster_gt_seg_label is None
    got = r.nn_crop_indexes[0].cpu().numpy()
    for j in range(2):
        assert np.array_equal(got[j], np_knn(rows[:, :3], cent[0][j], 1000))


@pytest.fixture(scope="module")
def cases():
    return op_cases()


@pytest.mark.parametrize("tag", ["s24", "ragged", "k4096", "dup", "single"])
def test_crops_match_the_reference_kdtree(dev, golden_r7, cases, tag):
    rows, labels, k = cases[tag]
    assert digest(rows, labels) == golden_r7[f"op_{tag}_digest"][0], "the case no longer rebuilds the fixture's input"
    assert k == int(golden_r7[f"op_{tag}_k"][0])
    r, _ = _run(dev, rows, labels, k)
    assert [t.shape[0] for t in r.nn_crop_indexes] == golden_r7[f"op_{tag}_teeth"].tolist()
    cent = torch.cat(r.centroids).cpu().numpy()
    assert np.array_equal(cent.view(np.uint32), golden_r7[f"op_{tag}_cent"].view(np.uint32)), "centroids differ from numpy's mean"
    got = torch.cat(r.nn_crop_indexes).cpu().numpy()
    ref = unpack_sets(golden_r7[f"op_{tag}_idxset"])           # KDTree's index sets
    scan = np.repeat(np.arange(rows.shape[0]), golden_r7[f"op_{tag}_teeth"])
    boundary_ties = 0
    for t in range(got.shape[0]):
        d_all = d64(rows[scan[t], :, :3], cent[t])
        d_got, d_ref = d_all[got[t]], np.sort(d_all[ref[t]])
        assert np.array_equal(d_got, d_ref), (tag, t, "distance sequence differs from KDTree's")
        full = np.sort(d_all)
        if k < full.size and full[k - 1] == full[k]:
            boundary_ties += 1
            assert np.array_equal(np.sort(got[t][d_got < full[k - 1]]), ref[t][d_all[ref[t]] < full[k - 1]])
        else:
            assert np.array_equal(np.sort(got[t]), ref[t]), (tag, t, "index set differs")
    if tag == "dup":
        assert boundary_ties >= 1, "the dup case must hold a tie across the k-th boundary"
    # the reference's centred crops, every CROP_STRIDE-th column in KDTree's order: that order is ours wherever no distances tie
    want = golden_r7[f"op_{tag}_crop"]
    stride = -(-k // want.shape[2])
    got_c = r.cropped.cpu().numpy()[:, :, ::stride]
    compared = 0
    for t in range(got.shape[0]):
        if np.any(np.diff(d64(rows[scan[t], :, :3], cent[t])[got[t]]) == 0):
            continue
        compared += 1
        assert np.array_equal(got_c[t, 3:], want[t, 3:]), (tag, t, "feature channels")
        assert float(np.abs(got_c[t, :3] - want[t, :3]).max()) <= 1e-6, (tag, t, "centred xyz")   # the reference's mean is torch fp32
    assert compared or tag == "dup"


def test_crop_errors_raise(dev):
    from toothgroupnetwork_amd import crops, synth
    rows, lab = synth.labelled_arch(3000, 4, seed=41)
    feats = torch.from_numpy(np.ascontiguousarray(rows.T))[None].to(dev)
    tl = torch.from_numpy(lab)[None].to(dev)
    with pytest.raises(ValueError, match="k ="):
        crops.tooth_crops(feats, tl, k=3001)
    big = torch.from_numpy(np.ascontiguousarray(synth.labelled_arch(5000, 4, seed=42)[0].T))[None].to(dev)
    with pytest.raises(ValueError, match="k ="):
        crops.tooth_crops(big, torch.zeros(1, 5000, dtype=torch.int64, device=dev), k=4097)
    with pytest.raises(ValueError, match="no tooth"):
        crops.tooth_crops(feats, torch.full_like(tl, -1), k=100)
    bad = tl.clone()
    bad[0, 123] = 16
    with pytest.raises(ValueError, match="outside"):
        crops.tooth_crops(feats, bad, k=100)
    bad[0, 123] = -2
    with pytest.raises(ValueError, match="outside"):
        crops.tooth_crops(feats, bad, k=100)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        crops.tooth_crops(feats.cpu(), tl.cpu(), k=100)
    # the stream is usable after the rejected calls: the next run is exact
    r, _ = _run(dev, rows[None], lab[None], 500)
    _check_against_restatement(r, rows[None], lab[None], 500)


def test_entry_points_reject_bad_arguments_without_launching(dev):
    from toothgroupnetwork_amd import _lib
    L, st = _lib.lib(), _lib.stream()
    x = torch.zeros(1, 3, 10, device=dev)
    assert L.tgn_crop_knn(1, 10, 3, _lib.ptr(x), 1, _lib.ptr(x), _lib.ptr(x), 11, _lib.ptr(x), st) == _lib.ERR_INVALID_ARGUMENT
    assert L.tgn_crop_knn(1, 10, 3, _lib.ptr(x), 1, _lib.ptr(x), _lib.ptr(x), 0, _lib.ptr(x), st) == _lib.ERR_INVALID_ARGUMENT
    assert L.tgn_label_centroids(1, 10, 3, _lib.ptr(x), _lib.ptr(x), 65, _lib.ptr(x), _lib.ptr(x), st) == _lib.ERR_INVALID_ARGUMENT
    assert L.tgn_crop_gather_center(1, 10, 2, 1, 4, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), None, _lib.ptr(x), None, st) == \
        _lib.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
