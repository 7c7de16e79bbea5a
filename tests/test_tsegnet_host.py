"""CPU: the written contracts of the tsegnet kernels (tests/tsegnet_ref.py, a numpy restatement of include/tgn_pointops.h) agree with
what the REFERENCE's own classes computed (tests/golden/make_golden_r11_tsegnet.py) on every case of the fixture -- this ties the
contract to the reference; tests/test_gpu_tsegnet.py ties the kernels to the contract.  Plus the host layer's argument validation and
the state_dict layout of nets.TSegNetModule against the reference class's."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_ref  # noqa: E402
import tsegnet_cases as TC  # noqa: E402
import tsegnet_ref as R  # noqa: E402
from crop_cases import unpack_sets  # noqa: E402
from tsegnet_ref import within_reference_noise  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r11_tsegnet.npz")))


@pytest.fixture(scope="module")
def case():
    return TC.module_case()


def _centres(moved, labels):
    return np.array([moved[labels == lab].mean(axis=0) for lab in np.unique(labels) if lab != -1], np.float32)


def test_inputs_rebuild_the_fixture(fx, case):
    assert TC.case_digest(case) == fx["mod_digest"][0]
    assert os.path.getsize(os.path.join(GOLDEN, "reference_cpu_r11_tsegnet.npz")) < 1_000_000


def test_proposal_contract_matches_the_reference(fx, case):
    moved, counts, kept = R.proposals(case["l3_xyz"], case["offset"], case["dist"])
    want = np.unpackbits(fx["mod_kept"])[:TC.N_COARSE].astype(bool)
    assert np.array_equal(kept[0], want) and counts.tolist() == [int(want.sum())]
    f0, f1, fn = TC.FORCED
    assert not kept[0, f0] and kept[0, f1] and not kept[0, fn]
    labels, _ = cluster_ref.dbscan(moved, 0.05, 3)
    assert np.array_equal(labels, fx["mod_db_labels"].astype(np.int64))
    assert np.array_equal(_centres(moved, labels).view(np.uint32), fx["mod_cent_bits"])
    np.random.seed(TC.PERM_SEED)
    assert np.array_equal(np.random.permutation(fx["mod_cent_bits"].shape[0])[:TC.MAX_CROPS], fx["mod_perm"])


def test_crop_contract_matches_the_reference(fx, case):
    cent = fx["mod_cent_bits"].view(np.float32)[fx["mod_perm"]]
    idx = unpack_sets(fx["mod_idxset"])                                    # each crop's index set, ascending
    x = case["feats"][0, :3].astype(np.float64)
    for t, c in enumerate(cent.astype(np.float64)):                        # tgn_crop_knn's contract gives the reference's sets
        d = ((0.0 + (x[0] - c[0]) ** 2) + (x[1] - c[1]) ** 2) + (x[2] - c[2]) ** 2
        assert np.array_equal(np.sort(np.lexsort((np.arange(d.size), d))[:TC.CROP_K]), idx[t])
    out, lab = R.crop_features(case["feats"], case["l0_points"], np.zeros(len(cent), np.int32), cent, idx, case["labels"])
    assert out.shape == (TC.MAX_CROPS, 36, TC.CROP_K)
    assert np.array_equal(out[:, :35, ::64].view(np.uint32), fx["mod_crop"].view(np.uint32))
    assert np.array_equal(lab[:, :, ::64], fx["mod_crop_labels"].astype(np.int64))
    assert lab.min() == -1 and lab.max() > 0, "raw labels: teeth keep their numbers"
    within_reference_noise("ddf (numpy contract)", out[:, 35, ::4], fx["mod_ddf32"], fx["mod_ddf64"])
    assert not np.isnan(out[:, 35]).any()
    within_reference_noise("ddf64 restatement", R.ddf64(out[:, :3], cent)[:, ::4], fx["mod_ddf64"], fx["mod_ddf64"])


def _scripted(case, fx):
    cent = fx["mod_cent_bits"].view(np.float32)[fx["mod_perm"]]
    idx = unpack_sets(fx["mod_idxset"])
    out, _ = R.crop_features(case["feats"], case["l0_points"], np.zeros(len(cent), np.int32), cent, idx)
    _, _, pd_2, id_pred = TC.fixed_seg(torch.from_numpy(out))
    return idx, torch.from_numpy(TC.plant(pd_2.numpy(), idx)), id_pred


def test_paint_contract_matches_the_reference(fx, case):
    idx, pd_2, id_pred = _scripted(case, fx)
    mask = (torch.sigmoid(pd_2[:, 0]) > 0.5).numpy()
    cols = np.argsort(idx[-1], kind="stable")[:len(TC.PLANTED)]
    assert mask[-1, cols].tolist() == [False, False, False, False, True, True], "sigmoid(x) > 0.5 in float32 is not x > 0"
    got = R.paint(1, TC.N_POINTS, np.zeros(len(idx), np.int32), idx, mask, id_pred.argmax(1).numpy())
    assert np.array_equal(got[0], fx["paint_labels"].astype(np.int64))


def test_paint_restatement_is_last_writer_wins_and_the_package_declares_the_kernel():
    """A self-check of tests/tsegnet_ref.paint on a hand-made case (the restatement is what the other tests lean on), next to the
    package's side of the same contract: the symbol is in the ctypes table with the header's arity."""
    from toothgroupnetwork_amd import _lib
    assert len(_lib.SIGNATURES["tgn_tsg_paint"][1]) == 10 and len(_lib.SIGNATURES["tgn_tsg_crop_features"][1]) == 15
    assert len(_lib.SIGNATURES["tgn_tsg_proposals"][1]) == 9
    idx = np.array([[0, 1, 2, 3], [2, 3, 4, 5], [9, 8, 3, 0]])
    mask = np.array([[1, 1, 1, 1], [0, 1, 1, 1], [1, 0, 1, 0]], np.uint8)
    got = R.paint(2, 10, np.array([0, 0, 1]), idx, mask, np.array([5, 7, 9]))
    assert got[0].tolist() == [5, 5, 5, 7, 7, 7, 0, 0, 0, 0] and got[1].tolist() == [0, 0, 0, 9, 0, 0, 0, 0, 0, 9]


def test_state_dict_layout_is_the_reference_class(fx):
    from toothgroupnetwork_amd import nets
    net = nets.TSegNetModule({"run_tooth_segmentation_module": True})
    keys = [f"{n}:{'x'.join(map(str, t.shape))}" for n, t in net.state_dict().items()]
    assert keys == fx["mod_state_keys"].tolist()
    assert keys[0].startswith("cent_module.") and keys[-1].startswith("seg_module.")
    other = nets.TSegNetModule({"run_tooth_segmentation_module": False})
    other.load_state_dict(net.state_dict(), strict=True)
    assert other.run_seg_module is False and net.run_seg_module is True


def test_host_layer_validates_its_arguments():
    from toothgroupnetwork_amd import tsegnet as T
    l3, off, dist = torch.zeros(1, 3, 8), torch.zeros(1, 3, 8), torch.zeros(1, 1, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.centroid_proposals(l3, off, dist)
    with pytest.raises(TypeError, match="torch tensor"):
        T.centroid_proposals(l3.numpy(), off, dist)
    with pytest.raises(TypeError, match="float32"):
        T.centroid_proposals(l3.double(), off, dist)
    with pytest.raises(ValueError, match="1 <= M <= 1024"):
        T.centroid_proposals(torch.zeros(1, 3, 1025), torch.zeros(1, 3, 1025), torch.zeros(1, 1, 1025))
    with pytest.raises(ValueError, match="offset"):
        T.centroid_proposals(l3, torch.zeros(1, 3, 9), dist)
    with pytest.raises(ValueError, match="dist"):
        T.centroid_proposals(l3, off, torch.zeros(1, 8))
    with pytest.raises(ValueError, match="NaN"):
        T.centroid_proposals(l3, off, dist, float("nan"))
    moved = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.cluster_centers(moved, [5])
    with pytest.raises(ValueError, match="sum to 5"):
        T.cluster_centers(moved, [4])
    with pytest.raises(ValueError, match="scan 1 has no centroid proposal"):
        T.cluster_centers(moved, [5, 0])
    with pytest.raises(ValueError, match=r"\(K, 3\) float32"):
        T.cluster_centers(torch.zeros(5, 2), [5])
    feats, l0 = torch.zeros(1, 6, 16), torch.zeros(1, 4, 16)
    cents = [np.zeros((2, 3), np.float32)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.crop_features(feats, l0, cents, k=4)
    with pytest.raises(ValueError, match="1 <= k"):
        T.crop_features(feats, l0, cents, k=17)
    with pytest.raises(ValueError, match="l0_points must be"):
        T.crop_features(feats, torch.zeros(1, 4, 15), cents, k=4)
    with pytest.raises(ValueError, match="list of 1 per-scan"):
        T.crop_features(feats, l0, cents * 2, k=4)
    with pytest.raises(TypeError, match="int64"):
        T.crop_features(feats, l0, cents, k=4, labels=torch.zeros(1, 16, dtype=torch.int32))
    with pytest.raises(ValueError, match="labels must be"):
        T.crop_features(feats, l0, cents, k=4, labels=torch.zeros(1, 15, dtype=torch.int64))
    with pytest.raises(ValueError, match="1 <= k"):
        T.crop_features(feats, l0, cents, k=0)
    with pytest.raises(ValueError, match="list of 1 per-scan"):
        T.crop_features(feats, l0, cents[0], k=4)                          # a bare array is not a list over scans
    with pytest.raises(ValueError, match=r"must be \(T_b, 3\)"):
        T.crop_features(feats, l0, [np.zeros((2, 2), np.float32)], k=4)
    with pytest.raises(ValueError, match=r"must be \(T_b, 3\)"):
        T.crop_features(feats, l0, [torch.zeros(6)], k=4)
    with pytest.raises(TypeError, match="int64"):
        T.crop_features(feats, l0, cents, k=4, labels=np.zeros((1, 16), np.int64))
    # the shared helpers of crops.py that crop_features, tooth_crops and the noise vote go through, on their own
    from toothgroupnetwork_amd import crops as C
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="centres must be a list of 2 per-scan"):
        C.stack_centres(cents, 2, cpu, "centres")
    with pytest.raises(ValueError, match=r"every scan's centroids must be \(T_b, 3\), got \(3, 2\)"):
        C.stack_centres((np.zeros((1, 3)), np.zeros((3, 2))), 2, cpu, "centroids")
    cent, scan, per_scan = C.stack_centres([np.ones((2, 3)), torch.zeros(0, 3), [[1, 2, 3]]], 3, cpu, "centres")
    assert cent.dtype == torch.float32 and cent.is_contiguous() and cent.tolist() == [[1, 1, 1], [1, 1, 1], [1, 2, 3]]
    assert scan.dtype == torch.int32 and scan.tolist() == [0, 0, 2] and per_scan == [2, 0, 1]
    assert C.scan_ids([1, 0, 2], cpu).tolist() == [0, 2, 2] and C.scan_ids([0], cpu).shape == (0,)
    for k, n in ((0, 16), (17, 16), (4097, 5000)):
        with pytest.raises(ValueError, match=rf"k = {k} must satisfy 1 <= k <= min\(N, 4096\) = {min(n, 4096)}"):
            C.crop_knn(torch.zeros(1, 3, n), scan, cent, k)
    assert C.check_k(4096, 5000) == 4096 and C.check_k(np.int64(16), 16) == 16 and (C.MAX_K, C.MAX_CLUSTERS) == (4096, 64)
    lab32 = torch.arange(16, dtype=torch.int32).reshape(1, 1, 16)
    with pytest.raises(TypeError, match="int64, got torch.int32"):
        C.labels_2d(lab32, 1, 16, (torch.int64,))
    with pytest.raises(TypeError, match="int32 or int64, got torch.float32"):
        C.labels_2d(lab32.float(), 1, 16, (torch.int32, torch.int64))
    with pytest.raises(ValueError, match="labels must be"):
        C.labels_2d(lab32, 1, 15, (torch.int32, torch.int64))
    got = C.labels_2d(lab32, 1, 16, (torch.int32, torch.int64))
    assert got.dtype == torch.int64 and got.is_contiguous() and got.tolist() == [list(range(16))]
    idx, pd_2, ids = [torch.zeros(2, 4, dtype=torch.int64)], torch.zeros(2, 1, 4), torch.zeros(2, 17)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.paint_labels(idx, pd_2, ids, 16)
    with pytest.raises(ValueError, match="pd_2 must be"):
        T.paint_labels(idx, torch.zeros(3, 1, 4), ids, 16)
    with pytest.raises(ValueError, match="id_pred must be"):
        T.paint_labels(idx, pd_2, torch.zeros(3, 17), 16)
    with pytest.raises(ValueError, match="n_points"):
        T.paint_labels(idx, pd_2, ids, 0)
    with pytest.raises(ValueError, match="non-empty list"):
        T.paint_labels([], pd_2, ids, 16)


def test_pipeline_class_refuses_what_it_cannot_pin():
    from toothgroupnetwork_amd import inference
    p = inference.TSegNetInferencePipeLine(model=object())
    assert (p.scaler, p.shifter, p.times) == (1.8, 0.8, {})
    assert set(fdi for fdi in inference.fdi_from_classes(np.arange(17)).tolist()) == {0, *range(11, 19), *range(21, 29)}
