"""CPU: the host parts of the tgnet pipeline -- the tooth numbering against the reference's own (tests/golden/make_golden_r16_tgnet.py ran
its InferencePipeLine and kept the locals of __call__), the two-stage network's names and shapes, the six-name factory, the map that
collapses duplicated vertices."""
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

FIVE = {"model_parameter": {"input_feat": 6, "stride": [1, 4, 4, 4, 4], "nstride": [2, 2, 2, 2], "nsample": [36, 24, 24, 24, 24],
                            "blocks": [2, 3, 4, 6, 3], "block_num": 5, "planes": [32, 64, 128, 256, 512], "crop_sample_size": 3072}}
TWO = {"model_parameter": {"input_feat": 6, "stride": [1, 1], "nsample": [36, 24], "blocks": [2, 3], "block_num": 2, "planes": [16, 32],
                           "crop_sample_size": 3072}}                                   # inference_pipeline_maker.py:43-54


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r16_tgnet.npz")))


@pytest.mark.parametrize("variant", TC.VARIANTS)
def test_number_teeth_gives_the_reference_numbers(fx, variant):
    """a full arch; one without classes 1 and 9 (the fallback loop); one with a classless instance (zeroed)"""
    from toothgroupnetwork_amd import tgnet
    sem_in = fx[f"teeth_{variant}_sem_in"].astype(np.int64)
    assert (int(np.sum(sem_in == 1) + np.sum(sem_in == 9)) <= 20) == (variant == "fallback")
    first_ins = fx["first_ins"].astype(np.int64)
    sem, ins = tgnet.number_teeth(fx["first_xyz"], first_ins, sem_in)
    assert sem.dtype == np.int64 and ins.dtype == np.int64
    assert np.array_equal(sem, fx[f"teeth_{variant}_sem"]) and np.array_equal(ins, fx[f"teeth_{variant}_ins"])
    assert (len(np.unique(ins)) < len(np.unique(first_ins))) == (variant == "classless")
    assert np.array_equal(first_ins, fx["first_ins"]), "the caller's instances are not written to"


def _arch(n_ins=4, per=30):
    rng = np.random.default_rng(3)
    centres = np.array([[np.cos(a), np.sin(a), 0.3] for a in np.linspace(0.3, 2.8, n_ins)])
    xyz = np.concatenate([rng.normal(size=(200, 3)) * 0.5 - [0, 0, 1.0]] + [c + rng.normal(size=(per, 3)) * 0.02 for c in centres])
    ins = np.concatenate([np.zeros(200, np.int64)] + [np.full(per, i + 1) for i in range(n_ins)])
    sem = np.concatenate([np.zeros(200, np.int64)] + [np.full(per, (1, 9, 2, 3, 4, 5)[i]) for i in range(n_ins)])
    return xyz, ins, sem


def test_number_teeth_raises_where_the_reference_has_an_accident():
    from toothgroupnetwork_amd import tgnet
    xyz, ins, sem = _arch()
    out_sem, out_ins = tgnet.number_teeth(xyz, ins, sem)
    assert set(np.unique(out_sem[ins == 1])) == {1} and set(np.unique(out_sem[ins == 2])) == {9} and np.array_equal(out_ins, ins)
    two = np.where(ins > 2, 0, ins)
    with pytest.raises(ValueError, match="three"):
        tgnet.number_teeth(xyz, two, sem)
    few = np.where(np.arange(len(sem)) % 30 < 5, sem, 0)            # 5 points per class: none has more than 20, 1 and 9 hold 10 together
    with pytest.raises(ValueError, match="more than 20"):
        tgnet.number_teeth(xyz, ins, few)
    mixed = out_sem.copy()
    mixed[np.flatnonzero(out_ins == 1)[0]] = 5                      # instance 1 carries two classes
    with pytest.raises(ValueError, match="sem label error"):
        tgnet.merge_votes(out_ins, mixed, np.array([1, 1, 2]), np.array([1, 1, 0]))


def test_merge_votes_smallest_label_on_equal_counts_and_zero_can_win():
    from toothgroupnetwork_amd import tgnet
    first_ins, first_sem = np.array([0, 0, 3, 3, 5, 5]), np.array([0, 0, 12, 12, 4, 4])
    bdl_ins = np.array([1, 1, 1, 1, 2, 2, 2, 0])
    near = np.array([5, 3, 3, 5, 0, 0, 3, 5])                       # cluster 1: 3 and 5 twice each -> 3; cluster 2: 0 wins; background stays 0
    ins, sem = tgnet.merge_votes(first_ins, first_sem, bdl_ins, near)
    assert ins.tolist() == [3, 3, 3, 3, 0, 0, 0, 0] and sem.tolist() == [12, 12, 12, 12, 0, 0, 0, 0]


def test_grouping_network_accepts_two_and_five_stages():
    from toothgroupnetwork_amd import nets
    five, two = nets.GroupingNetworkModule(FIVE), nets.GroupingNetworkModule(TWO)
    assert hasattr(five.first_ins_cent_model, "enc5") and not hasattr(two.first_ins_cent_model, "enc3")
    assert two.first_ins_cent_model.dec2[0].linear1[0].in_features == 64, "the top decoder stage is the head: Linear(2 * 32, 32)"
    for bad in (3, 4):
        with pytest.raises(ValueError, match="block_num"):
            nets.GroupingNetworkModule({"model_parameter": dict(FIVE["model_parameter"], block_num=bad)})
        with pytest.raises(ValueError, match="block_num"):
            nets.PointTransformerSeg(block_num=bad)


def test_boundary_module_state_dict_is_the_reference_classes(fx):
    from toothgroupnetwork_amd import nets
    sd = nets.GroupingNetworkModule(TWO).state_dict()
    assert [f"{n}:{'x'.join(map(str, v.shape))}" for n, v in sd.items()] == fx["net_module_keys"].tolist()
    net = nets.PointTransformerSeg(c=6, k=10, planes=(16, 32), blocks=(2, 3), stride=(1, 1), nsample=(36, 24), block_num=2)
    assert [f"{n}:{'x'.join(map(str, v.shape))}" for n, v in net.state_dict().items()] == fx["net_keys"].tolist()
    net.load_state_dict(torch.load(os.path.join(GOLDEN, "tgnet_boundary_weights.pt")), strict=True)
    assert net.cls_head.cls.in_features == 64, "the heads' latent width is the reference's base_fdim = 32 per stage, not planes[0] = 16"


def test_factory_knows_the_six_names(tmp_path, monkeypatch):
    from toothgroupnetwork_amd import inference, nets
    assert set(inference.MODEL_NAMES) == {"tsegnet", "tgnet", "pointnet", "pointnetpp", "dgcnn", "pointtransformer"}
    cfg = inference.inference_config("tgnet", ["a", "b"])
    assert cfg["fps_model_info"]["model_parameter"] == FIVE["model_parameter"] and cfg["fps_model_info"]["load_ckpt_path"] == "a"
    assert cfg["boundary_model_info"]["model_parameter"] == TWO["model_parameter"] and cfg["boundary_model_info"]["load_ckpt_path"] == "b"
    assert cfg["boundary_sampling_info"] == {"bdl_ratio": 0.7, "num_of_bdl_points": 20000, "num_of_all_points": 24000}
    with pytest.raises(ValueError, match="undefined model"):
        inference.make_inference_pipeline("tgnet2", [])
    # the modules' .cuda() is the one step that needs a GPU: every name builds its module, loads its checkpoint and picks its pipeline
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: self)
    made = {"tsegnet": lambda: nets.TSegNetModule(inference.inference_config("tsegnet")), "pointnet": lambda: nets.PointFirstModule({}),
            "pointnetpp": lambda: nets.PointPpFirstModule({}), "dgcnn": lambda: nets.DGCnnModule({}),
            "pointtransformer": lambda: nets.PointTransformerModule(inference.inference_config("pointtransformer")["model_info"])}
    kinds = {"tsegnet": inference.TSegNetInferencePipeLine}
    for name, make in made.items():
        path = str(tmp_path / (name + ".h5"))
        torch.save(make().state_dict(), path)
        pipe = inference.make_inference_pipeline(name, [path])
        assert type(pipe) is kinds.get(name, inference.InferencePipeLine) and not pipe.model.training
    paths = [str(tmp_path / "first.h5"), str(tmp_path / "bdl.h5")]
    torch.save(nets.GroupingNetworkModule(FIVE).state_dict(), paths[0])
    torch.save(nets.GroupingNetworkModule(TWO).state_dict(), paths[1])
    pipe = inference.make_inference_pipeline("tgnet", paths)
    assert type(pipe) is inference.TgnInferencePipeLine and pipe.boundary_sampling_info == cfg["boundary_sampling_info"]
    assert hasattr(pipe.first_module.first_ins_cent_model, "enc5") and not hasattr(pipe.bdl_module.first_ins_cent_model, "enc3")
    with pytest.raises(RuntimeError):                                # the boundary checkpoint does not fit the five-stage module
        inference.make_inference_pipeline("tgnet", paths[::-1])


def test_first_occurrences_against_a_loop():
    from toothgroupnetwork_amd import inference
    rng = np.random.default_rng(5)
    v = rng.integers(-3, 4, size=(400, 3)).astype(np.float64) / 4           # a 7^3 grid: most rows repeat
    v[10], v[11] = [0.0, 0.5, -0.0], [-0.0, 0.5, 0.0]                        # -0.0 == 0.0: one vertex
    keep, to_kept = inference.first_occurrences(v)
    want_keep, want_to = R.first_occurrences(v)
    assert np.array_equal(keep, want_keep) and np.array_equal(to_kept, want_to)
    assert keep.shape[0] < 400 and np.array_equal(v[keep][to_kept], v) and to_kept[11] == to_kept[10]
    keep, to_kept = inference.first_occurrences(rng.random((50, 3)))
    assert np.array_equal(keep, np.arange(50)) and np.array_equal(to_kept, np.arange(50))


def test_dense_rank_labels():
    from toothgroupnetwork_amd import tgnet
    assert tgnet.dense_rank_labels(np.array([0, 5, 101, 2, 0, 101])).tolist() == [-1, 1, 2, 0, -1, 2]
    assert tgnet.dense_rank_labels(np.array([[3.0], [1.0], [3.0]])).tolist() == [1, 0, 1]           # no background: teeth from 0
