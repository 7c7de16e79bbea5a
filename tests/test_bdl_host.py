"""Host: the boundary-sampled training inputs (training.BoundarySampler, training.BdlGroupingNetworkModel's configuration check)
against the REFERENCE's own BdlGroupingNetworkModel run on CPU (tests/golden/reference_cpu_r20_bdl.npz, make_golden_r20_bdl.py): what
needs no GPU -- the factory's refusal, the path maps, load_mesh, the cache-hit path, the short-mesh rule and the cache file's write."""
import os
import sys

import numpy as np
import pytest
import torch

import training_ref as R
from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import bdl_cases as BC  # noqa: E402

from toothgroupnetwork_amd import training  # noqa: E402


def _never(inputs):
    raise AssertionError("the base model must not run here")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r20_bdl.npz")))


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    """The case's mesh on disk and a sampler over it, made once: (root, sampler, vertices, labels)."""
    root = str(tmp_path_factory.mktemp("bdl"))
    BC.write_scan(root)
    sampler = training.BoundarySampler(BC.config(root), _never)
    vertices, labels = sampler.load_mesh(BC.BASE_NAME)
    return root, sampler, vertices, labels


def _tr_set(loss=True):
    cfg = {"tr_set": {"optimizer": {"lr": 1e-3, "NAME": "adam", "weight_decay": 1.0e-4},
                      "scheduler": {"sched": "cosine", "warmup_epochs": 0, "full_steps": 40, "schedueler_step": 2, "min_lr": 1e-5}}}
    if loss:
        cfg["tr_set"]["loss"] = {"cbl_loss_1": 1, "cbl_loss_2": 1, "tooth_class_loss_1": 1, "tooth_class_loss_2": 1, "offset_1_loss": 0.03,
                                 "offset_1_dir_loss": 0.03, "chamf_1_loss": 0.15}
    return cfg


# ---- 1. the factory -------------------------------------------------------------------------------------------------------------------

def test_the_factory_refuses_without_the_two_sections_and_reaches_the_class_with_them(monkeypatch):
    for present, missing in (((), "boundary_sampling_info and no fps_model_info"), (("fps_model_info",), "no boundary_sampling_info section"),
                             (("boundary_sampling_info",), "no fps_model_info section")):
        cfg = _tr_set(loss=False)                         # nothing else of the configuration is looked at before the sections
        cfg["tr_set"]["scheduler"]["sched"] = "step"
        cfg.update({name: {} for name in present})
        with pytest.raises(NotImplementedError, match="tgnet_bdl.*boundary-sampled.*" + missing) as refusal:
            training.make_training_model("tgnet_bdl", cfg)
        assert "\n" not in str(refusal.value)
    assert training._MODELS["tgnet_bdl"] is training.BdlGroupingNetworkModel
    assert issubclass(training.BdlGroupingNetworkModel, training.FpsGroupingNetworkModel)
    cfg = dict(_tr_set(), boundary_sampling_info={}, fps_model_info={})
    with pytest.raises(NotImplementedError, match="tgnet_bdl: the configuration weights cbl_loss_1 and cbl_loss_2"):
        training.make_training_model("tgnet_bdl", cfg)                       # the refusal names the model that was asked for
    with pytest.raises(NotImplementedError, match="tgnet_fps: the configuration weights"):
        training.make_training_model("tgnet_fps", _tr_set())
    cfg["tr_set"]["contrastive_boundary"] = True
    training.BdlGroupingNetworkModel.check_config(cfg)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="training needs a GPU"):          # past every configuration check, in the class's __init__
        training.make_training_model("tgnet_bdl", cfg)


# ---- 2. the path maps -----------------------------------------------------------------------------------------------------------------

def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "w").close()


def test_path_maps_skip_the_root_and_find_nested_directories(tmp_path):
    root = str(tmp_path)
    for rel in ("ROOT_upper.obj", "ROOT_upper.json", "A/A_upper.obj", "A/A_upper.json", "A/deep/er/B_lower.obj", "C/C_lower.v2.json",
                "A/notes.txt", "A/.hidden.obj"):
        _touch(os.path.join(root, rel))
    info = {"orginal_data_obj_path": root, "orginal_data_json_path": root, "bdl_cache_path": os.path.join(root, "cache")}
    sampler = training.BoundarySampler({"boundary_sampling_info": info}, _never)
    assert sampler.stl_path_map == {"A_upper": os.path.join(root, "A", "A_upper.obj"), "B_lower": os.path.join(root, "A", "deep", "er", "B_lower.obj")}
    assert sampler.json_path_map == {"A_upper": os.path.join(root, "A", "A_upper.json"), "C_lower": os.path.join(root, "C", "C_lower.v2.json")}
    with pytest.raises(KeyError, match="ROOT_upper.*" + os.path.basename(root)):
        sampler.load_mesh("ROOT_upper")                                      # files lying directly in the root are not in the maps
    with pytest.raises(KeyError, match="B_lower.json.*" + os.path.basename(root)):
        sampler.load_mesh("B_lower")                                         # an .obj without its .json
    _touch(os.path.join(root, "Z", "A_upper.obj"))
    with pytest.raises(ValueError, match="A_upper") as twice:
        training.BoundarySampler({"boundary_sampling_info": info}, _never)
    assert os.path.join("A", "A_upper.obj") in str(twice.value) and os.path.join("Z", "A_upper.obj") in str(twice.value)
    empty = training.BoundarySampler({"boundary_sampling_info": dict(info, orginal_data_obj_path=os.path.join(root, "absent"))}, _never)
    assert empty.stl_path_map == {}


# ---- 3. load_mesh ---------------------------------------------------------------------------------------------------------------------

def test_load_mesh_equals_the_reference(fx, scan):
    _, _, vertices, labels = scan
    assert vertices.dtype == np.float32 and vertices.shape == (15000, 6) and labels.shape == (15000, 1)
    assert np.issubdtype(labels.dtype, np.integer)
    assert np.array_equal(labels, fx["mesh_labels"].astype(np.int64)), "the lower jaw's labels: -20, 1x -> x, 2x -> x + 8, -1"
    assert np.array_equal(np.ascontiguousarray(vertices).view(np.uint32), fx["mesh_vertices_bits"]), "bit for bit"


# ---- 4. the cache-hit path ------------------------------------------------------------------------------------------------------------

def test_a_cache_hit_on_the_reference_made_file_equals_the_reference(fx, scan, tmp_path):
    root, _, vertices, labels = scan
    cfg = BC.config(root)
    cfg["boundary_sampling_info"]["bdl_cache_path"] = str(tmp_path / "cache")
    cache = BC.rebuild_cache(vertices, labels, fx["miss_rows"].astype(np.int64))      # the array the reference wrote (asserted by the maker)
    assert cache.dtype == np.float64 and cache.shape == (BC.INFO["num_of_all_points"], 7)
    os.makedirs(cfg["boundary_sampling_info"]["bdl_cache_path"])
    np.save(os.path.join(cfg["boundary_sampling_info"]["bdl_cache_path"], BC.BASE_NAME + ".npy"), cache)
    sampler = training.BoundarySampler(cfg, _never)
    feat, lab = sampler.sample(BC.batch(vertices, labels, root, BC.HIT_SEED))
    assert feat.dtype == torch.float32 and lab.dtype == torch.int64 and not feat.is_cuda and not lab.is_cuda
    assert tuple(feat.shape) == (1, 6, BC.INFO["num_of_all_points"]) and tuple(lab.shape) == (1, 1, BC.INFO["num_of_all_points"])
    assert np.array_equal(lab.numpy(), fx["miss_labels"].astype(np.int64))
    # the bound test_training_host.py holds augment.py to: the float64 3x3 product's summation order before the one float32 store
    assert R.within_one_ulp(np.ascontiguousarray(feat.numpy()), fx["hit_feat_bits"].view(np.float32))
    plain_feat, plain_lab = sampler.sample(BC.batch(vertices, labels, root))
    assert np.array_equal(plain_feat.numpy()[0].T, vertices[fx["miss_rows"].astype(np.int64)]) and torch.equal(plain_lab, lab)
    with pytest.raises(ValueError, match="one scan"):
        two = BC.batch(vertices, labels, root)
        two["mesh_path"] = two["mesh_path"] * 2
        sampler.sample(two)


# ---- 5. a mesh below num_of_all_points --------------------------------------------------------------------------------------------------

def test_a_short_mesh_returns_the_batch_and_writes_nothing(scan, tmp_path):
    root, _, vertices, labels = scan
    cfg = BC.config(root)
    cfg["boundary_sampling_info"].update(bdl_cache_path=str(tmp_path / "cache"), num_of_all_points=vertices.shape[0] + 1)
    sampler = training.BoundarySampler(cfg, _never)
    item = BC.batch(vertices, labels, root, BC.MISS_SEED)
    feat, lab = sampler.sample(item)
    assert feat is item["feat"] and lab is item["gt_seg_label"]
    assert not os.path.exists(str(tmp_path / "cache"))


# ---- 6. the cache file's write -----------------------------------------------------------------------------------------------------------

def test_the_cache_is_written_through_a_temporary_name(tmp_path, monkeypatch):
    path = str(tmp_path / "cache" / "P_upper.npy")
    array = np.arange(21, dtype=np.float64).reshape(3, 7)
    seen = []

    def failing_save(file, arr, *args, **kwargs):
        name = file if isinstance(file, str) else file.name
        seen.append(name)
        if not isinstance(file, str):
            file.write(b"\x93NUMPY half a file")
        raise OSError("disk full")
    keep = np.save
    monkeypatch.setattr(np, "save", failing_save)
    with pytest.raises(OSError, match="disk full"):
        training.BoundarySampler.write_cache(path, array)
    assert not os.path.exists(path) and os.listdir(os.path.dirname(path)) == [], "neither the file nor a leftover"
    assert len(seen) == 1 and seen[0] != path and os.path.dirname(seen[0]) == os.path.dirname(path), "a temporary name in the same directory"
    monkeypatch.setattr(np, "save", keep)
    training.BoundarySampler.write_cache(path, array)
    assert np.array_equal(np.load(path), array) and os.listdir(os.path.dirname(path)) == ["P_upper.npy"]
