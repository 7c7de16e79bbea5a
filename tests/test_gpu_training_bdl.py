"""GPU: training tgnet's second module (training.BoundarySampler, training.BdlGroupingNetworkModel, tools/train.py --model_name tgnet_bdl).

  1. the scripted case of tests/golden/bdl_cases.py through the sampler on the device, against what the REFERENCE's own
     BdlGroupingNetworkModel gave for it on the CPU (tests/golden/reference_cpu_r20_bdl.npz): the flags of all 15 000 vertices, the
     partition of the batch's points, the selection, the cache file, the returns of a cache miss, a cache hit and the validation path;
  2. the real modules at the smallest shapes that exercise every join: 4096 points a scan (3072 of them boundary rows at most), crops
     of 3072, the five-stage first module seeded with BASE_SEED and saved through FpsGroupingNetworkModel.save, the 15 000-vertex mesh;
  3. both checkpoints in inference.make_inference_pipeline("tgnet", ...); 4. the command line in a child process.

The file's name sorts behind test_gpu_hotpath_configs.py on purpose ("timing check")."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import training_ref as R
from conftest import GOLDEN, REPO

sys.path.insert(0, GOLDEN)
import bdl_cases as BC  # noqa: E402
import tgnet_cases as TC  # noqa: E402
import training_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

FIVE_STAGE = {"input_feat": 6, "stride": [1, 4, 4, 4, 4], "nstride": [2, 2, 2, 2], "nsample": [36, 24, 24, 24, 24], "blocks": [2, 3, 4, 6, 3],
              "block_num": 5, "planes": [32, 64, 128, 256, 512], "crop_sample_size": 3072}
TWO_STAGE = {"input_feat": 6, "stride": [1, 1], "nsample": [36, 24], "blocks": [2, 3], "block_num": 2, "planes": [16, 32], "crop_sample_size": 3072}
LOSS = {"cbl_loss_1": 1, "cbl_loss_2": 1, "tooth_class_loss_1": 1, "tooth_class_loss_2": 1, "offset_1_loss": 0.03, "offset_1_dir_loss": 0.03,
        "chamf_1_loss": 0.15}
N_ALL, N_BDL = 4096, 3072
# torch.manual_seed in front of the first module's construction.  Of the seeds 20..24 on this mesh, 20 gives 4048 foreground points of
# 4096 in 14 clusters and flags 2966 of the 15 000 vertices; 23 votes every point into the background, which the sampler refuses.
BASE_SEED = 20
N_VERTICES = TC.MESHES["small"][0] * TC.MESHES["small"][1]


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r20_bdl.npz")))


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    """The case's mesh on disk: (root, vertices, labels), load_mesh's."""
    from toothgroupnetwork_amd import training
    root = str(tmp_path_factory.mktemp("bdl"))
    BC.write_scan(root)
    vertices, labels = training.BoundarySampler(BC.config(root), None).load_mesh(BC.BASE_NAME)
    return root, vertices, labels


def _spied_sample(sampler, item):
    """sampler.sample(item) after np.random.seed(PERM_SEED) -> (feat, labels, what tgnet.boundary_flags and tgnet.second_instances returned)"""
    from toothgroupnetwork_amd import tgnet
    seen = {}
    keep = tgnet.boundary_flags, tgnet.second_instances

    def flags(*args, **kwargs):
        seen["flags"] = keep[0](*args, **kwargs)
        return seen["flags"]

    def instances(*args, **kwargs):
        seen["instances"] = keep[1](*args, **kwargs)
        return seen["instances"]
    tgnet.boundary_flags, tgnet.second_instances = flags, instances
    try:
        np.random.seed(BC.PERM_SEED)
        feat, labels = sampler.sample(item)
    finally:
        tgnet.boundary_flags, tgnet.second_instances = keep
    return feat, labels, seen


def _host_flags(seen):
    boundary = seen["flags"][0]
    return boundary.cpu().numpy() if isinstance(boundary, torch.Tensor) else np.asarray(boundary)


def _stored_flags(packed):
    return np.unpackbits(packed)[:N_VERTICES].astype(bool)


# ---- 1. the scripted case against the reference's class ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def miss(dev, fx, scan):
    """The cache-miss call under the MISS_SEED augmentation and the second call for the same scan under HIT_SEED's, made once."""
    from toothgroupnetwork_amd import training
    root, vertices, labels = scan
    base = BC.BaseStandIn(TC.device_knn, fx["centres_miss"])
    sampler = training.BoundarySampler(BC.config(root, "miss"), base)
    feat, lab, seen = _spied_sample(sampler, BC.batch(vertices, labels, root, BC.MISS_SEED))
    calls = base.calls
    cache_path = os.path.join(sampler.info["bdl_cache_path"], BC.BASE_NAME + ".npy")
    cache = np.load(cache_path)
    np.random.seed(7)
    hit_feat, hit_lab = sampler.sample(BC.batch(vertices, labels, root, BC.HIT_SEED))
    return dict(feat=feat, lab=lab, seen=seen, calls=calls, cache=cache, hit_feat=hit_feat, hit_lab=hit_lab, calls_after=base.calls,
                files=sorted(os.listdir(sampler.info["bdl_cache_path"])))


def test_every_vertex_has_the_reference_flag_and_the_batch_its_partition(fx, miss):
    flags = _host_flags(miss["seen"])
    want = _stored_flags(fx["miss_flags"])
    assert flags.shape == want.shape and np.array_equal(flags, want), f"{int((flags != want).sum())} of {want.shape[0]} flags differ"
    ins = miss["seen"]["instances"]["ins"].cpu().numpy() - 1
    want = fx["miss_point_labels"].astype(np.int64)
    assert np.array_equal(ins == -1, want == -1), "the background"
    assert BC.same_partition(ins, want), "the clusters, up to their numbers"


def test_the_selection_the_cache_file_and_the_returns_equal_the_reference(fx, scan, miss):
    _, vertices, labels = scan
    rows = fx["miss_rows"].astype(np.int64)
    assert miss["calls"] == 1
    cache = miss["cache"]
    assert cache.dtype == np.float64 and cache.shape == (BC.INFO["num_of_all_points"], 7) and miss["files"] == [BC.BASE_NAME + ".npy"]
    want = BC.rebuild_cache(vertices, labels, rows)                          # the reference's file (asserted by the maker)
    assert np.array_equal(cache.view(np.uint64), want.view(np.uint64)), "the selected rows, boundary rows first, and their labels: bit for bit"
    feat, lab = miss["feat"], miss["lab"]
    assert feat.dtype == torch.float32 and lab.dtype == torch.int64 and not feat.is_cuda and not lab.is_cuda
    assert tuple(feat.shape) == (1, 6, BC.INFO["num_of_all_points"])
    assert np.array_equal(lab.numpy(), fx["miss_labels"].astype(np.int64))
    # the bound test_training_host.py holds augment.py to: the float64 3x3 product's summation order before the float32 store
    assert R.within_one_ulp(np.ascontiguousarray(feat.numpy()), fx["miss_feat_bits"].view(np.float32))


def test_a_second_call_for_the_scan_is_served_from_the_cache(fx, miss):
    assert miss["calls_after"] == 1, "the base model ran again"
    assert np.array_equal(miss["hit_lab"].numpy(), fx["miss_labels"].astype(np.int64))
    assert miss["hit_feat"].dtype == torch.float32
    assert R.within_one_ulp(np.ascontiguousarray(miss["hit_feat"].numpy()), fx["hit_feat_bits"].view(np.float32))


def test_the_validation_path_equals_the_reference_bit_for_bit(dev, fx, scan):
    from toothgroupnetwork_amd import training
    root, vertices, labels = scan
    base = BC.BaseStandIn(TC.device_knn, fx["centres_val"])
    sampler = training.BoundarySampler(BC.config(root, "val"), base)
    feat, lab, seen = _spied_sample(sampler, BC.batch(vertices, labels, root))
    assert np.array_equal(_host_flags(seen), _stored_flags(fx["val_flags"]))
    rows = fx["val_rows"].astype(np.int64)
    assert feat.dtype == torch.float32 and np.array_equal(feat.numpy()[0].T.view(np.uint32), np.ascontiguousarray(vertices[rows]).view(np.uint32))
    assert np.array_equal(lab.numpy(), fx["val_labels"].astype(np.int64)) and np.array_equal(lab.numpy().reshape(-1), labels[rows].reshape(-1))
    cache = np.load(os.path.join(sampler.info["bdl_cache_path"], BC.BASE_NAME + ".npy"))
    assert np.array_equal(cache, BC.rebuild_cache(vertices, labels, rows)) and base.calls == 1


# ---- 2. the real modules -------------------------------------------------------------------------------------------------------------------

def _tr_set():
    return {"optimizer": {"lr": 1e-2, "NAME": "sgd", "momentum": 0.9, "weight_decay": 1.0e-4},
            "scheduler": {"sched": "cosine", "warmup_epochs": 0, "full_steps": 40, "schedueler_step": 15000000, "min_lr": 1e-5},
            "loss": dict(LOSS), "contrastive_boundary": True}


def _bdl_config(root, base_ckpt, ckpt, cache):
    info = {"orginal_data_obj_path": root, "orginal_data_json_path": root, "bdl_cache_path": cache, "bdl_ratio": 0.7,
            "num_of_bdl_points": N_BDL, "num_of_all_points": N_ALL}
    return {"tr_set": _tr_set(), "checkpoint_path": ckpt, "model_parameter": copy.deepcopy(TWO_STAGE), "boundary_sampling_info": info,
            "fps_model_info": {"model_parameter": copy.deepcopy(FIVE_STAGE), "load_ckpt_path": base_ckpt}}


@pytest.fixture(scope="module")
def world(dev, scan, tmp_path_factory):
    """The preprocessed scan of the case's mesh (N_ALL of its vertices, as preprocess_data.py writes them) and the saved first module."""
    from toothgroupnetwork_amd import training
    root, vertices, labels = scan
    work = tmp_path_factory.mktemp("bdl_real")
    data = work / "data"
    data.mkdir()
    pick = np.sort(np.random.default_rng(2020).choice(N_VERTICES, N_ALL, replace=False))
    np.save(str(data / f"{BC.BASE_NAME}_sampled_points.npy"), np.concatenate([vertices[pick].astype(np.float64), labels[pick] + 1.0], axis=1))
    base_ckpt = str(work / "ckpts" / "tgnet_fps")
    torch.manual_seed(BASE_SEED)
    fps_cfg = {"tr_set": _tr_set(), "checkpoint_path": base_ckpt, "model_parameter": copy.deepcopy(FIVE_STAGE)}
    training.FpsGroupingNetworkModel(fps_cfg).save("train")
    return dict(root=root, work=work, data=str(data), base_ckpt=base_ckpt)


def _loader(world, chain):
    from toothgroupnetwork_amd import training
    return torch.utils.data.DataLoader(training.DentalModelGenerator(world["data"], aug_obj_str=chain), shuffle=False, batch_size=1,
                                       collate_fn=training.collate_fn)


@pytest.fixture(scope="module")
def trained(dev, world):
    """make_training_model("tgnet_bdl", ...), two train steps and a validation step, save: made once."""
    from toothgroupnetwork_amd import training
    cfg = _bdl_config(world["root"], world["base_ckpt"], str(world["work"] / "ckpts" / "tgnet_bdl"), str(world["work"] / "cache"))
    torch.manual_seed(21)
    np.random.seed(21)
    model = training.make_training_model("tgnet_bdl", cfg)
    loaded = torch.load(world["base_ckpt"] + ".h5")
    at_load = {k: v.detach().clone() for k, v in model.base_model.state_dict().items()}
    before = {k: v.detach().clone() for k, v in model.module.state_dict().items()}
    (train_item,), (val_item,) = list(_loader(world, C.DEFAULT_CHAIN)), list(_loader(world, None))
    maps = [model.step(0, train_item, "train")]                              # a cache miss under an augmentation
    files = sorted(os.listdir(cfg["boundary_sampling_info"]["bdl_cache_path"]))
    maps.append(model.step(1, next(iter(_loader(world, C.DEFAULT_CHAIN))), "train"))      # a cache hit under another draw
    maps.append(model.step(0, val_item, "val"))
    model.save("train")
    return dict(model=model, cfg=cfg, loaded=loaded, at_load=at_load, before=before, maps=maps, files=files)


def test_the_base_model_is_loaded_strictly_and_stays_frozen(trained):
    from toothgroupnetwork_amd import nets, training
    model = trained["model"]
    assert isinstance(model, training.BdlGroupingNetworkModel) and isinstance(model.base_model, nets.GroupingNetworkModule)
    assert model.sampler.base_model is model.base_model and model.base_model.config["model_parameter"]["block_num"] == 5
    now = model.base_model.state_dict()
    assert set(now) == set(trained["loaded"]) == set(trained["at_load"]), "strict: every key of the checkpoint and no other"
    for key, value in now.items():                                           # parameters AND buffers (the BatchNorm statistics)
        assert torch.equal(value.cpu(), trained["loaded"][key].cpu()) and torch.equal(value, trained["at_load"][key]), key
    assert not model.base_model.training and not any(m.training for m in model.base_model.modules())
    assert not any(p.requires_grad for p in model.base_model.parameters())
    assert any(b.dtype.is_floating_point for b in model.base_model.buffers()), "the first module has running statistics to drift"


def test_the_optimiser_holds_the_trained_module_only_and_it_moved(trained):
    model = trained["model"]
    held = [id(p) for group in model.optimizer.param_groups for p in group["params"]]
    assert sorted(held) == sorted(id(p) for p in model.module.parameters()) and len(set(held)) == len(held)
    assert not set(held) & {id(p) for p in model.base_model.parameters()}
    assert model.module.config["model_parameter"]["block_num"] == 2
    after = model.module.state_dict()
    moved = [k for k, v in after.items() if v.is_floating_point() and not torch.equal(v, trained["before"][k])]
    assert any(k.startswith("first_ins_cent_model.") for k in moved) and any(k.startswith("second_ins_cent_model.") for k in moved)
    assert not model.module.training, "the validation step came last"


def test_the_loss_maps_hold_seven_terms_in_training_and_five_in_validation(trained):
    from toothgroupnetwork_amd import training
    five = set(training.FpsGroupingNetworkModel.TERMS)
    for lmap, post_fix, names in zip(trained["maps"], ("train", "step", "val"), (five | {"cbl_loss_1", "cbl_loss_2"},) * 2 + (five,)):
        assert set(lmap.loss_dict) == names and len(names) in (5, 7)
        printed = lmap.get_loss_dict_for_print(post_fix)
        print("  " + " ".join(f"{k}={v:.4g}" for k, v in printed.items()))
        assert all(np.isfinite(v) for v in printed.values()), printed
        assert {name: weight for name, (_, weight) in lmap.loss_dict.items()} == {name: LOSS[name] for name in names}
    assert trained["files"] == [BC.BASE_NAME + ".npy"], "the first step wrote the scan's cache file and nothing else"
    cache = np.load(os.path.join(trained["cfg"]["boundary_sampling_info"]["bdl_cache_path"], BC.BASE_NAME + ".npy"))
    assert cache.dtype == np.float64 and cache.shape == (N_ALL, 7)


# ---- 3. the two checkpoints in the inference pipeline --------------------------------------------------------------------------------------

def test_both_checkpoints_load_into_the_tgnet_pipeline(trained, world):
    from toothgroupnetwork_amd import inference
    paths = [world["base_ckpt"] + ".h5", trained["cfg"]["checkpoint_path"] + ".h5"]
    assert set(torch.load(paths[1])) == set(trained["model"].module.state_dict()), "save() holds the trained module and not the base"
    pipe = inference.make_inference_pipeline("tgnet", paths)                 # load_state_dict's default: strict
    for module, source in ((pipe.first_module, trained["model"].base_model), (pipe.bdl_module, trained["model"].module)):
        loaded = module.state_dict()
        assert set(loaded) == set(source.state_dict()) and all(torch.equal(loaded[k], v) for k, v in source.state_dict().items())
    assert not pipe.first_module.training and not pipe.bdl_module.training


# ---- 4. the command line ---------------------------------------------------------------------------------------------------------------------

def test_the_command_line_trains_one_epoch_in_a_child_process(world, tmp_path):
    from toothgroupnetwork_amd import training
    cfg = _bdl_config(world["root"], world["base_ckpt"], "unused", str(tmp_path / "cache"))
    del cfg["checkpoint_path"], cfg["tr_set"]["contrastive_boundary"]        # the reference's file has neither: tools/train.py sets both
    (tmp_path / "tgnet_bdl.py").write_text("config = " + repr(cfg) + "\n")
    (tmp_path / "split.txt").write_text(BC.PATIENT + "\n")
    cmd = [sys.executable, os.path.join(REPO, "tools", "train.py"), "--model_name", "tgnet_bdl", "--config_path", str(tmp_path / "tgnet_bdl.py"),
           "--experiment_name", "bdl_cli", "--input_data_dir_path", world["data"], "--train_data_split_txt_path", str(tmp_path / "split.txt"),
           "--val_data_split_txt_path", str(tmp_path / "split.txt"), "--epochs", "1", "--seed", "3"]
    done = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
    assert done.returncode == 0, done.stderr[-2000:]
    lines = [json.loads(x) for x in done.stdout.splitlines()]
    assert len(lines) == 2, done.stdout
    terms = set(training.FpsGroupingNetworkModel.TERMS)
    assert set(lines[0]) == {"step", "step_lr", "total_step"} | {f"{t}_step" for t in terms | {"cbl_loss_1", "cbl_loss_2"}}
    assert {f"{t}_train" for t in terms | {"cbl_loss_1", "cbl_loss_2"}} | {f"{t}_val" for t in terms} <= set(lines[1])
    assert "cbl_loss_1_val" not in lines[1] and all(np.isfinite(v) for v in lines[1].values())
    assert "train_set 1" in done.stderr and "validation_set 1" in done.stderr
    for suffix in (".h5", "_val.h5"):
        state = torch.load(str(tmp_path / "ckpts" / ("bdl_cli" + suffix)))
        assert any(k.startswith("first_ins_cent_model.") for k in state) and any(k.startswith("second_ins_cent_model.") for k in state)
    files = sorted(os.listdir(str(tmp_path / "cache")))
    assert files == [BC.BASE_NAME + ".npy"], "one cache file per scan"
    cache = np.load(str(tmp_path / "cache" / files[0]))
    assert cache.dtype == np.float64 and cache.shape == (N_ALL, 7)
