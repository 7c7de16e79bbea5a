"""GPU: inference.infer_paths -- many scans through the three pipeline classes -- and tools/infer.py on top of it.  The staged run of
the two-stage pipelines must give, on every vertex, what the single-scan call gives: equalities, no tolerance."""
import json
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import tgnet_cases as TC  # noqa: E402
import tsegnet_cases as SC  # noqa: E402
from pipeline_model import fixed_model  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = {**os.environ, "PYTHONDONTWRITEBYTECODE": "1"}
for _k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TGN_RUN_DIR"):
    ENV.pop(_k, None)

FIVE = {"model_parameter": {"input_feat": 6, "stride": [1, 4, 4, 4, 4], "nstride": [2, 2, 2, 2], "nsample": [36, 24, 24, 24, 24],
                            "blocks": [2, 3, 4, 6, 3], "block_num": 5, "planes": [32, 64, 128, 256, 512], "crop_sample_size": 3072}}
TWO = {"model_parameter": {"input_feat": 6, "stride": [1, 1], "nsample": [36, 24], "blocks": [2, 3], "block_num": 2, "planes": [16, 32],
                           "crop_sample_size": 3072}}
REAL_SEED = 0
# tests/test_gpu_subdivide.py's scans: 7 000 vertices (subdivided), 30 000, and 6 030 (23 807 points after the pass: refused)
EXTRA = {"seg_small": (100, 70, 61), "seg_big": (200, 150, 62), "too_small": (90, 67, 63)}


@pytest.fixture(scope="module")
def objs(tmp_path_factory):
    from toothgroupnetwork_amd import synth
    root = tmp_path_factory.mktemp("infer_paths")
    paths = {}
    for name, (nu, nv, seed) in {**TC.MESHES, **EXTRA}.items():
        paths[name] = str(root / (name + ".obj"))
        with open(paths[name], "w") as f:
            f.write(synth.obj_text(nu, nv, seed, "plain", with_tail=False))
    text, _ = TC.obj_with_duplicates(open(paths["main"]).read())
    paths["dup"] = str(root / "dup.obj")
    with open(paths["dup"], "w") as f:
        f.write(text)
    return paths


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) == {"sem", "ins"} and g["sem"].shape == w["sem"].shape
        assert np.array_equal(g["sem"], w["sem"]) and np.array_equal(g["ins"], w["ins"])


def _tseg_model():
    return types.SimpleNamespace(cent_module=SC.Stage(SC.fixed_cent), seg_module=SC.Stage(SC.fixed_seg), get_ddf=None)


def test_tgnet_stand_ins_equal_the_sequential_loop_and_the_reference(dev, objs):
    from toothgroupnetwork_amd import inference
    fx = np.load(os.path.join(GOLDEN, "reference_cpu_r16_tgnet.npz"))
    pipe = inference.TgnInferencePipeLine(*TC.stand_ins(TC.device_knn))
    paths = [objs["main"], objs["small"], objs["dup"], objs["main"]]
    np.random.seed(TC.PERM_SEED)
    want = [pipe(p) for p in paths]
    np.random.seed(TC.PERM_SEED)
    stats = {}
    got = inference.infer_paths(pipe, paths, batch=2, workers=2, staged=True, stats=stats)
    _same(got, want)                                    # (the two `main` entries need not equal each other: the generator has moved on)
    assert np.array_equal(got[0]["sem"], fx["pipe_main_sem"]) and np.array_equal(got[0]["ins"], fx["pipe_main_ins"])
    assert got[2]["sem"].shape == (fx["pipe_main_sem"].shape[0] + TC.N_DUPLICATES,)
    assert {"load", "sample", "compute", "finish", "first", "resample", "boundary", "merge"} <= set(stats)
    np.random.seed(TC.PERM_SEED)
    _same(inference.infer_paths(pipe, paths, batch=2, workers=2), want)         # whichever way the measurement routed the name


def test_tsegnet_stand_ins_equal_the_single_scan_pipeline(dev, objs):
    from toothgroupnetwork_amd import inference
    pipe = inference.TSegNetInferencePipeLine(_tseg_model())
    paths = [objs["seg_small"], objs["seg_big"], objs["seg_small"]]
    want = [pipe(p) for p in paths[:2]]
    assert (want[0]["sem"] > 0).any() and (want[1]["sem"] > 0).any(), "the scripted stages must paint some teeth"
    got = inference.infer_paths(pipe, paths, batch=2, workers=2, staged=True)
    assert [g["sem"].shape for g in got] == [(7000,), (30000,), (7000,)]
    _same(got, want + want[:1])
    _same(inference.infer_paths(pipe, paths, batch=2, workers=2), want + want[:1])


def test_tgnet_real_modules_equal_the_sequential_loop(dev, objs):
    """Two randomly initialised GroupingNetworkModules (the seed of tests/test_gpu_tgnet_pipeline.py, under which the scan gets through):
    one scan per network call, compute on the calling thread in path order, helper threads on their own streams -- so the staged run
    is the sequential loop's arithmetic, and every vertex gets the same label."""
    from toothgroupnetwork_amd import inference, nets
    torch.manual_seed(REAL_SEED)
    first, bdl = nets.GroupingNetworkModule(FIVE).to(dev).eval(), nets.GroupingNetworkModule(TWO).to(dev).eval()
    pipe = inference.TgnInferencePipeLine(first, bdl)
    paths = [objs["main"]] * 3
    np.random.seed(TC.PERM_SEED)
    want = [pipe(p) for p in paths]
    np.random.seed(TC.PERM_SEED)
    got = inference.infer_paths(pipe, paths, batch=2, workers=2, staged=True)
    _same(got, want)
    assert (got[0]["sem"] > 0).any()


def test_a_semantic_pipeline_equals_the_single_scan_pipeline(dev, objs):
    """two scans per network call, a ragged last call: `fixed_model` is exactly rounded, so the labels are the single-scan call's"""
    from toothgroupnetwork_amd import inference
    pipe = inference.InferencePipeLine(fixed_model)
    paths = [objs["seg_small"], objs["seg_big"], objs["main"]]
    want = [pipe(p) for p in paths]
    stats = {}
    _same(inference.infer_paths(pipe, paths, batch=2, workers=2, stats=stats), want)
    assert {"load", "sample", "compute", "finish", "model"} <= set(stats)


def test_a_mesh_one_pass_cannot_lift_fails_alone(dev, objs):
    from toothgroupnetwork_amd import inference
    pipe = inference.TSegNetInferencePipeLine(_tseg_model())
    paths = [objs["seg_big"], objs["too_small"], objs["seg_small"]]
    with pytest.raises(NotImplementedError, match="too_small.obj: .*the reference fails on such a mesh too"):
        inference.infer_paths(pipe, paths, batch=2, workers=2, staged=True)
    got = inference.infer_paths(pipe, paths, batch=2, workers=2, staged=True, on_error="skip")
    assert set(got[1]) == {"error"} and "NotImplementedError" in got[1]["error"] and objs["too_small"] in got[1]["error"]
    _same([got[0], got[2]], [pipe(paths[0]), pipe(paths[2])])
    one = inference.InferencePipeLine(fixed_model)
    semantic = inference.infer_paths(one, paths, batch=2, workers=2, on_error="skip")
    assert set(semantic[1]) == {"error"} and "NotImplementedError" in semantic[1]["error"] and objs["too_small"] in semantic[1]["error"]
    _same([semantic[0], semantic[2]], [one(paths[0]), one(paths[2])])
    # the pools left no stream mid-flight: the device answers, and the next run is right
    torch.cuda.synchronize()
    _same(inference.infer_paths(pipe, paths[:1], batch=2, workers=2, staged=True), [got[0]])


# ---- tools/infer.py --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dataset(dev, objs, tmp_path_factory):
    """two patients (one left out by the split file) and a randomly initialised pointnetpp checkpoint"""
    from toothgroupnetwork_amd import nets
    root = tmp_path_factory.mktemp("infer_cli")
    scans = {"PA/PA_upper.obj": "main", "PA/PA_lower.obj": "small", "PB/PB_upper.obj": "main"}
    for rel, name in scans.items():
        os.makedirs(os.path.dirname(str(root / "in" / rel)), exist_ok=True)
        shutil.copy(objs[name], str(root / "in" / rel))
    (root / "split.txt").write_text("PA\n")
    torch.manual_seed(3)
    module = nets.PointPpFirstModule({})
    with torch.no_grad():                       # the constructor's weights let the class biases decide: every vertex gets one label
        for p in module.parameters():
            if p.dim() > 1:
                p.mul_(4.0)
    torch.save(module.state_dict(), str(root / "pnpp.h5"))
    taken = sorted(str(root / "in" / rel) for rel in scans if rel.startswith("PA/"))
    return {"root": root, "argv": ["--input_dir_path", str(root / "in"), "--split_txt_path", str(root / "split.txt"), "--model_name", "pointnetpp",
                                   "--checkpoint_path", str(root / "pnpp")], "taken": taken}


LINE_KEYS = {"metric", "model_name", "scans", "written", "failed", "scans_per_s", "stage_ms", "ranks", "backend", "n_gpus"}


def test_infer_tool_in_process(dev, dataset, monkeypatch, capsys):
    """One network call per scan (--batch 1), so that the files equal results.predict on the single-scan pipeline by construction: the
    library GEMMs pick kernels by row count."""
    from toothgroupnetwork_amd import inference, launch, results
    import importlib.util
    spec = importlib.util.spec_from_file_location("tgn_tools_infer", os.path.join(REPO, "tools", "infer.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    save = str(dataset["root"] / "out_one")
    monkeypatch.setattr(launch, "_RUN", launch._Run())
    monkeypatch.setenv("TGN_RUN_DIR", str(dataset["root"] / "run_one"))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    tool.main(dataset["argv"] + ["--save_path", save, "--batch", "1", "--workers", "2", "--gt_dir", save])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert LINE_KEYS | {"iou", "f1", "acc", "sem_acc", "unscored", "scored"} <= set(line)
    assert line["model_name"] == "pointnetpp" and line["scans"] == line["written"] == 2 and line["failed"] == [] and line["scans_per_s"] > 0
    assert sorted(os.listdir(save)) == ["PA_lower.json", "PA_upper.json"]
    pipe = inference.make_inference_pipeline("pointnetpp", [str(dataset["root"] / "pnpp.h5")])
    for path in dataset["taken"]:
        labels, instances, jaw = results.predict(pipe, path)
        got = json.load(open(os.path.join(save, os.path.basename(path).replace(".obj", ".json"))))
        assert got["jaw"] == jaw and got["labels"] == labels and got["instances"] == instances
        assert len(set(labels)) > 1, "the random network must not label everything alike"
    assert line["scored"] == 2 and line["unscored"] == 0.0
    assert line["iou"] == line["f1"] == line["acc"] == line["sem_acc"] == 1.0


def test_infer_tool_gpus_2_on_one_gpu(dev, dataset):
    """a fresh child that starts two gloo ranks sharing this GPU, as tests/test_gpu_launch.py's runs do"""
    save = str(dataset["root"] / "out_two")
    cmd = [sys.executable, os.path.join(REPO, "tools", "infer.py"), *dataset["argv"], "--save_path", save, "--batch", "1", "--workers", "2",
           "--gpus", "2", "--backend", "gloo"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert LINE_KEYS <= set(line) and line["n_gpus"] == 2 and line["self_spawned"] is True and line["backend"] == "gloo"
    assert [r["rank"] for r in line["ranks"]] == [0, 1] and len({r["pid"] for r in line["ranks"]}) == 2
    assert line["scans"] == line["written"] == 2 and line["per_rank_scans"] == [1, 1] and line["failed"] == []
    assert sorted(os.listdir(save)) == ["PA_lower.json", "PA_upper.json"]
