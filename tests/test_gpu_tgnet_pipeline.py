"""GPU: inference.TgnInferencePipeLine end to end.  With tgnet_cases.py's stand-in modules it gives, on every vertex, the labels the
reference's own InferencePipeLine gave on the same OBJ with the same stand-ins (tests/golden/make_golden_r16_tgnet.py, where the
reference's answer was the same under 20 seeds of its k-means++); with two real, randomly initialised GroupingNetworkModules it runs
through, and twice the same."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import tgnet_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu

FIVE = {"model_parameter": {"input_feat": 6, "stride": [1, 4, 4, 4, 4], "nstride": [2, 2, 2, 2], "nsample": [36, 24, 24, 24, 24],
                            "blocks": [2, 3, 4, 6, 3], "block_num": 5, "planes": [32, 64, 128, 256, 512], "crop_sample_size": 3072}}
TWO = {"model_parameter": {"input_feat": 6, "stride": [1, 1], "nsample": [36, 24], "blocks": [2, 3], "block_num": 2, "planes": [16, 32],
                           "crop_sample_size": 3072}}
REAL_SEED = 0


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r16_tgnet.npz")))


@pytest.fixture(scope="module")
def objs(tmp_path_factory):
    from toothgroupnetwork_amd import synth
    root = tmp_path_factory.mktemp("tgnet_pipeline")
    paths = {}
    for name, (nu, nv, seed) in TC.MESHES.items():
        paths[name] = str(root / (name + ".obj"))
        with open(paths[name], "w") as f:
            f.write(synth.obj_text(nu, nv, seed, "plain", with_tail=False))
    text, rows = TC.obj_with_duplicates(open(paths["main"]).read())
    paths["dup"] = str(root / "dup.obj")
    with open(paths["dup"], "w") as f:
        f.write(text)
    return paths, rows


@pytest.fixture(scope="module")
def pipeline(dev):
    from toothgroupnetwork_amd import inference
    return inference.TgnInferencePipeLine(*TC.stand_ins(TC.device_knn))


def _run(pipeline, path):
    np.random.seed(TC.PERM_SEED)
    return pipeline(path)


@pytest.mark.parametrize("mesh", ["main", "small"])
def test_pipeline_labels_every_vertex_as_the_reference(fx, objs, pipeline, mesh):
    """30 000 vertices; 15 000 vertices (subdivided once before the sampling, the subdivided rows feed the boundary pass)"""
    res = _run(pipeline, objs[0][mesh])
    nu, nv, _ = TC.MESHES[mesh]
    assert res["sem"].shape == res["ins"].shape == (nu * nv,)
    assert np.array_equal(res["sem"], fx[f"pipe_{mesh}_sem"]) and np.array_equal(res["ins"], fx[f"pipe_{mesh}_ins"])
    assert set(pipeline.times) == set(pipeline.STAGES) and all(v > 0 for v in pipeline.times.values())


def test_pipeline_duplicated_vertices_take_their_originals_labels(fx, objs, pipeline):
    paths, rows = objs
    res = _run(pipeline, paths["dup"])
    n = fx["pipe_main_sem"].shape[0]
    assert res["sem"].shape == res["ins"].shape == (n + TC.N_DUPLICATES,) and np.array_equal(rows, fx["pipe_dup_rows"])
    assert np.array_equal(res["sem"][:n], fx["pipe_main_sem"]) and np.array_equal(res["ins"][:n], fx["pipe_main_ins"])
    assert np.array_equal(res["sem"][n:], fx["pipe_main_sem"][rows]) and np.array_equal(res["ins"][n:], fx["pipe_main_ins"][rows])


def test_pipeline_with_real_randomly_initialised_modules(dev, objs):
    """A five-stage and a two-stage GroupingNetworkModule with the constructors' random weights under torch.manual_seed(REAL_SEED).
    Random weights give arbitrary teeth: under this seed the scan gets through; under others a pass can find no foreground at all,
    which is tgnet.py's documented ValueError (the reference dies there too)."""
    from toothgroupnetwork_amd import inference, nets
    torch.manual_seed(REAL_SEED)
    first, bdl = nets.GroupingNetworkModule(FIVE).to(dev).eval(), nets.GroupingNetworkModule(TWO).to(dev).eval()
    pipe = inference.TgnInferencePipeLine(first, bdl)
    runs = [_run(pipe, objs[0]["main"]) for _ in range(2)]
    nu, nv, _ = TC.MESHES["main"]
    for res in runs:
        assert res["sem"].shape == res["ins"].shape == (nu * nv,)
        assert set(np.unique(res["sem"]).tolist()) <= {0} | set(range(11, 19)) | set(range(21, 29))
        assert np.array_equal(res["ins"] == 0, res["sem"] == 0)
    assert np.array_equal(runs[0]["sem"], runs[1]["sem"]) and np.array_equal(runs[0]["ins"], runs[1]["ins"])
