"""GPU: midpoint subdivision (csrc/subdivide.hip, preprocess.subdivide_midpoint) and the three inference entry points on meshes below
24 000 vertices.
  * on every case of tests/subdivide_ref.py's list the kernel's vertices, normals (float64 viewed as int64) and triangles equal the
    dictionary-loop reference, for one pass and for two; a second call and a call on a non-default stream give identical arrays;
  * the C ABI called directly with a workspace of exactly tgn_subdivide_midpoint_workspace_bytes(nf) bytes, and its error word;
  * the pipelines on a 7 000-vertex mesh against the same stages composed here with the REFERENCE subdivision in place of the kernel,
    infer_scans against the single-scan pipeline, and a mesh one pass cannot lift above 24 000 points.
Parity with open3d itself is unpinned: the contract is restated from its source."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subdivide_ref as S  # noqa: E402
import tsegnet_cases as TC  # noqa: E402
from pipeline_model import fixed_model  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ["one_triangle", "shared_edge_opposite", "shared_edge_same", "tetrahedron", "edge_of_three_triangles", "repeated_index",
         "unreferenced_vertex", "no_normals", "arch_shuffled", "arch_rotated"]


# ---- the kernel against the reference ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_one_pass_equals_the_reference_in_bits(dev, name):
    from toothgroupnetwork_amd import preprocess
    mesh = S.cases()[name]
    keep = {k: v.copy() for k, v in mesh.items()}
    got = preprocess.subdivide_midpoint(mesh)
    assert S.same_bits(mesh, keep), "the input is left alone"
    want = S.reference(name)
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
    assert np.array_equal(got["triangles"], want["triangles"])
    assert np.array_equal(got["vertices"].view(np.int64), want["vertices"].view(np.int64))
    if "vertex_normals" in want:
        assert np.array_equal(got["vertex_normals"].view(np.int64), want["vertex_normals"].view(np.int64))


@pytest.mark.parametrize("name", CASES)
def test_two_passes_equal_the_reference_applied_twice(dev, name):
    from toothgroupnetwork_amd import preprocess
    got = preprocess.subdivide_midpoint(S.cases()[name], number_of_iterations=2)
    assert S.same_bits(got, S.reference(name, 2))
    assert got["triangles"].shape[0] == 16 * S.cases()[name]["triangles"].shape[0]


def test_a_second_call_and_a_side_stream_give_identical_arrays(dev):
    from toothgroupnetwork_amd import preprocess
    for name in ("arch_shuffled", "edge_of_three_triangles"):
        mesh = S.cases()[name]
        first = preprocess.subdivide_midpoint(mesh)
        second = preprocess.subdivide_midpoint(mesh)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            side = preprocess.subdivide_midpoint(mesh)
            s.synchronize()
        assert S.same_bits(first, S.reference(name)) and S.same_bits(second, first) and S.same_bits(side, first)


def test_device_entry_keeps_the_tensors_on_the_gpu(dev):
    from toothgroupnetwork_amd import preprocess
    mesh = S.cases()["arch_rotated"]
    v, n, t = (torch.from_numpy(mesh[k].copy()).to(dev) for k in ("vertices", "vertex_normals", "triangles"))
    ov, on, ot = preprocess.subdivide_midpoint_device(v, n, t, 1)
    want = S.reference("arch_rotated")
    assert ov.is_cuda and on.is_cuda and ot.is_cuda
    assert S.same_bits({"vertices": ov.cpu().numpy(), "vertex_normals": on.cpu().numpy(), "triangles": ot.cpu().numpy()}, want)
    with pytest.raises(TypeError):
        preprocess.subdivide_midpoint_device(v.float(), None, t)
    bad = t.clone()
    bad[17, 2] = v.shape[0]                                          # checked on the device: latched, never dereferenced
    with pytest.raises(ValueError, match="triangle index outside"):
        preprocess.subdivide_midpoint_device(v, n, bad)


# ---- the C ABI, directly ---------------------------------------------------------------------------------------------------------------

def _call_capi(dev, mesh, pad_rows=5):
    """-> (n_new, out_vertices, out_normals or None, out_triangles) as numpy, the workspace EXACTLY as large as the library asks for and
    `pad_rows` sentinel rows behind every output's upper bound."""
    from toothgroupnetwork_amd import _lib as L
    v, t = torch.from_numpy(np.ascontiguousarray(mesh["vertices"])).to(dev), torch.from_numpy(np.ascontiguousarray(mesh["triangles"])).to(dev)
    n = torch.from_numpy(np.ascontiguousarray(mesh["vertex_normals"])).to(dev) if "vertex_normals" in mesh else None
    nv, nf = v.shape[0], t.shape[0]
    need = L.lib().tgn_subdivide_midpoint_workspace_bytes(nf)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out_v = torch.full((nv + 3 * nf + pad_rows, 3), -7.0, dtype=torch.float64, device=dev)
    out_n = torch.full_like(out_v, -7.0) if n is not None else None
    out_t = torch.full((4 * nf + pad_rows, 3), -7, dtype=torch.int64, device=dev)
    count = torch.full((1,), 12345, dtype=torch.int32, device=dev)
    L.check(L.lib().tgn_subdivide_midpoint(nv, nf, L.ptr(v), L.ptr(n), L.ptr(t), L.ptr(out_v), L.ptr(out_n), L.ptr(out_t), L.ptr(count),
                                          L.ptr(ws), need, L.stream()), "tgn_subdivide_midpoint")
    torch.cuda.synchronize()
    return int(count.item()), out_v.cpu().numpy(), (None if out_n is None else out_n.cpu().numpy()), out_t.cpu().numpy()


@pytest.mark.parametrize("name", ["tetrahedron", "no_normals", "arch_shuffled"])
def test_capi_with_the_exact_workspace(dev, name):
    mesh, want = S.cases()[name], S.reference(name)
    nv, nf = mesh["vertices"].shape[0], mesh["triangles"].shape[0]
    new, out_v, out_n, out_t = _call_capi(dev, mesh)
    assert new == want["vertices"].shape[0] - nv
    assert np.array_equal(out_v[:nv + new].view(np.int64), want["vertices"].view(np.int64))
    assert (out_v[nv + new:] == -7.0).all(), "rows behind nv + n_new stay untouched"
    assert np.array_equal(out_t[:4 * nf], want["triangles"]) and (out_t[4 * nf:] == -7).all()
    if "vertex_normals" in mesh:
        assert np.array_equal(out_n[:nv + new].view(np.int64), want["vertex_normals"].view(np.int64)) and (out_n[nv + new:] == -7.0).all()
    else:
        assert out_n is None


def test_capi_latches_a_bad_index_and_handles_an_empty_mesh(dev):
    mesh = {k: v.copy() for k, v in S.cases()["arch_shuffled"].items()}
    mesh["triangles"][1000, 1] = mesh["vertices"].shape[0]          # one past the end
    mesh["triangles"][5, 0] = -1
    new, _, _, _ = _call_capi(dev, mesh)
    assert new == -1, "n_new = -(error bits), bit 1 = a triangle index outside [0, nv)"
    good = S.cases()["arch_shuffled"]
    assert _call_capi(dev, good)[0] == S.reference("arch_shuffled")["vertices"].shape[0] - 1200, "the error word is per call"
    empty = {"vertices": good["vertices"][:7], "triangles": np.zeros((0, 3), dtype=np.int64)}
    new, out_v, _, out_t = _call_capi(dev, empty)
    assert new == 0 and np.array_equal(out_v[:7], good["vertices"][:7]) and (out_v[7:] == -7.0).all() and (out_t == -7).all()


# ---- the pipelines --------------------------------------------------------------------------------------------------------------------------

SMALL, BIG, TOO_SMALL = (100, 70, 61), (200, 150, 62), (90, 67, 63)      # 7 000, 30 000 and 6 030 vertices


@pytest.fixture(scope="module")
def scans(tmp_path_factory):
    from toothgroupnetwork_amd import synth
    d = tmp_path_factory.mktemp("subdivide_scans")
    paths = {}
    for name, (nu, nv, seed) in (("small", SMALL), ("big", BIG), ("too_small", TOO_SMALL)):
        paths[name] = str(d / f"{name}.obj")
        with open(paths[name], "w") as f:
            f.write(synth.obj_text(nu, nv, seed, "plain", with_tail=False))
    return paths


@pytest.fixture(scope="module")
def small_by_hand(scans):
    """The 7 000-vertex scan up to the sampling, composed here with the REFERENCE subdivision: (org (7000, 6), dense (27661, 6))."""
    from toothgroupnetwork_amd import inference, preprocess
    _, mesh = preprocess.read_txt_obj_ls(scans["small"], ret_mesh=True)
    assert mesh["vertices"].shape == (7000, 3) and mesh["triangles"].shape == (13662, 3)
    org = np.concatenate([inference.normalise_for_inference(mesh["vertices"]), mesh["vertex_normals"]], axis=1)
    sub = S.subdivide_loop({"vertices": org[:, :3], "triangles": mesh["triangles"], "vertex_normals": org[:, 3:]})
    assert sub["vertices"].shape == (27661, 3), "7 000 vertices + 20 661 edges"
    return org, np.concatenate([sub["vertices"], sub["vertex_normals"]], axis=1)


def test_semantic_pipeline_labels_a_small_mesh(dev, scans, small_by_hand):
    from toothgroupnetwork_amd import inference, preprocess, resample
    pipe = inference.InferencePipeLine(fixed_model)
    out = pipe(scans["small"])
    assert out["sem"].shape == (7000,) and np.array_equal(out["sem"], out["ins"])
    assert set(pipe.times) == {"load", "sample", "model", "transfer"}
    org, dense = small_by_hand
    sampled = dense[resample.fps(dense[:, :3], 24000)[:24000]]
    with torch.no_grad():
        cls = fixed_model([torch.from_numpy(sampled.astype("float32")[None]).to(dev).permute(0, 2, 1)])["cls_pred"].argmax(1).reshape(-1).cpu().numpy()
    want = preprocess.transfer_labels(sampled[:, :3], inference.fdi_from_classes(cls), org[:, :3])
    assert np.array_equal(out["sem"], want.reshape(-1))
    assert len(np.unique(out["sem"])) > 4, "the stand-in model must not label everything alike"


def test_tsegnet_pipeline_labels_a_small_mesh(dev, scans, small_by_hand):
    from toothgroupnetwork_amd import inference, preprocess, resample, tsegnet
    model = types.SimpleNamespace(cent_module=TC.Stage(TC.fixed_cent), seg_module=TC.Stage(TC.fixed_seg), get_ddf=None)
    pipe = inference.TSegNetInferencePipeLine(model)
    out = pipe(scans["small"])
    assert out["sem"].shape == (7000,) and np.array_equal(out["sem"], out["ins"])
    assert set(pipe.times) == {"load", "sample", "centroids", "join", "segmentation", "paint", "transfer"}
    org, dense = small_by_hand
    sampled = dense[resample.fps(dense[:, :3], 24000)[:24000]]
    with torch.no_grad():
        inp = torch.from_numpy(np.ascontiguousarray(sampled.astype("float32"))[None]).to(dev).permute(0, 2, 1).contiguous()
        l0_points, _, _, l3_xyz, offset_result, dist_result = TC.fixed_cent(inp)
        moved, counts = tsegnet.centroid_proposals(l3_xyz, offset_result, dist_result)
        centres = tsegnet.cluster_centers(moved, counts)
        cropped, nn_idx, _ = tsegnet.crop_features(inp, l0_points, centres, tsegnet.CROP_K)
        _, _, pd_2, id_pred = TC.fixed_seg(cropped)
        cls = tsegnet.paint_labels(nn_idx, pd_2, id_pred, 24000).reshape(-1).cpu().numpy()
    want = preprocess.transfer_labels(sampled[:, :3], inference.fdi_from_classes(cls), org[:, :3])
    assert np.array_equal(out["sem"], want.reshape(-1))
    assert (out["sem"] > 0).any(), "the scripted stages must paint some teeth"


def test_infer_scans_mixes_small_and_large_meshes(dev, scans):
    from toothgroupnetwork_amd import inference
    paths = [scans["small"], scans["big"], scans["small"]]
    one = inference.InferencePipeLine(fixed_model)
    want = [one(p)["sem"] for p in paths[:2]]
    got = inference.infer_scans(paths, fixed_model, batch=2, workers=2)
    assert [g["sem"].shape for g in got] == [(7000,), (30000,), (7000,)]
    for g, w in zip(got, want + want[:1]):
        assert np.array_equal(g["sem"], w) and np.array_equal(g["ins"], w)


def test_a_mesh_one_pass_cannot_lift_above_24000_is_refused_everywhere(dev, scans):
    """6 030 vertices and 17 777 edges: 23 807 points after the pass, not above 24 000 -- the reference fails in gen_utils.fps there."""
    from toothgroupnetwork_amd import inference, preprocess
    _, mesh = preprocess.read_txt_obj_ls(scans["too_small"], ret_mesh=True)
    assert mesh["vertices"].shape[0] == 6030 and 6030 + 3 * mesh["triangles"].shape[0] > 24000, "only the pass itself can tell"
    assert preprocess.subdivide_midpoint(mesh)["vertices"].shape[0] == 23807
    model = types.SimpleNamespace(cent_module=TC.Stage(TC.fixed_cent), seg_module=TC.Stage(TC.fixed_seg), get_ddf=None)
    with pytest.raises(NotImplementedError, match="the reference fails on such a mesh too"):
        inference.InferencePipeLine(fixed_model)(scans["too_small"])
    with pytest.raises(NotImplementedError, match="the reference fails on such a mesh too"):
        inference.TSegNetInferencePipeLine(model)(scans["too_small"])
    with pytest.raises(NotImplementedError, match="the reference fails on such a mesh too"):
        inference.infer_scans([scans["big"], scans["too_small"]], fixed_model, batch=2, workers=2)
