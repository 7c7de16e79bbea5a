#!/usr/bin/env python3
"""Fixtures of the tgnet inference pipeline (tests/golden/reference_cpu_r16_tgnet.npz, tests/golden/tgnet_boundary_weights.pt), produced by
running the REFERENCE's own InferencePipeLine (inference_pipelines/inference_pipeline_tgn.py) on CPU in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_r16_tgnet.py [seeds]

open3d and trimesh are served (the mesh class of make_golden_r2_io.py, plus remove_duplicated_vertices as a python loop over the rows
and subdivide_midpoint as tests/subdivide_ref.py's loop), gu.fps is the CPU oracle's FPS, `.cuda()` is the identity, __init__ is bypassed
(it loads checkpoints) and the two modules are tgnet_cases.py's stand-ins with an sklearn KDTree for their crops.  Everything else is
the reference's code: __call__, get_first_module_results, get_boundary_sampled_feats, get_second_module_results, ops_utils'
clustering, sklearn's KMeans with its random k-means++ seeds.

  pipe_*    `sem` and `ins` per vertex for the 30 000-vertex mesh, the 15 000-vertex mesh (subdivision path) and the copy of the first
            with 50 duplicated vertices (the reference answers for the de-duplicated vertices: the 30 000 of the first mesh)
  first_* / teeth_*   what number_teeth reads and writes (the locals of __call__ when it returns), for the three class tables
  vote_*, bd_*, merge_*   the crop vote's sums, get_boundary_sampled_feats' flags, nearest labels and selected rows, the boundary merge
  net_*     the two-stage boundary network: the reference GroupingNetworkModule's state_dict names and shapes, and the reference
            PointTransformerSeg(block_num=2, k=10) with seeded weights (saved next to the fixture) in eval mode at N = 1024, B = 1 and
            B = 2, in float32 and in float64 on the same kNN indices

Before anything is written the main case is run under `seeds` (default 20) different np.random.seed values -- other boundary
permutations, other k-means++ seeds -- and every run must give the same labels on every vertex: the reference alone defines the answer."""
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("TGN_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from sklearn.neighbors import KDTree  # noqa: E402

import subdivide_ref  # noqa: E402
import tgnet_cases as TC  # noqa: E402
from make_golden import load_reference  # noqa: E402
from make_golden_r2_io import _stub_open3d  # noqa: E402
from make_golden_r3 import cpu_as_cuda, rel_err  # noqa: E402
from make_golden_r4 import _serve_pointops  # noqa: E402
from oracle import cpu as O, meshio as OM  # noqa: E402
from seeded import seeded_fill  # noqa: E402
from toothgroupnetwork_amd import synth  # noqa: E402

INFO = {"bdl_ratio": 0.7, "num_of_bdl_points": 20000, "num_of_all_points": 24000}      # inference_pipeline_maker.py:56-60
BOUNDARY_CFG = {"model_parameter": {"input_feat": 6, "stride": [1, 1], "nsample": [36, 24], "blocks": [2, 3], "block_num": 2,
                                    "planes": [16, 32], "crop_sample_size": 3072}}      # inference_pipeline_maker.py:43-54
NET_N, NET_SEED, NET_SCAN_SEED = 1024, 61, 1661
NET_STRIDE = {"cls": (slice(None), slice(None), slice(0, None, 2)), "offset": (slice(None), slice(None), slice(0, None, 2)),
              "x1": (slice(0, None, 4),)}


def _open3d():
    o3d = _stub_open3d([])
    base = o3d.geometry.TriangleMesh

    class TriangleMesh(base):
        def remove_duplicated_vertices(self):
            v = np.asarray(self.vertices, dtype=np.float64)
            seen, keep, to = {}, [], np.empty(len(v), np.int64)
            for i, row in enumerate(map(tuple, v.tolist())):
                j = seen.get(row)
                if j is None:
                    j = seen[row] = len(keep)
                    keep.append(i)
                to[i] = j
            self.vertices, self.vertex_normals = v[keep], np.asarray(self.vertex_normals)[keep]
            self.triangles = to[np.asarray(self.triangles, dtype=np.int64)]
            return self

        def subdivide_midpoint(self, number_of_iterations=1):
            sub = subdivide_ref.subdivide_loop({"vertices": np.asarray(self.vertices), "triangles": np.asarray(self.triangles),
                                                "vertex_normals": np.asarray(self.vertex_normals)}, number_of_iterations)
            out = TriangleMesh()
            out.vertices, out.triangles, out.vertex_normals = sub["vertices"], sub["triangles"], sub["vertex_normals"]
            return out
    o3d.geometry = types.SimpleNamespace(TriangleMesh=TriangleMesh)
    return o3d


def _reference_modules():
    load_reference()
    sys.modules["open3d"] = _open3d()
    tri = types.ModuleType("trimesh")

    def load_mesh(path, process=False):
        v, f = OM.read_obj(path)
        return types.SimpleNamespace(vertices=v, faces=f - 1)
    tri.load_mesh = load_mesh
    sys.modules["trimesh"] = tri
    if REFERENCE not in sys.path:
        sys.path.append(REFERENCE)
    import gen_utils as gu
    import ops_utils as ou
    import inference_pipelines.inference_pipeline_tgn as IP
    assert all(m.__file__.startswith(REFERENCE) for m in (gu, ou, IP))
    memo = {}

    def fps(xyz, npoint):
        x = np.ascontiguousarray(np.asarray(xyz), dtype=np.float32)
        if x.shape[0] <= npoint:
            raise ValueError("new fps error")
        key = (hash(x.tobytes()), x.shape[0], npoint)
        if key not in memo:
            memo[key] = O.furthestsampling(x, [len(x)], [npoint]).reshape(-1)
        return memo[key]
    gu.fps = fps
    return gu, ou, IP


def kdtree_knn(xyz, centres, k):
    return torch.from_numpy(KDTree(xyz.numpy().astype(np.float64)).query(centres.numpy().astype(np.float64), k=k, return_distance=False))


def run_reference(IP, text, variant="full", seed=TC.PERM_SEED):
    """-> (result dict, locals of __call__, locals of get_boundary_sampled_feats)"""
    pipe = IP.InferencePipeLine.__new__(IP.InferencePipeLine)
    pipe.scaler, pipe.shifter, pipe.config = 1.8, 0.8, {"boundary_sampling_info": dict(INFO)}
    pipe.first_module, pipe.bdl_module = TC.stand_ins(kdtree_knn, variant)
    seen = {}
    codes = {IP.InferencePipeLine.__call__.__code__: "call", IP.InferencePipeLine.get_boundary_sampled_feats.__code__: "bd"}

    def profile(frame, event, arg):
        if event == "return" and frame.f_code in codes:
            seen[codes[frame.f_code]] = dict(frame.f_locals)
    with tempfile.TemporaryDirectory() as root:
        path = os.path.join(root, "scan.obj")
        with open(path, "w") as f:
            f.write(text)
        np.random.seed(seed)
        with cpu_as_cuda():
            sys.setprofile(profile)
            try:
                res = pipe(path)
            finally:
                sys.setprofile(None)
    return res, seen["call"], seen["bd"]


def pipeline_part(out, IP, seeds):
    texts = {name: synth.obj_text(nu, nv, seed, "plain", with_tail=False) for name, (nu, nv, seed) in TC.MESHES.items()}
    res, loc, bd = run_reference(IP, texts["main"])
    sem, ins = np.asarray(res["sem"]).reshape(-1), np.asarray(res["ins"]).reshape(-1)
    nu, nv, _ = TC.MESHES["main"]
    assert sem.shape[0] == nu * nv == ins.shape[0]
    vals, cnt = np.unique(sem, return_counts=True)
    print(f"  main: {sem.shape[0]} vertices, sem {dict(zip(vals.tolist(), cnt.tolist()))}, instances {np.unique(ins).tolist()}")
    assert set(vals.tolist()) == {0, 11, 12, 13, 14, 15, 16, 17, 21, 22, 23, 24, 25, 26, 27} and len(np.unique(ins)) == TC.TEETH + 1
    assert np.array_equal(sem == 0, ins == 0)
    for s in range(seeds):
        r, _, _ = run_reference(IP, texts["main"], seed=1000 + s)
        same = np.array_equal(np.asarray(r["sem"]).reshape(-1), sem) and np.array_equal(np.asarray(r["ins"]).reshape(-1), ins)
        assert same, f"np.random.seed({1000 + s}) gives other labels: the stand-ins must be tightened"
    print(f"  main: the same labels under {seeds} other np.random.seed values")
    out["pipe_main_sem"], out["pipe_main_ins"] = sem.astype(np.int8), ins.astype(np.int16)

    # what number_teeth reads and writes, per class table
    fr = loc["first_results"]
    first_xyz = fr["ins"]["full_ins_labeled_points"][:, :3]
    first_ins = fr["ins"]["full_ins_labeled_points"][:, 3].astype(np.int64)
    assert np.array_equal(first_xyz.astype(np.float32).astype(np.float64), first_xyz)
    out["first_xyz"], out["first_ins"] = first_xyz.astype(np.float32), first_ins.astype(np.int16)
    for variant in TC.VARIANTS:
        lv = loc if variant == "full" else run_reference(IP, texts["main"], variant)[1]
        assert np.array_equal(lv["first_results"]["ins"]["full_ins_labeled_points"][:, 3].astype(np.int64), first_ins)
        first_sem = lv["first_results"]["sem_1"]["full_labeled_points"][:, 3].astype(np.int64)
        new_sem, ins_after = np.asarray(lv["new_sem_labels"]), np.asarray(lv["first_ps_label"])
        zeroed = sorted(set(np.unique(first_ins).tolist()) - set(np.unique(ins_after).tolist()))
        took_fallback = int(np.sum(first_sem == 1) + np.sum(first_sem == 9)) <= 20
        print(f"  teeth[{variant}]: numbers {np.unique(new_sem).tolist()}, zeroed instances {zeroed}, fallback loop {took_fallback}")
        assert took_fallback == (variant == "fallback") and (len(zeroed) == 1) == (variant == "classless")
        out[f"teeth_{variant}_sem_in"], out[f"teeth_{variant}_sem"] = first_sem.astype(np.int8), new_sem.astype(np.int8)
        out[f"teeth_{variant}_ins"] = ins_after.astype(np.int16)

    # the pieces of the join (main mesh, full class table, np.random.seed(PERM_SEED))
    sums = fr["sem_2"]["whole_pd_mask"]
    assert np.array_equal(sums, np.round(sums)) and sums.max() < 100
    out["vote_sums"] = sums.astype(np.int8)
    flags, nearest = np.asarray(bd["bd_labels"]) == 1, np.asarray(bd["ps_labels"]).reshape(-1)
    rows_label = np.asarray(bd["results_label_cpu"]).reshape(-1)
    nb = bd["bd_org_feat_cpu"].shape[0]
    print(f"  boundary: {int(flags.sum())} of {flags.shape[0]} dense rows, {nb} kept, labels {np.unique(rows_label).astype(int).tolist()}")
    assert 0 < nb == int(flags.sum()) < INFO["num_of_bdl_points"]
    # no dense point whose 40th and 41st neighbours are equally far: the KDTree's answer is unique
    d, _ = KDTree(np.asarray(bd["xyz_cpu"]), leaf_size=40).query(np.asarray(bd["org_feats"])[:, :3], k=41)
    assert np.all(d[:, 40] > d[:, 39]) and np.all(d[:, 1] > d[:, 0]), "a distance tie at the k-th neighbour"
    out["bd_flags"], out["bd_nearest"] = np.packbits(flags), nearest.astype(np.int16)
    out["bd_rows_label"] = rows_label.astype(np.int16)
    out["bd_rows_xyz"] = np.asarray(bd["results_feat_cpu"])[::16, :3].astype(np.float64)
    out["bd_count"] = np.array([nb])
    out["merge_bdl_xyz"] = np.asarray(loc["bdl_xyz"]).astype(np.float32)
    assert np.array_equal(out["merge_bdl_xyz"].astype(np.float64), np.asarray(loc["bdl_xyz"]))
    # the second pass's cluster numbers are sklearn's (random); the partition is what every run shares: store it numbered by first appearance
    _, first_at, part = np.unique(np.asarray(loc["bdl_ps_label"]), return_index=True, return_inverse=True)
    out["merge_bdl_partition"] = np.argsort(np.argsort(first_at))[part.reshape(-1)].astype(np.int16)
    out["merge_bdl_background"] = np.asarray(loc["bdl_ps_label"]) == 0
    out["merge_ins"], out["merge_sem"] = np.asarray(loc["mod_bdl_ps_label"]).astype(np.int16), np.asarray(loc["mod_bdl_sem_label"]).astype(np.int8)

    # the subdivision path and the copy with duplicated vertices
    res, loc_s, _ = run_reference(IP, texts["small"])
    nu, nv, _ = TC.MESHES["small"]
    s_sem, s_ins = np.asarray(res["sem"]).reshape(-1), np.asarray(res["ins"]).reshape(-1)
    assert s_sem.shape[0] == nu * nv and loc_s["bdl_feats"].shape[0] > 24000 > nu * nv
    print(f"  small: {s_sem.shape[0]} vertices, {loc_s['bdl_feats'].shape[0]} after the subdivision, sem {np.unique(s_sem).tolist()}")
    out["pipe_small_sem"], out["pipe_small_ins"] = s_sem.astype(np.int8), s_ins.astype(np.int16)
    dup_text, pick = TC.obj_with_duplicates(texts["main"])
    res, _, _ = run_reference(IP, dup_text)
    d_sem, d_ins = np.asarray(res["sem"]).reshape(-1), np.asarray(res["ins"]).reshape(-1)
    assert np.array_equal(d_sem, sem) and np.array_equal(d_ins, ins), "duplicates appended behind the mesh change nothing for the reference"
    out["pipe_dup_rows"] = pick.astype(np.int32)
    print(f"  dup: {TC.N_DUPLICATES} duplicated vertices collapse, the reference labels the {d_sem.shape[0]} distinct ones as before")


def network_part(out):
    import models.modules.cbl_point_transformer.cbl_point_transformer_module as M
    import models.modules.cbl_point_transformer.blocks as RB
    from models.modules.grouping_network_module import GroupingNetworkModule
    RP = RB.pointops
    assert RP.__file__.startswith(REFERENCE), RP.__file__
    keep_cuda = torch.nn.Module.cuda
    torch.nn.Module.cuda = lambda self, *a, **k: self
    try:
        whole = GroupingNetworkModule(BOUNDARY_CFG)
    finally:
        torch.nn.Module.cuda = keep_cuda
    out["net_module_keys"] = np.array([f"{n}:{'x'.join(map(str, v.shape))}" for n, v in whole.state_dict().items()])
    mp = BOUNDARY_CFG["model_parameter"]
    net = M.get_model(c=6, k=10, planes=mp["planes"], stride=mp["stride"], nsample=mp["nsample"], blocks=mp["blocks"], block_num=2).eval()
    seeded_fill(net, NET_SEED)
    sd = {n: v.clone() for n, v in net.state_dict().items()}
    out["net_keys"] = np.array([f"{n}:{'x'.join(map(str, v.shape))}" for n, v in sd.items()])
    torch.save(sd, os.path.join(HERE, "tgnet_boundary_weights.pt"))
    scans = synth.scan_batch(2, NET_N, "arch", seed=NET_SCAN_SEED)
    keep = _serve_pointops(RP)
    try:
        for tag, rows in (("b1", scans[:1]), ("b2", scans)):
            feats = torch.from_numpy(np.ascontiguousarray(rows.transpose(0, 2, 1)))
            with torch.no_grad():
                with cpu_as_cuda(torch.FloatTensor):
                    y32 = net.float()([feats])
                with cpu_as_cuda(torch.DoubleTensor):
                    y64 = net.double()([feats.double()])
            for name, i in (("cls", 0), ("offset", 1), ("x1", 3)):
                if y32[i] is None:
                    continue
                print(f"  boundary net {tag} {name:7s} {tuple(y32[i].shape)}  |fp32 - fp64| / (1 + |fp64|) = {rel_err(y32[i].numpy(), y64[i].numpy()):.2e}")
                keep_rows = NET_STRIDE[name]                                     # strided, to keep the fixture small
                out[f"net_{tag}_{name}_32"], out[f"net_{tag}_{name}_64"] = y32[i].numpy()[keep_rows], y64[i].numpy()[keep_rows].astype(np.float32)
    finally:
        RP.furthestsampling, RP.knnquery = keep
    out["net_scan"] = np.array([NET_N, NET_SCAN_SEED])
    size = os.path.getsize(os.path.join(HERE, "tgnet_boundary_weights.pt"))
    print(f"  wrote tests/golden/tgnet_boundary_weights.pt ({size / 1e6:.2f} MB, {len(sd)} tensors)")


def main():
    torch.set_num_threads(8)
    seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out = {}
    gu, ou, IP = _reference_modules()
    network_part(out)
    pipeline_part(out, IP, seeds)
    path = os.path.join(HERE, "reference_cpu_r16_tgnet.npz")
    np.savez_compressed(path, **out)
    print(f"wrote tests/golden/reference_cpu_r16_tgnet.npz ({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
