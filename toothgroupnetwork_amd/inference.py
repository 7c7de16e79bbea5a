"""The semantic inference pipeline around the network (inference_pipelines/inference_pipeline_sem.py:8-60), end to end on this
package's operators: OBJ -> vertices + normals (native reader), the pipeline's own normalisation (:21-22), farthest-point sampling
to 24 000 points (:28, "#TODO slow processing speed" there), the model, the FDI relabelling (:32-34) and the nearest-sample label
transfer back onto every vertex (:37-39).

The sampled points reach the model in FPS order, and the Point-Transformer network's first transition-down level samples them
AGAIN (24 000 -> 6000): farthest-point sampling of an FPS sequence is the identity, so with the certificate the first launch leaves
behind (`resample.fps(prefix=True)`) that level costs the GPU a comparison instead of its 4.8 ms chain.  (On the wall clock of ONE
eager call nothing changes -- 11.2 against 11.5 ms for the model stage, `profiles/r03_inference_pipeline.txt`: the forward of a
single scan is bound by the host enqueuing its ~350 launches; the saving is the GPU's, for whatever shares it.)

Pinned against the reference's own class executed on CPU (tests/golden/make_golden_r3_pipeline.py: loader, FPS and .cuda() served,
everything else the reference's code): the same label on every vertex.
Meshes with fewer than 24 000 vertices are subdivided once at their edge midpoints first, as the reference does with open3d's
subdivide_midpoint(number_of_iterations=1) (:25-26): on the GPU (preprocess.subdivide_midpoint, csrc/subdivide.hip), inside the "sample"
stage, and the subdivided vertices with their interpolated normals are what is sampled (`points_to_sample`).  One iteration is all the
pipelines use.  Parity with open3d is unpinned: the vertex order is restated from open3d's source, and neither open3d nor trimesh is
available where the fixtures are made.  A mesh that still has no more than 24 000 points after the pass is NotImplementedError: the
reference fails on it too (gen_utils.py:136-137).

TSegNetInferencePipeLine is the same for tsegnet (inference_pipelines/inference_pipeline_tsegnet.py): the centroid module, the join and
the painting on the GPU (tsegnet.py), pinned against the reference's class in the same way (tests/golden/make_golden_r11_tsegnet.py).

TgnInferencePipeLine is tgnet's (inference_pipelines/inference_pipeline_tgn.py): two GroupingNetworkModules with the boundary-aware
resampling between them (tgnet.py), pinned in the same way (tests/golden/make_golden_r16_tgnet.py).  make_inference_pipeline is the
reference's factory (inference_pipelines/inference_pipeline_maker.py) with its six model names."""
import time

import numpy as np
import torch

from . import preprocess, resample, tgnet, tsegnet

N_POINTS = 24000


def normalise_for_inference(vertices, scaler=1.8, shifter=0.8):
    """inference_pipeline_sem.py:21-22: centre, then map the mesh's OWN y range to [-shifter, scaler - shifter] on every axis."""
    v = np.array(vertices, dtype=np.float64)
    v[:, :3] -= np.mean(v[:, :3], axis=0)
    lo, hi = np.min(v[:, 1]), np.max(v[:, 1])
    v[:, :3] = ((v[:, :3] - lo) / (hi - lo)) * scaler - shifter
    return v


_TOO_SMALL = ("a mesh that still has no more than 24 000 points after one midpoint subdivision cannot be sampled to 24 000: the reference "
              "fails on such a mesh too (gen_utils.py:136-137)")


def needs_subdivision(nv, nf):
    """True for a mesh below 24 000 vertices, which the reference's three pipelines subdivide once (inference_pipeline_sem.py:25-28,
    inference_pipeline_tsegnet.py:26-27, inference_pipeline_tgn.py:35-37).  A pass adds at most 3 nf vertices: where nv + 3 nf cannot
    exceed 24 000 the reference fails in gen_utils.fps afterwards, and this raises NotImplementedError before any launch."""
    if nv >= N_POINTS:
        return False
    if nv + 3 * nf <= N_POINTS:
        raise NotImplementedError(_TOO_SMALL)
    return True


def subdivided_rows(org_feats, triangles):
    """(nv, 6) normalised vertices + normals of a small mesh -> the (nv + edges, 6) rows of the mesh subdivided once on the GPU: old
    rows first, then every edge midpoint with the mean of its end points' normals (preprocess.subdivide_midpoint)."""
    sub = preprocess.subdivide_midpoint({"vertices": org_feats[:, :3], "triangles": triangles, "vertex_normals": org_feats[:, 3:6]}, 1)
    if sub["vertices"].shape[0] <= N_POINTS:
        raise NotImplementedError(_TOO_SMALL)
    return np.concatenate([sub["vertices"], sub["vertex_normals"]], axis=1)


def points_to_sample(org_feats, triangles):
    """The rows the pipelines sample 24 000 points from: the mesh's own (org_feats, which stays what the labels are transferred back
    onto) or, below 24 000 vertices, the subdivided mesh's."""
    if needs_subdivision(org_feats.shape[0], int(np.asarray(triangles).shape[0])):
        return subdivided_rows(org_feats, triangles)
    return org_feats


def fdi_from_classes(cls):
    """classes 0..16 -> FDI-style numbers as the pipeline writes them (:32-34): 1..8 -> 11..18, 9..16 -> 21..28."""
    cls = np.array(cls, dtype=np.int64)
    cls[cls >= 9] += 2
    cls[cls > 0] += 10
    return cls


class InferencePipeLine:
    """Same constructor and call as the reference class: pipeline(path) -> {"sem": labels per vertex, "ins": the same}.
    `model` maps [features (1, 6, 24000)] to a dict with "cls_pred" (the reference's model wrappers) or to a list whose first
    entry is the class logits (B, 17, N) (nets.PointTransformerSeg).  `times` holds the stage times of the last call."""

    def __init__(self, model):
        self.model = model
        self.scaler = 1.8
        self.shifter = 0.8
        self.times = {}

    def __call__(self, stl_path):
        t = [time.perf_counter()]
        feats, mesh = preprocess.read_txt_obj_ls(stl_path, ret_mesh=True)
        t.append(time.perf_counter())
        vertices = normalise_for_inference(mesh["vertices"], self.scaler, self.shifter)
        org_feats = np.concatenate([vertices, mesh["vertex_normals"]], axis=1)
        dense = points_to_sample(org_feats, mesh["triangles"])
        idx = resample.fps(dense[:, :3], N_POINTS, prefix=True)                   # gen_utils.resample_pcd(..., "fps")
        sampled_feats = dense[idx[:N_POINTS]]
        t.append(time.perf_counter())
        with torch.no_grad():
            inp = torch.from_numpy(np.ascontiguousarray(sampled_feats.astype("float32"))[None]).cuda().permute(0, 2, 1)
            out = self.model([inp])
            cls_pred = out["cls_pred"] if isinstance(out, dict) else out[0]
            cls_pred = cls_pred.argmax(dim=1).reshape(-1).cpu().numpy()
        t.append(time.perf_counter())
        labels = fdi_from_classes(cls_pred)
        result = preprocess.transfer_labels(sampled_feats[:, :3], labels, org_feats[:, :3])
        t.append(time.perf_counter())
        self.times = dict(zip(("load", "sample", "model", "transfer"), np.diff(t).tolist()))
        return {"sem": result.reshape(-1), "ins": result.reshape(-1)}


class TSegNetInferencePipeLine:
    """inference_pipelines/inference_pipeline_tsegnet.py:9-80 on this package's operators: same constructor and call as the
    reference class, pipeline(path) -> {"sem": labels per vertex, "ins": the same}.  `model` is anything with `cent_module`,
    `seg_module` and `get_ddf` (nets.TSegNetModule, the reference's own class, or a stand-in): the centroid module on the 24 000
    sampled points, then tsegnet.py's join WITHOUT crop subsampling (every cluster centre is cropped, :37-56; the fused crop kernel
    writes the distance feature, so `get_ddf` is not called), the segmentation module on all crops, the painting loop (:60-66) as
    tsegnet.paint_labels, the FDI relabelling (:69-70) and the nearest-sample transfer onto every vertex (:72-74).
    `times` holds the stage times of the last call.  Meshes below 24 000 vertices: subdivided once, as in InferencePipeLine."""

    def __init__(self, model):
        self.model = model
        self.scaler = 1.8
        self.shifter = 0.8
        self.times = {}

    def __call__(self, stl_path):
        t = [time.perf_counter()]
        feats, mesh = preprocess.read_txt_obj_ls(stl_path, ret_mesh=True)
        t.append(time.perf_counter())
        vertices = normalise_for_inference(mesh["vertices"], self.scaler, self.shifter)
        org_feats = np.concatenate([vertices, mesh["vertex_normals"]], axis=1)
        dense = points_to_sample(org_feats, mesh["triangles"])
        idx = resample.fps(dense[:, :3], N_POINTS)                                 # gen_utils.resample_pcd(..., "fps")
        sampled_feats = dense[idx[:N_POINTS]]
        t.append(time.perf_counter())
        with torch.no_grad():
            inp = torch.from_numpy(np.ascontiguousarray(sampled_feats.astype("float32"))[None]).cuda().permute(0, 2, 1).contiguous()
            l0_points, _, _, l3_xyz, offset_result, dist_result = self.model.cent_module(inp)
            torch.cuda.current_stream().synchronize()
            t.append(time.perf_counter())
            moved, counts = tsegnet.centroid_proposals(l3_xyz, offset_result, dist_result)
            centres = tsegnet.cluster_centers(moved, counts)
            cropped, nn_crop_indexes, _ = tsegnet.crop_features(inp, l0_points, centres, tsegnet.CROP_K)
            torch.cuda.current_stream().synchronize()
            t.append(time.perf_counter())
            _, _, pd_2, id_pred = self.model.seg_module(cropped)
            torch.cuda.current_stream().synchronize()
            t.append(time.perf_counter())
            cls_pred = tsegnet.paint_labels(nn_crop_indexes, pd_2, id_pred, N_POINTS).reshape(-1).cpu().numpy()
        t.append(time.perf_counter())
        labels = fdi_from_classes(cls_pred)
        result = preprocess.transfer_labels(sampled_feats[:, :3], labels, org_feats[:, :3])
        t.append(time.perf_counter())
        self.times = dict(zip(("load", "sample", "centroids", "join", "segmentation", "paint", "transfer"), np.diff(t).tolist()))
        return {"sem": result.reshape(-1), "ins": result.reshape(-1)}


def first_occurrences(vertices):
    """vertices (n, 3) -> (keep (u,) int64 ascending, to_kept (n,) int64): the rows open3d's remove_duplicated_vertices keeps -- the
    first occurrence, in file order, of every distinct coordinate triple (exact equality of the three coordinates) -- and for every
    row the position in `keep` of the row that stands for it."""
    v = np.ascontiguousarray(np.asarray(vertices)[:, :3])
    _, first, inverse = np.unique(v, axis=0, return_index=True, return_inverse=True)
    keep = np.sort(first)
    return keep.astype(np.int64), np.searchsorted(keep, first[inverse.reshape(-1)]).astype(np.int64)


class TgnInferencePipeLine:
    """inference_pipelines/inference_pipeline_tgn.py:10-157 (the "tgnet" model) on this package's operators: pipeline(path) ->
    {"sem": FDI-style tooth number per vertex, "ins": instance per vertex}.  `first_module` and `bdl_module` are two
    nets.GroupingNetworkModule (five-stage over the 24 000 sampled points, two-stage over the boundary-aware resampling), the
    reference's own classes, or stand-ins with the same call and output dict.  Stages, with `times` holding their durations:
      load       the native reader; duplicated vertices collapse to their first occurrence (first_occurrences), as open3d's
                 remove_duplicated_vertices does, a kept vertex keeping its normal and the triangles re-indexed
      sample     the pipeline's normalisation, one midpoint subdivision below 24 000 vertices (points_to_sample: those rows are then
                 also what the boundary pass resamples, :35-39), FPS to 24 000
      first      the first module without labels, tgnet.first_instances
      resample   tgnet.boundary_resample: boundary rows by np.random.permutation of numpy's GLOBAL generator, the rest by FPS
      boundary   the boundary module called as bdl_module([feats, labels - 1], test=True) -- the labels ranked densely first
                 (tgnet.dense_rank_labels) -- and tgnet.second_instances
      merge      tgnet.number_teeth, tgnet.merge_boundary
      transfer   the nearest of the 24 000 + boundary points per vertex (preprocess.transfer_labels), the FDI relabelling of `sem` only

    Deviations from the reference, all deliberate: k-means starts from the first-pass instances' means instead of k-means++ seeds
    drawn from numpy's global generator (tgnet.py); EVERY vertex of the file gets a label, a duplicate its first occurrence's (the
    reference returns labels for the de-duplicated vertices only, which results.process cannot write; identical where a file has no
    duplicates); the native reader keeps file order where the reference loads through trimesh, which "can change vertex order"
    (gen_utils.py:202).  Parity with open3d's subdivision and normals is unpinned as for the other pipelines.  A vertex equally near
    two of the 24 000 + boundary points takes the one with the lower index (the first pass's); the KDTree leaves that open.  Where the
    reference dies by accident -- no foreground, fewer than three instances -- tgnet.py raises ValueError saying which; more than 64
    first-pass instances are a ValueError too (crops.MAX_CLUSTERS)."""

    STAGES = ("load", "sample", "first", "resample", "boundary", "merge", "transfer")

    def __init__(self, first_module, bdl_module, boundary_sampling_info=None):
        self.first_module = first_module
        self.bdl_module = bdl_module
        self.boundary_sampling_info = dict(tgnet.DEFAULT_INFO if boundary_sampling_info is None else boundary_sampling_info)
        self.scaler = 1.8
        self.shifter = 0.8
        self.times = {}

    @classmethod
    def from_config(cls, config):
        """The reference's constructor (:11-22): config["fps_model_info"] and config["boundary_model_info"] each hold a
        "model_parameter" dict for GroupingNetworkModule and a "load_ckpt_path"; config["boundary_sampling_info"] is the resampling's."""
        from . import nets
        modules = []
        for key in ("fps_model_info", "boundary_model_info"):
            module = nets.GroupingNetworkModule(config[key])
            module.cuda()
            module.load_state_dict(torch.load(config[key]["load_ckpt_path"]))
            modules.append(module.eval())
        return cls(modules[0], modules[1], config.get("boundary_sampling_info"))

    def __call__(self, stl_path):
        t = [time.perf_counter()]
        _, mesh = preprocess.read_txt_obj_ls(stl_path, ret_mesh=True)
        keep, to_kept = first_occurrences(mesh["vertices"])
        triangles = to_kept[mesh["triangles"]]
        t.append(time.perf_counter())
        vertices = normalise_for_inference(mesh["vertices"][keep], self.scaler, self.shifter)
        org_feats = np.concatenate([vertices, mesh["vertex_normals"][keep]], axis=1)
        bdl_feats = points_to_sample(org_feats, triangles)
        idx = resample.fps(bdl_feats[:, :3], N_POINTS, prefix=True)
        sampled_feats = bdl_feats[idx[:N_POINTS]]
        t.append(time.perf_counter())
        with torch.no_grad():
            inp = torch.from_numpy(np.ascontiguousarray(sampled_feats.astype("float32"))[None]).cuda().permute(0, 2, 1).contiguous()
            first = tgnet.first_instances(inp, self.first_module([inp]))
            first = {k: v.cpu().numpy() for k, v in first.items()}
            t.append(time.perf_counter())
            feats, labels, only_bdl, _ = tgnet.boundary_resample(bdl_feats, sampled_feats, first["ins"], self.boundary_sampling_info)
            t.append(time.perf_counter())
            inp = torch.from_numpy(np.ascontiguousarray(feats.astype("float32"))[None]).cuda().permute(0, 2, 1).contiguous()
            lab = torch.from_numpy(tgnet.dense_rank_labels(labels)[None, None]).cuda()
            second = tgnet.second_instances(inp, lab, self.bdl_module([inp, lab], test=True))
            nb = only_bdl.shape[0]
            bdl_xyz, bdl_ins = second["xyz"][:nb].cpu().numpy(), second["ins"][:nb].cpu().numpy()
        t.append(time.perf_counter())
        sem, ins = tgnet.number_teeth(first["xyz"], first["ins"], first["sem"])
        points, ins, sem = tgnet.merge_boundary(first["xyz"], ins, sem, bdl_xyz, bdl_ins)
        t.append(time.perf_counter())
        nearest = preprocess.transfer_labels(points, np.arange(points.shape[0]), org_feats[:, :3])
        sem, ins = fdi_from_classes(sem[nearest]), ins[nearest]
        t.append(time.perf_counter())
        self.times = dict(zip(self.STAGES, np.diff(t).tolist()))
        return {"sem": sem[to_kept].reshape(-1), "ins": ins[to_kept].reshape(-1)}


_FIVE_STAGE = {"input_feat": 6, "stride": [1, 4, 4, 4, 4], "nstride": [2, 2, 2, 2], "nsample": [36, 24, 24, 24, 24], "blocks": [2, 3, 4, 6, 3],
               "block_num": 5, "planes": [32, 64, 128, 256, 512], "crop_sample_size": 3072}
_BOUNDARY = {"input_feat": 6, "stride": [1, 1], "nsample": [36, 24], "blocks": [2, 3], "block_num": 2, "planes": [16, 32],
             "crop_sample_size": 3072}
MODEL_NAMES = ("tsegnet", "tgnet", "pointnet", "pointnetpp", "dgcnn", "pointtransformer")


def inference_config(model_name, ckpt_path_ls=(None, None)):
    """The configuration dict inference_pipeline_maker.py:3-104 builds for a model name ({} for the three models it gives none)."""
    if model_name == "tsegnet":
        return {"model_info": {"model_parameter": dict(_FIVE_STAGE)}, "run_tooth_segmentation_module": True}
    if model_name == "tgnet":
        return {"fps_model_info": {"model_parameter": dict(_FIVE_STAGE), "load_ckpt_path": ckpt_path_ls[0]},
                "boundary_model_info": {"model_parameter": dict(_BOUNDARY), "load_ckpt_path": ckpt_path_ls[1]},
                "boundary_sampling_info": dict(tgnet.DEFAULT_INFO)}
    if model_name == "pointtransformer":
        return {"model_info": {"model_parameter": dict(_FIVE_STAGE)}}
    if model_name in MODEL_NAMES:
        return {}
    raise ValueError(f"undefined model {model_name!r}: the names are {', '.join(MODEL_NAMES)}")


def make_inference_pipeline(model_name, ckpt_path_ls):
    """inference_pipelines/inference_pipeline_maker.py:3-106: the pipeline of one of the reference's six model names with its
    checkpoints loaded (ckpt_path_ls: one path, two for "tgnet": first module, boundary module), on the GPU, in eval mode.  The one
    place that says which module and which pipeline a name means.  Another name: ValueError (the reference raises a string)."""
    from . import nets
    config = inference_config(model_name, ckpt_path_ls)
    if model_name == "tgnet":
        return TgnInferencePipeLine.from_config(config)
    module, pipeline = {"tsegnet": (lambda: nets.TSegNetModule(config), TSegNetInferencePipeLine),
                        "pointnet": (lambda: nets.PointFirstModule({}), InferencePipeLine),
                        "pointnetpp": (lambda: nets.PointPpFirstModule({}), InferencePipeLine),
                        "dgcnn": (lambda: nets.DGCnnModule({}), InferencePipeLine),
                        "pointtransformer": (lambda: nets.PointTransformerModule(config["model_info"]), InferencePipeLine)}[model_name]
    module = module()
    module.load_state_dict(torch.load(ckpt_path_ls[0]))
    module.cuda()
    return pipeline(module.eval())


def infer_scans(paths, model, batch=8, workers=None):
    """Many scans through the same pipeline, MI355X-shaped: what InferencePipeLine does one scan at a time (58 ms each: 17 ms of
    parsing, 30 of sampling, 11 of an eager forward) as three overlapped stages -- loader threads (native reader + normals, no
    interpreter lock), a sampler thread that packs 4 x `batch` scans into ONE FPS launch on its own stream, and the calling thread, which
    runs the network on (batch, 6, 24000) and hands the label transfer to helper threads.  Same stage functions, same results per scan
    as InferencePipeLine (tests/test_gpu_whole_nets.py); returns the list of {"sem", "ins"} in the order of `paths`.
    A mesh below 24 000 vertices is subdivided once in the sampler stage, on that thread's stream (the loaders only decide that it
    needs it), and joins the same FPS launch (tests/test_gpu_subdivide.py).
    `model`: as for InferencePipeLine, batch-capable (nets.PointTransformerSeg is)."""
    import os
    import threading
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    step = max(int(batch), 1)
    if workers is None:
        workers = max(1, min(32, (os.cpu_count() or 1)))
    loaders = ThreadPoolExecutor(max_workers=workers)
    sampler = ThreadPoolExecutor(max_workers=1)
    finishers = ThreadPoolExecutor(max_workers=4)
    local = threading.local()

    def on_own_stream(fn, *a):
        st = getattr(local, "stream", None)
        if st is None:
            st = local.stream = torch.cuda.Stream()
        with torch.cuda.stream(st):
            out = fn(*a)
            st.synchronize()
        return out

    def load(path):
        feats, mesh = preprocess.read_txt_obj_ls(path, ret_mesh=True)
        org = np.concatenate([normalise_for_inference(mesh["vertices"]), mesh["vertex_normals"]], axis=1)
        if needs_subdivision(org.shape[0], mesh["triangles"].shape[0]):           # (host arithmetic only: the pass itself is the sampler's)
            return org, None, mesh["triangles"]
        return org, np.ascontiguousarray(org[:, :3], dtype=np.float32), None

    def sample(loaded):
        # (sampler thread) small meshes are subdivided here, on this thread's stream, then one FPS launch over the whole chunk
        dense = [org if tri is None else on_own_stream(subdivided_rows, org, tri) for org, _, tri in loaded]
        xyz = [x32 if tri is None else np.ascontiguousarray(d[:, :3], dtype=np.float32) for (_, x32, tri), d in zip(loaded, dense)]
        idx = on_own_stream(resample.fps_batch, xyz, N_POINTS)
        return [d[ix[:N_POINTS]] for d, ix in zip(dense, idx)]

    def finish(sampled, cls, org):
        return on_own_stream(preprocess.transfer_labels, sampled[:, :3], fdi_from_classes(cls), org[:, :3]).reshape(-1)

    # an FPS launch costs the same for 1 or 64 scans (one workgroup each): it takes four model batches at a time
    fstep = 4 * step
    chunks = [paths[s:s + fstep] for s in range(0, len(paths), fstep)]
    results, pending = [], deque()
    try:
        loads = [[loaders.submit(load, p) for p in chunk] for chunk in chunks]
        sampled_f = [sampler.submit(lambda fs=fs: (lambda loaded: (loaded, sample(loaded)))([f.result() for f in fs])) for fs in loads]
        for sf in sampled_f:
            loaded, sampled = sf.result()
            for b0 in range(0, len(sampled), step):
                part = sampled[b0:b0 + step]
                with torch.no_grad():
                    inp = torch.from_numpy(np.stack([s_.astype("float32") for s_ in part])).cuda().permute(0, 2, 1).contiguous()
                    out = model([inp])
                    cls_pred = (out["cls_pred"] if isinstance(out, dict) else out[0]).argmax(dim=1).cpu().numpy()  # (B, N)
                for (org, _, _), s_, c in zip(loaded[b0:b0 + step], part, cls_pred):
                    pending.append(finishers.submit(finish, s_, c, org))
        for f in pending:
            r = f.result()
            results.append({"sem": r, "ins": r})
    finally:
        for pool in (loaders, sampler, finishers):
            pool.shutdown(wait=True, cancel_futures=True)
    return results
