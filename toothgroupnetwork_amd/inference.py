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
stage, and the subdivided vertices with their interpolated normals are what is sampled (`dense_rows`).  One iteration is all the
pipelines use.  Parity with open3d is unpinned: the vertex order is restated from open3d's source, and neither open3d nor trimesh is
available where the fixtures are made.  A mesh that still has no more than 24 000 points after the pass is NotImplementedError: the
reference fails on it too (gen_utils.py:136-137).

TSegNetInferencePipeLine is the same for tsegnet (inference_pipelines/inference_pipeline_tsegnet.py): the centroid module, the join and
the painting on the GPU (tsegnet.py), pinned against the reference's class in the same way (tests/golden/make_golden_r11_tsegnet.py).

TgnInferencePipeLine is tgnet's (inference_pipelines/inference_pipeline_tgn.py): two GroupingNetworkModules with the boundary-aware
resampling between them (tgnet.py), pinned in the same way (tests/golden/make_golden_r16_tgnet.py).  make_inference_pipeline is the
reference's factory (inference_pipelines/inference_pipeline_maker.py) with its six model names.

Each of the three classes states its stages once, as methods (_StagedPipeLine), and `__call__` composes them.  infer_paths runs many scans
through any of them on one engine, run_staged, which puts the same stage methods on loader, sampler and finisher threads around the
calling thread: the semantic pipelines with `batch` scans per network call, the two-stage ones with one (measured:
profiles/r18_inference.txt, profiles/inference_one_engine_before_after.txt)."""
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


def fdi_from_classes(cls):
    """classes 0..16 -> FDI-style numbers as the pipeline writes them (:32-34): 1..8 -> 11..18, 9..16 -> 21..28."""
    cls = np.array(cls, dtype=np.int64)
    cls[cls >= 9] += 2
    cls[cls > 0] += 10
    return cls


class _Laps:
    """Durations between marks: compute() of a pipeline marks the end of each of its parts; a part marked again adds up."""

    def __init__(self):
        self.durations, self.last = {}, time.perf_counter()

    @classmethod
    def given(cls, laps):
        """the caller's laps, or fresh ones for a caller that wants none"""
        return cls() if laps is None else laps

    def mark(self, name):
        now = time.perf_counter()
        self.durations[name], self.last = self.durations.get(name, 0.0) + now - self.last, now


def network_input(*rows):
    """(n, c) host rows of one scan each -> the networks' input: (scans, c, n) float32 on the GPU, contiguous"""
    return torch.from_numpy(np.stack([np.asarray(r, dtype=np.float32) for r in rows])).cuda().permute(0, 2, 1).contiguous()


class _StagedPipeLine:
    """What the three pipelines share: a scan goes through five stages, each a method, and `__call__` is their composition.
      load(path)                       host only: the reader (_mesh), the pipeline's normalisation (:21-22) and the decision whether the mesh
                                       is subdivided -> the scan: {"path", "org_feats" (n, 6), "triangles" (None unless it is), "to_kept"}
      dense_rows(scan)                 the rows that are sampled: the scan's own, or the once-subdivided mesh's (GPU)
      take_sample(dense, idx)          the 24 000 sampled rows, given the FPS indices of the dense rows
      compute(scan, dense, sampled)    the networks and what joins them -> what finish needs; the durations of its parts go into `laps`
      finish(scan, sampled, computed)  the label transfer onto every vertex (GPU), the FDI relabelling -> {"sem", "ins"}
    infer_paths runs the same methods over many scans, each stage on threads of its own, and computes through compute_many: the same
    stage for a list of scans, which a pipeline whose network takes several scans per call overrides.  No method keeps anything
    about a scan on the pipeline object besides `times`, which only `__call__` writes."""

    FPS_PREFIX = True       # leave the FPS-of-an-FPS-result certificate for the network's first level (resample.fps)

    def _mesh(self, path):
        """-> (vertices, vertex normals, triangles, to_kept or None)"""
        _, mesh = preprocess.read_txt_obj_ls(path, ret_mesh=True)
        return mesh["vertices"], mesh["vertex_normals"], mesh["triangles"], None

    def load(self, path):
        vertices, normals, triangles, to_kept = self._mesh(path)
        org_feats = np.concatenate([normalise_for_inference(vertices, self.scaler, self.shifter), normals], axis=1)
        small = needs_subdivision(org_feats.shape[0], int(np.asarray(triangles).shape[0]))
        return {"path": path, "org_feats": org_feats, "triangles": triangles if small else None, "to_kept": to_kept}

    def dense_rows(self, scan):
        return scan["org_feats"] if scan["triangles"] is None else subdivided_rows(scan["org_feats"], scan["triangles"])

    def take_sample(self, dense, idx):
        return dense[idx[:N_POINTS]]

    def compute_many(self, scans, dense, sampled, laps=None):
        return [self.compute(*one, laps) for one in zip(scans, dense, sampled)]

    def __call__(self, stl_path):
        t = [time.perf_counter()]
        scan = self.load(stl_path)
        t.append(time.perf_counter())
        dense = self.dense_rows(scan)
        idx = resample.fps(dense[:, :3], N_POINTS, prefix=self.FPS_PREFIX)         # gen_utils.resample_pcd(..., "fps")
        sampled_feats = self.take_sample(dense, idx)
        t.append(time.perf_counter())
        laps = _Laps()
        computed = self.compute(scan, dense, sampled_feats, laps)
        t.append(time.perf_counter())
        result = self.finish(scan, sampled_feats, computed)
        t.append(time.perf_counter())
        self.times = {"load": t[1] - t[0], "sample": t[2] - t[1], **laps.durations, "transfer": t[4] - t[3]}
        return result


class InferencePipeLine(_StagedPipeLine):
    """Same constructor and call as the reference class: pipeline(path) -> {"sem": labels per vertex, "ins": the same}.
    `model` maps [features (1, 6, 24000)] to a dict with "cls_pred" (the reference's model wrappers) or to a list whose first
    entry is the class logits (B, 17, N) (nets.PointTransformerSeg).  `times` holds the stage times of the last call."""

    def __init__(self, model):
        self.model = model
        self.scaler = 1.8
        self.shifter = 0.8
        self.times = {}

    def compute_many(self, scans, dense, sampled, laps=None):
        """ONE network call on (scans, 6, 24000) -> the (24000,) classes of every scan; `model` has to be batch-capable for more than one"""
        laps = _Laps.given(laps)
        with torch.no_grad():
            out = self.model([network_input(*sampled)])
            cls_pred = out["cls_pred"] if isinstance(out, dict) else out[0]
            cls_pred = cls_pred.argmax(dim=1).cpu().numpy()
        laps.mark("model")
        return list(cls_pred)

    def compute(self, scan, dense, sampled_feats, laps=None):
        return self.compute_many([scan], [dense], [sampled_feats], laps)[0]

    def finish(self, scan, sampled_feats, cls_pred):
        labels = fdi_from_classes(cls_pred)
        result = preprocess.transfer_labels(sampled_feats[:, :3], labels, scan["org_feats"][:, :3])
        return {"sem": result.reshape(-1), "ins": result.reshape(-1)}


class TSegNetInferencePipeLine(_StagedPipeLine):
    """inference_pipelines/inference_pipeline_tsegnet.py:9-80 on this package's operators: same constructor and call as the
    reference class, pipeline(path) -> {"sem": labels per vertex, "ins": the same}.  `model` is anything with `cent_module`,
    `seg_module` and `get_ddf` (nets.TSegNetModule, the reference's own class, or a stand-in): the centroid module on the 24 000
    sampled points, then tsegnet.py's join WITHOUT crop subsampling (every cluster centre is cropped, :37-56; the fused crop kernel
    writes the distance feature, so `get_ddf` is not called), the segmentation module on all crops, the painting loop (:60-66) as
    tsegnet.paint_labels, the FDI relabelling (:69-70) and the nearest-sample transfer onto every vertex (:72-74).
    `times` holds the stage times of the last call.  Meshes below 24 000 vertices: subdivided once, as in InferencePipeLine."""

    FPS_PREFIX = False

    def __init__(self, model):
        self.model = model
        self.scaler = 1.8
        self.shifter = 0.8
        self.times = {}

    def compute(self, scan, dense, sampled_feats, laps=None):
        laps = _Laps.given(laps)
        with torch.no_grad():
            inp = network_input(sampled_feats)
            l0_points, _, _, l3_xyz, offset_result, dist_result = self.model.cent_module(inp)
            torch.cuda.current_stream().synchronize()
            laps.mark("centroids")
            moved, counts = tsegnet.centroid_proposals(l3_xyz, offset_result, dist_result)
            centres = tsegnet.cluster_centers(moved, counts)
            cropped, nn_crop_indexes, _ = tsegnet.crop_features(inp, l0_points, centres, tsegnet.CROP_K)
            torch.cuda.current_stream().synchronize()
            laps.mark("join")
            _, _, pd_2, id_pred = self.model.seg_module(cropped)
            torch.cuda.current_stream().synchronize()
            laps.mark("segmentation")
            cls_pred = tsegnet.paint_labels(nn_crop_indexes, pd_2, id_pred, N_POINTS).reshape(-1).cpu().numpy()
        laps.mark("paint")
        return cls_pred

    finish = InferencePipeLine.finish


def first_occurrences(vertices):
    """vertices (n, 3) -> (keep (u,) int64 ascending, to_kept (n,) int64): the rows open3d's remove_duplicated_vertices keeps -- the
    first occurrence, in file order, of every distinct coordinate triple (exact equality of the three coordinates) -- and for every
    row the position in `keep` of the row that stands for it."""
    v = np.ascontiguousarray(np.asarray(vertices)[:, :3])
    _, first, inverse = np.unique(v, axis=0, return_index=True, return_inverse=True)
    keep = np.sort(first)
    return keep.astype(np.int64), np.searchsorted(keep, first[inverse.reshape(-1)]).astype(np.int64)


class TgnInferencePipeLine(_StagedPipeLine):
    """inference_pipelines/inference_pipeline_tgn.py:10-157 (the "tgnet" model) on this package's operators: pipeline(path) ->
    {"sem": FDI-style tooth number per vertex, "ins": instance per vertex}.  `first_module` and `bdl_module` are two
    nets.GroupingNetworkModule (five-stage over the 24 000 sampled points, two-stage over the boundary-aware resampling), the
    reference's own classes, or stand-ins with the same call and output dict.  Stages, with `times` holding their durations:
      load       the native reader; duplicated vertices collapse to their first occurrence (first_occurrences), as open3d's
                 remove_duplicated_vertices does, a kept vertex keeping its normal and the triangles re-indexed
      sample     the pipeline's normalisation, one midpoint subdivision below 24 000 vertices (dense_rows: those rows are then
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

    def _mesh(self, path):
        _, mesh = preprocess.read_txt_obj_ls(path, ret_mesh=True)
        keep, to_kept = first_occurrences(mesh["vertices"])
        return mesh["vertices"][keep], mesh["vertex_normals"][keep], to_kept[mesh["triangles"]], to_kept

    def compute(self, scan, bdl_feats, sampled_feats, laps=None):
        """(the only stage that draws from numpy's global generator: boundary_resample's permutation)"""
        laps = _Laps.given(laps)
        with torch.no_grad():
            inp = network_input(sampled_feats)
            first = tgnet.first_instances(inp, self.first_module([inp]))
            first = {k: v.cpu().numpy() for k, v in first.items()}
            laps.mark("first")
            feats, labels, only_bdl, _ = tgnet.boundary_resample(bdl_feats, sampled_feats, first["ins"], self.boundary_sampling_info)
            laps.mark("resample")
            inp = network_input(feats)
            lab = torch.from_numpy(tgnet.dense_rank_labels(labels)[None, None]).cuda()
            second = tgnet.second_instances(inp, lab, self.bdl_module([inp, lab], test=True))
            nb = only_bdl.shape[0]
            bdl_xyz, bdl_ins = second["xyz"][:nb].cpu().numpy(), second["ins"][:nb].cpu().numpy()
        laps.mark("boundary")
        sem, ins = tgnet.number_teeth(first["xyz"], first["ins"], first["sem"])
        points, ins, sem = tgnet.merge_boundary(first["xyz"], ins, sem, bdl_xyz, bdl_ins)
        laps.mark("merge")
        return points, ins, sem

    def finish(self, scan, sampled_feats, computed):
        points, ins, sem = computed
        nearest = preprocess.transfer_labels(points, np.arange(points.shape[0]), scan["org_feats"][:, :3])
        sem, ins = fdi_from_classes(sem[nearest]), ins[nearest]
        return {"sem": sem[scan["to_kept"]].reshape(-1), "ins": ins[scan["to_kept"]].reshape(-1)}


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
    """Many scans through the semantic pipeline around `model` (as for InferencePipeLine, batch-capable: nets.PointTransformerSeg is), the
    network on `batch` scans per call: infer_paths' staged run of an InferencePipeLine, under the name its callers know."""
    return infer_paths(InferencePipeLine(model), paths, batch, workers)


def default_workers():
    """Loader threads of a staged run: the host cores this rank may count on (sharding.cpus_for_this_rank: affinity mask and CPU quota,
    shared with the other ranks of the node), at most 16 -- the reader scales no further (profiles/r04_preprocess_host_scaling.txt)."""
    import os

    from . import sharding
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE") or os.environ.get("WORLD_SIZE") or 1)
    return max(1, min(16, sharding.cpus_for_this_rank(local_world)))


def _with_path(error, path):
    """the same kind of exception with the scan's path in front of its message"""
    try:
        named = type(error)(f"{path}: {error}")
    except Exception:  # noqa: BLE001  (a constructor that wants more than a message)
        named = RuntimeError(f"{path}: {type(error).__name__}: {error}")
    named.__cause__ = error
    return named


def _settle(results, i, path, error, on_error):
    named = _with_path(error, path)
    if on_error == "raise":
        raise named
    results[i] = {"error": f"{type(named).__name__}: {named}"}


def _one_each(stage, out, n):
    out = list(out)
    if len(out) != n:
        raise RuntimeError(f"the {stage} stage returned {len(out)} entries for {n} scans")
    return out


def run_staged(paths, load, prepare, sample, compute, finish, batch=8, workers=None, on_error="raise", on_thread=None, stats=None, group=1):
    """The engine of a staged run over many scans; the stages are the caller's:
      load(path) -> loaded                                    `workers` loader threads
      prepare(loaded) -> prepared                             the one sampler thread, scan by scan
      sample([prepared, ...]) -> [sampled, ...]               the sampler thread, ONE call per chunk of up to 4 x `batch` scans (the first: `batch`)
      compute([loaded, ...], [prepared, ...], [sampled, ...]) the CALLING thread, in the order of `paths`, ONE call per `group` scans: the
          -> [computed, ...]                                  scans of a chunk that got this far, taken `group` at a time (the last: the rest)
      finish(loaded, sampled, computed) -> result             up to four finisher threads
    -> the results in the order of `paths`.  on_thread(fn, *args) wraps what the sampler and the finishers run (infer_paths: a stream
    of the thread's own, synchronised before the result is handed on).  At most two chunks are in front of the calling thread, so a
    long list does not fill memory with loaded meshes.  A scan that fails in any stage raises its own exception with the path in
    front of the message (on_error="raise"), or leaves {"error": message} in its slot while the others go on ("skip"); a `sample`
    call that fails as a whole fails every scan of its chunk, a `compute` call every scan of its group (raised: the first of them).
    A chunk's failures before compute are settled before its groups are computed.  All pools have ended when this returns or raises.
    stats: a dict that receives the mean seconds per scan in "load", "sample", "compute", "finish"."""
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    if on_error not in ("raise", "skip"):
        raise ValueError(f"on_error is 'raise' or 'skip', not {on_error!r}")
    call = on_thread if on_thread is not None else (lambda fn, *a: fn(*a))
    paths = list(paths)
    # an FPS launch costs the same for 1 or 64 scans (one workgroup each), so a chunk is four batches -- but the first is one batch: the
    # calling thread has nothing to do until the first chunk is loaded and sampled
    step, group, n = max(int(batch), 1), max(int(group), 1), len(paths)
    edges = [0] + list(range(min(step, n), n, 4 * step)) + [n]
    chunks = [range(lo, hi) for lo, hi in zip(edges, edges[1:]) if hi > lo]
    results = [None] * len(paths)
    spent = {name: [] for name in ("load", "sample", "compute", "finish")}

    def timed(name, fn, *a):
        t0 = time.perf_counter()
        try:
            return fn(*a)
        finally:
            spent[name].append(time.perf_counter() - t0)

    def sample_chunk(loads):
        # (sampler thread) -> per scan (loaded, prepared, sampled), or the exception that stopped it
        got = []
        for f in loads:
            try:
                loaded = f.result()
                got.append((loaded, call(prepare, loaded)))
            except Exception as e:  # noqa: BLE001
                got.append(e)
        good = [g for g in got if not isinstance(g, Exception)]
        sampled = []
        if good:
            try:
                sampled = _one_each("sample", call(sample, [prepared for _, prepared in good]), len(good))
            except Exception as e:  # noqa: BLE001
                sampled = [e] * len(good)
        sampled = iter(sampled)
        out = []
        for g in got:
            s = g if isinstance(g, Exception) else next(sampled)
            out.append(s if isinstance(s, Exception) else (g[0], g[1], s))
        return out

    workers = default_workers() if workers is None else max(int(workers), 1)
    loaders = ThreadPoolExecutor(max_workers=workers, thread_name_prefix="tgn-load")
    sampler = ThreadPoolExecutor(max_workers=1, thread_name_prefix="tgn-sample")
    finishers = ThreadPoolExecutor(max_workers=4, thread_name_prefix="tgn-finish")

    def submit(c):
        return sampler.submit(timed, "sample", sample_chunk, [loaders.submit(timed, "load", load, paths[i]) for i in chunks[c]])

    pending = deque()

    def collect(wait):
        while pending and (wait or pending[0][1].done()):
            i, f = pending.popleft()
            try:
                results[i] = f.result()
            except Exception as e:  # noqa: BLE001
                _settle(results, i, paths[i], e, on_error)

    try:
        ahead = deque(submit(c) for c in range(min(2, len(chunks))))
        for c in range(len(chunks)):
            items = ahead.popleft().result()
            if c + 2 < len(chunks):
                ahead.append(submit(c + 2))
            good = []
            for i, item in zip(chunks[c], items):
                if isinstance(item, Exception):
                    _settle(results, i, paths[i], item, on_error)
                else:
                    good.append((i, *item))
            for g in range(0, len(good), group):
                members, loaded, prepared, sampled = map(list, zip(*good[g:g + group]))
                try:
                    computed = _one_each("compute", timed("compute", compute, loaded, prepared, sampled), len(members))
                except Exception as e:  # noqa: BLE001
                    for i in members:
                        _settle(results, i, paths[i], e, on_error)
                    continue
                for i, *one in zip(members, loaded, sampled, computed):
                    pending.append((i, finishers.submit(timed, "finish", call, finish, *one)))
                collect(False)
        collect(True)
    finally:
        for pool in (loaders, sampler, finishers):
            pool.shutdown(wait=True, cancel_futures=True)
    if stats is not None and paths:
        stats.update({name: sum(times) / len(paths) for name, times in spent.items()})
    return results


class _OwnStreams:
    """on_thread of a staged run on the GPU: every helper thread works on a stream of its own, on the calling thread's device, and the
    stream is synchronised before the result -- or the exception -- leaves the thread.  (The index-error word is per device and
    stream, so the checks of two threads do not cross.)"""

    def __init__(self):
        import threading
        self.local, self.device = threading.local(), torch.cuda.current_device()

    def __call__(self, fn, *a):
        with torch.cuda.device(self.device):
            st = getattr(self.local, "stream", None)
            if st is None:
                st = self.local.stream = torch.cuda.Stream()
            with torch.cuda.stream(st):
                try:
                    return fn(*a)
                finally:
                    st.synchronize()


def _one_by_one(pipeline, paths, on_error, stats):
    """[pipeline(p) for p in paths] with the staged run's error rules"""
    if on_error not in ("raise", "skip"):
        raise ValueError(f"on_error is 'raise' or 'skip', not {on_error!r}")
    results, sums = [None] * len(paths), {}
    for i, path in enumerate(paths):
        try:
            results[i] = pipeline(path)
        except Exception as e:  # noqa: BLE001
            _settle(results, i, path, e, on_error)
            continue
        for k, v in dict(getattr(pipeline, "times", None) or {}).items():
            sums[k] = sums.get(k, 0.0) + v
    if stats is not None and paths:
        stats.update({k: v / len(paths) for k, v in sums.items()})
    return results


# Whether the staged run of a two-stage pipeline is what infer_paths uses: decided by measurement (tools/inference_bench.py --model_name,
# profiles/r18_inference.txt), not by hope -- a name whose staged run is not faster than the loop by more than the spread of the
# repeats goes through the loop.
STAGED = {"tsegnet": True, "tgnet": True}


def infer_paths(pipeline, paths, batch=8, workers=None, on_error="raise", stats=None, staged=None):
    """Many scans through any pipeline -> the list of {"sem", "ins"} in the order of `paths`.
      the three pipeline classes   a staged run (run_staged) of the pipeline's own stage methods: loader threads; a sampler thread that
                                   subdivides small meshes and runs ONE resample.fps_batch launch per 4 x `batch` scans; compute_many on
                                   the calling thread, in the order of `paths`; the transfer on finisher threads
        InferencePipeLine            the network runs on `batch` scans per call (its compute_many)
        TSegNetInferencePipeLine,    ONE SCAN PER NETWORK CALL
        TgnInferencePipeLine
      anything else callable       [pipeline(p) for p in paths]
    The two-stage results equal pipeline(path) by construction, not by tolerance: the networks see the shapes the single-scan call
    gives them (the library GEMMs pick kernels by row count, and the 0.3 filter, the DBSCAN radius and the 0.7 boundary ratio turn
    last bits into other point sets), and only the calling thread draws from numpy's global generator, in path order -- after
    np.random.seed(s) the run equals [pipeline(p) for p in paths] after the same seed.  fps_batch leaves no prefix certificate; the
    certificate only short-cuts an identical result, so no label depends on it, and none left for a later scan can reach an earlier
    scan's network.
    workers: loader threads (default_workers()).  on_error: "raise" -- a failing scan raises its own exception with its path in front
    of the message; "skip" -- its slot holds {"error": message} and the others are answered (a network call that fails takes the
    scans of its call with it, no others).  stats receives mean seconds per scan and stage.  staged: overrides STAGED for a
    two-stage pipeline (the measurement's switch); InferencePipeLine is always staged."""
    paths = list(paths)
    if isinstance(pipeline, TgnInferencePipeLine):
        staged = STAGED["tgnet"] if staged is None else staged
    elif isinstance(pipeline, TSegNetInferencePipeLine):
        staged = STAGED["tsegnet"] if staged is None else staged
    else:
        staged = isinstance(pipeline, InferencePipeLine)
    if not staged:
        return _one_by_one(pipeline, paths, on_error, stats)
    laps_sum = {}

    def prepare(scan):
        dense = pipeline.dense_rows(scan)
        if dense.shape[0] <= N_POINTS:
            raise ValueError("new fps error")       # resample.fps's refusal, here: it fails this scan, not the chunk's launch
        return dense

    def sample(dense):
        return [pipeline.take_sample(d, idx) for d, idx in zip(dense, resample.fps_batch(dense, N_POINTS))]

    def compute(scans, dense, sampled):
        laps = _Laps()
        computed = pipeline.compute_many(scans, dense, sampled, laps)
        for k, v in laps.durations.items():
            laps_sum[k] = laps_sum.get(k, 0.0) + v
        return computed

    results = run_staged(paths, pipeline.load, prepare, sample, compute, pipeline.finish, batch=batch, workers=workers, on_error=on_error,
                         on_thread=_OwnStreams(), stats=stats, group=batch if isinstance(pipeline, InferencePipeLine) else 1)
    if stats is not None and paths:
        stats.update({k: v / len(paths) for k, v in laps_sum.items()})
    return results
