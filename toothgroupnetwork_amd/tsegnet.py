"""The join between the two stages of tsegnet (models/modules/tsegnet.py:57-81) and the painting loop of its inference pipeline
(inference_pipelines/inference_pipeline_tsegnet.py:60-66) on the GPU.  The reference does every step on the host -- numpy filters,
sklearn's DBSCAN, a KDTree over the whole scan, python gathers, a python loop over the crops -- with a device round trip at each;
here (csrc/tsegnet.hip; cluster.hip through cluster.py; crop.hip through crops.py's wrappers, operand builders and limits):

  centroid_proposals  (l3_xyz + offset)[dist < 0.3] in point order                      tgn_tsg_proposals
  cluster_centers     DBSCAN(0.05, 3) on them, the float32 mean of every cluster        cluster.dbscan_counts, crops.label_centroids
  crop_features       the k nearest scan points of every centre and the segmentation    crops.crop_knn, tgn_tsg_crop_features
                      module's 3 + Cf + 1 input channels (xyz, features, distance feature)
  paint_labels        every scan point takes the tooth id of the last crop that masks it   tgn_tsg_paint

Host synchronisations per forward: the two the data forces -- the kept counts (DBSCAN's ragged offsets are host integers) and the
cluster counts (T sizes every later tensor).  The reference copies l3_xyz + offset, dist and all of l0_xyz to the host and the
centres and indices back on the same stretch.
"""
import numpy as np
import torch

from . import _lib, cluster as _cluster, crops as _crops

THRESHOLD = 0.3                    # tsegnet.py:58
EPS, MIN_SAMPLES = 0.05, 3         # tsegnet.py:59
CROP_K = 3072                      # tsegnet.py:73
MAX_M = 1024                       # tgn_tsg_proposals: one workgroup per scan


class NoCentre(ValueError):
    """A scan without a tooth centre: no proposal below the threshold, or no cluster among the proposals (cluster_centers)."""


def _f32(t, what, shape_text, ok):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a torch tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {t.dtype}")
    if not ok(t):
        raise ValueError(f"{what} must be {shape_text}, got {tuple(t.shape)}")
    return t.detach().contiguous()


def centroid_proposals(l3_xyz, offset, dist, threshold=THRESHOLD):
    """l3_xyz, offset (B, 3, M) and dist (B, 1, M) float32 on the GPU (the centroid module's outputs), 1 <= M <= 1024 ->
    (moved (K, 3) float32 device tensor, counts: list of B ints, K = sum(counts)): per scan the points l3_xyz + offset (one float32
    addition per coordinate) whose dist < float32(threshold) -- the comparison numpy makes with the python 0.3; NaN is dropped -- in
    ascending point order, scan after scan (tsegnet.py:57-58 per scan).
    ONE host synchronisation: reading the B counts."""
    l3_xyz = _f32(l3_xyz, "l3_xyz", "(B, 3, M) with 1 <= M <= 1024", lambda t: t.dim() == 3 and t.shape[0] >= 1 and t.shape[1] == 3 and 1 <= t.shape[2] <= MAX_M)
    B, _, M = l3_xyz.shape
    offset = _f32(offset, "offset", f"({B}, 3, {M})", lambda t: tuple(t.shape) == (B, 3, M))
    dist = _f32(dist, "dist", f"({B}, 1, {M})", lambda t: tuple(t.shape) == (B, 1, M))
    threshold = float(threshold)
    if np.isnan(threshold):
        raise ValueError("threshold must not be NaN")
    _lib.require_cuda(l3_xyz, offset, dist)
    dev = l3_xyz.device
    moved = torch.empty(B * M, 3, dtype=torch.float32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.ops().tgn_tsg_proposals(B, M, l3_xyz, offset, dist, threshold, moved, counts, _lib.stream())
    counts = counts.cpu().tolist()                                                            # the synchronisation
    return moved[:sum(counts)], counts


def cluster_centers(moved, counts, eps=EPS, min_samples=MIN_SAMPLES):
    """moved (K, 3) float32 on the GPU and counts (B ints, sum K) from centroid_proposals -> list over scans of (T_b, 3) float32 device
    tensors: sklearn's DBSCAN(eps, min_samples) on every scan's points (one ragged launch, cluster.dbscan), noise dropped, and per
    cluster label ascending (np.unique's order) the float32 mean of its points, bit-equal to numpy's
    moved[labels == label].mean(axis=0) (tsegnet.py:59-66).
    ONE host synchronisation: reading the B cluster counts.  A scan without a cluster raises ValueError naming the scan (the
    reference dies there with an IndexError); more than 64 clusters in a scan: ValueError."""
    counts = [int(c) for c in counts]
    if not isinstance(moved, torch.Tensor):
        raise TypeError(f"moved must be a torch tensor, got {type(moved).__name__}")
    if moved.dim() != 2 or moved.shape[1] != 3 or moved.dtype != torch.float32:
        raise ValueError(f"moved must be (K, 3) float32, got {tuple(moved.shape)} {moved.dtype}")
    if not counts or any(c < 0 for c in counts) or sum(counts) != moved.shape[0]:
        raise ValueError(f"counts must be non-negative and sum to {moved.shape[0]} rows, got {counts}")
    for b, c in enumerate(counts):
        if c == 0:
            raise NoCentre(f"tsegnet: scan {b} has no centroid proposal with dist < threshold, so no cluster")
    _lib.require_cuda(moved)
    moved = moved.detach().contiguous()
    ends = np.cumsum(counts).tolist()
    labels, _, ncl = _cluster.dbscan_counts(moved, eps, min_samples, ends)
    ncl = ncl.cpu().tolist()                                                                  # the synchronisation
    for b, t in enumerate(ncl):
        if t == 0:
            raise NoCentre(f"tsegnet: DBSCAN found no cluster among the {counts[b]} proposals of scan {b}")
        if t > _crops.MAX_CLUSTERS:
            raise ValueError(f"tsegnet: {t} clusters in scan {b}: at most {_crops.MAX_CLUSTERS} are supported (tgn_label_centroids)")
    out, lo = [], 0
    for hi, t in zip(ends, ncl):                                  # one launch per scan
        pts = moved[lo:hi].t().contiguous()[None]                 # (1, 3, n_b) channel-first; noise (-1) is skipped by the kernel
        _, cent = _crops.label_centroids(pts, labels[None, lo:hi].contiguous(), t)
        out.append(cent[0])
        lo = hi
    return out


def crop_features(feats, l0_points, centres, k=CROP_K, labels=None):
    """feats (B, C >= 3, N) float32 with xyz in channels 0..2, l0_points (B, Cf, N) float32 (the centroid module's per-point features),
    centres: list over scans of (T_b, 3) float32 arrays or tensors, labels (B, N) or (B, 1, N) int64 or None ->
      cropped          (T, 3 + Cf + 1, k) float32, scan-major: xyz at the crop indices (NOT centred), l0_points at them, and
                       exp(-4 sqrt(square_distance(point, centre))) -- the reference's cat([cropped_input[:, :3], cropped_feature, ddf])
      nn_crop_indexes  list over scans of (T_b, k) int64 device tensors, KDTree.query order (ascending float64 squared distance)
      crop_labels      (T, 1, k) int64, labels at the crop indices unchanged; None without labels
    Under no_grad, or when l0_points does not require a gradient: tgn_crop_knn and ONE fused tgn_tsg_crop_features launch.  In a
    grad-enabled call where l0_points.requires_grad the feature channels are gathered by differentiable torch indexing instead (the
    reference's own autograd path: the segmentation loss reaches the centroid trunk through them) and concatenated with the kernel's xyz
    and distance channels.
    No host synchronisation (T comes from the centres' shapes); indices are the kernel's own, so the error word is not read."""
    for t in (feats, l0_points):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"feats and l0_points must be torch tensors, got {type(t).__name__}")
    if feats.dim() != 3 or feats.shape[1] < 3:
        raise ValueError(f"feats must be (B, C >= 3, N), got {tuple(feats.shape)}")
    B, C, N = feats.shape
    if l0_points.dim() != 3 or l0_points.shape[0] != B or l0_points.shape[2] != N:
        raise ValueError(f"l0_points must be ({B}, Cf, {N}), got {tuple(l0_points.shape)}")
    if feats.dtype != torch.float32 or l0_points.dtype != torch.float32:
        raise TypeError(f"feats and l0_points must be float32, got {feats.dtype} and {l0_points.dtype}")
    k = _crops.check_k(k, N)
    dev = feats.device
    lab = _crops.labels_2d(labels, B, N, (torch.int64,)) if labels is not None else None
    cent, scan, per_scan = _crops.stack_centres(centres, B, dev, "centres")
    _lib.require_cuda(feats, l0_points, lab)
    T = sum(per_scan)
    if T == 0:
        raise ValueError("crop_features: no centre in the batch")
    cent = cent.detach()                                          # the kernels read the centres; no gradient flows to them
    x = feats.detach().contiguous()
    differentiable = torch.is_grad_enabled() and l0_points.requires_grad
    f = l0_points.detach().contiguous()
    Cf = 0 if differentiable else int(f.shape[1])
    idx = _crops.crop_knn(x, scan, cent, k)
    out = torch.empty(T, 3 + Cf + 1, k, dtype=torch.float32, device=dev)
    crop_lab = torch.empty(T, 1, k, dtype=torch.int64, device=dev) if lab is not None else None
    _lib.ops().tgn_tsg_crop_features(B, N, C, Cf, T, k, x, f if Cf else None, scan, cent, idx, lab, out, crop_lab, _lib.stream())
    if differentiable:
        flat = (scan.to(torch.int64)[:, None] * N + idx).reshape(-1)                           # rows of the (B * N, Cf) features
        rows = l0_points.permute(0, 2, 1).reshape(B * N, -1).index_select(0, flat)
        out = torch.cat([out[:, :3], rows.view(T, k, -1).permute(0, 2, 1), out[:, 3:]], 1)
    return out, list(idx.split(per_scan)), crop_lab


def paint_labels(nn_crop_indexes, pd_2, id_pred, n_points):
    """nn_crop_indexes: list over scans of (T_b, k) int64 device tensors (crop_features), pd_2 (T, 1, k) or (T, k) float32 mask logits,
    id_pred (T, C) tooth-id logits, both scan-major over all crops -> (B, n_points) int64 class numbers (0 = gingiva): the loop of
    inference_pipeline_tsegnet.py:60-66 -- crop after crop, the points with sigmoid(pd_2) > 0.5 take id_pred.argmax(1) of the crop, so
    the last crop that masks a point wins.  The mask is the reference's, torch.sigmoid(pd_2) > 0.5 in float32, not pd_2 > 0:
    sigmoid(6e-8) rounds to 0.5 and is not painted.
    One host synchronisation: the stream's error word is read (an index outside [0, n_points) raises IndexError)."""
    if not isinstance(nn_crop_indexes, (list, tuple)) or not nn_crop_indexes:
        raise ValueError("nn_crop_indexes must be a non-empty list over scans of (T_b, k) int64 tensors")
    for t in list(nn_crop_indexes) + [pd_2, id_pred]:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"paint_labels takes torch tensors, got {type(t).__name__}")
    n_points = int(n_points)
    if n_points < 1:
        raise ValueError(f"n_points must be >= 1, got {n_points}")
    B = len(nn_crop_indexes)
    for i in nn_crop_indexes:
        if i.dim() != 2 or i.dtype != torch.int64 or i.shape[1] != nn_crop_indexes[0].shape[1]:
            raise ValueError(f"nn_crop_indexes: every scan's crop indices must be (T_b, k) int64 with one k, got {tuple(i.shape)} {i.dtype}")
    per_scan = [int(i.shape[0]) for i in nn_crop_indexes]
    T, k = sum(per_scan), int(nn_crop_indexes[0].shape[1])
    if pd_2.dim() == 3 and pd_2.shape[1] == 1:
        pd_2 = pd_2[:, 0]
    if tuple(pd_2.shape) != (T, k) or pd_2.dtype != torch.float32:
        raise ValueError(f"pd_2 must be ({T}, 1, {k}) or ({T}, {k}) float32, got {tuple(pd_2.shape)} {pd_2.dtype}")
    if id_pred.dim() != 2 or id_pred.shape[0] != T or id_pred.shape[1] < 1:
        raise ValueError(f"id_pred must be ({T}, C), got {tuple(id_pred.shape)}")
    _lib.require_cuda(pd_2, id_pred, *nn_crop_indexes)
    dev = pd_2.device
    idx = torch.cat(list(nn_crop_indexes)).contiguous()
    mask = (torch.sigmoid(pd_2.detach()) > 0.5).to(torch.uint8).contiguous()
    ids = id_pred.detach().argmax(dim=1).to(torch.int64).contiguous()
    scan = _crops.scan_ids(per_scan, dev)
    out = torch.empty(B, n_points, dtype=torch.int64, device=dev)
    L, st = _lib.ops(), _lib.stream()
    L.tgn_clear_index_error(st)
    L.tgn_tsg_paint(B, n_points, T, k, scan, idx, mask, ids, out, st)
    if L.tgn_take_index_error(st) & _lib.INDEX_ERROR_CROP:
        raise IndexError(f"paint_labels: a crop index outside [0, {n_points})")
    return out
