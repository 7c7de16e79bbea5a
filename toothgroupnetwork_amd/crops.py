"""On-device tooth crops: the step between the two stages of tgnet_fps's GroupingNetworkModule
(models/modules/grouping_network_module.py:45-72, labelled path).  The reference does it on the host -- numpy per-label means, an
sklearn KDTree queried for k points (ops_utils.get_nearest_neighbor_idx), fancy-index gathers (get_indexed_features) and a centring
loop (centering_object); here it is three HIP kernels (csrc/crop.hip, include/tgn_pointops.h):

  centroids   bit-equal to numpy's xyz[label == t].mean(axis=0) for every label t != -1 present in the scan, ascending (np.unique)
  crops       the k nearest points of each centroid in ascending float64 squared distance, equal distances by ascending index
              (KDTree leaves that order unspecified; the index set and the distance sequence are the same)
  centring    channels 0..2 minus their mean over the crop: a float64 sum rounded once to float32, subtracted in float32

Centroids from clustering (the unlabelled path: ops_utils.get_clustering_labels) come from cluster.py -- nets.GroupingNetworkModule
computes them there and passes them as `centroids`, as any caller that has centroids may; tooth_crops itself needs labels or
centroids.

This is also the one host layer over crop.hip for cluster.py (noise vote, cluster centroids) and tsegnet.py (cluster means, the join's
crops): the launches crop_knn and label_centroids, their operands (stack_centres, scan_ids, labels_2d), the limits MAX_K, MAX_CLUSTERS.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib

NUM_LABELS = 16          # tooth labels 0..15, -1 = gingiva (generator.py:46-47)
MAX_K = 4096             # ops_utils.get_nearest_neighbor_idx's default crop_num; tgn_crop_knn's limit
MAX_CLUSTERS = 64        # tgn_label_centroids' label limit

ToothCrops = namedtuple("ToothCrops", "cropped nn_crop_indexes cluster_gt_seg_label centroids")


def labels_2d(labels, B, N, dtypes):
    """(B, N) or (B, 1, N) labels of one of `dtypes` -> (B, N) int64 contiguous."""
    if not isinstance(labels, torch.Tensor) or labels.dtype not in dtypes:
        names = " or ".join(str(d).replace("torch.", "") for d in dtypes)
        raise TypeError(f"labels must be a torch tensor of {names}, got {getattr(labels, 'dtype', type(labels).__name__)}")
    if labels.dim() == 3 and labels.shape[1] == 1:
        labels = labels[:, 0]
    if tuple(labels.shape) != (B, N):
        raise ValueError(f"labels must be (B, N) or (B, 1, N) = ({B}, {N}), got {tuple(labels.shape)}")
    return labels.to(torch.int64).contiguous()


def scan_ids(per_scan, dev):
    """per_scan: the number of centres of every scan -> (T,) int32 on dev, the scan of every centre (scan-major)."""
    return torch.from_numpy(np.repeat(np.arange(len(per_scan), dtype=np.int32), per_scan)).to(dev, non_blocking=True)


def stack_centres(centres, B, dev, what):
    """centres: list or tuple over the B scans of (T_b, 3) arrays or tensors -> tgn_crop_knn's operands (cent (T, 3) float32
    contiguous on dev, scan (T,) int32 on dev, per_scan: list of the T_b).  `what` names the argument in the errors."""
    if not isinstance(centres, (list, tuple)) or len(centres) != B:
        raise ValueError(f"{what} must be a list of {B} per-scan (T_b, 3) arrays or tensors")
    parts = []
    for c in centres:
        c = c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(c), dtype=np.float32))
        if c.dim() != 2 or c.shape[1] != 3:
            raise ValueError(f"every scan's {what} must be (T_b, 3), got {tuple(c.shape)}")
        parts.append(c.to(dev, torch.float32))
    per_scan = [int(p.shape[0]) for p in parts]
    return torch.cat(parts).contiguous(), scan_ids(per_scan, dev), per_scan


def _operand(t, what, dtype):
    """crop_knn and label_centroids hand raw pointers to the kernels: their operands are `dtype` and contiguous, or it is an error."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise TypeError(f"{what} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous, got strides {tuple(t.stride())}")


def check_k(k, N):
    """k as an int within tgn_crop_knn's range for scans of N points; callers with GPU work ahead of crop_knn ask before that work."""
    k = int(k)
    if not 1 <= k <= min(N, MAX_K):
        raise ValueError(f"k = {k} must satisfy 1 <= k <= min(N, {MAX_K}) = {min(N, MAX_K)} (KDTree.query raises for k > N too)")
    return k


def crop_knn(feats, scan, cent, k):
    """feats (B, C >= 3, N) float32 contiguous with xyz in channels 0..2, scan (T,) int32 and cent (T, 3) float32 (stack_centres) ->
    idx (T, k) int64: per centre the k nearest points of its scan, ascending (float64 squared distance, index).  No synchronisation."""
    _operand(feats, "feats", torch.float32), _operand(scan, "scan", torch.int32), _operand(cent, "cent", torch.float32)
    B, C, N = feats.shape
    k = check_k(k, N)
    T = cent.shape[0]
    idx = torch.empty(T, k, dtype=torch.int64, device=feats.device)
    _lib.ops().tgn_crop_knn(B, N, C, feats, T, scan, cent, k, idx, _lib.stream())
    return idx


def label_centroids(feats, labels, nlab, f64_sum=False):
    """feats (B, C >= 3, N) float32 and labels (B, N) int64, contiguous -> (counts (B, nlab) int32, cent (B, nlab, 3) float32): per scan
    and label 0..nlab-1 its point count and float32 mean, bit-equal to numpy's xyz[label == t].mean(axis=0); with f64_sum the mean of a
    float64 sum rounded once (tgn_label_centroids_f64: the mean to half an ulp however many points a label has).  -1 is skipped; another
    label outside [0, nlab) latches _lib.INDEX_ERROR_CROP, which is neither cleared nor read here.  No synchronisation."""
    _operand(feats, "feats", torch.float32), _operand(labels, "labels", torch.int64)
    B, C, N = feats.shape
    counts = torch.empty(B, nlab, dtype=torch.int32, device=feats.device)
    cent = torch.empty(B, nlab, 3, dtype=torch.float32, device=feats.device)
    launch = _lib.ops().tgn_label_centroids_f64 if f64_sum else _lib.ops().tgn_label_centroids
    launch(B, N, C, feats, labels, nlab, counts, cent, _lib.stream())
    return counts, cent


def tooth_crops(feats, labels=None, centroids=None, k=3072, num_labels=NUM_LABELS):
    """feats (B, C, N) float32 with xyz in channels 0..2; labels (B, N) or (B, 1, N), int32 or int64, -1 = gingiva, teeth
    0..num_labels-1.  Returns ToothCrops:
      cropped               (T, C, k) float32, scan-major, teeth ascending: the reference's centred cropped_feature_ls
      nn_crop_indexes       list over scans of (T_b, k) int64 device tensors (the reference's list of KDTree results)
      cluster_gt_seg_label  (T, 1, k) int64, every label >= 0 set to 0 (gingiva stays -1); None without labels
      centroids             list over scans of (T_b, 3) float32 device tensors (the reference's cluster_centroids)
    `centroids` (a list over scans of (T_b, 3) arrays or tensors) replaces the label centroids, e.g. cluster centres.

    ONE host synchronisation, with labels and no centroids: reading the per-label point counts to learn T and which teeth are
    present -- the reference has to know that on the host as well (np.unique).  The label check behind it reads the stream's error
    word, which by then waits on nothing.  Raises ValueError for labels outside [-1, num_labels) and when no tooth is present."""
    _lib.require_cuda(feats, labels if isinstance(labels, torch.Tensor) else None)
    if labels is None and centroids is None:
        raise ValueError("tooth_crops needs labels or centroids: centroids from clustering (DBSCAN on the moved foreground points, "
                         "cluster.get_clustering_labels and cluster.cluster_centroids) are the caller's to compute, as "
                         "nets.GroupingNetworkModule does")
    if feats.dim() != 3 or feats.shape[1] < 3:
        raise ValueError(f"feats must be (B, C >= 3, N), got {tuple(feats.shape)}")
    if feats.dtype != torch.float32:
        raise TypeError(f"feats must be float32, got {feats.dtype}")
    feats = feats.detach().contiguous()
    B, C, N = feats.shape
    k = check_k(k, N)
    lab = labels_2d(labels, B, N, (torch.int32, torch.int64)) if labels is not None else None
    L, dev, st = _lib.ops(), feats.device, _lib.stream()
    if centroids is None:
        L.tgn_clear_index_error(st)
        counts, cent_all = label_centroids(feats, lab, num_labels)
        present = counts.cpu().numpy() > 0                                        # the one synchronisation
        if L.tgn_take_index_error(st) & _lib.INDEX_ERROR_CROP:
            raise ValueError(f"tooth_crops: a label outside [-1, {num_labels}) (gingiva -1, teeth 0..{num_labels - 1})")
        per_scan = present.sum(1).tolist()
        rows = torch.from_numpy(np.flatnonzero(present.reshape(-1))).to(dev, non_blocking=True)
        cent = cent_all.view(-1, 3).index_select(0, rows).contiguous()
        scan = scan_ids(per_scan, dev)
    else:
        flat = [(c if isinstance(c, torch.Tensor) else np.asarray(c, np.float32)).reshape(-1, 3) for c in centroids]
        cent, scan, per_scan = stack_centres(flat, B, dev, "centroids")
    T = int(sum(per_scan))
    if T == 0:
        raise ValueError("tooth_crops: no tooth in the batch (every point is gingiva, label -1)")
    idx = crop_knn(feats, scan, cent, k)
    cropped = torch.empty(T, C, k, dtype=torch.float32, device=dev)
    crop_lab = torch.empty(T, 1, k, dtype=torch.int64, device=dev) if lab is not None else None
    L.tgn_crop_gather_center(B, N, C, T, k, feats, scan, idx, lab, cropped, crop_lab, st)
    return ToothCrops(cropped, list(idx.split(per_scan)), crop_lab, list(cent.split(per_scan)))
