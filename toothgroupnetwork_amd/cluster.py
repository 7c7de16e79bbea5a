"""On-device clustering: the step of tgnet_fps's unlabelled path that turns the first network's moved foreground points into teeth
(ops_utils.get_clustering_labels, called from models/modules/grouping_network_module.py:57-69).  The reference runs sklearn on the
host; here the per-point work is HIP (csrc/cluster.hip, include/tgn_pointops.h):

  dbscan                 sklearn's DBSCAN(eps, min_samples).fit(X): equal labels and core flags
  mean_shift             sklearn's MeanShift(bandwidth) with its defaults: equal labels_; cluster_centers_ equal to rounding (sklearn
                         sums each seed's neighbours in its KDTree's order, the kernel in ascending point order)
  get_clustering_labels  ops_utils.get_clustering_labels step by step (the noise vote's kNN is crop.hip's, through crops.crop_knn)
  cluster_centroids      the float32 mean of every cluster's points (crop.hip's label means, through crops.label_centroids)

sklearn picks a brute-force neighbour search (the expanded distance formula) for fewer than 12 points; the kernels always use the
KDTree's rdist, so results on such tiny inputs can differ where a pair lies within rounding of the radius.
"""
import numpy as np
import torch

from . import _lib, crops as _crops

DBSCAN_EPS, DBSCAN_MIN_SAMPLES = 0.03, 30     # ops_utils.py:96
SPLIT_RATIO, SPLIT_BANDWIDTH = 8, 0.07        # ops_utils.py:127, :132
VOTE_K = 10                                   # ops_utils.py:136
MAX_ITER = 300                                # MeanShift's default


def _points(points, what, dtype):
    if not isinstance(points, torch.Tensor):
        raise TypeError(f"{what}: points must be a torch tensor, got {type(points).__name__}")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{what}: points must be (N, 3), got {tuple(points.shape)}")
    if points.dtype != dtype:
        raise TypeError(f"{what}: points must be {dtype}, got {points.dtype}")
    if points.shape[0] < 1:
        raise ValueError(f"{what}: no points")
    return points.detach().contiguous()


def _offsets(offset, n):
    if offset is None:
        return [n]
    off = [int(v) for v in (offset.tolist() if isinstance(offset, torch.Tensor) else offset)]
    if not off or any(o < 1 for o in np.diff([0] + off)) or off[-1] != n:
        raise ValueError(f"offset must be strictly increasing cumulative cloud ends ending at N = {n}, got {off}")
    return off


def dbscan(points, eps, min_samples, offset=None):
    """points (N, 3) float32 on the GPU; offset: pointops-style cumulative cloud ends (a list or tensor, last = N) for a ragged batch,
    None for one cloud.  -> (labels (N,) int64, core (N,) bool), device tensors, sklearn's DBSCAN(eps, min_samples).fit on each cloud
    (labels numbered per cloud from 0, noise -1).  No host synchronisation (the per-cloud counts: dbscan_counts)."""
    return dbscan_counts(points, eps, min_samples, offset)[:2]


def dbscan_counts(points, eps, min_samples, offset=None):
    """dbscan plus the per-cloud cluster counts (B,) int32 as a third device tensor."""
    eps, min_samples = float(eps), int(min_samples)
    if not eps > 0 or not np.isfinite(eps):
        raise ValueError(f"eps must be a positive finite number, got {eps}")
    if min_samples < 1:
        raise ValueError(f"min_samples must be >= 1, got {min_samples}")
    pts = _points(points, "dbscan", torch.float32)
    _lib.require_cuda(pts)
    n = pts.shape[0]
    off = _offsets(offset, n)
    L, dev, st = _lib.ops(), pts.device, _lib.stream()
    b = len(off)
    off_t = torch.tensor(off, dtype=torch.int32).to(dev, non_blocking=True)
    labels = torch.empty(n, dtype=torch.int64, device=dev)
    core = torch.empty(n, dtype=torch.uint8, device=dev)
    counts = torch.empty(b, dtype=torch.int32, device=dev)
    wsb = L.tgn_dbscan_workspace_bytes(b, n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    L.tgn_dbscan(b, n, pts, off_t, eps, min_samples, labels, core, counts, ws, wsb, st)
    return labels, core.bool(), counts


def _mean_shift_seeds(pts, bandwidth, max_iter):
    L, dev = _lib.ops(), pts.device
    n = pts.shape[0]
    means = torch.empty(n, 3, dtype=torch.float64, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    L.tgn_mean_shift(n, pts, bandwidth, max_iter, means, counts, _lib.stream())
    return means, counts


def _rdist(a, b):
    d = a - b
    return ((0.0 + d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _post_process(means, counts, bandwidth):
    """MeanShift.fit's host part (sklearn/cluster/_mean_shift.py) on the seeds' results: the dict keyed by the exact mean, the sort by
    (intensity, centre) descending, the suppression of centres within the bandwidth of a stronger one."""
    intensity = {}
    for m, c in zip(map(tuple, means.tolist()), counts.tolist()):
        if c:
            intensity[m] = c
    ranked = sorted(intensity.items(), key=lambda tup: (tup[1], tup[0]), reverse=True)
    centers = np.array([tup[0] for tup in ranked], np.float64).reshape(-1, 3)
    unique = np.ones(len(centers), dtype=bool)
    r2 = bandwidth * bandwidth
    for i in range(len(centers)):
        if unique[i]:
            unique[_rdist(centers, centers[i]) <= r2] = False
            unique[i] = True
    return centers[unique]


def mean_shift(points, bandwidth, max_iter=MAX_ITER):
    """points (N, 3) float64 on the GPU -> (labels (N,) int64 device tensor, centers (K, 3) float64 device tensor): sklearn's
    MeanShift(bandwidth).fit(points) with bin_seeding=False, cluster_all=True -- labels_ equal, cluster_centers_ equal to rounding
    (module docstring).  ONE host synchronisation: reading the N seed means and counts for the de-duplication."""
    bandwidth = float(bandwidth)
    if not bandwidth > 0 or not np.isfinite(bandwidth):
        raise ValueError(f"bandwidth must be a positive finite number, got {bandwidth}")
    if int(max_iter) < 0:
        raise ValueError(f"max_iter must be >= 0, got {max_iter}")
    pts = _points(points, "mean_shift", torch.float64)
    _lib.require_cuda(pts)
    means, counts = _mean_shift_seeds(pts, bandwidth, int(max_iter))
    centers = _post_process(means.cpu().numpy(), counts.cpu().numpy(), bandwidth)            # the one synchronisation
    cent = torch.from_numpy(centers).to(pts.device)
    labels = torch.empty(pts.shape[0], dtype=torch.int64, device=pts.device)
    _lib.ops().tgn_nearest_center(pts.shape[0], pts, cent.shape[0], cent, labels, _lib.stream())
    return labels, cent


def _eigen_first(counts, cov):
    """PCA(3).fit(core points).explained_variance_[0] per cluster (ops_utils.get_eg_values): the largest eigenvalue of the ddof = 1
    covariance, 0 for fewer than 3 points."""
    first = np.zeros(len(counts))
    for i, (c, m) in enumerate(zip(counts, cov)):
        if c >= 3:
            first[i] = max(np.linalg.eigvalsh(m)[-1], 0.0)
    return first


def split_candidates(first):
    """ops_utils.py:122-128 on the clusters' first eigenvalues: the clusters, among the three largest, whose value exceeds 8x the
    mean of all but the three largest -- in that order.  Fewer than 3 clusters: none (the reference raises IndexError)."""
    if len(first) < 3:
        return []
    order = np.argsort(-first)
    top = first[order]
    with np.errstate(divide="ignore", invalid="ignore"):
        rest = top[3:].mean() if len(top) > 3 else np.float64(np.nan)      # three clusters: the mean of nothing is NaN, no split
        return [int(order[i]) for i in range(3) if top[i] / rest > SPLIT_RATIO]


def get_clustering_labels(moved_points, labels):
    """ops_utils.get_clustering_labels (ops_utils.py:86-144): moved_points (N, 3), labels (N,) or (N, 1) class per point, 0 =
    gingiva; numpy arrays or GPU tensors -> the cluster label of every foreground point (labels != 0) in point order, (M,) int64 of the
    same kind as moved_points.  The coordinates are taken as float32 (the network's moved points are; the reference's float64 copies
    of them hold the same values).  Steps:
      1. DBSCAN(0.03, 30) on the foreground points (tgn_dbscan);
      2. per cluster the largest eigenvalue of its core points' covariance (PCA(3).explained_variance_[0]; tgn_cluster_moments);
      3. among the three largest, a cluster above 8x the mean of the others is re-split with MeanShift(0.07) over all its points,
         labelled ms_label + 100 * (position in that list + 1);
      4. every noise point takes the most frequent label among its 10 nearest labelled points (ascending (rdist, index), crops.crop_knn),
         equal counts to the smallest label (tgn_cluster_vote).
    Host synchronisations: 3, plus 2 per re-split cluster -- the foreground compaction, the cluster count, the moments, per split its
    point compaction and its seed means, and the noise compaction.
    Where the reference crashes, this raises or picks one behaviour: no cluster at all -> ValueError (the reference: IndexError);
    fewer than 3 clusters -> no split test (the reference: IndexError); fewer than 10 labelled points -> ValueError (as KDTree.query).
    """
    as_numpy = not isinstance(moved_points, torch.Tensor)
    if as_numpy:
        dev = torch.device("cuda", torch.cuda.current_device())
        moved = torch.from_numpy(np.ascontiguousarray(np.asarray(moved_points), dtype=np.float32)).to(dev)
        lab = torch.from_numpy(np.asarray(labels).reshape(-1).astype(np.int64)).to(dev)
    else:
        _lib.require_cuda(moved_points, labels if isinstance(labels, torch.Tensor) else None)
        dev = moved_points.device
        moved = moved_points.detach().to(torch.float32)
        lab = torch.as_tensor(labels, device=dev).reshape(-1)
    if moved.dim() != 2 or moved.shape[1] != 3:
        raise ValueError(f"moved_points must be (N, 3), got {tuple(moved.shape)}")
    if lab.shape[0] != moved.shape[0]:
        raise ValueError(f"labels must hold one class per point ({moved.shape[0]}), got {lab.shape[0]}")
    pts = moved[lab != 0].contiguous()                                                        # sync 1
    if pts.shape[0] == 0:
        raise ValueError("get_clustering_labels: no foreground point (every label is 0); the reference's DBSCAN raises here too")
    L, st = _lib.ops(), _lib.stream()
    dl, core, ncl = dbscan_counts(pts, DBSCAN_EPS, DBSCAN_MIN_SAMPLES)
    K = int(ncl.item())                                                                       # sync 2
    if K == 0:
        raise ValueError("get_clustering_labels: DBSCAN found no cluster (the reference raises IndexError here)")
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    mean = torch.empty(K, 3, dtype=torch.float64, device=dev)
    cov = torch.empty(K, 3, 3, dtype=torch.float64, device=dev)
    core8 = core.to(torch.uint8)
    L.tgn_cluster_moments(pts.shape[0], pts, dl, core8, K, counts, mean, cov, st)
    first = _eigen_first(counts.cpu().numpy(), cov.cpu().numpy())                             # sync 3
    out = dl.clone()
    for i, c in enumerate(split_candidates(first)):
        sel = dl == c
        ms_labels, _ = mean_shift(pts[sel].to(torch.float64), SPLIT_BANDWIDTH)                # syncs: the compaction, the seed means
        out[sel] = ms_labels + 100 * (i + 1)
    noise = out == -1
    cand = ~noise
    cand_pts = pts[cand]                                                                      # last sync
    m = cand_pts.shape[0]
    if m < VOTE_K:
        raise ValueError(f"get_clustering_labels: {m} labelled points, fewer than the {VOTE_K} the noise vote needs "
                         "(the reference's KDTree.query raises here too)")
    q = pts[noise].contiguous()
    if q.shape[0]:
        scan = torch.zeros(q.shape[0], dtype=torch.int32, device=dev)                         # one cloud: the labelled points
        idx = _crops.crop_knn(cand_pts.t().contiguous()[None], scan, q, VOTE_K)
        cand_labels = out[cand].contiguous()
        vote = torch.empty(q.shape[0], dtype=torch.int64, device=dev)
        L.tgn_cluster_vote(q.shape[0], VOTE_K, idx, m, cand_labels, vote, st)
        out[noise] = vote
    return out.cpu().numpy() if as_numpy else out


def cluster_centroids(moved_fg, cluster_labels):
    """grouping_network_module.py:66-68: the mean of the moved foreground points (M, 3) float32 of every final label, in ascending
    label order -> (T, 3) float32, bit-equal to numpy's float32 mean(axis=0) (crops.label_centroids on the dense-ranked labels).
    ONE host synchronisation (the number of labels).  More than 64 clusters: ValueError."""
    uniq, rank = torch.unique(cluster_labels, sorted=True, return_inverse=True)
    T = int(uniq.shape[0])
    if T > _crops.MAX_CLUSTERS:
        raise ValueError(f"{T} clusters: at most {_crops.MAX_CLUSTERS} tooth centroids are supported (tgn_label_centroids)")
    feats = moved_fg.to(torch.float32).t().contiguous()[None]
    _, cent = _crops.label_centroids(feats, rank.to(torch.int64).contiguous()[None], T)
    return cent[0]
