"""The second half of tgnet (inference_pipelines/inference_pipeline_tgn.py): what lies between the first GroupingNetworkModule's
outputs and a label on every vertex.  The reference runs each step on the host -- sklearn KDTrees, numpy votes, sklearn's KMeans --
with a device round trip between them; here every step is one of the library's existing kernels plus torch glue, no new entry point:

  crop_vote          the crop masks' logits summed back onto the scan, crop after crop (:186-195, :235-258)     torch, fp32 adds in order
  first_instances    class, mask, moved points and cluster.get_clustering_labels on the foreground (:159-216)   cluster.py's kernels
  boundary_flags     the 40 nearest sampled points of every dense point and the share that carry the nearest   pointops.knnquery (fp32
                     one's label (:289-304)                                                                     candidates), float64 re-rank
  boundary_resample  boundary rows by numpy's global permutation, the rest by FPS (:305-315)                    resample.fps
  kmeans             Lloyd's iteration from given centres                                                       tgn_nearest_center,
                                                                                                                tgn_cluster_moments
  second_instances   the boundary module's mask and moved points, k-means into len(unique(labels)) - 1 (:218-286)
  number_teeth       the tooth numbering from the first pass (:61-104)                                          host numpy, 24 000 rows
  merge_boundary     every second-pass cluster takes the first-pass instance most of its points lie nearest    preprocess.transfer_labels
                     to (:106-133)

Inputs are GPU tensors or numpy arrays, one scan at a time (the reference pipeline is B = 1); a function returns the kind its first
argument has, except number_teeth and merge_boundary's vote, which are host numpy throughout.  Functions that hand a tensor to the
library cast and pack it first (float32 / float64 / int64, contiguous, on the GPU) or raise naming the argument.

Deliberate deviations from the reference:
  * k-means seeding.  The reference seeds sklearn's k-means++ from numpy's global generator, so its second pass is not a function of its
    inputs.  Here the seeds are the means of the first-pass instances' moved points: a deterministic warm start.  What is merged
    afterwards depends on the partition only, not on the clusters' numbers.
  * Where the reference dies with an accident (a NameError, `raise "..."`, an IndexError), these raise ValueError saying which.
"""
import warnings

import numpy as np
import torch

from . import _lib, cluster as _cluster, pointops, preprocess, resample

BOUNDARY_K = 40            # inference_pipeline_tgn.py:295
EXTRA_CANDIDATES = 8       # fp32 candidates beyond k that the float64 re-rank chooses from (preprocess.transfer_labels takes 4 for k = 1)
MIN_CLASS_POINTS = 20      # :77, :81
DEFAULT_INFO = {"bdl_ratio": 0.7, "num_of_bdl_points": 20000, "num_of_all_points": 24000}   # inference_pipeline_maker.py:56-60


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _rows(x, what, dtype, width=3, dev=None):
    """x (n, >= width) array or tensor of a floating dtype -> (n, width) `dtype` contiguous on the GPU."""
    if isinstance(x, torch.Tensor):
        _lib.require_cuda(x)
        t = x.detach()
    else:
        t = torch.from_numpy(np.asarray(x))
    if t.dim() != 2 or t.shape[1] < width:
        raise ValueError(f"{what} must be (n, >= {width}), got {tuple(t.shape)}")
    if not t.is_floating_point():
        raise TypeError(f"{what} must be of a floating dtype, got {t.dtype}")
    return t[:, :width].to(dev or (t.device if t.is_cuda else _device()), dtype).contiguous()


def _labels(x, what, n, dev):
    """x: n labels, integers or integer-valued floats (the reference keeps its labels in float64 columns) -> (n,) int64 contiguous on dev."""
    t = x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
    if t.dtype == torch.bool or t.is_complex():
        raise TypeError(f"{what} must hold integer labels, got {t.dtype}")
    t = t.reshape(-1)
    if t.shape[0] != n:
        raise ValueError(f"{what} must hold one label per point ({n}), got {t.shape[0]}")
    return t.to(dev, torch.int64).contiguous()


def _argmax_first(x):
    """np.argmax over dim 0: the FIRST index of the maximum (torch.argmax does not promise which on equal values), a NaN counting as
    the maximum."""
    top = x.max(dim=0, keepdim=True).values
    hit = (x == top) | torch.isnan(x)
    rows = torch.arange(x.shape[0], device=x.device).view(-1, *([1] * (x.dim() - 1)))
    return torch.where(hit, rows, torch.full_like(rows, x.shape[0])).min(dim=0).values


def _rdist(a, b):
    """KDTree's euclidean rdist in float64, ((0 + dx dx) + dy dy) + dz dz, over the last axis."""
    d = a - b
    return ((0.0 + d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


# -----------------------------------------------------------------------------------------------------------------------------------
# the vote of the crop masks back onto the scan
# -----------------------------------------------------------------------------------------------------------------------------------
def crop_vote(sem_2, nn_crop_indexes, n):
    """sem_2 (T, 2, k) mask logits of the crops, nn_crop_indexes (T, k) point indices (or the module's list holding that one tensor),
    n points -> (mask (n,) int64, sums (n, 2) float32), device tensors: starting from zeros, every crop's (k, 2) logits are added at its
    indices, one crop at a time in ascending crop order (:188-192; the indices within a crop are distinct, so every step is one fp32
    addition per entry, in the reference's order), and mask = np.argmax over the two sums: 1 where sums[:, 1] > sums[:, 0] (or only
    channel 1 is NaN), else 0; a point in no crop keeps (0, 0) and gets 0.  sem_2 is taken as float32, the indices as int64."""
    if isinstance(nn_crop_indexes, (list, tuple)):
        if len(nn_crop_indexes) != 1:
            raise ValueError(f"nn_crop_indexes must hold the crops of ONE scan, got a list of {len(nn_crop_indexes)}")
        nn_crop_indexes = nn_crop_indexes[0]
    for t, what in ((sem_2, "sem_2"), (nn_crop_indexes, "nn_crop_indexes")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what} must be a torch tensor, got {type(t).__name__}")
    _lib.require_cuda(sem_2, nn_crop_indexes)
    if sem_2.dim() != 3 or sem_2.shape[1] != 2 or not sem_2.is_floating_point():
        raise ValueError(f"sem_2 must be (T, 2, k) of a floating dtype, got {tuple(sem_2.shape)} {sem_2.dtype}")
    T, _, k = sem_2.shape
    if tuple(nn_crop_indexes.shape) != (T, k) or nn_crop_indexes.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"nn_crop_indexes must be ({T}, {k}) int32 or int64, got {tuple(nn_crop_indexes.shape)} {nn_crop_indexes.dtype}")
    n = int(n)
    idx = nn_crop_indexes.detach().to(torch.int64)
    if T and k and (int(idx.min()) < 0 or int(idx.max()) >= n):
        raise IndexError(f"nn_crop_indexes: a crop index outside [0, {n})")
    logits = sem_2.detach().to(torch.float32).permute(0, 2, 1)                    # (T, k, 2)
    sums = torch.zeros(n, 2, dtype=torch.float32, device=sem_2.device)
    for t in range(T):
        sums[idx[t]] += logits[t]
    s0, s1 = sums[:, 0], sums[:, 1]
    mask = ((s1 > s0) | (torch.isnan(s1) & ~torch.isnan(s0))).to(torch.int64)
    return mask, sums


def _scan_outputs(feats, out):
    """The per-point pieces both passes take from a module's outputs: xyz (N, 3) float32, moved = xyz + offset_1 in float32 (the
    reference adds its float32 numpy copies, :202 / :265) and the crop_vote mask."""
    if not isinstance(feats, torch.Tensor) or feats.dim() != 3 or feats.shape[0] != 1 or feats.shape[1] < 3:
        raise ValueError(f"feats must be a (1, C >= 3, N) tensor (one scan), got {tuple(getattr(feats, 'shape', ()))}")
    offset = out["offset_1"]
    if offset is None or tuple(offset.shape) != (1, 3, feats.shape[2]):
        raise ValueError(f"out['offset_1'] must be (1, 3, {feats.shape[2]}): the offset head runs for one scan")
    xyz = feats[0, :3].detach().to(torch.float32).t().contiguous()
    moved = (xyz + offset[0].detach().to(torch.float32).t()).contiguous()
    mask, _ = crop_vote(out["sem_2"], out["nn_crop_indexes"], feats.shape[2])
    return xyz, moved, mask


def first_instances(feats, out):
    """feats (1, C, N) the first module's input, out its output dict -> dict of device tensors over the N points (:159-216):
      xyz (N, 3) float32, sem (N,) int64 = argmax of sem_1 (the first index on ties), mask (N,) int64 = crop_vote of sem_2,
      moved (N, 3) float32 = xyz + offset_1, ins (N,) int64 = 0 for background (mask == 0), else 1 + the label
      cluster.get_clustering_labels(moved, mask) gives the point."""
    xyz, moved, mask = _scan_outputs(feats, out)
    sem = _argmax_first(out["sem_1"][0].detach())
    fg = _cluster.get_clustering_labels(moved, mask)
    ins = torch.zeros(xyz.shape[0], dtype=torch.int64, device=xyz.device)
    ins[mask != 0] = fg + 1
    return {"xyz": xyz, "sem": sem, "mask": mask, "moved": moved, "ins": ins}


# -----------------------------------------------------------------------------------------------------------------------------------
# boundary-aware resampling
# -----------------------------------------------------------------------------------------------------------------------------------
def _knn64(points, queries, k):
    """points (n, 3), queries (m, 3) float64 device tensors -> (m, k) int64: per query its k nearest points in KDTree order, ascending
    (float64 rdist, index).  preprocess.transfer_labels' scheme: pointops.knnquery proposes min(k + EXTRA_CANDIDATES, n) candidates in
    fp32, they are re-ranked by their float64 distance.  The KDTree's answer unless fp32 rounding carries a point across more than
    EXTRA_CANDIDATES ranks, or more than that many points tie with the k-th in fp32."""
    n, m = points.shape[0], queries.shape[0]
    cand = min(k + EXTRA_CANDIDATES, n)
    dev = points.device
    o = torch.tensor([n], dtype=torch.int32, device=dev)
    n_o = torch.tensor([m], dtype=torch.int32, device=dev)
    idx, _ = pointops.knnquery(cand, points.float().contiguous(), queries.float().contiguous(), o, n_o)      # (m, cand) int32
    idx = idx.long().sort(dim=1).values                                                                      # equal distances: by index
    d = _rdist(points[idx.reshape(-1)].view(m, cand, 3), queries[:, None, :])
    order = d.sort(dim=1, stable=True).indices[:, :k]
    return idx.gather(1, order)


def boundary_flags(dense_xyz, sampled_xyz, point_labels, k=BOUNDARY_K, ratio=0.7):
    """dense_xyz (n, >= 3) and sampled_xyz (ns, >= 3) coordinates (taken as float64), point_labels: the ns sampled points' instance
    labels -> (boundary (n,) bool, nearest_label (n,) int64) (:289-304): per dense point its k nearest sampled points in KDTree order
    (ascending float64 distance, equal distances by index; _knn64), nearest_label = label[nn_0] and
        boundary = #{j < k : label[nn_j] == label[nn_0]} / k < ratio.
    The count is that of the NEAREST neighbour's label among the k, not of the most frequent label: gen_utils.count_unique_by_row
    writes every label's count at its first column, and column 0 is read.  Needs 1 <= k <= ns and k + 8 <= 128 (the kNN kernel)."""
    as_numpy = not isinstance(dense_xyz, torch.Tensor)
    dense = _rows(dense_xyz, "dense_xyz", torch.float64)
    dev = dense.device
    sampled = _rows(sampled_xyz, "sampled_xyz", torch.float64, dev=dev)
    ns = sampled.shape[0]
    labels = _labels(point_labels, "point_labels", ns, dev)
    k = int(k)
    if not 1 <= k <= min(ns, 128 - EXTRA_CANDIDATES):
        raise ValueError(f"k = {k} must satisfy 1 <= k <= min(number of sampled points = {ns}, {128 - EXTRA_CANDIDATES})")
    if dense.shape[0] == 0:
        boundary, nearest = torch.zeros(0, dtype=torch.bool, device=dev), torch.zeros(0, dtype=torch.int64, device=dev)
    else:
        lab = labels[_knn64(sampled, dense, k)]                                   # (n, k)
        nearest = lab[:, 0].contiguous()
        same = (lab == lab[:, :1]).sum(dim=1)
        boundary = same.to(torch.float64) / float(k) < float(ratio)
    if as_numpy:
        return boundary.cpu().numpy(), nearest.cpu().numpy()
    return boundary, nearest


def _take(a, rows):
    if isinstance(a, torch.Tensor):
        return a[torch.from_numpy(rows).to(a.device)]
    return np.asarray(a)[rows]


def boundary_resample(dense_feats, sampled_feats, point_labels, info=None, carry=()):
    """dense_feats (n, C >= 3) rows of the dense mesh, sampled_feats (ns, >= 3) the sampled points, point_labels their instance labels,
    info: {"bdl_ratio", "num_of_bdl_points", "num_of_all_points"} (DEFAULT_INFO) -> the reference's four values (:305-330)
      feats (num_of_all_points, C), labels (num_of_all_points, 1) int64, boundary_feats (nb, C), boundary_labels (nb, 1) int64
    where the labels are boundary_flags' nearest_label.  The boundary rows are taken in the order
    np.random.permutation(n_boundary)[:num_of_bdl_points] of numpy's GLOBAL generator (gen_utils.resample_pcd "uniformly"; the same
    np.random.seed gives the reference's rows), the other rows by FPS down to num_of_all_points - nb (resample.fps), boundary rows first.
    `carry`: further per-dense-row arrays taken through the same selection (the training path selects its ground-truth labels this
    way); with a non-empty carry a fifth value is returned, the list of the selected arrays.
    Raises ValueError when the non-boundary rows are too few for the FPS (it needs more rows than it returns; the reference raises a
    string there)."""
    info = dict(DEFAULT_INFO if info is None else info)
    n_bdl, n_all = int(info["num_of_bdl_points"]), int(info["num_of_all_points"])
    n = dense_feats.shape[0]
    for c in carry:
        if c.shape[0] != n:
            raise ValueError(f"carry: every array must have one row per dense row ({n}), got {c.shape[0]}")
    boundary, nearest = boundary_flags(dense_feats, sampled_feats, point_labels, BOUNDARY_K, info["bdl_ratio"])
    if isinstance(boundary, torch.Tensor):
        boundary, nearest_host = boundary.cpu().numpy(), nearest.cpu().numpy()
    else:
        nearest_host = nearest
    bd_rows, other_rows = np.flatnonzero(boundary), np.flatnonzero(~boundary)
    bd_rows = bd_rows[np.random.permutation(bd_rows.shape[0])[:n_bdl]]
    need = n_all - bd_rows.shape[0]
    if other_rows.shape[0] <= need:
        raise ValueError(f"boundary_resample: {other_rows.shape[0]} non-boundary points, FPS to {need} needs more than that "
                         f"({bd_rows.shape[0]} boundary points kept of {int(boundary.sum())})")
    fps_idx = resample.fps(_host(_take(dense_feats[:, :3], other_rows)), need)[:need]
    rows = np.concatenate([bd_rows, other_rows[fps_idx]])
    lab = nearest_host.astype(np.int64).reshape(-1, 1)
    if isinstance(dense_feats, torch.Tensor):
        lab = torch.from_numpy(lab).to(dense_feats.device)
    result = (_take(dense_feats, rows), _take(lab, rows), _take(dense_feats, bd_rows), _take(lab, bd_rows))
    if len(carry):
        result += ([_take(c, rows) for c in carry],)
    return result


# -----------------------------------------------------------------------------------------------------------------------------------
# k-means and the second pass
# -----------------------------------------------------------------------------------------------------------------------------------
def _label_means(pts32, labels, nlab):
    """(counts (nlab,) int32, mean (nlab, 3) float64) of pts32 (n, 3) float32 per label: tgn_cluster_moments."""
    dev = pts32.device
    counts = torch.empty(nlab, dtype=torch.int32, device=dev)
    mean = torch.empty(nlab, 3, dtype=torch.float64, device=dev)
    cov = torch.empty(nlab, 3, 3, dtype=torch.float64, device=dev)
    _lib.ops().tgn_cluster_moments(pts32.shape[0], pts32, labels, None, nlab, counts, mean, cov, _lib.stream())
    return counts, mean


def kmeans(points, init_centres, max_iter=300):
    """Lloyd's iteration on the device.  points (n, 3), taken as float32 (the moved points are); init_centres (m, 3), taken as float64
    -> (labels (n,) int64, centres (m, 3) float64), of the kind `points` has.
      assign   every point to its nearest centre by float64 rdist, equal distances to the lower centre (tgn_nearest_center)
      update   every centre to the float64 mean of its points (tgn_cluster_moments: per label, lane t of 256 sums the points
               t, t + 256, ... in order, a fixed tree adds the lanes, the sum is divided by the count); an empty cluster keeps its centre
    labels = assign(init); then up to max_iter times: update, assign again, stop when no assignment changed.  The returned labels are
    always the assignment to the returned centres (max_iter = 0: to init_centres).  One host synchronisation per iteration (the
    changed flag).  This is not sklearn's KMeans: no k-means++ seeding (module docstring), no tolerance on the centres' shift."""
    as_numpy = not isinstance(points, torch.Tensor)
    pts32 = _rows(points, "points", torch.float32)
    dev = pts32.device
    cent = _rows(init_centres, "init_centres", torch.float64, dev=dev)
    n, m = pts32.shape[0], cent.shape[0]
    if n < 1 or m < 1:
        raise ValueError(f"kmeans needs at least one point and one centre, got {n} points and {m} centres")
    max_iter = int(max_iter)
    if max_iter < 0:
        raise ValueError(f"max_iter must be >= 0, got {max_iter}")
    if not bool(torch.isfinite(cent).all()):
        raise ValueError("init_centres must be finite")
    L, st = _lib.ops(), _lib.stream()
    pts64 = pts32.to(torch.float64).contiguous()

    def assign(c):
        out = torch.empty(n, dtype=torch.int64, device=dev)
        L.tgn_nearest_center(n, pts64, m, c, out, st)
        return out
    labels = assign(cent)
    for _ in range(max_iter):
        counts, mean = _label_means(pts32, labels, m)
        cent = torch.where((counts > 0)[:, None], mean, cent).contiguous()
        new = assign(cent)
        changed = bool((new != labels).any())                                     # the synchronisation
        labels = new
        if not changed:
            break
    if as_numpy:
        return labels.cpu().numpy(), cent.cpu().numpy()
    return labels, cent


def second_instances(feats, labels, out):
    """feats (1, C, M) the boundary module's input, labels the (M,) instance labels it was given (background the smallest), out its
    output dict -> dict of device tensors over the M points (:218-286): xyz, mask, moved as first_instances, centres (k, 3) float64
    and ins (M,) int64 = 0 for background (mask == 0), else 1 + the k-means cluster of the moved point, with
      k = len(unique(labels)) - 1, exactly that arithmetic (:269), and
      initial centres = the float64 mean of the moved points of each distinct label other than the smallest, ascending (this
      package's deterministic seeding; the reference draws k-means++ seeds from numpy's global generator)."""
    xyz, moved, mask = _scan_outputs(feats, out)
    M = xyz.shape[0]
    lab = _labels(labels, "labels", M, xyz.device)
    uniq, rank = torch.unique(lab, sorted=True, return_inverse=True)
    k = int(uniq.shape[0]) - 1
    if k < 1:
        raise ValueError("second_instances: the labels hold one distinct value, so k = len(unique(labels)) - 1 = 0 clusters "
                         "(sklearn's KMeans raises there too)")
    _, means = _label_means(moved, rank.contiguous(), k + 1)
    fg = moved[mask != 0].contiguous()
    if fg.shape[0] == 0:
        raise ValueError("second_instances: no foreground point (the crop vote masks every point out)")
    fg_labels, centres = kmeans(fg, means[1:], max_iter=300)
    ins = torch.zeros(M, dtype=torch.int64, device=xyz.device)
    ins[mask != 0] = fg_labels + 1
    return {"xyz": xyz, "mask": mask, "moved": moved, "ins": ins, "centres": centres}


def dense_rank_labels(labels):
    """Instance labels minus one, as the boundary module takes them (-1 = background), ranked densely in ascending (np.unique) order:
    labels from clustering can exceed what crops.tooth_crops takes (MeanShift splits are numbered from 100), their order is what the
    reference's centroid list follows.  labels (n,) integer array, 0 = background -> (n,) int64 with -1 for background, teeth 0, 1, ..."""
    lab = np.asarray(labels).reshape(-1).astype(np.int64) - 1
    uniq, rank = np.unique(lab, return_inverse=True)
    rank = rank.reshape(-1).astype(np.int64)
    return rank - 1 if uniq.size and uniq[0] == -1 else rank


# -----------------------------------------------------------------------------------------------------------------------------------
# tooth numbering and the merge of the two passes (host)
# -----------------------------------------------------------------------------------------------------------------------------------
def _host(x):
    """array or tensor -> numpy, float64 for a floating dtype (numpy has no bfloat16) and int64 otherwise"""
    if isinstance(x, torch.Tensor):
        x = x.detach()
        return x.to(torch.float64 if x.is_floating_point() else torch.int64).cpu().numpy()
    x = np.asarray(x)
    return x.astype(np.float64 if np.issubdtype(x.dtype, np.floating) else np.int64)


def number_teeth(first_xyz, first_ins, first_sem):
    """first_xyz (N, 3), first_ins (N,) instance labels (0 = background), first_sem (N,) classes 0..9 of the first pass ->
    (sem (N,) int64 tooth numbers 0..16, ins (N,) int64: first_ins with the classless instances zeroed) (:61-104), on the host:
      the gingiva and teeth means; the instances' centres; the third principal axis of the centres (the right singular vector of the
      centred centres: sklearn's PCA components_[2] up to the sign that is fixed next) oriented by teeth_mean - gin_mean; the middle of
      the incisors -- the mean of the class 1 and class 9 means when those classes hold more than 20 points together, else the mean of
      the first class 2..8 with more than 20 points and the centres' mean; per instance the most frequent non-zero class, plus 8 when
      it is not 1 or 9 and the instance lies on the negative side of cross(axis, centre line); an instance without a non-zero class
      becomes background.
    ValueError where the reference dies by accident: fewer than three instances (PCA(3) refuses), no class with more than 20 points
    (a NameError there)."""
    xyz = _host(first_xyz).astype(np.float64)[:, :3]
    ins = _host(first_ins).reshape(-1).astype(np.int64).copy()
    sem_in = _host(first_sem).reshape(-1).astype(np.int64)
    gin_mean = np.mean(xyz[ins == 0], axis=0).reshape(1, 3)
    teeth_mean = np.mean(xyz[ins != 0], axis=0).reshape(1, 3)
    uniq = np.unique(ins)
    uniq = uniq[uniq != 0]
    if uniq.shape[0] < 3:
        raise ValueError(f"number_teeth: {uniq.shape[0]} instances, the principal axes need at least three (the reference's PCA(3) raises)")
    centres = np.array([np.mean(xyz[ins == label], axis=0) for label in uniq])
    axis = np.linalg.svd(centres - centres.mean(axis=0), full_matrices=False)[2][2]
    axis = axis if np.dot((teeth_mean - gin_mean).reshape(3), axis) > 0 else -axis
    if np.sum(sem_in == 1) + np.sum(sem_in == 9) > MIN_CLASS_POINTS:
        with np.errstate(invalid="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")                   # one of the two classes may be empty: a NaN middle, as in the reference
            middle = np.array(np.mean([np.mean(xyz[sem_in == 1], axis=0), np.mean(xyz[sem_in == 9], axis=0)], axis=0))
    else:
        for i in range(2, 9):
            if np.sum(sem_in == i) > MIN_CLASS_POINTS:
                middle = np.array(np.mean([np.mean(xyz[sem_in == i], axis=0), np.mean(centres, axis=0)], axis=0))
                break
        else:
            raise ValueError(f"number_teeth: no class 1..9 with more than {MIN_CLASS_POINTS} points, so the incisors' middle is undefined "
                             "(the reference: NameError)")
    centre_line = middle - np.mean(centres, axis=0)
    checking = np.cross(axis, centre_line)
    sem = np.zeros(ins.shape[0], dtype=np.int64)
    for label in uniq:
        sel = ins == label
        centre = xyz[sel].mean(axis=0)
        classes = sem_in[sel]
        classes = classes[classes != 0]
        if classes.shape[0] == 0:
            ins[sel] = 0
            continue
        best = int(np.argmax(np.bincount(classes)))
        if best not in (1, 9) and np.dot(centre - middle, checking) < 0:
            best += 8
        sem[sel] = best
    return sem, ins


def merge_boundary(first_xyz, first_ins, first_sem, bdl_xyz, bdl_ins):
    """first_xyz (N, 3), first_ins, first_sem (N,): the first pass after number_teeth; bdl_xyz (nb, 3), bdl_ins (nb,): the boundary
    points and their second-pass instances -> (points (N + nb, 3) float64, ins, sem (N + nb,) int64), numpy (:106-133): per second-pass
    cluster other than 0, the nearest first-pass point of each of its points (k = 1 in float64, preprocess.transfer_labels), the
    np.bincount(...).argmax() of those points' first-pass instances -- the smallest label on equal counts, and 0 can win -- and the
    cluster takes that instance and its class; second-pass background stays 0.  Then the two passes are concatenated, first pass first.
    ValueError when the points of the winning instance carry more than one class (the reference: `raise "sem label error"`)."""
    xyz1 = _host(first_xyz).astype(np.float64)[:, :3]
    ins1 = _host(first_ins).reshape(-1).astype(np.int64)
    sem1 = _host(first_sem).reshape(-1).astype(np.int64)
    xyz2 = _host(bdl_xyz).astype(np.float64)[:, :3]
    ins2 = _host(bdl_ins).reshape(-1).astype(np.int64)
    if ins1.min(initial=0) < 0:
        raise ValueError("merge_boundary: first_ins must be non-negative instance labels")
    near = np.zeros(0, np.int64)
    if ins2.shape[0]:
        near = np.asarray(preprocess.transfer_labels(xyz1, ins1, xyz2)).reshape(-1)           # first-pass instance of the nearest point
    out_ins, out_sem = merge_votes(ins1, sem1, ins2, near)
    return np.concatenate([xyz1, xyz2]), np.concatenate([ins1, out_ins]), np.concatenate([sem1, out_sem])


def merge_votes(first_ins, first_sem, bdl_ins, near_ins):
    """The host half of merge_boundary: near_ins (nb,) the first-pass instance of every boundary point's nearest first-pass point ->
    (ins (nb,), sem (nb,)) int64 of the boundary points."""
    ins1, sem1, ins2, near = (np.asarray(a).reshape(-1).astype(np.int64) for a in (first_ins, first_sem, bdl_ins, near_ins))
    out_ins, out_sem = np.zeros(ins2.shape[0], np.int64), np.zeros(ins2.shape[0], np.int64)
    for cluster in np.unique(ins2):
        if cluster == 0:
            continue
        sel = ins2 == cluster
        winner = int(np.argmax(np.bincount(near[sel])))
        classes = np.unique(sem1[ins1 == winner])
        if classes.shape[0] != 1:
            raise ValueError(f"merge_boundary: first-pass instance {winner} carries the classes {classes.tolist()} (sem label error)")
        out_ins[sel], out_sem[sel] = winner, classes[0]
    return out_ins, out_sem
