"""Numpy restatements of the contracts of tgn_mean_shift, tgn_nearest_center, tgn_cluster_moments, tgn_cluster_vote and of
tgn_crop_knn's order (include/tgn_pointops.h), written from the header and from sklearn's documented MeanShift algorithm; independent
of toothgroupnetwork_amd/cluster.py, whose host parts are code under test.  Everything is float64 unless it says otherwise."""
import numpy as np


def rdist(a, b):
    """KDTree's euclidean rdist, ((0 + dx*dx) + dy*dy) + dz*dz, over the last axis (broadcasting)."""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return ((0.0 + dx * dx) + dy * dy) + dz * dz


def mean_shift_seeds(X, bandwidth, max_iter, margin=None):
    """The climb of every point of X (n, 3) float64 as a seed -> (means (n, 3) float64, counts (n,) int32).  A step: the points within the
    bandwidth of the mean (rdist <= bw*bw), their row-by-row sum in ascending index order divided by their count; the seed stops when
    the step's length is <= 1e-3 * bw or when the steps completed before it number max_iter; with no point within the bandwidth it
    stays where it is with count 0.  The sum starts from -0.0, the identity of IEEE addition, so it is p0 + p1 + ... and nothing else;
    numpy's default start is +0.0, which differs in one place only: a column of nothing but -0.0 sums to +0.0 there and to -0.0 here
    (and in the kernel).  margin: a one-element list that receives the smallest |rdist - bw^2| / bw^2 met."""
    X = np.ascontiguousarray(X, np.float64)
    n, bw2, stop = len(X), bandwidth * bandwidth, 1e-3 * bandwidth
    means, counts = X.copy(), np.zeros(n, np.int32)
    done_iters = np.zeros(n, np.int64)
    active = np.ones(n, bool)
    with np.errstate(invalid="ignore"):
        while active.any():
            for lo in range(0, n, 256):
                rows = lo + np.flatnonzero(active[lo:lo + 256])
                if not len(rows):
                    continue
                rd = rdist(means[rows][:, None, :], X[None, :, :])
                if margin is not None and np.isfinite(rd).any():
                    margin[0] = min(margin[0], float(np.nanmin(np.abs(rd - bw2)) / bw2))
                within = rd <= bw2
                for r, s in enumerate(rows):
                    pts = X[within[r]]
                    c = len(pts)
                    if c == 0:
                        counts[s] = 0
                        active[s] = False
                        continue
                    new = np.add.reduce(pts, axis=0, initial=-0.0) / c      # p0 + p1 + ...: see the docstring
                    dx, dy, dz = new - means[s]
                    shift = np.sqrt((dx * dx + dy * dy) + dz * dz)
                    means[s] = new
                    counts[s] = c
                    if shift <= stop or done_iters[s] == max_iter:
                        active[s] = False
                    else:
                        done_iters[s] += 1
    return means, counts


def mean_shift_centers(means, counts, bandwidth):
    """MeanShift.fit after the climbs: one candidate per distinct final mean (exact equality) with the count of its last step as
    intensity, seeds of count 0 dropped; candidates in descending (intensity, centre) order; going down that order, a candidate
    still standing removes every later candidate within the bandwidth of it."""
    cand = {}
    for m, c in zip(means.tolist(), counts.tolist()):
        if c:
            cand[tuple(m)] = c
    order = sorted(cand, key=lambda m: (cand[m], m), reverse=True)
    cen = np.array(order, np.float64).reshape(-1, 3)
    keep = np.ones(len(cen), bool)
    for i in range(len(cen)):
        if keep[i]:
            near = rdist(cen, cen[i]) <= bandwidth * bandwidth
            near[i] = False
            keep &= ~near
    return cen[keep]


def nearest_center(X, C):
    """-> (n,) int64: argmin over the centres of rdist, the first minimum (the lower index) on equal distances."""
    return np.argmin(rdist(np.asarray(X, np.float64)[:, None, :], np.asarray(C, np.float64)[None, :, :]), axis=1).astype(np.int64)


def mean_shift_fit(X, bandwidth, max_iter, margin=None):
    """-> (labels (n,) int64, centers (K, 3) float64), as MeanShift(bandwidth, max_iter=max_iter).fit(X) with its defaults."""
    means, counts = mean_shift_seeds(X, bandwidth, max_iter, margin)
    centers = mean_shift_centers(means, counts, bandwidth)
    return nearest_center(X, centers), centers


def moments_exact(x32, labels, mask, nlab):
    """Per label l in [0, nlab) over the points with labels == l (and mask != 0 where a mask is given), in np.longdouble from the
    float32 values: -> count (nlab,) int64, mean (nlab, 3), cov (nlab, 3, 3) with ddof = 1, sum|x| (nlab, 3), sum|dx*dy| (nlab, 3, 3).
    A label with no point has a NaN mean; fewer than 2 points give a NaN covariance."""
    x = np.asarray(x32, np.float32).astype(np.longdouble)
    labels = np.asarray(labels).reshape(-1)
    keep = np.ones(len(x), bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    count = np.zeros(nlab, np.int64)
    mean = np.full((nlab, 3), np.nan, np.longdouble)
    cov = np.full((nlab, 3, 3), np.nan, np.longdouble)
    absx = np.zeros((nlab, 3), np.longdouble)
    absd = np.zeros((nlab, 3, 3), np.longdouble)
    for l in range(nlab):
        p = x[keep & (labels == l)]
        c = count[l] = len(p)
        if c == 0:
            continue
        mean[l] = p.sum(0) / c
        absx[l] = np.abs(p).sum(0)
        d = p - mean[l]
        absd[l] = (np.abs(d)[:, :, None] * np.abs(d)[:, None, :]).sum(0)
        if c >= 2:
            cov[l] = (d[:, :, None] * d[:, None, :]).sum(0) / (c - 1)
    return count, mean, cov, absx, absd


U = 2.0 ** -53
MOMENTS_C0 = 8


def moments_bounds(n, count, absx, absd):
    """The error bounds of tgn_cluster_moments' mean and covariance against moments_exact (derivation: the docstring of
    tests/test_gpu_cluster_kernels.py::test_moments_within_the_derived_bound) -> (bound_mean (nlab, 3), bound_cov (nlab, 3, 3)),
    longdouble; NaN where the count makes the quantity undefined."""
    D = -(-n // 256) + 8
    c = count.astype(np.longdouble)
    with np.errstate(divide="ignore", invalid="ignore"):
        bm = (D + 1) * U * absx / c[:, None]
        bc = ((D + MOMENTS_C0) * U * absd + c[:, None, None] * bm[:, :, None] * bm[:, None, :]) / (c[:, None, None] - 1)
    return bm, bc


def vote(nn_idx, cand_labels):
    """Row by row: the most frequent of cand_labels[nn_idx[i]], equal counts to the smallest label (np.unique sorts; argmax takes the
    first maximum)."""
    cand_labels = np.asarray(cand_labels)
    out = np.empty(len(nn_idx), np.int64)
    for i, row in enumerate(np.asarray(nn_idx)):
        u, c = np.unique(cand_labels[row], return_counts=True)
        out[i] = u[np.argmax(c)]
    return out


def knn_order(cand32, q32, k):
    """The k candidates nearest to q in ascending (float64 rdist of the float32 values, index) order."""
    d = rdist(np.asarray(cand32, np.float32).astype(np.float64), np.asarray(q32, np.float32).astype(np.float64))
    return np.lexsort((np.arange(d.size), d))[:k]


def moments_within(n, mean, cov, exact):
    """mean (nlab, 3), cov (nlab, 3, 3) float64 against exact = moments_exact(...) over n points -> (mean_ok (nlab, 3) bool, cov_ok
    (nlab, 3, 3) bool, the largest error / bound): |error| <= bound where the quantity is defined (count >= 1, count >= 2), NaN where
    it is not."""
    count, em, ec, absx, absd = exact
    bm, bc = moments_bounds(n, count, absx, absd)
    has1, has2 = (count >= 1)[:, None], (count >= 2)[:, None, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        err_m, err_c = np.abs(mean.astype(np.longdouble) - em), np.abs(cov.astype(np.longdouble) - ec)
        mean_ok = np.where(has1, err_m <= bm, np.isnan(mean))
        cov_ok = np.where(has2, err_c <= bc, np.isnan(cov))
        ratios = np.concatenate([(err_m / bm)[np.broadcast_to(has1, err_m.shape) & (bm > 0)],
                                 (err_c / bc)[np.broadcast_to(has2, err_c.shape) & (bc > 0)]])
    return mean_ok, cov_ok, float(ratios.max()) if ratios.size else 0.0
