"""An O(N^2) float64 numpy restatement of DBSCAN from the rules tgn_dbscan implements (include/tgn_pointops.h), independent of
sklearn and of the kernels: the neighbour test is ((0 + dx*dx) + dy*dy) + dz*dz <= eps*eps on the float64 values of the float32
inputs; core = at least min_samples neighbours, self included; clusters = connected components of core points, numbered by their
smallest core index; a border point takes the smallest number among its core neighbours' clusters; the rest is noise (-1)."""
import numpy as np


def neighbour_matrix(x, eps, rows=None):
    x = np.asarray(x, np.float64)
    r = x if rows is None else x[rows]
    d = r[:, None, :] - x[None, :, :]
    rd = ((0.0 + d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return rd <= eps * eps


def dbscan(x, eps, min_samples, chunk=512):
    n = len(x)
    nbrs = []
    for s in range(0, n, chunk):
        m = neighbour_matrix(x, eps, np.arange(s, min(n, s + chunk)))
        nbrs.extend(np.flatnonzero(row) for row in m)
    core = np.array([len(v) >= min_samples for v in nbrs], bool)
    parent = np.arange(n)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for p in np.flatnonzero(core):
        for q in nbrs[p]:
            if core[q]:
                a, b = find(p), find(q)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    labels = np.full(n, -1, np.int64)
    roots = {}
    for p in np.flatnonzero(core):              # ascending: a component is first met at its smallest core index
        r = find(p)
        if r not in roots:
            roots[r] = len(roots)
        labels[p] = roots[r]
    for p in np.flatnonzero(~core):
        c = [labels[q] for q in nbrs[p] if core[q]]
        if c:
            labels[p] = min(c)
    return labels, core


def dbscan_ragged(x, eps, min_samples, offset):
    labels, core, lo = [], [], 0
    for hi in offset:
        lab, c = dbscan(x[lo:hi], eps, min_samples)
        labels.append(lab)
        core.append(c)
        lo = hi
    return np.concatenate(labels), np.concatenate(core)
