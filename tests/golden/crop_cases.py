"""The scans of the op-level crop fixtures (make_golden_r7_grouping.py `ops`), shared by the generator and the GPU tests so that the
fixture stores a digest of each input instead of the input itself; and the compact form of a KDTree result the fixture keeps."""
import hashlib

import numpy as np

from toothgroupnetwork_amd import synth


def op_cases():
    """-> {tag: (rows (B, N, 6) float32, labels (B, N) int64, k)}"""
    cases = {}
    f, l = synth.labelled_arch(24000, 14, seed=701)
    cases["s24"] = (f[None], l[None], 3072)
    f1, l1 = synth.labelled_arch(12000, 16, seed=702)
    f2, l2 = synth.labelled_arch(12000, 11, seed=703)
    cases["ragged"] = (np.stack([f1, f2]), np.stack([l1, l2]), 3072)
    f, l = synth.labelled_arch(8000, 12, seed=704)
    cases["k4096"] = (f[None], l[None], 4096)
    # 600 duplicated vertices, plus one copy (label -1, so that no centroid moves) of the 3072nd-nearest point of the first tooth:
    # a distance tie across the k-th boundary
    f, l = synth.labelled_arch(6000, 10, seed=705, dup=600)
    c = f[l == np.unique(l[l >= 0])[0], :3].mean(axis=0)
    x = f[:, :3].astype(np.float64)
    d = ((0.0 + (x[:, 0] - c[0]) ** 2) + (x[:, 1] - c[1]) ** 2) + (x[:, 2] - c[2]) ** 2
    kth = np.lexsort((np.arange(d.size), d))[3071]
    f, l = np.concatenate([f, f[kth:kth + 1]]), np.concatenate([l, [-1]])
    cases["dup"] = (f[None], l[None], 3072)
    f, l = synth.labelled_arch(5000, 8, seed=706)
    l[np.flatnonzero(l == -1)[17]] = 15                       # tooth 15 is a single point
    cases["single"] = (f[None], l[None], 512)
    return cases


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def pack_sets(idx):
    """(T, k) indices (< 65536) -> (T, k) uint16: each row's index SET, ascending, as differences (the first entry absolute).
    KDTree's order among equal distances is unspecified, and the distance sequence follows from the set."""
    s = np.sort(np.asarray(idx, np.int64), axis=1)
    assert s.size == 0 or s.max() < 65536
    return np.diff(s, axis=1, prepend=0).astype(np.uint16)


def unpack_sets(packed):
    return np.cumsum(packed.astype(np.int64), axis=1)
