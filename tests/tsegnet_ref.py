"""numpy restatements of the three kernel contracts of csrc/tsegnet.hip (include/tgn_pointops.h), test-only: what
tests/test_tsegnet_host.py holds against the reference's fixture and tests/test_gpu_tsegnet.py holds the kernels against."""
import numpy as np


def proposals(l3_xyz, offset, dist, threshold=0.3):
    """tgn_tsg_proposals: l3_xyz, offset (B, 3, M), dist (B, 1, M) float32 -> (moved (K, 3) float32 packed scan after scan in ascending
    point order, counts (B,), kept (B, M) bool)."""
    l3_xyz, offset, dist = (np.asarray(a, np.float32) for a in (l3_xyz, offset, dist))
    kept = dist[:, 0, :] < np.float32(threshold)                            # NaN compares false
    moved = (l3_xyz + offset).transpose(0, 2, 1)                            # one float32 addition per coordinate
    return np.ascontiguousarray(moved[kept]), kept.sum(1), kept


def _fma32(a, b, c):
    """float32 fused multiply-add: the product of two float32 values is exact in float64; the sum is rounded to float64 and then to
    float32 (a double rounding that differs from a true fma only in rare half-way cases: the distance feature is held to a tolerance)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def ddf32(xyz, cent):
    """xyz (T, 3, k) float32, cent (T, 3) float32 -> (T, k) float32: expf(-4 sqrtf(d)), d the expanded squared distance in the
    contract's operation order."""
    x, y, z = (xyz[:, a, :].astype(np.float32) for a in range(3))
    cx, cy, cz = (np.broadcast_to(cent[:, a, None].astype(np.float32), x.shape) for a in range(3))
    s1 = ((x * x) + (y * y)) + (z * z)
    s2 = ((cx * cx) + (cy * cy)) + (cz * cz)
    dot = _fma32(z, cz, _fma32(y, cy, x * cx))
    d = ((np.float32(-2.0) * dot) + s1) + s2
    with np.errstate(invalid="ignore"):
        return np.exp(np.sqrt(d) * np.float32(-4.0)).astype(np.float32)


def ddf64(xyz, cent):
    """The same feature with every operation in float64 on the float32 inputs' values."""
    p = np.asarray(xyz, np.float64)
    c = np.asarray(cent, np.float64)[:, :, None]
    d = -2.0 * (p * c).sum(1) + (p * p).sum(1) + (c * c).sum(1)
    return np.exp(-4.0 * np.sqrt(np.maximum(d, 0.0)))


def crop_features(feats, l0_points, crop_scan, cent, idx, labels=None):
    """tgn_tsg_crop_features: feats (B, C, N), l0_points (B, Cf, N), crop_scan (T,), cent (T, 3), idx (T, k) ->
    (out (T, 3 + Cf + 1, k) float32, out_labels (T, 1, k) int64 or None)."""
    feats, l0_points = np.asarray(feats, np.float32), np.asarray(l0_points, np.float32)
    T, k = idx.shape
    cf = l0_points.shape[1]
    out = np.empty((T, 3 + cf + 1, k), np.float32)
    for t in range(T):
        b = int(crop_scan[t])
        out[t, :3] = feats[b, :3][:, idx[t]]
        out[t, 3:3 + cf] = l0_points[b][:, idx[t]]
    out[:, 3 + cf] = ddf32(out[:, :3], np.asarray(cent, np.float32))
    lab = None
    if labels is not None:
        labels = np.asarray(labels).reshape(feats.shape[0], -1)
        lab = np.stack([labels[int(crop_scan[t])][idx[t]] for t in range(T)])[:, None, :].astype(np.int64)
    return out, lab


def paint(b, n, crop_scan, idx, mask, ids):
    """tgn_tsg_paint by its definition: the crops written one after the other in ascending crop number."""
    out = np.zeros((b, n), np.int64)
    for t in range(idx.shape[0]):
        m = np.asarray(mask[t]).astype(bool)
        out[int(crop_scan[t]), idx[t][m]] = ids[t]
    return out


def sorted_columns(values, idx):
    """values (T, C, k) reordered along k by ascending point index idx (T, k): a column order that does not depend on how equal
    distances were ordered."""
    order = np.argsort(idx, axis=1, kind="stable")
    return np.take_along_axis(values, order[:, None, :], axis=2)


def _err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / (1.0 + np.abs(want))))


def _rms(got, want):
    return float(np.sqrt(np.mean((np.asarray(got, np.float64) - np.asarray(want, np.float64)) ** 2)))


def within_reference_noise(name, got, ref32, exact):
    """The rule of tests/test_gpu_grouping_network.py: the distance from the exact (float64) value against the reference's own float32
    distance on the same entries, within 2x in root mean square and 4x in maximum, floors 1e-6 / 1e-5."""
    e_max, own_max = _err(got, exact), _err(ref32, exact)
    e_rms, own_rms = _rms(got, exact), _rms(ref32, exact)
    print(f"{name}: max {e_max:.3e} (reference's own {own_max:.3e}), rms {e_rms:.3e} (reference's own {own_rms:.3e})")
    assert e_rms <= max(1e-6, 2.0 * own_rms), (name, "rms", e_rms, own_rms)
    assert e_max <= max(1e-5, 4.0 * own_max), (name, "max", e_max, own_max)
