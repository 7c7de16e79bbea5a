"""The cases of the contrastive-boundary criterion's fixture (tests/golden/reference_cpu_r19_cbl.npz, written by
make_golden_r19_cbl.py) and of its tests: hand-made decoder stages, the smallest that reach every rule of the criterion, rebuilt from
seeds on both sides so the fixture stores results only.

Hand-made stages (`build(name)`): B = 2 scans of 96 / 24 / 6 points that fill the SAME unit square (z within 0.1), so a neighbour list
that ignores the offsets mixes them; C = 32 latent channels; stride [1, 4, 4] (kr = 1 and 4), nsample [9, 9, 9]: the last stage has
fewer points than nsample, so its lists hold the padding (the scan's first point).  Stage-0 targets are the quadrants of the square
(blobs4: 4 classes) or its halves (binary2: targets 0 / 1, the second network's shape of problem), which leaves interior points (every
neighbour positive), boundary points, and one planted point whose neighbours all carry another label (no positive).  Scan 0 holds one
exactly duplicated point pair (rows 4 and 5), so column 0 of a neighbour list need not be the point itself.

  blobs4    stage 2 of either scan sits inside one quadrant (labels 1 and 2: a list across scans would be mixed), so no point is mixed
            and the stage loss is 0; one of scan 0's stage-2 points has an exact 2 : 2 vote between labels 1 (lowest, two FARTHEST
            votes) and 3, and belongs to the unmixed stage only under the lowest-label rule
  binary2   stage 2 is drawn from the whole square: mixed points over padded lists
  flat0     (GPU test only: the reference raises) blobs4's geometry with one target everywhere: no mixed point at any stage

Network cases (NET_CASES): PointTransformerSeg with seeded weights (seeded.py) on synthetic arch scans, labels along the arch.

BOUNDS: per case the reference's own float32 error against the float64 restatement (tests/cbl_ref.py), in units of float32 epsilon
times the sum of the magnitudes of the terms added (cbl_ref's scales), as make_golden_r19_cbl.py measured and printed it, and the bound
the GPU is held to: twice the largest such value, rounded up to a power of two.  The factor two covers another summation order and the
float atomics of tgn_subtraction_backward."""
import numpy as np

C = 32
PER_SCAN = (96, 24, 6)
STRIDE = (1, 4, 4)
NSAMPLE = (9, 9, 9)
HAND_CASES = ("blobs4", "binary2")
DUPLICATE = (4, 5)                    # rows of scan 0, stage 0
SEEDS = {"blobs4": 1901, "binary2": 1902, "flat0": 1901}


def _nearest(points, centre, n, skip=()):
    d = ((points[:, :2] - np.asarray(centre, np.float32)) ** 2).sum(1)
    d[list(skip)] = np.inf
    return np.argsort(d, kind="stable")[:n]


def build(name):
    """-> dict(p, o, f: lists over the three stages of (m, 3) float32, (2,) int32, (m, 32) float32; target (192,) int64 in [0, ncls);
    ncls, nsample, stride, planted: the stage-0 row without a positive neighbour, tie: the stage-2 row with the 2 : 2 vote or None)"""
    rng = np.random.default_rng(SEEDS[name])
    n0 = PER_SCAN[0]
    scans = [(rng.random((n0, 3)) * np.array([1.0, 1.0, 0.1])).astype(np.float32) for _ in range(2)]
    scans[0][DUPLICATE[1]] = scans[0][DUPLICATE[0]]
    p0 = np.concatenate(scans)
    right, top = p0[:, 0] >= 0.5, p0[:, 1] >= 0.5
    binary = name == "binary2"
    target = right.astype(np.int64) if binary else (right + 2 * top).astype(np.int64)
    ncls = 2 if binary else 4
    # the planted point: deep inside scan 1's top right quadrant, with another label than everything around it
    planted = n0 + int(_nearest(scans[1], (0.8, 0.8), 1)[0])
    target[planted] = 0
    tie = None
    rows1 = [b * n0 + np.sort(rng.choice(n0, PER_SCAN[1], replace=False)) for b in range(2)]
    if binary:
        rows2 = [b * n0 + np.sort(rng.choice(n0, PER_SCAN[2], replace=False)) for b in range(2)]
    else:
        # scan 0: five points deep inside the bottom right quadrant (label 1) and the tie point; scan 1: six deep inside the top left (2)
        deep0 = _nearest(scans[0], (0.8, 0.2), PER_SCAN[2] - 1, skip=DUPLICATE)
        tie_row = int(_nearest(scans[0], (0.75, 0.5), 1, skip=DUPLICATE)[0])
        d = ((scans[0] - scans[0][tie_row]) ** 2).sum(1)
        d[list(DUPLICATE)] = np.inf
        near4 = np.argsort(d, kind="stable")[:4]                   # the tie point itself first
        assert not set(near4) & set(deep0) and tie_row not in deep0
        target[near4] = [3, 3, 1, 1]                               # the two nearest votes for the HIGHER label
        rows2 = [np.concatenate([deep0, [tie_row]]), n0 + _nearest(scans[1], (0.2, 0.8), PER_SCAN[2])]
        tie = PER_SCAN[2] - 1
    if name == "flat0":
        target[:] = 1
    p = [p0, p0[np.concatenate(rows1)], p0[np.concatenate(rows2)]]
    o = [np.array([m, 2 * m], np.int32) for m in PER_SCAN]
    f = [(rng.standard_normal((2 * m, C)) * 0.5).astype(np.float32) for m in PER_SCAN]
    return dict(p=p, o=o, f=f, target=target, ncls=ncls, nsample=NSAMPLE, stride=STRIDE, planted=planted, tie=tie)


# ---- the network cases --------------------------------------------------------------------------------------------------------------

FIVE = dict(c=6, planes=[32, 64, 128, 256, 512], stride=[1, 4, 4, 4, 4], nsample=[36, 24, 24, 24, 24], blocks=[2, 3, 4, 6, 3], block_num=5)
TWO = dict(c=6, planes=[16, 32], stride=[1, 1], nsample=[36, 24], blocks=[2, 3], block_num=2)
# name: (architecture, k, B, N, weight seed, scan seed)
NET_CASES = {"five_b1": (FIVE, 10, 1, 6144, 71, 1971), "five_b2": (FIVE, 10, 2, 6144, 71, 1972), "two_b2": (TWO, 2, 2, 512, 72, 1973)}


def arch_labels(xyz, k):
    """Labels -1 (the lower 35 % in z) and 0 .. k-2 along the arch angle, the value range the networks' inputs[1] has: k = 10 the
    half-jaw labels of the first network, k = 2 the crop labels of the second (every tooth 0)."""
    ang = np.arctan2(xyz[:, 1], xyz[:, 0])
    lo, hi = np.quantile(ang, 0.02), np.quantile(ang, 0.98)
    t = np.clip(((ang - lo) / (hi - lo) * (k - 1)).astype(np.int64), 0, k - 2)
    t[xyz[:, 2] < np.quantile(xyz[:, 2], 0.35)] = -1
    return t


def net_inputs(name):
    """-> (features (B, 6, N) float32, labels (B, 1, N) int64) as numpy arrays"""
    from toothgroupnetwork_amd import synth
    _, k, B, N, _, scan_seed = NET_CASES[name]
    scans = synth.scan_batch(B, N, "arch", seed=scan_seed)
    labels = np.stack([arch_labels(s[:, :3], k) for s in scans])[:, None, :]
    return np.ascontiguousarray(scans.transpose(0, 2, 1)), labels


# ---- bounds (see the module docstring; the measured values are make_golden_r19_cbl.py's output) ---------------------------------------

def _pow2_at_least(x):
    return float(2 ** int(np.ceil(np.log2(x))))


MEASURED = {
    # case: (largest loss error, largest latent-gradient error) over the stages, of the reference's float32 CPU run against the float64
    # restatement, in the units above (rounded up in the last digit)
    "blobs4": (0.1712, 45.4355),
    "binary2": (0.1346, 12.7546),
}
# The criterion alone: twice the largest value over the hand-made cases, rounded up to a power of two.  (The loss errors are small
# because a stage loss is a mean over tens of points whose roundings average out; what is left is mostly the one rounding of the
# float32 result, about 0.1 of a unit.)
LOSS_BOUND = _pow2_at_least(2 * max(v[0] for v in MEASURED.values()))          # 0.5
GRAD_BOUND = _pow2_at_least(2 * max(v[1] for v in MEASURED.values()))          # 128
NET_MEASURED = {
    # case: largest loss error over the stages of the reference's float32 NETWORK against its float64 network on the same indices, same
    # units: here the latent features themselves carry the float32 error of up to 23 residual blocks
    "five_b1": 194.9264,
    "five_b2": 208.1232,
    "two_b2": 0.1389,
}
# Through a network: twice the largest value over the network cases, rounded up to a power of two -- one bound for the family, as the
# criterion has one: the two-stage network's own 0.14 is the float32 rounding of its result, not a measure of a network's error.
NET_LOSS_BOUND = _pow2_at_least(2 * max(NET_MEASURED.values()))                # 512
