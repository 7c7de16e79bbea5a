"""The inputs of the clustering fixtures (make_golden_r9_cluster.py), shared by the generator and the tests so that the fixture stores
a digest of each input instead of the input itself; the packing of labels and core flags the fixture keeps."""
import numpy as np

from crop_cases import digest  # noqa: F401  (re-exported for the tests)
from toothgroupnetwork_amd import synth


def _blobs(rng, centres, per, sigma):
    return np.concatenate([c + rng.normal(0.0, sigma, size=(per, 3)) for c in centres])


def _arch_centres(k, radius=1.0):
    a = np.linspace(0.15 * np.pi, 0.85 * np.pi, k)
    return np.stack([radius * np.cos(a), radius * np.sin(a), np.zeros(k)], 1)


def dbscan_cases():
    """-> {tag: (xyz (N, 3) float32, eps, min_samples, offset list)}"""
    cases = {}
    rng = np.random.default_rng(901)
    # 16 collapsed tooth blobs of 1 100 points (sigma 0.012) and 600 points of noise: ~18 k points, hundreds of neighbours each
    x = np.concatenate([_blobs(rng, _arch_centres(16), 1100, 0.012), rng.uniform(-0.6, 0.6, size=(600, 3)) * [1, 1, 0.3]])
    x = x[rng.permutation(len(x))]
    cases["blobs"] = (x.astype(np.float32), 0.03, 30, [len(x)])
    # two blobs joined by a thin chain of core points 0.5 long: connectivity across ~17 cells
    t = np.linspace(0.0, 0.5, 500)
    chain = np.stack([t, 0.002 * np.sin(40 * t), np.zeros_like(t)], 1)
    x = np.concatenate([_blobs(rng, [[-0.02, 0, 0], [0.52, 0, 0]], 400, 0.01), chain, rng.uniform(-0.3, 0.8, size=(100, 3))])
    x = x[rng.permutation(len(x))]
    cases["chain"] = (x.astype(np.float32), 0.03, 30, [len(x)])
    # two parallel chains 0.05 apart (never connected) and border points 0.029 from both: each border point sees core points of
    # both clusters and too few points to be core; chain B comes first in index order, so it is cluster 0
    y = np.arange(480) * 0.0021
    chain_a = np.stack([np.zeros_like(y), y, np.zeros_like(y)], 1)
    chain_b = np.stack([np.full_like(y, 0.05), y, np.zeros_like(y)], 1)
    zb = np.sqrt(0.029 ** 2 - 0.025 ** 2)
    yb = 0.05 + 0.1 * np.arange(9) + 0.0007
    border = np.stack([np.full_like(yb, 0.025), yb, np.full_like(yb, zb)], 1)
    x = np.concatenate([chain_b, border, chain_a])
    cases["border"] = (x.astype(np.float32), 0.03, 20, [len(x)])
    # 600 exact duplicates among tooth blobs
    x = _blobs(rng, _arch_centres(8), 600, 0.01)
    x = np.concatenate([x, x[rng.integers(0, len(x), 600)], rng.uniform(-0.5, 0.5, size=(200, 3)) * [1, 1, 0.3]])
    x = x[rng.permutation(len(x))]
    cases["dups"] = (x.astype(np.float32), 0.03, 30, [len(x)])
    # a 12^3 lattice with spacing exactly eps (2^-5): the six axis neighbours lie AT eps, so interior points have exactly 7
    g = np.arange(12) * 0.03125 + 0.5
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    x = x[rng.permutation(len(x))]
    cases["lattice"] = (x.astype(np.float32), 0.03125, 7, [len(x)])
    # sparse uniform points: all noise
    x = rng.uniform(0.0, 1.0, size=(500, 3))
    cases["noise"] = (x.astype(np.float32), 0.01, 5, [len(x)])
    # min_samples = 1: every point is core
    x = rng.uniform(0.0, 1.0, size=(1000, 3))
    cases["ms1"] = (x.astype(np.float32), 0.05, 1, [len(x)])
    # tsegnet's parameters (tsegnet.py:59) on ~2 000 points
    x = np.concatenate([_blobs(rng, _arch_centres(16), 120, 0.015), rng.uniform(-0.6, 0.6, size=(80, 3)) * [1, 1, 0.3]])
    x = x[rng.permutation(len(x))]
    cases["tsegnet"] = (x.astype(np.float32), 0.05, 3, [len(x)])
    # a ragged batch of three clouds
    parts = []
    for k, per in ((6, 500), (4, 500), (9, 440)):
        p = np.concatenate([_blobs(rng, _arch_centres(k), per, 0.012), rng.uniform(-0.6, 0.6, size=(60, 3)) * [1, 1, 0.3]])
        parts.append(p[rng.permutation(len(p))].astype(np.float32))
    cases["ragged"] = (np.concatenate(parts), 0.03, 30, list(np.cumsum([len(p) for p in parts])))
    return cases


def labelling_cases():
    """-> {tag: (moved (N, 3) float32, cls (N,) int64)}: a scan from synth.labelled_arch whose tooth points are pulled toward
    their tooth's centroid (what a trained first stage's offsets do), gingiva class 0, 2 % of the tooth points thrown far off
    (DBSCAN noise: the vote).  `split`: teeth 6 and 7 collapse into one elongated cluster -- tooth 7's blob 0.17 from tooth 6's,
    joined by a bridge of 40 % of tooth 7's points -- that passes the ratio test; the two sub-blobs differ in size."""
    cases = {}
    for tag, seed in (("nosplit", 911), ("split", 912)):
        rows, lab = synth.labelled_arch(24000, 14, seed=seed)
        rng = np.random.default_rng(seed)
        xyz = rows[:, :3].astype(np.float64)
        cls = np.where(lab >= 0, lab % 9 + 1, 0).astype(np.int64)
        moved = xyz.copy()
        cent = {t: xyz[lab == t].mean(0) for t in range(14)}
        target = dict(cent)
        if tag == "split":
            d = cent[7] - cent[6]
            target[7] = cent[6] + 0.17 * d / np.linalg.norm(d)
        for t in range(14):
            sel = np.flatnonzero(lab == t)
            moved[sel] = target[t] + (xyz[sel] - cent[t]) * 0.04 + rng.normal(0.0, 0.004, size=(len(sel), 3))
            if tag == "split" and t == 7:
                bridge = sel[rng.permutation(len(sel))[: int(0.4 * len(sel))]]
                s = rng.uniform(0.0, 1.0, size=len(bridge))[:, None]
                moved[bridge] = cent[6] + s * (target[7] - cent[6]) + rng.normal(0.0, 0.002, size=(len(bridge), 3))
        fg = np.flatnonzero(lab >= 0)
        far = fg[rng.permutation(len(fg))[: len(fg) // 50]]
        moved[far] += rng.uniform(-0.25, 0.25, size=(len(far), 3))
        xyz32 = rows[:, :3]
        offset = moved.astype(np.float32) - xyz32
        cases[tag] = (xyz32 + offset, cls)                # exactly xyz + offset_1 in float32, as the network's moved points are
    return cases


def pack_labels(labels):
    return np.asarray(labels).astype(np.int16)


def pack_core(core):
    return np.packbits(np.asarray(core, bool))


def unpack_core(packed, n):
    return np.unpackbits(packed)[:n].astype(bool)


MS_BANDWIDTH = 0.07


def _bar(rng, n=900):
    """A tapered bar 0.5 long whose density falls along it (beta(2, 5)): seeds at the thin end climb for tens of iterations."""
    t = rng.beta(2, 5, n)[:, None]
    x = t * [0.5, 0.05, 0.0] + rng.normal(0.0, 0.006, size=(n, 3))
    return x.astype(np.float32).astype(np.float64)


def mean_shift_cases():
    """-> {tag: (X (n, 3) float64, bandwidth, max_iters tuple, compare_with_sklearn)} for make_golden_r10_cluster_kernels.py and the
    tests of tgn_mean_shift / tgn_nearest_center.  Not compared with sklearn: `lattice` (its symmetric centres tie) and `nan`
    (sklearn rejects the input)."""
    cases = {}
    rng = np.random.default_rng(1001)
    two = np.concatenate([rng.normal(0, 0.012, (400, 3)), rng.normal(0, 0.012, (300, 3)) + [0.17, 0, 0]])
    for n in (1, 2, 13, 255, 256, 257):                   # around the 256-point LDS tile; half the points in a second blob 0.2 away
        x = rng.normal(0, 0.01, (n, 3))
        x[n // 2 + 1:] += [0.2, 0.0, 0.0]
        cases[f"n{n}"] = (x, MS_BANDWIDTH, (300,), True)
    cases["two"] = (two, MS_BANDWIDTH, (300,), True)
    dups = np.concatenate([two, two[rng.integers(0, len(two), 100)]])
    cases["dups"] = (dups[rng.permutation(len(dups))], MS_BANDWIDTH, (300,), True)
    three = np.concatenate([rng.normal(0, 0.012, (257, 3)) + [0.12 * k, 0.01 * k, 0] for k in range(3)])
    cases["three"] = (three, MS_BANDWIDTH, (300,), True)
    cases["f32"] = (three.astype(np.float32).astype(np.float64), MS_BANDWIDTH, (300,), True)
    bar = _bar(rng)
    cases["bar"] = (bar, MS_BANDWIDTH, (0, 1, 5, 300), True)
    # a tight blob and the bar interleaved by index: the seeds of one workgroup retire at different iterations
    blob = rng.normal(0, 0.004, (900, 3)) + [0.25, 0.4, 0.1]
    mixed = np.empty((1800, 3))
    mixed[0::2], mixed[1::2] = blob, bar
    cases["mixed"] = (mixed, MS_BANDWIDTH, (300,), True)
    # z = -0.0 everywhere: a sum that starts from -0.0 keeps the sign, one that starts from +0.0 loses it
    nz = np.concatenate([rng.normal(0, 0.012, (150, 3)), rng.normal(0, 0.012, (150, 3)) + [0.2, 0, 0]])
    nz[:, 2] = -0.0
    cases["negzero"] = (nz, MS_BANDWIDTH, (300,), True)
    # a 9^3 lattice with spacing and bandwidth 2^-4: the six axis neighbours lie AT the bandwidth
    g = np.arange(9) * 0.0625 + 0.5
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    cases["lattice"] = (lat[rng.permutation(len(lat))], 0.0625, (300,), False)
    # one all-NaN row among two blobs
    nan = two[rng.permutation(len(two))[:300]].copy()
    nan[137] = np.nan
    cases["nan"] = (nan, MS_BANDWIDTH, (300,), False)
    return cases


def _pulled_scan(seed, merges, keep_teeth=None):
    """labelling_cases' scan (synth.labelled_arch(24000, 14, seed), tooth points pulled toward their centroid, 2 % thrown off) with
    every (a, b) of merges collapsed as `split` collapses teeth 6 and 7, and only keep_teeth in the foreground (None: all)."""
    rows, lab = synth.labelled_arch(24000, 14, seed=seed)
    rng = np.random.default_rng(seed)
    xyz = rows[:, :3].astype(np.float64)
    cls = np.where(lab >= 0, lab % 9 + 1, 0).astype(np.int64)
    if keep_teeth is not None:
        cls[~np.isin(lab, keep_teeth)] = 0
    moved = xyz.copy()
    cent = {t: xyz[lab == t].mean(0) for t in range(14)}
    target = dict(cent)
    for a, b in merges:
        d = cent[b] - cent[a]
        target[b] = cent[a] + 0.17 * d / np.linalg.norm(d)
    for t in range(14):
        sel = np.flatnonzero(lab == t)
        moved[sel] = target[t] + (xyz[sel] - cent[t]) * 0.04 + rng.normal(0.0, 0.004, size=(len(sel), 3))
        for a, b in merges:
            if t == b:
                bridge = sel[rng.permutation(len(sel))[: int(0.4 * len(sel))]]
                s = rng.uniform(0.0, 1.0, size=len(bridge))[:, None]
                moved[bridge] = cent[a] + s * (target[b] - cent[a]) + rng.normal(0.0, 0.002, size=(len(bridge), 3))
    fg = np.flatnonzero(lab >= 0)
    far = fg[rng.permutation(len(fg))[: len(fg) // 50]]
    moved[far] += rng.uniform(-0.25, 0.25, size=(len(far), 3))
    return rows, lab, cls, moved, far, rng


def _float32_moved(rows, moved):
    xyz32 = rows[:, :3]
    return xyz32 + (moved.astype(np.float32) - xyz32)      # exactly xyz + offset_1 in float32, as labelling_cases


def _rd(a, b):
    d = a - b
    return ((0.0 + d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def kernel_labelling_cases():
    """-> {tag: (moved (N, 3) float32, cls (N,) int64)}, the branches of get_clustering_labels that labelling_cases leaves out:
    split2   teeth 6+7 and teeth 2+3 collapse into two elongated clusters that both pass the ratio test (labels >= 100 and >= 200);
    three    only teeth 4, 7 and 10 are foreground: exactly three clusters, the reference divides by the mean of nothing;
    votetie  between each pair of neighbouring teeth one gingiva point becomes a foreground point placed on the line between the two
             centroids where its 10 nearest tooth points are 5 of one tooth and 5 of the other (found by bisection on the float32
             values; the generator checks the tie against DBSCAN's labels)."""
    cases = {}
    rows, lab, cls, moved, far, rng = _pulled_scan(913, [(6, 7), (2, 3)])
    cases["split2"] = (_float32_moved(rows, moved), cls)
    rows, lab, cls, moved, far, rng = _pulled_scan(914, [], keep_teeth=[4, 7, 10])
    cases["three"] = (_float32_moved(rows, moved), cls)
    rows, lab, cls, moved, far, rng = _pulled_scan(915, [])
    m32 = _float32_moved(rows, moved)
    placed = np.zeros(len(lab), bool)
    placed[far] = True
    gingiva = np.flatnonzero(lab < 0)
    for a in range(13):
        ia, ib = np.flatnonzero((lab == a) & ~placed), np.flatnonzero((lab == a + 1) & ~placed)
        pa, pb = m32[ia].astype(np.float64), m32[ib].astype(np.float64)
        ca, cb = pa.mean(0), pb.mean(0)
        both, from_a = np.concatenate([pa, pb]), np.arange(len(ia) + len(ib)) < len(ia)
        lo, hi = 0.0, 1.0                                  # at lo the 10 nearest are mostly of a, at hi mostly of a + 1
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            q = (ca + mid * (cb - ca)).astype(np.float32)
            na = int(from_a[np.argsort(_rd(both, q.astype(np.float64)), kind="stable")[:10]].sum())
            if na == 5:
                g = gingiva[a]
                m32[g], cls[g] = q, a % 9 + 1
                break
            lo, hi = (mid, hi) if na > 5 else (lo, mid)
    cases["votetie"] = (m32, cls)
    return cases


def moments_far_cloud():
    """-> (xyz (n, 3) float32, labels (n,) int64, mask (n,) uint8): 15 600 points in 14 labels around (40, -25, 3), so that the mean
    cancels eight digits; the mask keeps the points within 1.5 sigma in x of their centre, so that ignoring it changes every moment."""
    rng = np.random.default_rng(7)
    n = 15600
    cent, lab = rng.uniform(-0.5, 0.5, (14, 3)), rng.integers(0, 14, n)
    noise = rng.normal(0, 1, (n, 3))
    x = (cent[lab] + noise * [0.02, 0.006, 0.004] + [40.0, -25.0, 3.0]).astype(np.float32)
    return x, lab.astype(np.int64), (np.abs(noise[:, 0]) < 1.5).astype(np.uint8)
