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
