"""The scripted cases of the tgnet pipeline, shared by tests/golden/make_golden_r16_tgnet.py (which runs the REFERENCE's pipeline on
them, on the CPU) and the tests (which run this package's, on the GPU): the synthetic meshes and the two stand-in modules.

The stand-ins are fixed functions of the coordinates, built from exactly rounded float32 operations only (subtract, multiply, add,
abs, compare, gather), each a torch call of its own, so the CPU run and the GPU run see the same bits:
  teeth     14 boxes of half-width W = 3/32 in x and y around CENTRES, a table on the 1/1024 grid along the arch's centre line
            (normalised coordinates of synth.obj_text's horseshoe); a point inside box i is tooth i, every other point is gingiva
  sem_1     one-hot logits of the tooth's class (CLASSES[variant]: 1..7 counted from the midline on either side, 1 and 9 for the two
            central teeth, as number_teeth expects them before its side test); gingiva class 0
  offset_1  (centre - xyz) * shrink for a tooth's points, 0 for gingiva.  The first stand-in shrinks every tooth to 1/16 of its size
            (shrink 15/16: genuine, similar covariances for the clustering's split test) and leaves the points within STRAY of the
            box's middle line in x where they are: DBSCAN noise, which the 10-nearest vote hands to their tooth (the reference's
            get_clustering_labels dies without a noise point); the boundary stand-in moves every point onto its centre (shrink 1, no
            strays: blobs a rounding wide, for which any seeding of k-means finds the one partition)
  crops     the K nearest points of every centre (the caller supplies the kNN: an sklearn KDTree there, crops.crop_knn here)
  sem_2     per crop point (1, 0) for gingiva and (0, 1) for a tooth's point: sums of small integers, exact in any order
Both passes label a point by the same function of its coordinates, so a vertex that is equally near a first-pass point and a
boundary point (the same vertex sampled twice) gets the same label from either.
"""
import numpy as np
import torch

TEETH = 14
W = 3.0 / 32.0
STRAY = 1.0 / 256.0
K_CROP = 3072
MESHES = {"main": (250, 120, 1601), "small": (150, 100, 1602)}       # synth.obj_text(n_u, n_v, seed): 30 000 and 15 000 vertices
N_DUPLICATES = 50
PERM_SEED = 1616
VARIANTS = ("full", "fallback", "classless")


def _centres():
    u = np.pi * (np.arange(TEETH) + 0.5) / TEETH
    c = np.stack([22.0 * np.cos(u) * 0.05525 + 0.2035, 28.6 * np.sin(u) * 0.05525 - 0.8, np.full(TEETH, 0.2)], axis=1)
    c = (np.round(c * 1024.0) / 1024.0).astype(np.float32)
    for i in range(TEETH):
        for j in range(i + 1, TEETH):
            assert max(abs(c[i, 0] - c[j, 0]), abs(c[i, 1] - c[j, 1])) > 2 * W + 1 / 64, "the boxes must not touch"
    return c


CENTRES = _centres()


def _classes(variant):
    """class of tooth 0..13 (tooth i sits at angle pi (i + 0.5) / 14: 0..6 have x above the middle, 7..13 below)"""
    cls = [7 - i for i in range(7)] + [9] + [i - 6 for i in range(8, 14)]
    if variant == "fallback":                        # no class 1 and no class 9: number_teeth takes its fallback loop
        cls[6], cls[7] = 8, 8
    elif variant == "classless":                     # every point of tooth 3 is class 0: the instance is zeroed
        cls[3] = 0
    return np.array([0] + cls, np.int64)             # entry 0: gingiva


CLASSES = {v: _classes(v) for v in VARIANTS}


def tooth_of(xyz):
    """xyz (..., 3) float32 tensor -> (...,) int64: the tooth 0..13 whose box holds the point, -1 for gingiva"""
    c = torch.from_numpy(CENTRES).to(xyz.device)
    inside = ((xyz[..., None, 0] - c[:, 0]).abs() < W) & ((xyz[..., None, 1] - c[:, 1]).abs() < W)
    tooth = inside.to(torch.int64).argmax(dim=-1)
    return torch.where(inside.any(dim=-1), tooth, torch.full_like(tooth, -1))


class StandIn:
    """A GroupingNetworkModule's call and output dict.  knn(xyz (N, 3) float32 tensor, centres (T, 3) float32 tensor, k) -> (T, k)
    int64 indices as a tensor on xyz's device."""

    def __init__(self, knn, shrink, strays, variant="full", k=K_CROP):
        self.knn, self.shrink, self.strays, self.classes, self.k = knn, float(shrink), strays, CLASSES[variant], k

    def cuda(self):
        return self

    def __call__(self, inputs, test=False):
        feats = inputs[0]
        assert feats.dim() == 3 and feats.shape[0] == 1 and feats.dtype == torch.float32
        dev = feats.device
        xyz = feats[0, :3].t().contiguous()
        tooth = tooth_of(xyz)
        cls = torch.from_numpy(self.classes).to(dev)[tooth + 1]
        sem_1 = torch.nn.functional.one_hot(cls, 10).to(torch.float32).t().contiguous()[None]
        centres = torch.from_numpy(CENTRES).to(dev)
        to_centre = centres[tooth.clamp(min=0)] - xyz
        moves = (tooth >= 0) & ~(to_centre[:, 0].abs() < STRAY) if self.strays else tooth >= 0
        offset = torch.where(moves[:, None], to_centre * self.shrink, torch.zeros_like(to_centre))
        idx = self.knn(xyz, centres, self.k)
        fg = (tooth >= 0)[idx]
        sem_2 = torch.stack([~fg, fg], dim=1).to(torch.float32)
        return {"sem_1": sem_1, "offset_1": offset.t().contiguous()[None], "mask_1": None, "first_features": None, "sem_2": sem_2,
                "offset_2": None, "mask_2": None, "nn_crop_indexes": [idx]}


def stand_ins(knn, variant="full"):
    """(first module, boundary module)"""
    return StandIn(knn, 15.0 / 16.0, True, variant), StandIn(knn, 1.0, False, variant)


def device_knn(xyz, centres, k):
    """crops.crop_knn: ascending (float64 squared distance, index)"""
    from toothgroupnetwork_amd import crops
    scan = torch.zeros(centres.shape[0], dtype=torch.int32, device=xyz.device)
    return crops.crop_knn(xyz.t().contiguous()[None], scan, centres.contiguous(), k)


def obj_with_duplicates(text, n_dup=N_DUPLICATES, seed=7):
    """-> (the OBJ text with n_dup `v` lines appended that repeat earlier vertices verbatim, the zero-based rows they repeat)"""
    lines = text.rstrip("\n").split("\n")
    v_rows = [i for i, line in enumerate(lines) if line.startswith("v ")]
    pick = np.random.default_rng(seed).choice(len(v_rows), n_dup, replace=False)
    return "\n".join(lines + [lines[v_rows[p]] for p in pick]) + "\n", pick
