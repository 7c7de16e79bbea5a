"""The inputs of the tsegnet fixtures (make_golden_r11_tsegnet.py), shared by the generator and the tests so that the fixture stores a
digest of each input instead of the input itself; and the scripted stages that stand in for the two networks.  Everything scripted is
built from exactly-rounded float32 operations (multiply, add, subtract, floor, remainder, abs, min, max), so a CPU run of the reference
and a GPU run of this package see the same values bit for bit."""
import numpy as np
import torch

from toothgroupnetwork_amd import synth

from crop_cases import digest  # noqa: F401

N_POINTS, N_COARSE, CROP_K, MAX_CROPS = 24000, 256, 3072, 8
PERM_SEED = 1105                              # np.random.seed in front of the module's forward: the 8-of-T choice
FORCED = (5, 6, 7)                            # coarse points whose dist is float32(0.3), the float32 below it, NaN
PLANTED = (0.0, -0.0, 1e-8, 6e-8, 1.2e-7, 2e-7)      # mask logits around sigmoid's rounding to 0.5: false x4, true x2
MASK_R2 = 0.0225                              # scripted mask: inside 0.15 of the crop's bounding-box centre
MESH = (200, 150, 43)                         # n_u, n_v, seed -> 30 000 vertices for the pipeline case


def module_case():
    """One 24 000-point scan with 14 teeth and scripted outputs of the centroid stage: 256 coarse points spread over the arch, offsets to
    the nearest true tooth centre plus jitter (5 % strays), the distance to it; three forced dist entries."""
    rows, labels = synth.labelled_arch(N_POINTS, 14, seed=1101)
    xyz = rows[:, :3]
    pick = np.random.default_rng(1102).permutation(N_POINTS)[:N_COARSE]
    l3 = xyz[pick]
    centres = np.stack([xyz[labels == t].astype(np.float64).mean(axis=0) for t in range(14)])
    d = ((l3[:, None, :].astype(np.float64) - centres[None]) ** 2).sum(-1)
    near = d.argmin(axis=1)
    rng = np.random.default_rng(1103)
    jitter = rng.normal(0.0, 0.004, (N_COARSE, 3))
    jitter[rng.random(N_COARSE) < 0.05] *= 40.0
    offset = (centres[near] - l3 + jitter).astype(np.float32)
    dist = np.sqrt(d.min(axis=1)).astype(np.float32)
    dist[FORCED[0]] = np.float32(0.3)
    dist[FORCED[1]] = np.nextafter(np.float32(0.3), np.float32(0.0))
    dist[FORCED[2]] = np.float32(np.nan)
    l0_points = np.random.default_rng(1104).standard_normal((1, 32, N_POINTS), dtype=np.float32)
    return dict(feats=np.ascontiguousarray(rows.T)[None], labels=labels.reshape(1, 1, -1).astype(np.int64),
                l3_xyz=np.ascontiguousarray(l3.T)[None], offset=np.ascontiguousarray(offset.T)[None], dist=dist.reshape(1, 1, -1),
                l0_points=l0_points)


def case_digest(case):
    return digest(*(case[n] for n in ("feats", "labels", "l3_xyz", "offset", "dist", "l0_points")))


def fixed_cent(feats):
    """The pipeline case's centroid stage, (1, 6, N) -> the six outputs of tsg_centroid_module: 32 feature channels that are scaled
    input channels; the first 256 points (the input is in farthest-point order, so they are spread over the scan); offsets that snap
    them to a 0.25 lattice, so that the moved points of one cell form one cluster; dist = the offset's L1 norm."""
    xyz = feats[:, :3, :]
    l0_points = torch.cat([feats * (0.5 * (i + 1)) for i in range(5)] + [feats[:, :2, :] * 3.0], 1)
    l3_xyz = xyz[:, :, :N_COARSE].contiguous()
    offset = torch.floor(l3_xyz * 4.0 + 0.5) * 0.25 - l3_xyz
    a = offset.abs()
    dist = (a[:, 0:1, :] + a[:, 1:2, :]) + a[:, 2:3, :]
    return l0_points, None, xyz, l3_xyz, offset, dist


def fixed_seg(cropped):
    """The scripted segmentation stage, (T, C >= 3, k) -> (pd_1, weight_1, pd_2 (T, 1, k), id_pred (T, 17)), a function of the xyz
    channels alone (the distance channel is equal only to rounding) that does not depend on the order of the k columns: the mask logit
    is MASK_R2 minus the squared distance from the crop's bounding-box centre, the tooth id a hash of the box's upper corner."""
    xyz = cropped[:, :3, :]
    hi, lo = xyz.max(dim=2).values, xyz.min(dim=2).values
    c = (hi + lo) * 0.5
    d = xyz - c[:, :, None]
    d = d * d
    r2 = (d[:, 0, :] + d[:, 1, :]) + d[:, 2, :]
    pd_2 = (MASK_R2 - r2)[:, None, :]
    s = hi[:, 0] * 7.0
    s = s + hi[:, 1] * 3.0
    cls = (torch.remainder(torch.floor(s * 16.0), 16.0) + 1.0).long()
    return None, None, pd_2, torch.nn.functional.one_hot(cls, 17).float()


def plant(pd_2, idx):
    """pd_2 (T, 1, k) float32 numpy with PLANTED written, in the last crop (no later crop overwrites it), at the six entries of smallest point index (idx (T, k))."""
    out = np.array(pd_2, np.float32)
    cols = np.argsort(idx[-1], kind="stable")[:len(PLANTED)]
    out[-1, 0, cols] = np.array(PLANTED, np.float32)
    return out


def clumped_scan(seed):
    """A 24 000-point scan of 14 separated teeth (every tooth of an arch scan shrunk towards its centre) -> ((6, N) float32 rows,
    (N,) int64 labels): the 256 coarse points of the centroid network then form one DBSCAN(0.05, 3) cluster per tooth without any help
    from a trained offset head."""
    rows, labels = synth.labelled_arch(40000, 14, seed=seed)
    keep = np.flatnonzero(labels >= 0)[:N_POINTS]
    rows, labels = rows[keep].copy(), labels[keep]
    for t in range(14):
        m = labels == t
        c = rows[m, :3].mean(axis=0)
        rows[m, :3] = c + 0.4 * (rows[m, :3] - c)
    return np.ascontiguousarray(rows.T), labels


def set_heads(net):
    """The two heads of a seeded TSegNetModule's centroid network as the reference initialises them (zero weights), with biases that
    let every proposal pass the 0.3 filter (share kept: all 256) and move every coarse point by one small seeded vector."""
    with torch.no_grad():
        net.cent_module.dist_conv_2.weight.zero_()
        net.cent_module.dist_conv_2.bias.fill_(0.25)
        net.cent_module.offset_conv_2.weight.zero_()
        net.cent_module.offset_conv_2.bias.mul_(0.1)
    return net


class Stage(torch.nn.Module):
    """A network stage replaced by a function of its input."""

    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x):
        return self.fn(x)
