"""GPU: fps_bucket_kernel takes the box test of an iteration behind the hand-off of the one before, and the winning wave takes it
from the mask it worked out against its own candidate while it waited at the barrier (csrc/fps_bucket.hip, TGN_FPS_OWN_MASK).
Neither changes a result: indices equal the oracle's and centroids are the points the indices name, bit for bit, on the three
instances the headline and the 4-wave path use -- <256,8> (2048 points, fps_bucket_min = 2048), <512,16> (4096 points, dense, local
indices, TGN_FPS_LOW_VALU) and <512,48> (24 000 points) -- in the first-index and the tree tie mode and once in the FMA arithmetic.

Clouds: eight far-apart clusters (the winner changes wave all the time: the reuse path); a 64-point spread outlier cluster beside a
tight blob (one wave wins over and over and searches its candidate again each time: the fall-back and the reset of the own mask);
a lattice with duplicated vertices (exact ties between waves and inside a bucket); NaN / +Inf / -Inf coordinates, also in point 0,
which the mask in front of the loop is taken from; a ragged batch whose small clouds (130 and 40 points: the dispatch goes by the
largest cloud of a launch, so any size is admitted beside it) leave whole waves without points; launches of one and of two samples."""
import numpy as np
import pytest
import torch

from toothgroupnetwork_amd import synth

pytestmark = pytest.mark.gpu

M = 128
MODES = [0, 2, 1]   # oracle mode: 0 = first-index ties, 2 = the reference kernel's tree tie order, 1 = FMA arithmetic (once per instance)


def _flags(mode):
    from toothgroupnetwork_amd import _lib
    return (_lib.FPS_TREE_TIES if mode & 2 else 0) | (_lib.FPS_FMA if mode & 1 else 0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _clusters(n, seed):
    rng = np.random.default_rng(seed)
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float32)
    xyz = corners[rng.integers(0, 8, size=n)] + rng.normal(scale=0.02, size=(n, 3))
    return xyz.astype(np.float32)


def _outlier(n, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.normal(scale=0.001, size=(n, 3))
    at = rng.choice(np.arange(1, n), size=64, replace=False)          # point 0 stays in the blob
    xyz[at] = 10.0 + rng.random((64, 3))
    return xyz.astype(np.float32)


def _lattice(n, seed):
    return synth.lattice_cloud(12, dup=n - 1728, seed=seed)


def _nonfinite(n, seed, first=None):
    rng = np.random.default_rng(seed)
    xyz = synth.uniform_cloud(n, seed + 1)
    at = rng.choice(np.arange(3, n * 3), size=64, replace=False)
    flat = xyz.reshape(-1)
    flat[at[:24]] = np.nan
    flat[at[24:44]] = np.inf
    flat[at[44:]] = -np.inf
    if first is not None:
        xyz[0] = first
    return xyz


def _clouds(n, seed):
    return [_clusters(n, seed), _outlier(n, seed + 1), _lattice(n, seed + 2), _nonfinite(n, seed + 3),
            _nonfinite(n, seed + 5, (np.nan, 0.1, 0.2)), _nonfinite(n, seed + 7, (np.inf, -np.inf, 0.3))]


def _check_packed(dev, oracle, clouds, ms, mode, bucket_min=-1, flags=0):
    """One launch over the packed clouds; indices against the oracle, centroids against the points the indices name."""
    from toothgroupnetwork_amd import _lib
    xyz_np = np.ascontiguousarray(np.concatenate(clouds), dtype=np.float32)
    off_np = np.cumsum([c.shape[0] for c in clouds]).astype(np.int32)
    noff_np = np.cumsum(ms).astype(np.int32)
    want = oracle.furthestsampling(xyz_np, off_np, noff_np, mode=mode)
    xyz = torch.from_numpy(xyz_np).to(dev)
    off, noff = torch.from_numpy(off_np).to(dev), torch.from_numpy(noff_np).to(dev)
    idx = torch.full((int(noff_np[-1]),), -7, dtype=torch.int32, device=dev)
    new_xyz = torch.full((int(noff_np[-1]), 3), -7.0, dtype=torch.float32, device=dev)
    n_max = max(c.shape[0] for c in clouds)
    with _lib.tuning(fps_bucket_min=bucket_min):
        _lib.check(_lib.lib().tgn_furthestsampling(len(clouds), n_max, _lib.ptr(xyz), _lib.ptr(off), _lib.ptr(noff), None, _lib.ptr(idx),
                                                   _lib.ptr(new_xyz), _flags(mode) | flags, _lib.stream()), "fps")
    got = idx.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(_bits(new_xyz.cpu().numpy()), _bits(xyz_np[want.astype(np.int64)]))


def _check_dense(dev, oracle, xyz_np, S, mode):
    """tgn_furthestsampling_dense as level 2 of the phased schedule calls it: local indices, TGN_FPS_LOW_VALU."""
    from toothgroupnetwork_amd import _lib
    B, N = xyz_np.shape[:2]
    xyz = torch.from_numpy(xyz_np).to(dev)
    idx = torch.full((B, S), -7, dtype=torch.int32, device=dev)
    new_xyz = torch.full((B, S, 3), -7.0, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().tgn_furthestsampling_dense(B, N, S, _lib.ptr(xyz), None, _lib.ptr(idx), _lib.ptr(new_xyz),
                                                     _flags(mode) | _lib.FPS_LOCAL_INDEX | _lib.FPS_LOW_VALU, _lib.stream()), "fps")
    want = oracle.farthest_point_sample(xyz_np, S, mode=mode)
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(_bits(new_xyz.cpu().numpy()), _bits(np.take_along_axis(xyz_np, want[:, :, None], axis=1)))


def _ragged(n, seed):
    return [synth.arch_cloud(n, seed, False), synth.arch_cloud(130, seed + 1, False), synth.uniform_cloud(40, seed + 2)], [M, 128, 40]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,bucket_min", [(2048, 2048), (24000, -1)])
def test_four_waves_and_level_one(dev, oracle, n, bucket_min, mode):
    """<256,8> (lane-0 hand-off record) and <512,48>: every cloud with 128 samples, then one and two samples (the mask in front of
    the loop alone), then the ragged batch."""
    clouds = _clouds(n, 90)
    _check_packed(dev, oracle, clouds + [clouds[0], clouds[4], clouds[5]], [M] * len(clouds) + [1, 2, 2], mode, bucket_min)
    _check_packed(dev, oracle, *_ragged(n, 96), mode, bucket_min)


@pytest.mark.parametrize("mode", MODES)
def test_level_two_low_valu(dev, oracle, mode):
    """<512,16> with half-empty slot sets (4096 points on eight waves), as level 2 of the headline runs it."""
    from toothgroupnetwork_amd import _lib
    xyz_np = np.stack(_clouds(4096, 100))
    for S in (M, 1, 2):
        _check_dense(dev, oracle, xyz_np, S, mode)
    _check_packed(dev, oracle, *_ragged(4096, 106), mode, flags=_lib.FPS_LOW_VALU)


def test_hotpath_step_against_the_oracle(dev, oracle):
    """One step of the phased three-stream schedule, Shape A at B = 2: <512,48> at level 1 and <512,16> low-VALU at level 2, beside
    the groupings and ball queries they run with; indices of all three levels against the oracle's chain."""
    from toothgroupnetwork_amd import hotpath
    B = 2
    shape = hotpath.SHAPE_A
    pts = torch.from_numpy(synth.scan_batch(B, shape["n"], "arch", 110)).to(dev)
    xyz = pts[:, :, :3].contiguous()
    g = torch.Generator().manual_seed(0)
    feats = [pts] + [torch.randn(B, s, d, generator=g).to(dev) for s, d in zip(shape["npoint"][:-1], shape["d"][1:])]
    hp = hotpath.HotPath(B, dev, shape=shape, pipeline=True)
    levels = hp.run(xyz, feats, more=False)
    torch.cuda.synchronize()
    cur = xyz.cpu().numpy()
    for li, (lv, S) in enumerate(zip(levels, shape["npoint"])):
        want = oracle.farthest_point_sample(cur, S)
        assert np.array_equal(lv["fps_idx"].cpu().numpy().astype(np.int64), want), f"level {li + 1}"
        cur = oracle.index_points(cur, want)
        assert np.array_equal(_bits(lv["new_xyz"].cpu().numpy()), _bits(cur)), f"level {li + 1}"
