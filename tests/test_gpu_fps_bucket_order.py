"""GPU: fps_bucket_kernel deals its buckets out along a Hilbert curve over the cloud's 16^3 grid cells.  The order decides only which
bucket a point lands in, never a result: indices and centroids equal the oracle's bit for bit in the default and the tree tie
mode, at every instance the dispatch can reach (at its capacity and with a last bucket of one point), on clouds where the cell
code collapses, and on one confined to a single cell column, where the curve reverses direction from cell to cell."""
import numpy as np
import pytest
import torch

from toothgroupnetwork_amd import synth

pytestmark = pytest.mark.gpu

M = 128
MODES = [0, 2]      # oracle mode: 0 = first-index ties (default), 2 = the reference kernel's tree tie order


def _flags(mode):
    from toothgroupnetwork_amd import _lib
    return _lib.FPS_TREE_TIES if mode & 2 else 0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _check_packed(dev, oracle, clouds, ms, mode, bucket_min=-1):
    """One launch over the packed clouds; indices against the oracle, centroids against the points the indices name."""
    from toothgroupnetwork_amd import _lib
    xyz_np = np.ascontiguousarray(np.concatenate(clouds), dtype=np.float32)
    off_np = np.cumsum([c.shape[0] for c in clouds]).astype(np.int32)
    noff_np = np.cumsum(ms).astype(np.int32)
    want = oracle.furthestsampling(xyz_np, off_np, noff_np, mode=mode)      # what oracle.farthest_point_sample calls per batch
    xyz = torch.from_numpy(xyz_np).to(dev)
    off, noff = torch.from_numpy(off_np).to(dev), torch.from_numpy(noff_np).to(dev)
    idx = torch.full((int(noff_np[-1]),), -7, dtype=torch.int32, device=dev)
    new_xyz = torch.full((int(noff_np[-1]), 3), -7.0, dtype=torch.float32, device=dev)
    n_max = max(c.shape[0] for c in clouds)
    with _lib.tuning(fps_bucket_min=bucket_min):
        _lib.check(_lib.lib().tgn_furthestsampling(len(clouds), n_max, _lib.ptr(xyz), _lib.ptr(off), _lib.ptr(noff), None, _lib.ptr(idx),
                                                   _lib.ptr(new_xyz), _flags(mode), _lib.stream()), "fps")
    got = idx.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(_bits(new_xyz.cpu().numpy()), _bits(xyz_np[want.astype(np.int64)]))


# n_max -> instance (bucket_launch_mode: the smallest capacity NT * P that holds n_max; bucket kernel from 4097 points, from
# fps_bucket_min when that is set): 2048 <256,8> and 4096 <256,16> (both reachable through fps_bucket_min only), 4097 / 8129 /
# 8192 <512,16>, 12 288 <512,24>, 16 321 <512,32>, 24 000 / 24 576 <512,48>, 28 672 <512,56>
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_max,bucket_min", [(2048, 2048), (4096, 2048), (4097, -1), (8129, -1), (8192, -1), (12288, -1), (16321, -1),
                                              (24000, -1), (24576, -1), (28672, -1)])
def test_every_instance_at_capacity_and_one_point_into_a_bucket_ragged(dev, oracle, n_max, bucket_min, mode):
    small = 2048 if bucket_min > 0 else 4097
    clouds = [synth.arch_cloud(n_max, 60, False), synth.uniform_cloud(max(small, (2 * n_max) // 3 | 1), 61),
              synth.lattice_cloud(12, dup=max(small, n_max // 2 + 1) - 1728, seed=62)]          # exact ties, duplicated vertices
    _check_packed(dev, oracle, clouds, [M, M, M], mode, bucket_min)


@pytest.mark.parametrize("mode", MODES)
def test_level_two_of_the_headline_through_the_low_valu_path(dev, oracle, mode):
    """4096 -> 64 with TGN_FPS_LOW_VALU: fps_bucket_kernel<512,16> with half-empty slot sets."""
    from toothgroupnetwork_amd import _lib
    xyz_np = np.stack([synth.arch_cloud(4096, s, False) for s in (70, 71, 72)])
    xyz = torch.from_numpy(xyz_np).to(dev)
    idx = torch.full((3, 64), -7, dtype=torch.int32, device=dev)
    new_xyz = torch.full((3, 64, 3), -7.0, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().tgn_furthestsampling_dense(3, 4096, 64, _lib.ptr(xyz), None, _lib.ptr(idx), _lib.ptr(new_xyz),
                                                     _flags(mode) | _lib.FPS_LOCAL_INDEX | _lib.FPS_LOW_VALU, _lib.stream()), "fps")
    want = oracle.farthest_point_sample(xyz_np, 64, mode=mode)
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(_bits(new_xyz.cpu().numpy()), _bits(np.take_along_axis(xyz_np, want[:, :, None], axis=1)))


def _degenerate(kind):
    n = 5000
    rng = np.random.default_rng(80)
    xyz = synth.uniform_cloud(n, 81)
    if kind == "plane":             # one gscale is 0
        xyz[:, 1] = np.float32(0.25)
    elif kind == "line":
        xyz[:, 0] = np.float32(-0.5)
        xyz[:, 2] = np.float32(0.125)
    elif kind == "identical":
        xyz[:] = np.array([0.3, -0.7, 0.9], dtype=np.float32)
    elif kind == "thin":            # one axis spanning 1e-30: a finite, huge gscale
        xyz[:, 2] = (rng.random(n) * 1e-30).astype(np.float32)
    elif kind == "duplicates":      # half of the points are exact copies of the other half
        xyz[n // 2:] = xyz[:n // 2]
    elif kind == "nonfinite":       # 64 coordinates NaN / +Inf / -Inf
        at = rng.choice(n * 3, size=64, replace=False)
        flat = xyz.reshape(-1)
        flat[at[:24]] = np.nan
        flat[at[24:44]] = np.inf
        flat[at[44:]] = -np.inf
    elif kind == "column":          # x and y inside ONE cell, z spread over all 16; two corner points pin the bounding box
        xyz[:, 0] = (0.05 + 0.05 * rng.random(n)).astype(np.float32)
        xyz[:, 1] = (-0.45 + 0.05 * rng.random(n)).astype(np.float32)
        xyz[0], xyz[1] = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    else:
        raise ValueError(kind)
    return xyz


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["plane", "line", "identical", "thin", "duplicates", "nonfinite", "column"])
def test_clouds_where_the_cell_code_collapses(dev, oracle, kind, mode):
    _check_packed(dev, oracle, [_degenerate(kind)], [M], mode)
