"""GPU: the kernels of crop.hip, loss.hip, edgeconv.hip, cbl.hip, tsegnet.hip, metrics.hip, subdivide.hip and linear_max.hip at the sizes
on both sides of their internal constants (docs/KERNEL_SEAMS.md lists every constant, the sizes around it and the test that runs each
size).

Nothing here has a reference or a tolerance of its own.  Every test builds an input that lands on a seam and hands it to the check
the kernel's own test file uses:
  tgn_crop_knn          np.lexsort((index, float64 rdist)) of test_gpu_tooth_crops.py, bit equality; coordinates on a 1/16 grid (or as
                        stated) so that float64 distances tie exactly
  tgn_label_centroids   the sequential float32 sum of test_gpu_tooth_crops.py, bit equality
  tgn_offset_loss_*, tgn_centroid_loss_*   losses_ref's float64 restatement under _check_loss / _check_grad of test_gpu_losses.py
  tgn_edgeconv{1,2}_max edge_level64 under chain_const of test_gpu_dgcnn_edgeconv.py
  tgn_feature_knn       _check_contract of test_gpu_dgcnn_knn.py, bit equality
  tgn_cbl_stage_*       cbl_ref's float64 stage under cbl_cases' bounds, as test_gpu_losses_cbl_fused.py
  tgn_subdivide_midpoint  subdivide_ref.subdivide_loop, bit equality
  tsegnet.hip, linear_max.hip   the parametrised cases of test_gpu_tsegnet.py and test_gpu_linear_max.py, called at more sizes
  tgn_seg_confusion_logits      torch.argmax + tgn_seg_confusion and metrics_ref.tables, equality, as test_gpu_metrics.py"""
import numpy as np
import pytest
import torch

import losses_ref as R
import subdivide_ref as S
from test_gpu_dgcnn_edgeconv import U_RND, _layers, chain_const, edge_level64
from test_gpu_dgcnn_knn import _check_contract
from test_gpu_losses import TGN_NAMES, TSG_NAMES, _check_grad, _check_loss, _run_tgn, _run_tsg, _term_grads, tgn_inputs, tsg_inputs
from test_gpu_losses_cbl_fused import CC, _exact_lists, _gpu_lists, _lists_case, _touched, cbl_ref
from test_gpu_tooth_crops import np_centroids, np_knn

pytestmark = pytest.mark.gpu


# ---- tgn_crop_knn: 1024 threads, compaction chunks of 1024 points, waves of 64, radix digits 11,11,11,11,11,9, k <= 4096 ---------------

def _crop_knn(dev, clouds, scan, cents, k):
    """clouds (B, n, 3) float32, scan (T,) the cloud of every centre, cents (T, 3) -> (T, k) int64 through the package's one launch"""
    from toothgroupnetwork_amd import crops
    feats = torch.from_numpy(np.ascontiguousarray(np.asarray(clouds, np.float32).transpose(0, 2, 1))).to(dev)
    idx = crops.crop_knn(feats, torch.from_numpy(np.asarray(scan, np.int32)).to(dev),
                         torch.from_numpy(np.ascontiguousarray(cents, dtype=np.float32)).to(dev), k)
    return idx.cpu().numpy()


def _check_crop_knn(dev, clouds, scan, cents, k):
    clouds, cents = np.asarray(clouds, np.float32), np.asarray(cents, np.float32)
    got = _crop_knn(dev, clouds, scan, cents, k)
    assert got.shape == (len(scan), k) and got.dtype == np.int64
    want = {}
    for t, b in enumerate(scan):
        key = (int(b), cents[t].tobytes())
        if key not in want:
            want[key] = np_knn(clouds[b], cents[t], k)
        assert np.array_equal(got[t], want[key]), (t, int(b), k)
    return got


def _grid_cloud(n, seed):
    return (np.random.default_rng(seed).integers(-64, 65, (n, 3)) / 16.0).astype(np.float32)


CROP_SIZES = [(n, k) for n in (1, 1023, 1024, 1025, 3000) for k in sorted({1, 2, 1023, 1024, 1025, n}) if k <= min(n, 4096)]


@pytest.mark.parametrize("n,k", CROP_SIZES)
def test_crop_knn_around_the_chunk_of_1024(dev, n, k):
    xyz = _grid_cloud(n, seed=n)
    cents = np.stack([np.zeros(3, np.float32), xyz[n // 2], np.array([9.0, -7.5, 8.25], np.float32)])
    _check_crop_knn(dev, xyz[None], [0, 0, 0], cents, k)


@pytest.mark.parametrize("n,k", [(1, 1), (1025, 1), (1025, 1025), (3000, 70), (3000, 3000), (5000, 4096)])
def test_crop_knn_of_identical_points_is_the_first_k_indices(dev, n, k):
    """nless = 0 and need_eq = k: every slot is filled by the tie prefix"""
    xyz = np.tile(np.array([[0.25, -1.5, 0.75]], np.float32), (n, 1))
    got = _check_crop_knn(dev, xyz[None], [0, 0], np.array([[0.25, -1.5, 0.75], [1.0, 1.0, 1.0]], np.float32), k)
    assert np.array_equal(got, np.tile(np.arange(k), (2, 1)))


_LATTICE = np.stack(np.meshgrid(*[np.arange(-5, 6)] * 3, indexing="ij"), -1).reshape(-1, 3)
_NORM2 = (_LATTICE ** 2).sum(1)
INSIDE, SHELL = _LATTICE[_NORM2 < 25], _LATTICE[_NORM2 == 25]         # 30 distinct points at squared distance 25 / 256 exactly


def _shell_cloud(n, less_at, tie_at, seed):
    """A cloud about the origin: the points at indices less_at lie inside the shell |p|^2 = 25 / 256, those at tie_at on it (distinct
    points while there are at most 30), every other one outside."""
    rng = np.random.default_rng(seed)
    xyz = rng.integers(-64, 65, (n, 3))
    near = (xyz ** 2).sum(1) <= 25
    xyz[near, 0] = 6 + np.abs(xyz[near, 0])
    xyz[less_at] = INSIDE[rng.integers(0, len(INSIDE), len(less_at))]
    xyz[tie_at] = SHELL[np.arange(len(tie_at)) % len(SHELL)]
    return (xyz / 16.0).astype(np.float32)


@pytest.mark.parametrize("first,boundary", [(58, 64), (1018, 1024)], ids=["wave-64", "chunk-1024"])
@pytest.mark.parametrize("need", [1, 7, 9, 14])
def test_crop_knn_tie_group_across_a_boundary_keeps_the_lowest_indices(dev, first, boundary, need):
    n, nless = 3000, 40
    tie_at = np.arange(first, first + 15)                               # 58..72 or 1018..1032
    rest = np.setdiff1d(np.arange(n), tie_at)
    less_at = np.random.default_rng(first).choice(rest, nless, replace=False)
    xyz = _shell_cloud(n, less_at, tie_at, seed=first + need)
    got = _check_crop_knn(dev, xyz[None], [0], np.zeros((1, 3), np.float32), nless + need)
    assert tie_at[0] < boundary <= tie_at[-1] and np.array_equal(np.sort(got[0, nless:]), tie_at[:need])


def _exit_clouds(n, nless):
    """(ties first, count first): in the first the threshold point sits at index 0 (a second copy of its distance at index 1) and every
    smaller key at an index >= 2048, so the tie condition holds two chunks before the count condition; the second is the mirror:
    the smaller keys all below index 1024, the threshold points at 2500 and 2600."""
    rng = np.random.default_rng(n + nless)
    ties_first = _shell_cloud(n, 2048 + rng.choice(n - 2048, nless, replace=False), np.array([0, 1]), seed=n + 1)
    count_first = _shell_cloud(n, rng.choice(1024, nless, replace=False), np.array([2500, 2600]), seed=n + 2)
    return np.stack([ties_first, count_first])


@pytest.mark.parametrize("nless", [40, 1000])
def test_crop_knn_exit_conditions_met_in_different_chunks(dev, nless):
    """The compaction loop leaves when the ties AND the smaller keys are all placed; here one holds chunks before the other."""
    clouds = _exit_clouds(3500, nless)
    got = _check_crop_knn(dev, clouds, [0, 1], np.zeros((2, 3), np.float32), nless + 1)
    assert got[0, -1] == 0 and got[1, -1] == 2500


def test_crop_knn_exit_conditions_in_the_vote_regime(dev):
    """k = 10 and 320 queries in one launch, as cluster.py's noise vote runs the kernel: one workgroup per query"""
    clouds = _exit_clouds(3200, 9)
    scan = np.arange(320) % 2
    got = _check_crop_knn(dev, clouds, scan, np.zeros((320, 3), np.float32), 10)
    assert (got[0::2, -1] == 0).all() and (got[1::2, -1] == 2500).all()


def test_crop_knn_leaves_after_the_first_chunk_of_a_large_cloud(dev):
    n, nless = 100000, 300
    less_at = np.random.default_rng(5).choice(1000, nless, replace=False)
    tie_at = np.setdiff1d(np.arange(1000), less_at)[:3]
    xyz = _shell_cloud(n, less_at, tie_at, seed=6)
    got = _check_crop_knn(dev, xyz[None], [0], np.zeros((1, 3), np.float32), nless + 2)
    assert got.max() < 1000


@pytest.mark.parametrize("k", [1, 7, 23])
def test_crop_knn_when_only_the_last_radix_digit_decides(dev, k):
    """Points (1, j 2^-26, 0), j = 0..22, about the origin: their float64 keys are 1 + j^2 2^-52 exactly (j^2 < 2^9), equal in the top
    55 bits, so the five 11-bit passes see one bin and the 9-bit pass alone orders them."""
    n = 1500
    rng = np.random.default_rng(26)
    xyz = _grid_cloud(n, seed=27)
    xyz[(xyz.astype(np.float64) ** 2).sum(1) < 2.0] += np.float32(3.0)
    at = rng.choice(n, 23, replace=False)                               # shuffled index order
    j = rng.permutation(23)
    xyz[at] = np.stack([np.ones(23), j * 2.0 ** -26, np.zeros(23)], 1).astype(np.float32)
    d = (xyz[at].astype(np.float64) ** 2).sum(1)
    assert np.array_equal(d, 1.0 + (j.astype(np.float64) ** 2) * 2.0 ** -52) and np.unique(d.view(np.int64) >> 9).size == 1
    got = _check_crop_knn(dev, xyz[None], [0], np.zeros((1, 3), np.float32), k)
    assert np.array_equal(got[0], at[np.argsort(j)][:k])


# ---- tgn_label_centroids: chunks of 1024 points, at most 64 labels (3 summing lanes per label) ------------------------------------------

def _check_centroids(dev, xyz, lab, nlab, f64_sum=False):
    """f64_sum (tgn_label_centroids_f64): the float64 sum in point order (np.cumsum adds one by one), divided and rounded once"""
    from toothgroupnetwork_amd import crops
    feats = torch.from_numpy(np.ascontiguousarray(xyz.T))[None].to(dev)
    counts, cent = crops.label_centroids(feats, torch.from_numpy(lab.astype(np.int64))[None].to(dev), nlab, f64_sum=f64_sum)
    counts, cent = counts.cpu().numpy()[0], cent.cpu().numpy()[0]
    if f64_sum:
        want = {t: (np.cumsum(xyz[lab == t].astype(np.float64), axis=0)[-1] / float((lab == t).sum())).astype(np.float32)
                for t in range(nlab) if (lab == t).any()}
    else:
        want = np_centroids(xyz, lab)
    for t in range(nlab):
        if t in want:
            assert counts[t] == int((lab == t).sum()) and np.array_equal(cent[t].view(np.uint32), want[t].view(np.uint32)), t
        else:
            assert counts[t] == 0 and np.isnan(cent[t]).all(), t
    return counts


def _centroid_case(n, nlab, seed):
    rng = np.random.default_rng(seed)
    xyz = (rng.random((n, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
    lab = rng.integers(-1, nlab, n)
    return xyz, lab


@pytest.mark.parametrize("f64_sum", [False, True], ids=["f32-sum", "f64-sum"])
@pytest.mark.parametrize("nlab", [1, 16, 17, 64])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_label_centroids_around_the_chunk_of_1024(dev, n, nlab, f64_sum):
    xyz, lab = _centroid_case(n, nlab, seed=100 * n + nlab)
    tail = (n - 1) // 1024 * 1024                                       # first index of the last, partial or full, chunk
    if nlab >= 4:
        lab[lab == 1] = 2                                               # an absent label: NaN centroid, count 0
        lab[:tail][lab[:tail] == nlab - 1] = 2                          # a label present in the last chunk only
        lab[n - 1] = nlab - 1
    if n >= 2048:
        lab[1024:2048] = 0                                              # one label owns every point of a full chunk
    counts = _check_centroids(dev, xyz, lab, nlab, f64_sum)
    if nlab >= 4:
        assert counts[1] == 0 and counts[nlab - 1] >= 1


@pytest.mark.parametrize("f64_sum", [False, True], ids=["f32-sum", "f64-sum"])
@pytest.mark.parametrize("n", [1024, 1025])
def test_label_centroids_one_label_owns_the_full_chunk(dev, n, f64_sum):
    xyz, lab = _centroid_case(n, 16, seed=n)
    lab[:1024] = 7
    lab[1024:] = 15
    assert _check_centroids(dev, xyz, lab, 16, f64_sum)[7] == 1024


@pytest.mark.parametrize("f64_sum", [False, True], ids=["f32-sum", "f64-sum"])
@pytest.mark.parametrize("n", [1, 1025])
def test_label_centroids_of_gingiva_alone(dev, n, f64_sum):
    xyz, _ = _centroid_case(n, 16, seed=n)
    assert not _check_centroids(dev, xyz, np.full(n, -1), 16, f64_sum).any()


# ---- tgn_offset_loss_*: 256 points per block, the forward's grid capped at 128 blocks (32 768 points), the backward's at 1024 ----------

def _offset_case(B, n, seed):
    """tgn_inputs with the points reordered: one valid tooth (label 0) and a tooth of three points (label 15, taken from the gingiva)
    come last.  Above 65 536 points tooth 0 is last, so that all its points lie beyond index 32 768; below, the three points are, so
    that at n = 32 769 the forward's second grid-stride pass holds a point of a tooth that is skipped.  The few moved points whose
    two nearest valid centroids are almost equally far are re-aimed at the nearer one (the centroids depend on xyz alone)."""
    off, xyz, lab = tgn_inputs(B, n, seed)
    for b in range(B):
        lab[b, torch.nonzero(lab[b] == -1)[:3, 0]] = 15
        small, big = torch.nonzero(lab[b] == 15)[:, 0], torch.nonzero(lab[b] == 0)[:, 0]
        keep = torch.nonzero((lab[b] != 15) & (lab[b] != 0))[:, 0]
        order = torch.cat([keep, small, big] if n > 65536 else [keep, big, small])
        off[b], xyz[b], lab[b] = off[b][:, order], xyz[b][:, order], lab[b][order]
        if n > 65536:
            assert int(torch.nonzero(lab[b] == 0).min()) > 32768 and int((lab[b] == 0).sum()) >= 5
        p, o = xyz[b].double().t(), off[b].double().t()
        one_hot = lab[b][:, None] == torch.arange(16)
        n_t = one_hot.sum(0)
        cent = (one_hot.double().t() @ p) / n_t.clamp_min(1)[:, None]
        d2 = (((p + o)[:, None, :] - cent[None, n_t >= 5]) ** 2).sum(-1)
        two, arg = d2.topk(2, dim=1, largest=False)
        fix = (lab[b] >= 0) & ((two[:, 1] - two[:, 0]) / two[:, 1] < 1e-3)
        target = cent[n_t >= 5][arg[:, 0]]
        off[b][:, fix] = (0.9 * (target - p))[fix].t().float()
    return off, xyz, lab


def _check_offset_terms(dev, B, n, seed):
    off, xyz, lab = _offset_case(B, n, seed)
    mg = R.tgn_margins(off, xyz, lab)
    assert mg["norm"] >= 5e-5 and mg["ratio_gap"] >= 1e-4 and not bool(((mg["counts"] >= 4) & (mg["counts"] <= 6)).any()), mg
    assert bool((mg["counts"][:, 15] == 3).all())                      # the tooth with fewer than 5 points
    vals, grads = _run_tgn(dev, off, xyz, lab)
    o64 = off.double().requires_grad_()
    exact = R.tgn_terms(o64, xyz.double(), lab)
    exact_g = _term_grads(exact, o64)
    print(f"\ntgn B = {B}, N = {n}:")
    for i, name in enumerate(TGN_NAMES):
        _check_loss(name, vals[i], float(exact[i].detach()))
        _check_grad(name, grads[i], exact_g[i])
    assert not np.transpose(grads[:2], (0, 1, 3, 2))[:, lab.numpy() == 15].any()    # a skipped tooth: no offset or direction gradient


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("n", [32767, 32768, 32769, 65537])
def test_offset_loss_around_the_forward_grid_cap(dev, B, n):
    _check_offset_terms(dev, B, n, seed=700 + n + B)


def test_offset_loss_above_the_backward_grid_cap(dev):
    _check_offset_terms(dev, 1, 262145, seed=262)


# ---- tgn_centroid_loss_*: one block of 256 threads per scan strides over the points; the reverse argmin is a packed (distance, index) --

def _check_centroid_terms(dev, off, xyz, dist, cent):
    B, _, M = off.shape
    vals, g_off, g_dist = _run_tsg(dev, off, xyz, dist, cent)
    o64, d64 = off.double().requires_grad_(), dist.double().view(B, M).requires_grad_()
    exact = R.centroid_terms(o64, xyz.double(), d64, cent.double())
    for i, name in enumerate(TSG_NAMES):
        _check_loss(name, vals[i], float(exact[i].detach()))
    eg = _term_grads(exact, o64)
    for i, name in enumerate(TSG_NAMES):
        _check_grad(f"{name} / offset", g_off[i], eg[i])
    _check_grad("dist_loss / distance", g_dist[0].reshape(B, M), _term_grads(exact[:1], d64)[0])
    return g_off, eg


@pytest.mark.parametrize("M", [255, 256, 257, 513])
def test_centroid_loss_around_the_stride_of_256(dev, M):
    for seed in range(3000 + M, 4000 + M):              # the first seed whose inputs keep their margins (host arithmetic only)
        off, xyz, dist, cent = tsg_inputs(2, M, 16, seed)
        mg = R.centroid_margins(off, xyz, dist.view(2, M), cent)
        if mg["mask"] >= 1e-3 and mg["ratio_gap"] >= 1e-4 and mg["arg_gap"] >= 1e-4:
            break
    else:
        raise AssertionError("no seed keeps the margins")
    print(f"\ntsg B = 2, M = {M}, C = 16 (seed {seed}):")
    _check_centroid_terms(dev, off, xyz, dist, cent)


@pytest.mark.parametrize("lo,hi", [(10, 200), (10, 266), (10, 300), (255, 256)],
                         ids=["same-pass", "same-thread-next-pass", "next-pass", "last-and-first-thread"])
def test_centroid_loss_reverse_gradient_goes_to_the_lower_of_two_equal_points(dev, lo, hi):
    """The point nearest to centroid 0 exists twice, at indices lo and hi: in the same 256-stride pass, or in different ones.  The
    reverse term's argmin is the lower index (torch's min returns the first of equal values, too), and it takes the whole gradient."""
    M, C = 513, 5
    for seed in range(4000 + hi, 5000 + hi):
        off, xyz, dist, cent = tsg_inputs(1, M, C, seed)
        for j in (lo, hi):
            xyz[0, :, j] = cent[0, :, 0] + torch.tensor([0.001, 0.002, -0.001])
            off[0, :, j] = torch.tensor([0.0003, -0.0002, 0.0001])
            dist[0, 0, j] = 0.05
        mg = R.centroid_margins(off, xyz, dist.view(1, M), cent)
        d2 = (((xyz + off)[0].double().t()[:, None, :] - cent[0].double().t()[None, :, :]) ** 2).sum(-1)     # (M, C)
        srt, arg = d2.sort(dim=0)
        others = bool((((srt[1, 1:] - srt[0, 1:]) / srt[1, 1:]) >= 1e-4).all())
        tie = sorted(arg[:2, 0].tolist()) == [lo, hi] and float(srt[0, 0]) == float(srt[1, 0]) and float(srt[2, 0]) > 1.01 * float(srt[0, 0])
        if mg["mask"] >= 1e-3 and mg["ratio_gap"] >= 1e-4 and others and tie:
            break
    else:
        raise AssertionError("no seed keeps the margins")
    print(f"\ntsg duplicated nearest point at {lo} and {hi} (seed {seed}):")
    g_off, eg = _check_centroid_terms(dev, off, xyz, dist, cent)
    rev, rev64 = g_off[1][0, :, lo] - g_off[1][0, :, hi], eg[1][0, :, lo] - eg[1][0, :, hi]    # the two differ by the reverse term alone
    assert np.abs(rev64).max() > 0 and np.abs(rev - rev64).max() <= 2e-5 * np.abs(eg[1]).max()    # two entries, each within 1e-5 max|exact|
    assert np.sign(rev).tolist() == np.sign(rev64).tolist()


# ---- tgn_edgeconv{2,1}_max: one wave per query, 4 waves per block, at most 2048 blocks (8192 waves, grid-stride beyond), K <= 32 ------

def _check_edgeconv(dev, x, idx, C, two, seed, coff=None):
    from toothgroupnetwork_amd import dgcnn
    B, _, N = x.shape
    conv1, bn1, conv2, bn2 = _layers(C, dev, seed=seed)
    first = dgcnn._edge_first_layer(conv1, bn1)
    second = dgcnn._second_layer(conv2, bn2) if two else None
    x, idx = x.to(dev), idx.to(dev)
    if coff is None:
        got = dgcnn.edgeconv_max(x, idx, first, second)
    else:
        out = torch.full((B, 192, N), float("nan"), device=dev)
        dgcnn.edgeconv_max(x, idx, first, second, out=out, coff=coff)
        got = out[:, coff:coff + 64]
        assert torch.isnan(out[:, :coff]).all() and torch.isnan(out[:, coff + 64:]).all()     # only its channel slice is written
    want, M, n = edge_level64(x, idx, conv1, bn1, *((conv2, bn2) if two else ()))
    ratio = ((got.double() - want).abs() / (U_RND * M)).max().item()
    print(f"\nedgeconv B={B} N={N} C={C} K={idx.shape[-1]} two={two}: worst |got - want| / (u M) = {ratio:.2f} (bound {chain_const(n):.1f})")
    assert ratio <= chain_const(n)
    return want, (conv1, bn1, conv2, bn2)


@pytest.mark.parametrize("two", [True, False], ids=["edgeconv2", "edgeconv1"])
@pytest.mark.parametrize("B,N", [(1, 1), (1, 3), (3, 1), (1, 4), (1, 5), (1, 8191), (1, 8192), (1, 8193), (3, 2731)])
def test_edgeconv_around_one_block_and_the_grid_cap(dev, B, N, two):
    """B N = 1, 3: one block with idle waves; 4, 5: a full block, and a second one; 8191 .. 8193: the cap of 8192 waves, after which a
    wave takes a second query.  B = 3 holds different data per scan, so a neighbour read from another scan shows."""
    g = torch.Generator().manual_seed(B * 10000 + N)
    K = min(N, 20) if N > 1 else 3                                      # (N = 1: three copies of the one point)
    x = torch.randn(B, 6, N, generator=g)
    idx = torch.randint(0, N, (B, N, K), generator=g)
    _check_edgeconv(dev, x, idx, 6, two, seed=N)


def _planted_rows(B, N, K, C, seed):
    """x and idx with K distinct neighbours per row out of the points 0 .. N-3, except that every row's LAST slot names point N-2, whose
    features are 8 times a unit-variance draw: its first-layer pre-activation is the largest of the row in about every second channel."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, N, generator=g)
    x[:, :, N - 2] *= 8.0
    idx = torch.rand(B, N, N - 2, generator=g).argsort(-1)[..., :K].contiguous()
    idx[..., K - 1] = N - 2
    assert all(idx[..., s].ne(idx[..., t]).all() for s in range(K) for t in range(s))
    return x, idx


@pytest.mark.parametrize("two", [True, False], ids=["edgeconv2", "edgeconv1"])
@pytest.mark.parametrize("K", [1, 2, 31, 32])
def test_edgeconv_every_slot_distinct_with_the_largest_in_the_last(dev, K, two):
    B, N, C = 2, 300, 64
    x, idx = _planted_rows(B, N, K, C, seed=K)
    if K == 31:
        # a row of 31 ends one slot before the next row begins: a point larger than every other, named only as the FIRST neighbour of
        # the odd rows, must not reach the even rows' outputs (a kernel that read 32 slots of a row would take it in)
        x[:, :, N - 1] *= 64.0
        idx[:, 1::2, 0] = N - 1
        assert not (idx[:, 0::2] == N - 1).any()
    want, layers = _check_edgeconv(dev, x, idx, C, two, seed=K + 40)
    if K > 1:                                                           # the last slot decides a good part of the outputs
        fewer = idx.clone()
        fewer[..., K - 1] = fewer[..., 0]
        without = edge_level64(x.to(dev), fewer.to(dev), layers[0], layers[1], *(layers[2:] if two else ()))[0]
        assert (want > without).float().mean().item() >= 0.2
    if K == 31:
        even = idx.clone()
        even[:, 0::2, 30] = N - 1                                       # what reading one slot too many would have computed
        leaked = edge_level64(x.to(dev), even.to(dev), layers[0], layers[1], *(layers[2:] if two else ()))[0]
        assert (leaked[:, :, 0::2] > want[:, :, 0::2]).float().mean().item() >= 0.2


@pytest.mark.parametrize("two", [True, False], ids=["edgeconv2", "edgeconv1"])
@pytest.mark.parametrize("coff", [0, 64, 128])
def test_edgeconv_writes_its_channel_slice_only(dev, coff, two):
    g = torch.Generator().manual_seed(coff + 1)
    x = torch.randn(2, 6, 257, generator=g)
    idx = torch.randint(0, 257, (2, 257, 20), generator=g)
    _check_edgeconv(dev, x, idx, 6, two, seed=coff, coff=coff)


# ---- tgn_feature_knn: 256 queries per block, candidate tiles of 128, splits of the candidate range (at most 16, at least 512 long) -----

def _splits(B, N):
    """knn_splits and knn_chunk of csrc/edgeconv.hip, restated: (S, chunk, length of the last split)"""
    tiles = B * ((N + 255) // 256)
    s = max(1, min(16, (1024 + tiles - 1) // tiles, (N + 511) // 512))
    chunk = ((N + s - 1) // s + 1) & ~1
    return s, chunk, N - (s - 1) * chunk


# (B, N, D, k), what the case is for, (S, chunk, last split) worked out by hand from knn_splits / knn_chunk
KNN_CASES = [
    ((1, 1, 1, 1), "N=k=1", (1, 2, 1)),
    ((1, 32, 4, 32), "N=k=32", (1, 32, 32)),
    ((5, 17, 5, 17), "N=k=17-B5", (1, 18, 17)),
    ((1, 255, 8, 8), "S1-below-a-query-block", (1, 256, 255)),
    ((5, 256, 9, 9), "S1-one-query-block-B5", (1, 256, 256)),
    ((1, 257, 16, 16), "S1-two-query-blocks", (1, 258, 257)),
    ((1, 511, 17, 17), "S1-odd-tail", (1, 512, 511)),
    ((1, 513, 32, 32), "S2-odd-chunk-257-rounded-to-258-odd-last-split-255", (2, 258, 255)),
    ((5, 513, 33, 1), "S2-B5-odd-chunk-rounded", (2, 258, 255)),
    ((1, 1001, 64, 8), "S2-odd-chunk-501-rounded-to-502-odd-last-split-499", (2, 502, 499)),
    ((5, 1001, 1, 9), "S2-B5-D1", (2, 502, 499)),
    ((1, 1025, 4, 16), "S3-even-chunk-342-odd-last-split-341", (3, 342, 341)),
    ((1, 2049, 5, 17), "S5-even-chunk-410-odd-last-split-409", (5, 410, 409)),
    ((5, 2049, 8, 32), "S5-B5", (5, 410, 409)),
    ((1, 7681, 4, 8), "S16-odd-chunk-481-rounded-to-482-odd-last-split-451", (16, 482, 451)),
]


@pytest.mark.parametrize("shape,what,split", KNN_CASES, ids=[f"{s[0]}x{s[1]}-D{s[2]}-k{s[3]}-{w}" for s, w, _ in KNN_CASES])
def test_feature_knn_at_its_split_and_tile_seams(dev, shape, what, split):
    B, N, D, k = shape
    assert _splits(B, N) == split
    x = torch.randn(B, D, N, generator=torch.Generator().manual_seed(N + D + k))
    _check_contract(x.to(dev), k)


def test_the_feature_knn_cases_cover_every_seam():
    """host arithmetic only: the case list holds what it is there for"""
    seen = [(B, N) + _splits(B, N) for (B, N, _, _), _, _ in KNN_CASES]
    assert {1, 2, 16} <= {s for _, _, s, _, _ in seen}
    assert any(s > 1 and ((N + s - 1) // s) % 2 for _, N, s, _, _ in seen)          # an odd chunk, rounded up to even
    assert any(s > 1 and last % 2 for _, _, s, _, last in seen)                     # an odd-length last split
    assert {N for _, N, _, _, _ in seen} >= {255, 256, 257, 511, 513, 1001, 1025, 2049} and {B for B, _, _, _, _ in seen} == {1, 5}
    assert {c[0][2] for c in KNN_CASES} >= {1, 4, 5, 8, 9, 16, 17, 32, 33, 64} and {c[0][3] for c in KNN_CASES} >= {1, 8, 9, 16, 17, 32}


def test_feature_knn_ties_across_splits_resolve_by_index(dev):
    """N = 1025 runs as three splits of 342, 342 and 341 candidates.  Points 700 .. 1024 are copies of points 0 .. 324, so every such
    pair ties at every query with one copy in the first split and the other in the third: the merge must put the lower index first."""
    assert _splits(1, 1025) == (3, 342, 341)
    x = torch.randn(1, 3, 1025, generator=torch.Generator().manual_seed(77))
    x[:, :, 700:] = x[:, :, :325]
    idx, dist = _check_contract(x.to(dev), 16)
    assert (dist[0, :325, :2] == 0).all() and torch.equal(idx[0, :325, 0], torch.arange(325, device=dev))
    assert torch.equal(idx[0, :325, 1], torch.arange(700, 1025, device=dev)) and torch.equal(idx[0, 700:, :2], idx[0, :325, :2])


# ---- tgn_cbl_stage_backward: LP = 1, 2, 4, 8, 16, 32 lanes per point (the power of two holding c / 4), 256 / LP points per block --------

CBL_LP = [(c, lp, 256 // lp + d) for c, lp in ((4, 1), (8, 2), (12, 4), (16, 4), (20, 8), (32, 8), (36, 16), (64, 16), (68, 32), (128, 32))
          for d in (-1, 0, 1)]


@pytest.mark.parametrize("c,lp,m", CBL_LP, ids=[f"c{c}-LP{lp}-m{m}" for c, lp, m in CBL_LP])
def test_cbl_stage_around_a_block_of_every_lanes_per_point(dev, c, lp, m):
    """m = 256 / LP - 1, 256 / LP, 256 / LP + 1: one block not full, full, and a second block of one point; c / 4 below LP leaves lanes idle"""
    assert lp // 2 < c // 4 <= lp
    f, idx, labels = _lists_case("random", m, 6, c)
    s = _exact_lists(f, idx, labels)
    loss, count, g = _gpu_lists(f, idx, labels, dev)
    assert int(count) == s["count"] and int(count) > 0
    g = g.double().cpu().numpy()
    g64, scale = s["grad"]()
    lu = cbl_ref.loss_units(float(loss), float(s["loss"].detach()), s["loss_scale"])
    gu = cbl_ref.grad_units(g, g64, scale)
    print(f"  cbl c={c} LP={lp} m={m}: loss {lu:.3f} units (bound {CC.LOSS_BOUND:g}); gradient {gu:.2f} units (bound {CC.GRAD_BOUND:g})")
    assert np.isfinite(g).all() and lu <= CC.LOSS_BOUND and gu <= CC.GRAD_BOUND
    assert not g[~_touched(s)].any()


# ---- tgn_subdivide_midpoint: sub_rank_kernel scans the 3 nf half-edges in chunks of 4096 (1024 threads x 4) -----------------------------

@pytest.mark.parametrize("nf", [1365, 1366], ids=["4095-half-edges", "4098-half-edges"])
def test_subdivide_around_the_rank_chunk_of_4096_half_edges(dev, nf):
    """3 nf is never 4096: the sizes next to it are 4095 (one chunk, its last thread one item short) and 4098 (a second chunk of two
    half-edges, ranked from the first chunk's carry)"""
    from toothgroupnetwork_amd import preprocess
    base = S.cases()["arch_shuffled"]
    mesh = dict(base, triangles=np.ascontiguousarray(base["triangles"][:nf]))
    assert S.same_bits(preprocess.subdivide_midpoint(mesh), S.subdivide_loop(mesh))


# ---- tsegnet.hip: tgn_tsg_proposals one lane per coarse point (waves of 64, m <= 1024); crop features and paint 256 entries per block ----
# (the cases of test_gpu_tsegnet.py at the sizes it leaves out)

@pytest.mark.parametrize("M", [63, 65, 1023, 1024])
def test_tsegnet_proposals_around_a_wave_and_at_the_limit(dev, M):
    import test_gpu_tsegnet as TS
    for mode in ("none", "all", "mixed"):
        TS.test_proposals_kernel(dev, M, mode)


@pytest.mark.parametrize("k", [255, 256, 257])
def test_tsegnet_crop_features_and_paint_around_a_block_of_256(dev, k):
    import test_gpu_tsegnet as TS
    TS.test_crop_features_kernel(dev, 5, k)
    TS.test_paint_kernel(dev, k)


# ---- metrics.hip: seg_confusion_logits_kernel takes 2048 vertices of a scan per workgroup, four per lane and load when N % 4 == 0 --------

@pytest.mark.parametrize("N", [2047, 2048, 2049, 4095, 4096, 4097])
def test_confusion_from_logits_around_the_chunk_of_2048(dev, N):
    import metrics_ref
    from toothgroupnetwork_amd import metrics
    B, C = 2, 17
    rng = np.random.default_rng(N)
    x = rng.standard_normal((B, C, N)).astype(np.float32)
    x[1, 3, N - 1] = x[1, 9, N - 1] = 7.0                               # two equal maxima in the last vertex: the lower channel
    gt = rng.integers(-1, C - 1, (B, N))
    logits, g = torch.from_numpy(x).to(dev), torch.from_numpy(gt).to(dev)
    pred = torch.argmax(logits, 1)
    assert int(pred[1, N - 1]) == 3
    want_a, want_s = metrics.confusion(g + 1, pred, pred, C)
    a, s = metrics.confusion_from_logits(logits, g)
    assert torch.equal(a, want_a) and torch.equal(s, want_s)
    for b in range(B):
        A, T = metrics_ref.tables(gt[b] + 1, pred[b].cpu().numpy(), pred[b].cpu().numpy(), C)
        assert np.array_equal(a[b].cpu().numpy(), A) and np.array_equal(s[b].cpu().numpy(), T) and int(A.sum()) == N


# ---- linear_max.hip: tiles of 128 points x 128 channels x 16 inputs ------------------------------------------------------------------

LM_CASES = [(1, 16, 128, 127, "relu"), (1, 16, 128, 128, "relu"),       # N one below a point tile, and the full tile
            (2, 15, 127, 128, "leaky"), (2, 17, 129, 128, "leaky"),     # K and C one either side of a tile
            (1, 16, 128, 257, "identity")]                              # two full point tiles and one row


@pytest.mark.parametrize("B,K,C,N,act", LM_CASES)
def test_linear_act_max_around_its_tiles(dev, B, K, C, N, act):
    import test_gpu_linear_max as TL
    TL.test_accuracy_against_float64_with_the_derived_bound(dev, B, K, C, N, act)


# ---- crop_gather_center_kernel: 256 threads stride over the k crop points and reduce their float64 sums in a tree ------------------------

@pytest.mark.parametrize("k", [255, 256, 257])
def test_crop_gather_center_around_its_stride_of_256(dev, k):
    from test_gpu_tooth_crops import _check_against_restatement, _random_case, _run
    rows, lab = _random_case(1500, 4, seed=k, dup=50)
    r, _ = _run(dev, rows, lab, k)
    _check_against_restatement(r, rows, lab, k)
