"""GPU: every clustering entry point of csrc/cluster.hip through the C ABI, each against the restatement of its contract
(tests/cluster_kernels_ref.py; tests/cluster_ref.py for DBSCAN) -- exactly where the contract is exact, within a float64 bound scaled by
the terms where it is not (tgn_cluster_moments) -- plus tgn_crop_knn in the regime the noise vote drives it in, and
get_clustering_labels on the branches tests/test_gpu_cluster.py leaves out (tests/golden/reference_cpu_r10_cluster_kernels.npz, written by
make_golden_r10_cluster_kernels.py).  No tolerance here comes from GPU output; tests/test_cluster_kernels_host.py shows without a GPU that
the restatements equal sklearn and that the moments bound rejects wrong kernels.  The gpu_* helpers launch on the current stream;
tests/cluster_stream_launcher.py runs them on a stream of its own, in a child process."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import cluster_kernels_ref as R  # noqa: E402
import cluster_ref  # noqa: E402
from cluster_cases import digest, kernel_labelling_cases, labelling_cases, mean_shift_cases, moments_far_cloud  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = np.load(os.path.join(HERE, "golden", "reference_cpu_r10_cluster_kernels.npz"))
FIX9 = np.load(os.path.join(HERE, "golden", "reference_cpu_r9_cluster.npz"))
DEV = torch.device("cuda", 0)
MS = mean_shift_cases()
MS_ALL = [(tag, mi) for tag, (_, _, mis, _) in MS.items() for mi in mis]
MS_SKLEARN = [(tag, mi) for tag, (_, _, mis, sk) in MS.items() if sk for mi in mis]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _api():
    from toothgroupnetwork_amd import _lib
    return _lib, _lib.lib(), _lib.stream()


# ---- tgn_mean_shift ---------------------------------------------------------------------------------------------------------

def gpu_seeds(x, bw, max_iter):
    _lib, L, st = _api()
    pts, n = _t(x), len(x)
    means = torch.empty(n, 3, dtype=torch.float64, device=DEV)
    counts = torch.empty(n, dtype=torch.int32, device=DEV)
    assert L.tgn_mean_shift(n, _lib.ptr(pts), bw, max_iter, _lib.ptr(means), _lib.ptr(counts), st) == 0
    return means.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("tag, max_iter", MS_ALL)
def test_mean_shift_seeds_equal_the_restatement_bit_for_bit(tag, max_iter):
    """The header's promise: a seed's sum is p0 + p1 + ... in ascending point order, IEEE division and square root (no fast-math,
    -ffp-contract=off), so means and counts equal the numpy restatement's bits; and two runs are identical."""
    x, bw, _, _ = MS[tag]
    assert FIX[f"ms_{tag}_digest"][0] == digest(x), "the case builder changed: regenerate the fixture"
    want_m, want_c = R.mean_shift_seeds(x, bw, max_iter)
    got_m, got_c = gpu_seeds(x, bw, max_iter)
    assert np.array_equal(got_c, want_c)
    diff = np.flatnonzero((got_m.view(np.int64) != want_m.view(np.int64)).any(1))
    assert diff.size == 0, (tag, max_iter, f"{diff.size} seeds differ, first {diff[:5]}", got_m[diff[:2]], want_m[diff[:2]])
    again_m, again_c = gpu_seeds(x, bw, max_iter)
    assert np.array_equal(again_m.view(np.int64), got_m.view(np.int64)) and np.array_equal(again_c, got_c)
    if tag == "negzero":
        assert np.array_equal(got_m[:, 2].view(np.int64), np.full(len(x), -0.0).view(np.int64)), "a sum of -0.0 is -0.0"
    if tag == "nan":
        clean_m, clean_c = gpu_seeds(np.delete(x, 137, 0), bw, max_iter)
        assert got_c[137] == 0 and np.isnan(got_m[137]).all()
        assert np.array_equal(np.delete(got_m, 137, 0).view(np.int64), clean_m.view(np.int64)) and np.array_equal(np.delete(got_c, 137), clean_c)
    if tag == "bar" and max_iter == 5:
        full_m, _ = gpu_seeds(x, bw, 300)
        assert np.any((full_m != got_m).any(1)), "the cap must stop some climbs early"


@pytest.mark.parametrize("tag, max_iter", MS_SKLEARN)
def test_mean_shift_equals_sklearn_on_every_case(tag, max_iter):
    from toothgroupnetwork_amd import cluster
    x, bw, _, _ = MS[tag]
    labels, centers = cluster.mean_shift(_t(x), bw, max_iter=max_iter)
    want = FIX[f"ms_{tag}_{max_iter}_centers"]
    assert np.array_equal(labels.cpu().numpy(), FIX[f"ms_{tag}_{max_iter}_labels"].astype(np.int64))
    assert centers.shape == want.shape and np.max(np.abs(centers.cpu().numpy() - want)) <= 1e-14


def test_mean_shift_fit_equals_the_restatement_where_sklearn_is_not_compared():
    from toothgroupnetwork_amd import cluster
    for tag in ("lattice", "nan"):
        x, bw, _, _ = MS[tag]
        labels, centers = cluster.mean_shift(_t(x), bw)
        want_l, want_c = R.mean_shift_fit(x, bw, 300)
        assert np.array_equal(centers.cpu().numpy().view(np.int64), want_c.view(np.int64)), tag
        assert np.array_equal(labels.cpu().numpy(), want_l), tag


# ---- tgn_nearest_center -----------------------------------------------------------------------------------------------------

def gpu_nearest(x, c):
    _lib, L, st = _api()
    pts, cen = _t(x), _t(c)
    out = torch.full((len(x),), -7, dtype=torch.int64, device=DEV)
    assert L.tgn_nearest_center(len(x), _lib.ptr(pts), len(c), _lib.ptr(cen), _lib.ptr(out), st) == 0
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 255, 257, 5000])
@pytest.mark.parametrize("m", [1, 2, 3, 17, 64])
def test_nearest_center_equals_the_restatement(n, m):
    rng = np.random.default_rng(100 * n + m)
    x, c = rng.normal(0, 0.1, (n, 3)), rng.normal(0, 0.1, (m, 3)) / 3.0          # float64 values no float32 holds
    assert np.any(c != c.astype(np.float32))
    assert np.array_equal(gpu_nearest(x, c), R.nearest_center(x, c))
    if m >= 3:                                               # duplicate centres: the lower index wins
        c2 = c.copy()
        c2[m - 1], c2[m // 2] = c[0], c[1]
        got = gpu_nearest(x, c2)
        assert np.array_equal(got, R.nearest_center(x, c2)) and not np.any(got == m - 1) and not (m // 2 > 1 and np.any(got == m // 2))


def test_nearest_center_ties_go_to_the_lower_index():
    g = np.arange(4) * 0.125
    c = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)           # 64 lattice centres, index = 16 i + 4 j + k
    c = c[np.random.default_rng(9).permutation(64)]
    edge = c[:, None, :] + np.array([[0.0625, 0, 0], [0, 0.0625, 0], [0, 0, 0.0625]])[None]        # equidistant from two centres
    face = c[:, None, :] + np.array([[0.0625, 0.0625, 0], [0, 0.0625, 0.0625], [0.0625, 0, 0.0625]])[None]   # from four
    x = np.concatenate([edge.reshape(-1, 3), face.reshape(-1, 3)])
    x = x[(x <= 0.375).all(1)]
    d = R.rdist(x[:, None, :], c[None])
    ties = (d == d.min(1, keepdims=True)).sum(1)
    assert set(ties.tolist()) == {2, 4}
    want = np.array([np.flatnonzero(row == row.min())[0] for row in d])
    got = gpu_nearest(x, c)
    assert np.array_equal(got, want) and np.array_equal(got, R.nearest_center(x, c))


# ---- tgn_cluster_moments ----------------------------------------------------------------------------------------------------

def gpu_moments(x, labels, mask, nlab):
    _lib, L, st = _api()
    pts, lab = _t(x), _t(labels.astype(np.int64))
    msk = None if mask is None else _t(mask.astype(np.uint8))
    counts = torch.full((nlab,), -7, dtype=torch.int32, device=DEV)
    mean = torch.full((nlab, 3), 7.0, dtype=torch.float64, device=DEV)
    cov = torch.full((nlab, 3, 3), 7.0, dtype=torch.float64, device=DEV)
    assert L.tgn_cluster_moments(len(x), _lib.ptr(pts), _lib.ptr(lab), _lib.ptr(msk), nlab, _lib.ptr(counts), _lib.ptr(mean),
                                 _lib.ptr(cov), st) == 0
    return counts.cpu().numpy(), mean.cpu().numpy(), cov.cpu().numpy()


def _moments_case(name):
    """-> (xyz float32, labels int64 with -1 and values >= nlab among them, mask or None, nlab)"""
    if name.startswith("far"):
        x, lab, mask = moments_far_cloud()
        lab = lab.copy()
        lab[::97], lab[5::101] = -1, 14
        return x, lab, mask if name == "far_mask" else None, 14
    n, nlab, masked = {"n3": (3, 1, False), "n255": (255, 14, True), "n100000": (100000, 100, True), "n100000_nomask": (100000, 14, False)}[name]
    rng = np.random.default_rng(n + nlab)
    lab = rng.integers(-1, nlab + 2, n) if n > 3 else np.zeros(3, np.int64)
    cent = rng.uniform(-2, 2, (nlab + 2, 3))
    x = (cent[lab] + rng.normal(0, 1, (n, 3)) * [0.05, 0.01, 0.2]).astype(np.float32)
    mask = (rng.random(n) < 0.7).astype(np.uint8) if masked else None
    if name == "n255":                                       # label 5: two points, label 6: one point, label 7: none
        keep = np.ones(n, bool) if mask is None else mask != 0
        for l, want in ((5, 2), (6, 1), (7, 0)):
            idx = np.flatnonzero((lab == l) & keep)
            lab[idx[want:]] = 0
            assert np.sum((lab == l) & keep) == want
    return x, lab, mask, nlab


@pytest.mark.parametrize("name", ["far_mask", "far_nomask", "n3", "n255", "n100000", "n100000_nomask"])
def test_moments_within_the_derived_bound(name):
    """Against cluster_kernels_ref.moments_exact (longdouble) with u = 2^-53 and D = ceil(n / 256) + 8, the longest chain of additions
    behind a sum (a thread's strided sequential sum of at most ceil(n / 256) terms, then the eight levels of the 256-way tree):
      mean  |mean - exact| <= (D + 1) u sum|x| / c: the float32 -> float64 conversion is exact, a sum of D chained additions carries a
            relative error of at most D u against sum|x| (first order), the division by c adds one rounding;
      cov   |cov - exact| <= ((D + c0) u sum|dx dy| + c bm_x bm_y) / (c - 1), bm the mean's bound.  With the computed mean m + e the
            centred sum is sum (dx - e_x)(dy - e_y) = sum dx dy + c e_x e_y, because sum dx = sum dy = 0: the mean's error enters at
            second order only, bounded by c bm_x bm_y.  Every term carries three roundings (the two subtractions x - mean, y - mean and
            the product), the sum D, the division by c - 1 one: D + 4 to first order.  c0 = 8 doubles those four for everything of
            second order (products of roundings, and the roundings being relative to the perturbed |dx - e_x| |dy - e_y| instead of
            |dx| |dy|: a relative excess of about |e| / |dx|, below 1e-9 for every case here).  The CPU emulation of the kernel's order
            stays at 0.03 of this bound, and ddof = 0, a float32 mean, swapped entries and an ignored mask all exceed it by factors above
            1e6 (tests/test_cluster_kernels_host.py).
    Counts are exact; labels -1 and >= nlab are ignored; a label with one point has that point as its mean and a NaN covariance; a label
    with no point has count 0 and NaN mean and covariance (as np.mean and np.cov of nothing); cov is bitwise symmetric; two runs are
    bitwise identical."""
    x, lab, mask, nlab = _moments_case(name)
    exact = R.moments_exact(x, lab, mask, nlab)
    count, mean, cov = gpu_moments(x, lab, mask, nlab)
    assert np.array_equal(count, exact[0])
    mean_ok, cov_ok, worst = R.moments_within(len(x), mean, cov, exact)
    print(f"moments {name}: counts {exact[0].min()}..{exact[0].max()}, largest error / bound {worst:.3f}")
    assert mean_ok.all() and cov_ok.all(), (name, worst, np.argwhere(~mean_ok), np.argwhere(~cov_ok))
    assert np.array_equal(cov.view(np.int64), cov.transpose(0, 2, 1).copy().view(np.int64)), "cov[a][b] and cov[b][a] differ"
    again = gpu_moments(x, lab, mask, nlab)
    for a, b in zip((count, mean, cov), again):
        assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)
    if name == "n255":
        keep = mask != 0
        assert count[5] == 2 and count[6] == 1 and count[7] == 0
        assert np.array_equal(mean[6], x[np.flatnonzero((lab == 6) & keep)[0]].astype(np.float64)) and np.isnan(cov[6]).all()
        assert np.isnan(mean[7]).all() and np.isnan(cov[7]).all()
        assert np.isfinite(cov[5]).all()
    if name == "far_mask":                                   # the mask matters: without it the counts differ
        assert not np.array_equal(gpu_moments(x, lab, None, nlab)[0], count)


# ---- tgn_cluster_vote -------------------------------------------------------------------------------------------------------

def gpu_vote(nn_idx, cand_labels):
    _lib, L, st = _api()
    idx, lab = _t(nn_idx.astype(np.int64)), _t(cand_labels.astype(np.int64))
    out = torch.full((len(nn_idx),), -7, dtype=torch.int64, device=DEV)
    assert L.tgn_cluster_vote(nn_idx.shape[0], nn_idx.shape[1], _lib.ptr(idx), len(cand_labels), _lib.ptr(lab), _lib.ptr(out), st) == 0
    return out.cpu().numpy()


ALPHABETS = {"two": [3, 7], "three": [100, 101, 205], "wide": [5, 200, (1 << 40) + 3, 101, 0]}


@pytest.mark.parametrize("k", [1, 2, 10, 31, 32])
@pytest.mark.parametrize("m", [1, 255, 257, 10000])
def test_vote_equals_the_restatement(k, m):
    _lib, L, st = _api()
    L.tgn_take_index_error(st)
    rng = np.random.default_rng(1000 * k + m)
    for name, alphabet in ALPHABETS.items():
        cand = np.array(alphabet, np.int64)[rng.integers(0, len(alphabet), 500)]
        idx = rng.integers(0, 500, (m, k))
        want = R.vote(idx, cand)
        if k in (2, 10, 32) and m >= 255 and name != "wide":
            counts = np.stack([(cand[idx] == a).sum(1) for a in alphabet], 1)
            assert np.any(np.sort(counts, 1)[:, -1] == np.sort(counts, 1)[:, -2]), "the case must hold tied votes"
        got = gpu_vote(idx, cand)
        assert np.array_equal(got, want), (name, np.flatnonzero(got != want)[:5])
    assert L.tgn_take_index_error(st) == 0, "in-range indices must leave the error word clear"


@pytest.mark.parametrize("bad", ["n_cand", -1])
def test_vote_out_of_range_index_reads_candidate_0_and_latches_the_error_word(bad):
    _lib, L, st = _api()
    L.tgn_take_index_error(st)
    rng = np.random.default_rng(77)
    cand = np.array([3, 7, 9], np.int64)[rng.integers(0, 3, 50)]
    idx = rng.integers(0, 50, (300, 10))
    assert np.array_equal(gpu_vote(idx, cand), R.vote(idx, cand)) and L.tgn_take_index_error(st) == 0
    idx[123, 4] = 50 if bad == "n_cand" else -1
    as_zero = idx.copy()
    as_zero[123, 4] = 0
    assert np.array_equal(gpu_vote(idx, cand), R.vote(as_zero, cand))
    assert L.tgn_take_index_error(st) == 1 << 1, "bit 1 of the word (the gather family latches bit 0)"
    assert L.tgn_take_index_error(st) == 0, "taking the word clears it"


# ---- tgn_crop_knn as the noise vote calls it --------------------------------------------------------------------------------

def _vote_candidates(name):
    rng = np.random.default_rng(len(name) * 31 + sum(map(ord, name)))
    if name == "dups":
        c = rng.normal(0, 0.1, (3000, 3)).astype(np.float32)
        c[rng.permutation(3000)[:300]] = c[rng.integers(0, 3000, 300)]
        return c
    return rng.normal(0, 0.1, (int(name), 3)).astype(np.float32)


@pytest.mark.parametrize("name", ["10", "11", "1023", "1025", "15000", "dups"])
@pytest.mark.parametrize("t_total", [1, 300, 5000])
def test_crop_knn_in_the_vote_regime(name, t_total):
    """b = 1, c_stride = 3, k = 10, one workgroup per query: hundreds to thousands of arbitrary queries, as few as k candidates."""
    _lib, L, st = _api()
    cand = _vote_candidates(name)
    n, k = len(cand), 10
    rng = np.random.default_rng(t_total + n)
    q = rng.normal(0, 0.12, (t_total, 3)).astype(np.float32)
    q[0::3] = cand[rng.integers(0, n, len(q[0::3]))]          # queries AT a candidate: distance 0
    q[1::7] *= 50.0                                           # far outside the cloud
    feats = _t(cand.T)                                        # (3, n) channel-first, b = 1
    scan = torch.zeros(t_total, dtype=torch.int32, device=DEV)
    idx = torch.full((t_total, k), -7, dtype=torch.int64, device=DEV)
    L.tgn_take_index_error(st)
    assert L.tgn_crop_knn(1, n, 3, _lib.ptr(feats), t_total, _lib.ptr(scan), _lib.ptr(_t(q)), k, _lib.ptr(idx), st) == 0
    got = idx.cpu().numpy()
    assert L.tgn_take_index_error(st) == 0
    for t in range(t_total):
        assert np.array_equal(got[t], R.knn_order(cand, q[t], k)), (name, t)


# ---- get_clustering_labels --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["split2", "three", "votetie"])
def test_get_clustering_labels_equals_the_reference_on_the_other_branches(tag):
    from toothgroupnetwork_amd import cluster
    moved, cls = kernel_labelling_cases()[tag]
    assert FIX[f"cl_{tag}_digest"][0] == digest(moved, cls), "the case builder changed: regenerate the fixture"
    want = FIX[f"cl_{tag}_labels"].astype(np.int64)
    if tag == "split2":
        assert np.any((want >= 100) & (want < 200)) and np.any(want >= 200)
    got_np = cluster.get_clustering_labels(moved, cls)
    assert isinstance(got_np, np.ndarray) and np.array_equal(got_np, want)
    got_t = cluster.get_clustering_labels(_t(moved), _t(cls))
    assert got_t.is_cuda and np.array_equal(got_t.cpu().numpy(), want)


def test_get_clustering_labels_takes_labels_of_shape_n1():
    from toothgroupnetwork_amd import cluster
    moved, cls = labelling_cases()["split"]
    assert FIX9["cl_split_digest"][0] == digest(moved, cls)
    want = FIX9["cl_split_labels"].astype(np.int64)
    assert np.array_equal(cluster.get_clustering_labels(moved, cls.reshape(-1, 1)), want)
    assert np.array_equal(cluster.get_clustering_labels(_t(moved), _t(cls.reshape(-1, 1))).cpu().numpy(), want)


# ---- tgn_dbscan: the edges the fixtures leave out ---------------------------------------------------------------------------

def _dbscan_edge(name):
    rng = np.random.default_rng(42)
    if name in ("one_ms1", "one_ms2"):
        return np.array([[0.3, -0.2, 0.1]], np.float32), 0.03, 1 if name == "one_ms1" else 2
    if name == "identical":                                  # one bucket holds everything
        return np.tile(np.array([[0.25, 0.5, -0.125]], np.float32), (3000, 1)), 0.03, 30
    if name == "min_samples_above_n":
        return rng.normal(0, 0.01, (50, 3)).astype(np.float32), 0.03, 51
    if name == "translated":                                 # float32 spacing 6e-5 at 1000
        c = rng.uniform(-0.4, 0.4, (5, 3))
        x = np.concatenate([c[rng.integers(0, 5, 2500)] + rng.normal(0, 0.012, (2500, 3)), rng.uniform(-0.5, 0.5, (150, 3))])
        return (x + [1000.0, -1000.0, 1000.0]).astype(np.float32), 0.03, 30
    if name == "tiny_eps":                                   # every cell index clamps: one cell, only exact duplicates are neighbours
        x = (rng.uniform(-1, 1, (900, 3)) + [1000.0, 1200.0, -900.0]).astype(np.float32)
        x[rng.permutation(900)[:200]] = x[rng.integers(0, 900, 200)]
        return x, 1e-7, 2
    raise KeyError(name)


@pytest.mark.parametrize("name", ["one_ms1", "one_ms2", "identical", "min_samples_above_n", "translated", "tiny_eps"])
def test_dbscan_edges_against_the_brute_force_rules(name):
    from toothgroupnetwork_amd import cluster
    x, eps, ms = _dbscan_edge(name)
    want_l, want_c = cluster_ref.dbscan(x, eps, ms)
    if name in ("translated", "tiny_eps", "identical", "one_ms1"):
        assert want_l.max() >= 0, "the case must form a cluster"
    lab, core, counts = cluster.dbscan_counts(_t(x), eps, ms)
    assert np.array_equal(lab.cpu().numpy(), want_l) and np.array_equal(core.cpu().numpy(), want_c)
    assert counts.cpu().tolist() == [want_l.max() + 1]


# ---- arguments ---------------------------------------------------------------------------------------------------------

def test_entry_points_reject_bad_arguments_without_launching():
    _lib, L, st = _api()
    bad = _lib.ERR_INVALID_ARGUMENT
    x = torch.zeros(64, 3, dtype=torch.float64, device=DEV)
    p = _lib.ptr(x)
    for bw in (0.0, -1.0, float("nan")):
        assert L.tgn_mean_shift(10, p, bw, 300, p, p, st) == bad
    assert L.tgn_mean_shift(10, p, 0.07, -1, p, p, st) == bad
    assert L.tgn_mean_shift(0, None, 0.07, 300, None, None, st) == 0
    assert L.tgn_nearest_center(10, p, 0, p, p, st) == bad
    assert L.tgn_nearest_center(0, None, 1, None, None, st) == 0
    for k in (0, 33):
        assert L.tgn_cluster_vote(4, k, p, 10, p, p, st) == bad
    assert L.tgn_cluster_vote(4, 10, p, 0, p, p, st) == bad
    assert L.tgn_cluster_vote(0, 10, None, 10, None, None, st) == 0
    assert L.tgn_cluster_moments(0, p, p, None, 1, p, p, p, st) == bad
    assert L.tgn_cluster_moments(10, p, p, None, 0, None, None, None, st) == 0
    need = L.tgn_dbscan_workspace_bytes(1, 10)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert need > 0 and L.tgn_dbscan(1, 10, p, p, 0.03, 3, p, p, p, _lib.ptr(ws), need - 1, st) == bad
    assert b"tgn_dbscan" in L.tgn_last_error()
    torch.cuda.synchronize()
    assert torch.count_nonzero(x).item() == 0, "a rejected call must not write"

