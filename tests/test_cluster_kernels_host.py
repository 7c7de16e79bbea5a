"""Host-side checks behind tests/test_gpu_cluster_kernels.py (no GPU): the restatements of tests/cluster_kernels_ref.py against sklearn,
the proof that the moments bound separates the kernel's summation order from wrong kernels, and _eigen_first against sklearn's PCA."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import cluster_kernels_ref as R  # noqa: E402
from cluster_cases import digest, kernel_labelling_cases, labelling_cases, mean_shift_cases, moments_far_cloud  # noqa: E402

FIX = np.load(os.path.join(HERE, "golden", "reference_cpu_r10_cluster_kernels.npz"))
MS = mean_shift_cases()
MS_SKLEARN = [(tag, mi) for tag, (_, _, mis, sk) in MS.items() if sk for mi in mis]


@pytest.mark.parametrize("tag, max_iter", MS_SKLEARN)
def test_mean_shift_restatement_equals_sklearn(tag, max_iter):
    sk = pytest.importorskip("sklearn.cluster")
    x, bw, _, _ = MS[tag]
    assert FIX[f"ms_{tag}_digest"][0] == digest(x), "the case builder changed: regenerate the fixture"
    want = sk.MeanShift(bandwidth=bw, max_iter=max_iter).fit(x)
    labels, centers = R.mean_shift_fit(x, bw, max_iter)
    assert np.array_equal(labels, want.labels_)
    assert centers.shape == want.cluster_centers_.shape and np.max(np.abs(centers - want.cluster_centers_)) <= 1e-14
    # the fixture the GPU tests compare with holds this sklearn result (another sklearn may sum in another order: rounding)
    assert np.array_equal(want.labels_, FIX[f"ms_{tag}_{max_iter}_labels"])
    assert np.max(np.abs(want.cluster_centers_ - FIX[f"ms_{tag}_{max_iter}_centers"])) <= 1e-14


def test_mean_shift_restatement_edges():
    # the cap: max_iter = 0 is one step; a lone point is its own mean; an all-NaN row stays, with count 0, and moves nobody else
    x = np.array([[0.0, 0, 0], [0.05, 0, 0], [0.1, 0, 0]])
    m, c = R.mean_shift_seeds(x, 0.07, 0)
    assert c.tolist() == [2, 3, 2] and np.array_equal(m[:, 0], [(0.0 + 0.05) / 2, ((0.0 + 0.05) + 0.1) / 3, (0.05 + 0.1) / 2])
    m, c = R.mean_shift_seeds(np.array([[1.0, 2.0, -0.0]]), 0.07, 300)
    assert c.tolist() == [1] and np.array_equal(m.view(np.int64), np.array([[1.0, 2.0, -0.0]]).view(np.int64))
    x, bw, _, _ = MS["nan"]
    m, c = R.mean_shift_seeds(x, bw, 300)
    clean = np.delete(x, 137, 0)
    m2, c2 = R.mean_shift_seeds(clean, bw, 300)
    assert c[137] == 0 and np.isnan(m[137]).all()
    assert np.array_equal(np.delete(m, 137, 0).view(np.int64), m2.view(np.int64)) and np.array_equal(np.delete(c, 137), c2)


def test_small_restatements():
    c = np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 0, 0]])
    assert R.nearest_center(np.array([[0.5, 0, 0], [0.1, 0, 0], [0.9, 0, 0]]), c).tolist() == [0, 0, 1]     # ties and duplicates: lower index
    lab = np.array([7, 3, 3, 7, 200, 1 << 41])
    assert R.vote(np.array([[0, 1, 2, 3], [4, 5, 4, 5], [0, 0, 1, 5]]), lab).tolist() == [3, 200, 7]
    cand = np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 0, 0], [0.5, 0, 0]], np.float32)
    assert R.knn_order(cand, np.array([0.0, 0, 0], np.float32), 3).tolist() == [0, 2, 3]


def _tree(v):
    v = v.copy()
    w = v.shape[0] // 2
    while w > 0:
        v[:w] = v[:w] + v[w:2 * w]
        w >>= 1
    return v[0]


def _strided_tree(vals, sel, dtype=np.float64):
    """tgn_cluster_moments' order: thread t sums vals[i] over the selected i = t, t + 256, ... in ascending order from 0.0, then the
    256-way tree s[t] += s[t + w], w = 128 .. 1.  vals (n,) or (n, m)."""
    n = len(vals)
    pad = np.zeros((-(-n // 256) * 256,) + vals.shape[1:], dtype)
    pad[:n][sel] = vals[sel].astype(dtype)
    acc = np.zeros((256,) + vals.shape[1:], dtype)
    for row in pad.reshape((-1, 256) + vals.shape[1:]):      # adding 0.0 for an unselected point changes nothing
        acc = acc + row
    return _tree(acc)


def emulate_moments(x32, labels, mask, nlab, ddof=1, mean_dtype=np.float64):
    x = x32.astype(np.float64)
    keep = np.ones(len(x), bool) if mask is None else mask != 0
    count, mean, cov = np.zeros(nlab, np.int64), np.empty((nlab, 3)), np.empty((nlab, 3, 3))
    for l in range(nlab):
        sel = keep & (labels == l)
        tot = float(sel.sum())
        count[l] = sel.sum()
        with np.errstate(invalid="ignore", divide="ignore"):
            mean[l] = _strided_tree(x, sel, mean_dtype).astype(np.float64) / tot
            d = x - mean[l]
            prod = d[:, :, None] * d[:, None, :]
            cov[l] = _strided_tree(prod.reshape(-1, 9), sel).reshape(3, 3) / (tot - ddof) if tot >= 2 else np.nan
    return count, mean, cov


def test_the_moments_bound_holds_the_kernel_order_and_rejects_wrong_kernels():
    x, lab, mask = moments_far_cloud()
    n = len(x)
    exact = R.moments_exact(x, lab, mask, 14)
    count, mean, cov = emulate_moments(x, lab, mask, 14)
    mean_ok, cov_ok, worst = R.moments_within(n, mean, cov, exact)
    print(f"kernel-order emulation: largest error / bound {worst:.3f}")
    assert np.array_equal(count, exact[0]) and mean_ok.all() and cov_ok.all()
    mutants = {}
    _, m, c = emulate_moments(x, lab, mask, 14, ddof=0)
    mutants["ddof = 0"] = (m, c)
    _, m, c = emulate_moments(x, lab, mask, 14, mean_dtype=np.float32)
    mutants["float32-accumulated mean"] = (m, c)
    sw = cov.copy()
    sw[:, 0, 2], sw[:, 1, 2] = cov[:, 1, 2], cov[:, 0, 2]
    sw[:, 2, 0], sw[:, 2, 1] = sw[:, 0, 2], sw[:, 1, 2]
    mutants["cov[0][2] and cov[1][2] swapped"] = (mean, sw)
    _, m, c = emulate_moments(x, lab, None, 14)
    mutants["mask ignored"] = (m, c)
    for name, (m, c) in mutants.items():
        mean_ok, cov_ok, worst = R.moments_within(n, m, c, exact)
        bad = [l for l in range(14) if not (mean_ok[l].all() and cov_ok[l].all())]
        print(f"mutant {name}: largest error / bound {worst:.1e}, labels outside the bound {len(bad)} of 14")
        assert len(bad) == 14, f"the bound accepts a wrong kernel ({name}) on labels {sorted(set(range(14)) - set(bad))}"


def test_moments_restatement_equals_numpy_on_a_small_cloud():
    rng = np.random.default_rng(3)
    x = rng.normal(0, 1, (50, 3)).astype(np.float32)
    lab = rng.integers(-1, 4, 50)
    lab[lab == 2] = 0                                       # label 2 is empty
    lab[0], lab[1:50][lab[1:50] == 3] = 3, 1                # label 3 holds one point
    count, mean, cov, _, _ = R.moments_exact(x, lab, None, 5)
    assert count[2] == 0 and count[3] == 1 and count[4] == 0
    for l in (0, 1):
        p = x[lab == l].astype(np.float64)
        assert np.allclose(mean[l].astype(np.float64), p.mean(0), rtol=1e-13, atol=0)
        assert np.allclose(cov[l].astype(np.float64), np.cov(p.T), rtol=1e-12, atol=1e-15)
    assert np.isnan(mean[2]).all() and np.isnan(cov[2]).all() and np.isnan(cov[3]).all()
    assert np.array_equal(mean[3].astype(np.float32), x[0])


@pytest.mark.parametrize("tag", ["nosplit", "split", "split2", "three", "votetie"])
def test_eigen_first_equals_sklearn_pca(tag):
    """The tolerance is 16x the largest relative difference between PCA(3).explained_variance_[0] and eigvalsh of the exact covariance
    that make_golden_r10_cluster_kernels.py measured on these cases (its docstring: 3.86e-11); it must stay below the 1e-6 that the
    generators keep between every split ratio and 8."""
    cl = pytest.importorskip("sklearn.cluster")
    dec = pytest.importorskip("sklearn.decomposition")
    from toothgroupnetwork_amd import cluster
    tol = 16 * float(FIX["pca_rel"][0])
    assert 0 < tol < 1e-6
    moved, cls = {**labelling_cases(), **kernel_labelling_cases()}[tag]
    fg = moved[cls != 0]
    r = cl.DBSCAN(eps=0.03, min_samples=30).fit(fg)
    core = np.zeros(len(fg), bool)
    core[r.core_sample_indices_] = True
    K = r.labels_.max() + 1
    count, _, cov, _, _ = R.moments_exact(fg, r.labels_, core, K)
    first = cluster._eigen_first(count, cov.astype(np.float64))
    want = np.array([dec.PCA(3).fit(fg[core & (r.labels_ == k)].astype(np.float64)).explained_variance_[0] for k in range(K)])
    assert np.all(np.abs(first - want) <= tol * want), float(np.max(np.abs(first - want) / want))
