#!/usr/bin/env python3
"""Fixtures of the per-kernel clustering tests (tests/golden/reference_cpu_r10_cluster_kernels.npz), produced on CPU with sklearn and the
REFERENCE's own Python in the build container, as make_golden_r9_cluster.py does:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_r10_cluster_kernels.py

  ms_<tag>_<max_iter>_*  sklearn's MeanShift(bandwidth, max_iter=max_iter).fit on the sklearn-compared cases of
         cluster_cases.mean_shift_cases: labels_ as int16, cluster_centers_ as float64.
  cl_*   the reference's ops_utils.get_clustering_labels on cluster_cases.kernel_labelling_cases (split2, three, votetie).
  pca_rel  the largest relative difference, over the clusters of all five labelling cases, between PCA(3).explained_variance_[0] on a
         cluster's core points and the largest eigenvalue (numpy's eigvalsh) of their exact covariance (cluster_kernels_ref.moments_exact,
         longdouble, rounded once to float64).  MEASURED 3.86e-11 (sklearn 1.7.2, whose PCA takes the eigenvalues of the uncentred
         X^T X form here); tests/test_cluster_kernels_host.py allows 16x the stored value, which must stay below the 1e-6 that
         separates every split ratio from 8.
Every input is stored as a digest (cluster_cases.py rebuilds it); the file is written with fixed zip timestamps, so a re-run reproduces
it byte for byte.  The generator asserts, and prints the margins it found:
  - during no climb of a sklearn-compared case a (mean, point) rdist within 1e-12 relative of bandwidth^2;
  - no point of such a case equidistant from its two nearest centres within 1e-12 relative;
  - the restatement (tests/cluster_kernels_ref.py) equal to sklearn: labels equal, centres within 1e-14;
  - each labelling case takes its branch; no split ratio within 1e-6 of 8.
"""
import io
import os
import sys
import warnings
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
from sklearn.cluster import DBSCAN, MeanShift  # noqa: E402
from sklearn.decomposition import PCA  # noqa: E402

import cluster_kernels_ref as R  # noqa: E402
from cluster_cases import digest, kernel_labelling_cases, labelling_cases, mean_shift_cases, pack_labels  # noqa: E402
from make_golden_r9_cluster import _reference_modules  # noqa: E402

NAME = "reference_cpu_r10_cluster_kernels.npz"


def mean_shift_part(out):
    for tag, (x, bw, max_iters, with_sklearn) in mean_shift_cases().items():
        out[f"ms_{tag}_digest"] = np.array([digest(x)])
        for mi in max_iters:
            margin = [np.inf]
            labels, centers = R.mean_shift_fit(x, bw, mi, margin)
            sizes = np.bincount(labels).tolist() if len(centers) <= 8 else "..."
            line = f"  ms {tag} max_iter={mi}: n={len(x)} centres={len(centers)} sizes={sizes}"
            if not with_sklearn:
                print(line + f" (restatement only; closest rdist to bw^2 {margin[0]:.1e})")
                continue
            assert margin[0] > 1e-12, f"{tag}: a (mean, point) pair at the bandwidth within 1e-12"
            sk = MeanShift(bandwidth=bw, max_iter=mi).fit(x)
            assert sk.cluster_centers_.shape == centers.shape and np.array_equal(sk.labels_, labels), f"{tag}: restatement != sklearn"
            dc = float(np.abs(sk.cluster_centers_ - centers).max())
            assert dc <= 1e-14, (tag, dc)
            tie = np.inf
            if len(centers) > 1:
                d = np.sort(R.rdist(x[:, None, :], sk.cluster_centers_[None]), axis=1)
                tie = float(((d[:, 1] - d[:, 0]) / d[:, 1]).min())
                assert tie > 1e-12, f"{tag}: a point equidistant from two centres"
            print(line + f" | bw margin {margin[0]:.1e}  centre tie margin {tie:.1e}  max|centre - sklearn| {dc:.1e}")
            out[f"ms_{tag}_{mi}_labels"] = pack_labels(sk.labels_)
            out[f"ms_{tag}_{mi}_centers"] = sk.cluster_centers_


def _dbscan(moved, cls):
    fg = moved[cls != 0]
    r = DBSCAN(eps=0.03, min_samples=30).fit(fg)
    core = np.zeros(len(fg), bool)
    core[r.core_sample_indices_] = True
    return fg, r.labels_, core


def _pca_rel(fg, lab, core):
    worst = 0.0
    K = lab.max() + 1
    count, _, cov, _, _ = R.moments_exact(fg, lab, core, K)
    for k in range(K):
        ev = PCA(3).fit(fg[core & (lab == k)].astype(np.float64)).explained_variance_[0]
        mine = np.linalg.eigvalsh(cov[k].astype(np.float64))[-1]
        worst = max(worst, abs(ev - mine) / ev)
    return worst


def labelling_part(out, ou):
    pca_rel = 0.0
    for tag, (moved, cls) in labelling_cases().items():
        pca_rel = max(pca_rel, _pca_rel(*_dbscan(moved, cls)))
    for tag, (moved, cls) in kernel_labelling_cases().items():
        fg, lab, core = _dbscan(moved, cls)
        pca_rel = max(pca_rel, _pca_rel(fg, lab, core))
        K = lab.max() + 1
        ev = np.array([PCA(3).fit(fg[core & (lab == k)].astype(np.float64)).explained_variance_[0] for k in range(K)])
        s = np.sort(ev)[::-1]
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            ratios = s[:3] / s[3:].mean()
            got = ou.get_clustering_labels(moved, cls)
        runtime = [w for w in caught if issubclass(w.category, RuntimeWarning)]
        noise = lab == -1
        assert noise.sum() > 0, "votes must be cast"
        print(f"  cl {tag}: fg={len(got)} clusters={K} ratios={np.round(ratios, 2)} votes={noise.sum()} final labels={np.unique(got).tolist()}")
        if tag == "three":
            assert K == 3 and runtime and got.max() < 100, "three clusters: a RuntimeWarning and no split"
            print(f"    the reference ran with {len(runtime)} RuntimeWarning(s) and split nothing")
        else:
            assert not np.any(np.abs(ratios - 8) <= 1e-6 * 8), f"{tag}: a split ratio within 1e-6 of 8"
        if tag == "split2":
            assert int(np.sum(ratios > 8)) == 2
            v = got[noise]
            n1, n2 = int(np.sum((v >= 100) & (v < 200))), int(np.sum(v >= 200))
            assert np.any((got >= 100) & (got < 200) & ~noise) and np.any((got >= 200) & ~noise) and n1 and n2
            print(f"    noise points voted into the first split: {n1}, into the second: {n2}")
        if tag == "votetie":
            assert got.max() < 100
            cand, cl = fg[~noise].astype(np.float64), lab[~noise]
            ties = 0
            for q in fg[noise].astype(np.float64):
                d = R.rdist(cand, q)
                order = np.lexsort((np.arange(d.size), d))
                assert d[order[9]] < d[order[10]], "the 10th and 11th neighbour must differ"
                c = np.sort(np.unique(cl[order[:10]], return_counts=True)[1])[::-1]
                ties += len(c) == 2 and c[0] == 5
            assert ties >= 1, "votetie must hold a 5/5 vote"
            print(f"    noise points with a 5/5 vote: {ties}")
        out[f"cl_{tag}_digest"] = np.array([digest(moved, cls)])
        out[f"cl_{tag}_labels"] = pack_labels(got)
    assert 16 * pca_rel < 1e-6
    print(f"  pca: largest relative difference PCA explained_variance_[0] vs eigvalsh(exact covariance) = {pca_rel:.2e}")
    out["pca_rel"] = np.array([pca_rel])


def save(path, arrays):
    """np.savez_compressed with fixed member timestamps (numpy stamps the members with the time of writing)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    out = {}
    _, ou = _reference_modules()
    mean_shift_part(out)
    labelling_part(out, ou)
    path = os.path.join(HERE, NAME)
    save(path, out)
    print(f"wrote tests/golden/{NAME} ({os.path.getsize(path) / 1e3:.1f} kB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
