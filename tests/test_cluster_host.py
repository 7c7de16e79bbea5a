"""Host-side checks of the clustering (no GPU): the brute-force DBSCAN restatement (tests/cluster_ref.py) against sklearn, the
split test's edge cases, and argument validation that never reaches the library."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import cluster_ref  # noqa: E402
from cluster_cases import dbscan_cases  # noqa: E402


@pytest.mark.parametrize("tag", ["border", "lattice", "noise", "ms1", "tsegnet", "ragged"])
def test_brute_force_dbscan_equals_sklearn(tag):
    sk = pytest.importorskip("sklearn.cluster")
    x, eps, ms, offset = dbscan_cases()[tag]
    want_l, want_c, lo = [], [], 0
    for hi in offset:
        r = sk.DBSCAN(eps=eps, min_samples=ms).fit(x[lo:hi])
        c = np.zeros(hi - lo, bool)
        c[r.core_sample_indices_] = True
        want_l.append(r.labels_)
        want_c.append(c)
        lo = hi
    got_l, got_c = cluster_ref.dbscan_ragged(x, eps, ms, offset)
    assert np.array_equal(got_l, np.concatenate(want_l))
    assert np.array_equal(got_c, np.concatenate(want_c))


def test_brute_force_dbscan_rules_on_a_tiny_cloud():
    # points 0-2 within eps of each other (core with min_samples 3), point 3 within eps of point 2 only (border), point 4 alone
    x = np.array([[0, 0, 0], [0.01, 0, 0], [0.02, 0, 0], [0.045, 0, 0], [1, 1, 1]], np.float32)
    labels, core = cluster_ref.dbscan(x, 0.03, 3)
    assert core.tolist() == [True, True, True, False, False]
    assert labels.tolist() == [0, 0, 0, 0, -1]


def test_split_candidates_edge_cases():
    from toothgroupnetwork_amd import cluster
    assert cluster.split_candidates(np.array([5.0, 1.0])) == []                 # fewer than 3 clusters: no split test
    assert cluster.split_candidates(np.array([100.0, 1.0, 1.0])) == []          # 3 clusters: the mean of nothing is NaN
    assert cluster.split_candidates(np.array([1.0, 90.0, 1.0, 1.0, 1.0])) == [1]
    assert cluster.split_candidates(np.array([1.0, 90.0, 80.0, 1.0, 1.0])) == [1, 2]
    assert cluster.split_candidates(np.array([8.0, 1.0, 1.0, 1.0])) == []       # 8x exactly is not above 8x


def _no_library(monkeypatch):
    from toothgroupnetwork_amd import _lib
    monkeypatch.setattr(_lib, "require_cuda", lambda *t: None)
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))


@pytest.mark.parametrize("kw, exc", [
    (dict(eps=0.0), ValueError), (dict(eps=float("nan")), ValueError), (dict(min_samples=0), ValueError),
    (dict(points=torch.zeros(10, 2)), ValueError), (dict(points=torch.zeros(10, 3, dtype=torch.float64)), TypeError),
    (dict(offset=[4, 10]), None), (dict(offset=[6, 4, 10]), ValueError), (dict(offset=[4, 9]), ValueError),
    (dict(points=np.zeros((10, 3), np.float32)), TypeError),
])
def test_dbscan_argument_checks_run_before_any_launch(monkeypatch, kw, exc):
    from toothgroupnetwork_amd import cluster
    _no_library(monkeypatch)
    args = dict(points=torch.zeros(10, 3), eps=0.03, min_samples=3, offset=None)
    args.update(kw)
    if exc is None:                                 # valid arguments: the first thing after the checks is the library
        with pytest.raises(pytest.fail.Exception, match="library was reached"):
            cluster.dbscan(**args)
    else:
        with pytest.raises(exc):
            cluster.dbscan(**args)


@pytest.mark.parametrize("kw, exc", [
    (dict(bandwidth=-1.0), ValueError), (dict(max_iter=-1), ValueError), (dict(points=torch.zeros(10, 3)), TypeError),
    (dict(points=torch.zeros(0, 3, dtype=torch.float64)), ValueError),
])
def test_mean_shift_argument_checks_run_before_any_launch(monkeypatch, kw, exc):
    from toothgroupnetwork_amd import cluster
    _no_library(monkeypatch)
    args = dict(points=torch.zeros(10, 3, dtype=torch.float64), bandwidth=0.07)
    args.update(kw)
    with pytest.raises(exc):
        cluster.mean_shift(**args)
