#!/usr/bin/env python3
"""Child process of tests/test_gpu_cluster.py: the clustering on a non-default stream, checked against the fixtures, and the four
direct kernel calls of tests/test_gpu_cluster_kernels.py on the same stream, checked against their restatements.

It runs in a process of its own because a stream, once created, stays with the process for its lifetime, and the runtime maps
every stream of a process onto a few hardware queues (toothgroupnetwork_amd/_lib.py): an extra stream in the test process would
change which queues the streams of later tests share.  Prints "cluster stream ok" and exits 0 when every result matches."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cluster_kernels_ref as R  # noqa: E402
import test_gpu_cluster_kernels as K  # noqa: E402  (its gpu_* helpers launch on the current stream)
from cluster_cases import dbscan_cases, labelling_cases, mean_shift_cases, unpack_core  # noqa: E402
from toothgroupnetwork_amd import cluster  # noqa: E402


def main():
    fix = np.load(os.path.join(HERE, "golden", "reference_cpu_r9_cluster.npz"))
    dev = torch.device("cuda", 0)
    x, eps, ms, _ = dbscan_cases()["blobs"]
    pts = torch.from_numpy(x).to(dev)
    moved, cls = labelling_cases()["split"]
    m, c = torch.from_numpy(moved).to(dev), torch.from_numpy(cls).to(dev)
    ms_x, ms_bw, _, _ = mean_shift_cases()["n257"]
    rng = np.random.default_rng(17)
    nc_x, nc_c = rng.normal(0, 0.1, (700, 3)), rng.normal(0, 0.1, (17, 3))
    mo_x, mo_lab, mo_mask, mo_nlab = K._moments_case("n255")
    vo_lab, vo_idx = np.array([3, 7, 205], np.int64)[rng.integers(0, 3, 400)], rng.integers(0, 400, (600, 10))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        lab, core = cluster.dbscan(pts, eps, ms)
        fg = cluster.get_clustering_labels(m, c)
        assert torch.cuda.current_stream() == s
        seeds_m, seeds_c = K.gpu_seeds(ms_x, ms_bw, 300)
        near = K.gpu_nearest(nc_x, nc_c)
        mo_count, mo_mean, mo_cov = K.gpu_moments(mo_x, mo_lab, mo_mask, mo_nlab)
        votes = K.gpu_vote(vo_idx, vo_lab)
    s.synchronize()
    want_m, want_c = R.mean_shift_seeds(ms_x, ms_bw, 300)
    exact = R.moments_exact(mo_x, mo_lab, mo_mask, mo_nlab)
    mean_ok, cov_ok, _ = R.moments_within(len(mo_x), mo_mean, mo_cov, exact)
    checks = {
        "dbscan labels": np.array_equal(lab.cpu().numpy(), fix["db_blobs_labels"].astype(np.int64)),
        "dbscan core": np.array_equal(core.cpu().numpy(), unpack_core(fix["db_blobs_core"], len(x))),
        "get_clustering_labels": np.array_equal(fg.cpu().numpy(), fix["cl_split_labels"].astype(np.int64)),
        "tgn_mean_shift": np.array_equal(seeds_m.view(np.int64), want_m.view(np.int64)) and np.array_equal(seeds_c, want_c),
        "tgn_nearest_center": np.array_equal(near, R.nearest_center(nc_x, nc_c)),
        "tgn_cluster_moments": np.array_equal(mo_count, exact[0]) and bool(mean_ok.all() and cov_ok.all()),
        "tgn_cluster_vote": np.array_equal(votes, R.vote(vo_idx, vo_lab)),
    }
    bad = [k for k, v in checks.items() if not v]
    if bad:
        print("cluster stream mismatch:", ", ".join(bad))
        return 1
    print("cluster stream ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
