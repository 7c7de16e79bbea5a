#!/usr/bin/env python3
"""Child process of tests/test_gpu_cluster.py: the clustering on a non-default stream, checked against the fixtures.

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

from cluster_cases import dbscan_cases, labelling_cases, unpack_core  # noqa: E402
from toothgroupnetwork_amd import cluster  # noqa: E402


def main():
    fix = np.load(os.path.join(HERE, "golden", "reference_cpu_r9_cluster.npz"))
    dev = torch.device("cuda", 0)
    x, eps, ms, _ = dbscan_cases()["blobs"]
    pts = torch.from_numpy(x).to(dev)
    moved, cls = labelling_cases()["split"]
    m, c = torch.from_numpy(moved).to(dev), torch.from_numpy(cls).to(dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        lab, core = cluster.dbscan(pts, eps, ms)
        fg = cluster.get_clustering_labels(m, c)
    s.synchronize()
    checks = {
        "dbscan labels": np.array_equal(lab.cpu().numpy(), fix["db_blobs_labels"].astype(np.int64)),
        "dbscan core": np.array_equal(core.cpu().numpy(), unpack_core(fix["db_blobs_core"], len(x))),
        "get_clustering_labels": np.array_equal(fg.cpu().numpy(), fix["cl_split_labels"].astype(np.int64)),
    }
    bad = [k for k, v in checks.items() if not v]
    if bad:
        print("cluster stream mismatch:", ", ".join(bad))
        return 1
    print("cluster stream ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
