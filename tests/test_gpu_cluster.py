"""GPU: the clustering of tgnet_fps's unlabelled path (toothgroupnetwork_amd/cluster.py, csrc/cluster.hip) against sklearn and the
reference's own ops_utils.get_clustering_labels / GroupingNetworkModule (tests/golden/reference_cpu_r9_cluster.npz, written by
make_golden_r9_cluster.py), and against the brute-force restatement of DBSCAN's rules (tests/cluster_ref.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import cluster_ref  # noqa: E402
from cluster_cases import dbscan_cases, digest, labelling_cases, unpack_core  # noqa: E402
from crop_cases import unpack_sets  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = np.load(os.path.join(HERE, "golden", "reference_cpu_r9_cluster.npz"))
DEV = torch.device("cuda", 0)
CONFIG = {"model_parameter": {"input_feat": 6, "stride": [1, 4, 4, 4, 4], "nsample": [36, 24, 24, 24, 24], "blocks": [2, 3, 4, 6, 3],
                              "block_num": 5, "planes": [32, 64, 128, 256, 512], "crop_sample_size": 3072}}


def _db(tag):
    x, eps, ms, offset = dbscan_cases()[tag]
    assert FIX[f"db_{tag}_digest"][0] == digest(x), "the case builder changed: regenerate the fixture"
    return x, eps, ms, offset, FIX[f"db_{tag}_labels"].astype(np.int64), unpack_core(FIX[f"db_{tag}_core"], len(x))


@pytest.mark.parametrize("tag", ["blobs", "chain", "border", "dups", "lattice", "noise", "ms1", "tsegnet", "ragged"])
def test_dbscan_equals_sklearn_per_cloud(tag):
    from toothgroupnetwork_amd import cluster
    x, eps, ms, offset, want_l, want_c = _db(tag)
    lo = 0
    for hi in offset:
        lab, core = cluster.dbscan(torch.from_numpy(x[lo:hi]).to(DEV), eps, ms)
        assert np.array_equal(lab.cpu().numpy(), want_l[lo:hi]), f"{tag} [{lo}, {hi}): labels"
        assert np.array_equal(core.cpu().numpy(), want_c[lo:hi]), f"{tag} [{lo}, {hi}): core flags"
        lo = hi


def test_dbscan_ragged_batch_equals_sklearn_and_counts():
    from toothgroupnetwork_amd import cluster
    x, eps, ms, offset, want_l, want_c = _db("ragged")
    lab, core, counts = cluster.dbscan_counts(torch.from_numpy(x).to(DEV), eps, ms, offset=torch.tensor(offset, dtype=torch.int32))
    assert np.array_equal(lab.cpu().numpy(), want_l) and np.array_equal(core.cpu().numpy(), want_c)
    lo, want_counts = 0, []
    for hi in offset:
        want_counts.append(want_l[lo:hi].max() + 1)
        lo = hi
    assert counts.cpu().tolist() == want_counts


def test_dbscan_bitwise_repeatable():
    from toothgroupnetwork_amd import cluster
    x, eps, ms, _, want_l, want_c = _db("blobs")
    pts = torch.from_numpy(x).to(DEV)
    a = [t.cpu().numpy() for t in cluster.dbscan(pts, eps, ms)]
    b = [t.cpu().numpy() for t in cluster.dbscan(pts, eps, ms)]
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert np.array_equal(a[0], want_l) and np.array_equal(a[1], want_c)


def test_clustering_on_a_non_default_stream():
    """In a child process (tests/cluster_stream_launcher.py): a stream created here would stay with the test process and change
    which hardware queues the streams of later tests share."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "cluster_stream_launcher.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "cluster stream ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _lab_case(tag):
    moved, cls = labelling_cases()[tag]
    assert FIX[f"cl_{tag}_digest"][0] == digest(moved, cls), "the case builder changed: regenerate the fixture"
    return moved, cls


def test_mean_shift_equals_sklearn():
    from toothgroupnetwork_amd import cluster
    moved, cls = _lab_case("split")
    fg = moved[cls != 0]
    lab, _ = cluster.dbscan(torch.from_numpy(np.ascontiguousarray(fg)).to(DEV), 0.03, 30)
    sel = lab.cpu().numpy() == int(FIX["ms_cluster"][0])
    pts = torch.from_numpy(fg[sel].astype(np.float64)).to(DEV)
    labels, centers = cluster.mean_shift(pts, 0.07)
    want = FIX["ms_centers"]
    assert np.array_equal(labels.cpu().numpy(), FIX["ms_labels"].astype(np.int64))
    assert centers.shape == want.shape
    # sklearn sums each seed's neighbours in its KDTree's order, the kernel in ascending order: equal to rounding
    assert np.max(np.abs(centers.cpu().numpy() - want)) <= 1e-14


@pytest.mark.parametrize("tag", ["nosplit", "split"])
def test_get_clustering_labels_equals_the_reference(tag):
    from toothgroupnetwork_amd import cluster
    moved, cls = _lab_case(tag)
    want = FIX[f"cl_{tag}_labels"].astype(np.int64)
    got_np = cluster.get_clustering_labels(moved, cls)
    assert isinstance(got_np, np.ndarray) and np.array_equal(got_np, want)
    got_t = cluster.get_clustering_labels(torch.from_numpy(moved).to(DEV), torch.from_numpy(cls).to(DEV))
    assert got_t.is_cuda and np.array_equal(got_t.cpu().numpy(), want)


class _Stub(torch.nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, inputs, **kwargs):
        return self.fn(inputs)


def test_grouping_module_unlabelled_forward_equals_the_reference():
    from toothgroupnetwork_amd import nets, synth
    moved, cls = _lab_case("split")
    rows, _ = synth.labelled_arch(24000, 14, seed=912)
    assert FIX["mod_digest"][0] == digest(rows, moved, cls)
    feats = torch.from_numpy(np.ascontiguousarray(rows.T))[None].to(DEV)
    sem_1 = torch.from_numpy(np.eye(10, dtype=np.float32)[cls].T.copy())[None].to(DEV)
    offset_1 = torch.from_numpy(np.ascontiguousarray((moved - rows[:, :3]).T))[None].to(DEV)
    net = nets.GroupingNetworkModule(CONFIG).to(DEV).eval()
    seen = {}
    net.first_ins_cent_model = _Stub(lambda inp: (sem_1, offset_1, None, None))

    def second(inp):
        seen["crops"] = inp[0]
        return None, None, None, None
    net.second_ins_cent_model = _Stub(second)
    out = net([feats])
    cents = net._cluster_centroids(feats[0], sem_1[0], offset_1[0])
    assert np.array_equal(cents.cpu().numpy().view(np.uint32), FIX["mod_cent_bits"])
    idx = torch.cat(out["nn_crop_indexes"]).cpu().numpy()
    assert np.array_equal(np.sort(idx, axis=1), unpack_sets(FIX["mod_idxset"]))
    got, want = seen["crops"].cpu().numpy()[:, :, ::64], FIX["mod_crop"]
    assert np.array_equal(got[:, 3:], want[:, 3:]), "feature channels"
    assert float(np.abs(got[:, :3] - want[:, :3]).max()) <= 1e-6, "centred xyz"     # the reference's centring mean is torch fp32


def test_grouping_module_unlabelled_forward_batch_is_per_scan():
    from toothgroupnetwork_amd import nets, synth
    moved, cls = _lab_case("split")
    rows, _ = synth.labelled_arch(24000, 14, seed=912)
    one = torch.from_numpy(np.ascontiguousarray(rows.T))[None]
    feats = torch.cat([one, one]).to(DEV)
    sem_1 = torch.from_numpy(np.eye(10, dtype=np.float32)[cls].T.copy())[None].repeat(2, 1, 1).to(DEV)
    offset_1 = torch.from_numpy(np.ascontiguousarray((moved - rows[:, :3]).T))[None].repeat(2, 1, 1).to(DEV)
    net = nets.GroupingNetworkModule(CONFIG).to(DEV).eval()
    net.first_ins_cent_model = _Stub(lambda inp: (sem_1, offset_1, None, None))
    net.second_ins_cent_model = _Stub(lambda inp: (None, None, None, None))
    out = net([feats])
    a, b = [t.cpu().numpy() for t in out["nn_crop_indexes"]]
    assert np.array_equal(np.sort(a, axis=1), unpack_sets(FIX["mod_idxset"])) and np.array_equal(a, b)


def test_edge_cases_raise_or_skip():
    from toothgroupnetwork_amd import cluster
    rng = np.random.default_rng(5)
    # no cluster at all: ValueError
    sparse = rng.uniform(0, 1, size=(200, 3)).astype(np.float32)
    with pytest.raises(ValueError, match="no cluster"):
        cluster.get_clustering_labels(sparse, np.ones(200, np.int64))
    # two clusters: no split test (the reference raises IndexError), noise voted
    blobs = np.concatenate([rng.normal(0, 0.005, size=(100, 3)), rng.normal(0.5, 0.005, size=(100, 3)), [[0.05, 0, 0], [0.45, 0.5, 0.5]]])
    got = cluster.get_clustering_labels(blobs.astype(np.float32), np.ones(len(blobs), np.int64))
    assert got[:100].tolist() == [0] * 100 and got[100:200].tolist() == [1] * 100 and got[200:].tolist() == [0, 1]
    # fewer than 10 labelled points: ValueError
    tiny = np.concatenate([np.zeros((5, 3)), rng.uniform(2, 3, size=(5, 3))]).astype(np.float32)
    lab_mod = cluster.DBSCAN_MIN_SAMPLES
    try:
        cluster.DBSCAN_MIN_SAMPLES = 3
        with pytest.raises(ValueError, match="fewer than the 10"):
            cluster.get_clustering_labels(tiny, np.ones(len(tiny), np.int64))
    finally:
        cluster.DBSCAN_MIN_SAMPLES = lab_mod


@pytest.mark.parametrize("seed", range(8))
def test_dbscan_random_sweep_against_the_brute_force_rules(seed):
    from toothgroupnetwork_amd import cluster
    rng = np.random.default_rng(1000 + seed)
    clouds = []
    for _ in range(int(rng.integers(1, 4))):
        k = int(rng.integers(1, 6))
        c = rng.uniform(-0.5, 0.5, size=(k, 3))
        p = np.concatenate([c[rng.integers(0, k, 300)] + rng.normal(0, rng.uniform(0.005, 0.03), size=(300, 3)),
                            rng.uniform(-0.6, 0.6, size=(int(rng.integers(0, 60)), 3))])
        if rng.integers(0, 2):
            p = np.concatenate([p, p[rng.integers(0, len(p), 40)]])
        clouds.append(p.astype(np.float32))
    x = np.concatenate(clouds)
    offset = list(np.cumsum([len(p) for p in clouds]))
    eps, ms = float(rng.uniform(0.01, 0.06)), int(rng.integers(1, 40))
    want_l, want_c = cluster_ref.dbscan_ragged(x, eps, ms, offset)
    lab, core = cluster.dbscan(torch.from_numpy(x).to(DEV), eps, ms, offset=offset)
    assert np.array_equal(lab.cpu().numpy(), want_l) and np.array_equal(core.cpu().numpy(), want_c)
