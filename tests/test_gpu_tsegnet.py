"""GPU: tsegnet's join and painting (csrc/tsegnet.hip, toothgroupnetwork_amd/tsegnet.py), nets.TSegNetModule and
inference.TSegNetInferencePipeLine.
  * against the REFERENCE's own classes run on CPU (tests/golden/reference_cpu_r11_tsegnet.npz, make_golden_r11_tsegnet.py): kept mask,
    compaction order, DBSCAN labels, cluster centres (float32 bits), chosen crops, index sets, crop channels 0..34 (bits), raw crop
    labels, painted labels, the pipeline's label per vertex -- equal; the distance channel by the project's rule for float32 results
    (within_reference_noise: at most 2x the reference's own float32 error against its float64 evaluation in rms, 4x in maximum,
    floors 1e-6 / 1e-5);
  * each kernel alone through the C ABI against tests/tsegnet_ref.py on small seeded shapes, bad indices and a non-default stream;
  * the module with real seeded networks against composing the two networks and the host functions by hand.
Reads fixtures only: neither the reference tree nor sklearn."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsegnet_cases as TC  # noqa: E402
import tsegnet_ref as R  # noqa: E402
from crop_cases import unpack_sets  # noqa: E402
from seeded import seeded_fill  # noqa: E402
from tsegnet_ref import within_reference_noise  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_BIT = 2


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r11_tsegnet.npz")))


@pytest.fixture(scope="module")
def case(fx):
    c = TC.module_case()
    assert TC.case_digest(c) == fx["mod_digest"][0], "the case no longer rebuilds the fixture's input"
    return c


@pytest.fixture(scope="module")
def joined(dev, fx, case):
    """The join on the module case, stage by stage through the host layer."""
    from toothgroupnetwork_amd import cluster, tsegnet as T
    t = {n: torch.from_numpy(v).to(dev) for n, v in case.items()}
    moved, counts = T.centroid_proposals(t["l3_xyz"], t["offset"], t["dist"])
    labels, _ = cluster.dbscan(moved, T.EPS, T.MIN_SAMPLES, np.cumsum(counts).tolist())
    cents = T.cluster_centers(moved, counts)
    np.random.seed(TC.PERM_SEED)
    perm = np.random.permutation(cents[0].shape[0])[:TC.MAX_CROPS]
    chosen = [cents[0][torch.from_numpy(perm).to(dev)]]
    cropped, idx, crop_labels = T.crop_features(t["feats"], t["l0_points"], chosen, TC.CROP_K, t["labels"])
    torch.cuda.synchronize()
    return dict(t=t, moved=moved, counts=counts, labels=labels, cents=cents, perm=perm, cropped=cropped, idx=idx, crop_labels=crop_labels)


# ---- against the reference's fixture ------------------------------------------------------------------------------------------

def test_proposals_clusters_and_centres_equal_the_reference(joined, fx, case):
    want_moved, want_counts, kept = R.proposals(case["l3_xyz"], case["offset"], case["dist"])
    assert np.array_equal(kept[0], np.unpackbits(fx["mod_kept"])[:TC.N_COARSE].astype(bool))
    assert joined["counts"] == want_counts.tolist()
    assert np.array_equal(joined["moved"].cpu().numpy().view(np.uint32), want_moved.view(np.uint32)), "kept points or their order"
    assert np.array_equal(joined["labels"].cpu().numpy(), fx["mod_db_labels"].astype(np.int64))
    assert len(joined["cents"]) == 1
    assert np.array_equal(joined["cents"][0].cpu().numpy().view(np.uint32), fx["mod_cent_bits"]), "cluster centres are not bit-equal"
    assert np.array_equal(joined["perm"], fx["mod_perm"])


def test_crops_equal_the_reference(joined, fx):
    assert len(joined["idx"]) == 1
    idx = joined["idx"][0].cpu().numpy()
    assert idx.shape == (TC.MAX_CROPS, TC.CROP_K)
    assert np.array_equal(np.sort(idx, axis=1), unpack_sets(fx["mod_idxset"]))
    cropped = joined["cropped"].cpu().numpy()
    assert cropped.shape == (TC.MAX_CROPS, 36, TC.CROP_K)
    srt = R.sorted_columns(cropped, idx)
    assert np.array_equal(srt[:, :35, ::64].view(np.uint32), fx["mod_crop"].view(np.uint32)), "channels 0..34 are bit copies"
    lab = R.sorted_columns(joined["crop_labels"].cpu().numpy(), idx)
    assert lab.dtype == np.int64 and np.array_equal(lab[:, :, ::64], fx["mod_crop_labels"].astype(np.int64))
    assert not np.isnan(cropped[:, 35]).any()
    within_reference_noise("ddf channel (kernel)", srt[:, 35, ::4], fx["mod_ddf32"], fx["mod_ddf64"])


def _scripted(joined, dev):
    _, _, pd_2, id_pred = TC.fixed_seg(joined["cropped"])
    idx = joined["idx"][0].cpu().numpy()
    return torch.from_numpy(TC.plant(pd_2.cpu().numpy(), idx)).to(dev), id_pred, idx


def test_painted_labels_equal_the_reference(joined, fx, dev):
    from toothgroupnetwork_amd import tsegnet as T
    pd_2, id_pred, idx = _scripted(joined, dev)
    cols = np.argsort(idx[-1], kind="stable")[:len(TC.PLANTED)]
    mask = (torch.sigmoid(pd_2[:, 0]) > 0.5).cpu().numpy()
    assert mask[-1, cols].tolist() == [False, False, False, False, True, True], "the mask is sigmoid(x) > 0.5 in float32"
    got = T.paint_labels(joined["idx"], pd_2, id_pred, TC.N_POINTS)
    assert got.dtype == torch.int64 and tuple(got.shape) == (1, TC.N_POINTS)
    assert np.array_equal(got[0].cpu().numpy(), fx["paint_labels"].astype(np.int64))
    assert torch.equal(got, T.paint_labels(joined["idx"], pd_2[:, 0].contiguous(), id_pred, TC.N_POINTS))


def test_pipeline_labels_equal_the_reference(fx, dev, tmp_path):
    from toothgroupnetwork_amd import inference, synth
    assert tuple(fx["pipe_mesh"]) == TC.MESH
    path = str(tmp_path / "scan.obj")
    with open(path, "w") as f:
        f.write(synth.obj_text(TC.MESH[0], TC.MESH[1], TC.MESH[2], "plain", with_tail=False))
    model = types.SimpleNamespace(cent_module=TC.Stage(TC.fixed_cent), seg_module=TC.Stage(TC.fixed_seg), get_ddf=None)
    pipe = inference.TSegNetInferencePipeLine(model)
    out = pipe(path)
    assert np.array_equal(out["sem"], out["ins"]) and out["sem"].shape == (TC.MESH[0] * TC.MESH[1],)
    assert np.array_equal(np.asarray(out["sem"]).astype(np.int64), fx["pipe_sem"].astype(np.int64))
    assert set(pipe.times) == {"load", "sample", "centroids", "join", "segmentation", "paint", "transfer"}
    small = str(tmp_path / "small.obj")
    with open(small, "w") as f:
        f.write(synth.obj_text(40, 30, 5, "plain", with_tail=False))
    with pytest.raises(NotImplementedError):
        pipe(small)


# ---- each kernel alone, through the C ABI ----------------------------------------------------------------------------------------

def _lib():
    from toothgroupnetwork_amd import _lib as L
    return L


def _take_error():
    L = _lib()
    return L.lib().tgn_take_index_error(L.stream())


def _run(fn, side_stream):
    """fn() on the current stream or on a fresh non-default one."""
    if not side_stream:
        return fn()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = fn()
        s.synchronize()
    return out


@pytest.mark.parametrize("mode", ["none", "all", "mixed"])
@pytest.mark.parametrize("M", [1, 64, 256, 1000])
def test_proposals_kernel(dev, M, mode):
    L = _lib()
    B = 3
    rng = np.random.default_rng(100 + M)
    l3 = rng.standard_normal((B, 3, M)).astype(np.float32)
    off = (rng.standard_normal((B, 3, M)) * 0.1).astype(np.float32)
    dist = {"none": np.full((B, 1, M), 0.5, np.float32), "all": np.full((B, 1, M), 0.1, np.float32),
            "mixed": (rng.random((B, 1, M)) * 0.6).astype(np.float32)}[mode]
    if mode == "mixed":                                         # ragged: scan 1 keeps nothing, the boundary values in scan 2
        dist[1] = 0.4
        dist[2, 0, 0] = np.float32(0.3)
        dist[2, 0, M // 2] = np.nextafter(np.float32(0.3), np.float32(0))
        dist[2, 0, M - 1] = np.nan
    want, want_counts, _ = R.proposals(l3, off, dist)
    a, b, c = (torch.from_numpy(v).to(dev) for v in (l3, off, dist))
    moved = torch.full((B * M, 3), -7.0, dtype=torch.float32, device=dev)
    counts = torch.full((B,), -1, dtype=torch.int32, device=dev)

    def launch():
        L.check(L.lib().tgn_tsg_proposals(B, M, L.ptr(a), L.ptr(b), L.ptr(c), 0.3, L.ptr(moved), L.ptr(counts), L.stream()), "tgn_tsg_proposals")
    _run(launch, side_stream=(M == 256))
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == want_counts.tolist()
    K = int(want_counts.sum())
    assert np.array_equal(moved[:K].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert bool((moved[K:] == -7.0).all()), "rows behind the kept points must stay untouched"


def test_proposals_kernel_refuses_bad_shapes(dev):
    L = _lib()
    z = torch.zeros(4, device=dev)
    assert L.lib().tgn_tsg_proposals(1, 1025, L.ptr(z), L.ptr(z), L.ptr(z), 0.3, L.ptr(z), L.ptr(z), L.stream()) == L.ERR_INVALID_ARGUMENT
    assert L.lib().tgn_tsg_proposals(0, 4, L.ptr(z), L.ptr(z), L.ptr(z), 0.3, L.ptr(z), L.ptr(z), L.stream()) == L.ERR_INVALID_ARGUMENT
    assert L.lib().tgn_tsg_proposals(1, 4, None, L.ptr(z), L.ptr(z), 0.3, L.ptr(z), L.ptr(z), L.stream()) == L.ERR_INVALID_ARGUMENT


def _crop_inputs(k, cf, seed, B=3, N=5000, per_scan=(2, 0, 3)):
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((B, 6, N)).astype(np.float32)
    feats[:, :3] *= np.float32(0.3)                             # distances of about 0.5: the distance feature is about 0.1
    l0 = rng.standard_normal((B, cf, N)).astype(np.float32)
    labels = rng.integers(-1, 16, (B, N)).astype(np.int64)
    scan = np.repeat(np.arange(B, dtype=np.int32), per_scan)
    T = len(scan)
    idx = rng.integers(0, N, (T, k)).astype(np.int64)
    cent = (rng.standard_normal((T, 3)) * 0.3).astype(np.float32)
    return feats, l0, labels, scan, idx, cent


def _launch_crop_features(dev, feats, l0, labels, scan, idx, cent, side_stream=False):
    L = _lib()
    B, C, N = feats.shape
    cf, (T, k) = l0.shape[1], idx.shape
    d = [torch.from_numpy(v).to(dev) for v in (feats, l0, labels, scan, idx, cent)]
    out = torch.full((T, 3 + cf + 1, k), -7.0, dtype=torch.float32, device=dev)
    out_lab = torch.full((T, 1, k), -7, dtype=torch.int64, device=dev)

    def launch():
        L.check(L.lib().tgn_clear_index_error(L.stream()), "clear")
        L.check(L.lib().tgn_tsg_crop_features(B, N, C, cf, T, k, L.ptr(d[0]), L.ptr(d[1]) if cf else None, L.ptr(d[3]), L.ptr(d[5]), L.ptr(d[4]),
                                              L.ptr(d[2]), L.ptr(out), L.ptr(out_lab), L.stream()), "tgn_tsg_crop_features")
        return _take_error()
    err = _run(launch, side_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_lab.cpu().numpy(), err


@pytest.mark.parametrize("k", [1, 100, 3072])
@pytest.mark.parametrize("cf", [0, 5, 32])
def test_crop_features_kernel(dev, cf, k):
    feats, l0, labels, scan, idx, cent = _crop_inputs(k, cf, 200 + 7 * cf + k)
    got, got_lab, err = _launch_crop_features(dev, feats, l0, labels, scan, idx, cent, side_stream=(cf == 5))
    want, want_lab = R.crop_features(feats, l0, scan, cent, idx, labels)
    assert err == 0
    assert np.array_equal(got[:, :3 + cf].view(np.uint32), want[:, :3 + cf].view(np.uint32))
    assert np.array_equal(got_lab, want_lab)
    assert not np.isnan(got[:, 3 + cf]).any()
    within_reference_noise(f"ddf cf={cf} k={k}", got[:, 3 + cf], want[:, 3 + cf], R.ddf64(want[:, :3], cent))


def test_crop_features_kernel_latches_bad_indices(dev):
    feats, l0, labels, scan, idx, cent = _crop_inputs(100, 5, 311)
    N = feats.shape[2]
    idx[1, 7], idx[3, 99] = N, -1
    got, got_lab, err = _launch_crop_features(dev, feats, l0, labels, scan, idx, cent)
    assert err & ERR_BIT, "an index outside [0, N) must latch bit 1 of the error word"
    fixed = idx.copy()
    fixed[1, 7] = fixed[3, 99] = 0                               # ... and read point 0
    want, want_lab = R.crop_features(feats, l0, scan, cent, fixed, labels)
    assert np.array_equal(got[:, :8].view(np.uint32), want[:, :8].view(np.uint32)) and np.array_equal(got_lab, want_lab)
    bad_scan = scan.copy()
    bad_scan[0] = 3
    _, _, err = _launch_crop_features(dev, feats, l0, labels, bad_scan, fixed, cent)
    assert err & ERR_BIT
    _, _, err = _launch_crop_features(dev, feats, l0, labels, scan, fixed, cent)
    assert err == 0, "the error word is cleared by reading it"


def test_crop_features_and_paint_launch_nothing_for_no_crops(dev):
    L = _lib()
    x = torch.zeros(1, 3, 16, device=dev)
    assert L.lib().tgn_tsg_crop_features(1, 16, 3, 0, 0, 4, L.ptr(x), None, None, None, None, None, None, None, L.stream()) == 0
    out = torch.full((1, 16), 5, dtype=torch.int64, device=dev)
    assert L.lib().tgn_tsg_paint(1, 16, 0, 4, None, None, None, None, L.ptr(out), L.stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())
    assert L.lib().tgn_tsg_crop_features(1, 16, 2, 0, 0, 4, L.ptr(x), None, None, None, None, None, None, None, L.stream()) == L.ERR_INVALID_ARGUMENT
    assert L.lib().tgn_tsg_paint(1, 16, 1, 4, None, None, None, None, L.ptr(out), L.stream()) == L.ERR_INVALID_ARGUMENT


def _launch_paint(dev, B, N, scan, idx, mask, ids, side_stream=False):
    L = _lib()
    T, k = idx.shape
    d = [torch.from_numpy(v).to(dev) for v in (scan, idx, mask, ids)]
    out = torch.full((B, N), -7, dtype=torch.int64, device=dev)

    def launch():
        L.check(L.lib().tgn_clear_index_error(L.stream()), "clear")
        L.check(L.lib().tgn_tsg_paint(B, N, T, k, L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), L.ptr(d[3]), L.ptr(out), L.stream()), "tgn_tsg_paint")
        return _take_error()
    err = _run(launch, side_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), err


@pytest.mark.parametrize("k", [1, 100, 3072])
def test_paint_kernel(dev, k):
    B, N, per_scan = 3, 4000, (4, 0, 5)
    rng = np.random.default_rng(400 + k)
    scan = np.repeat(np.arange(B, dtype=np.int32), per_scan)
    T = len(scan)
    idx = rng.integers(0, N if k > 1 else 3, (T, k)).astype(np.int64)          # heavy overlap between the crops
    mask = (rng.random((T, k)) < 0.6).astype(np.uint8) * rng.integers(1, 255, (T, k)).astype(np.uint8)
    ids = rng.integers(1, 17, T).astype(np.int64)
    got, err = _launch_paint(dev, B, N, scan, idx, mask, ids, side_stream=(k == 100))
    assert err == 0
    assert np.array_equal(got, R.paint(B, N, scan, idx, mask, ids))
    assert bool((got[1] == 0).all()), "a scan without crops is gingiva"


def test_paint_kernel_skips_and_latches_bad_indices(dev):
    B, N = 2, 500
    rng = np.random.default_rng(450)
    scan = np.array([0, 0, 1], np.int32)
    idx = rng.integers(0, N, (3, 64)).astype(np.int64)
    mask = np.ones((3, 64), np.uint8)
    ids = np.array([3, 9, 12], np.int64)
    idx[0, 5], idx[2, 9] = N, -3
    got, err = _launch_paint(dev, B, N, scan, idx, mask, ids)
    assert err & ERR_BIT
    keep = mask.copy()
    keep[0, 5] = keep[2, 9] = 0                                 # skipped
    fixed = np.clip(idx, 0, N - 1)
    assert np.array_equal(got, R.paint(B, N, scan, fixed, keep, ids))
    masked_out = mask.copy()
    masked_out[0, 5] = masked_out[2, 9] = 0                     # a bad index under a zero mask is never looked at
    _, err = _launch_paint(dev, B, N, scan, idx, masked_out, ids)
    assert err == 0
    from toothgroupnetwork_amd import tsegnet as T
    with pytest.raises(IndexError):
        T.paint_labels([torch.from_numpy(idx[:2]).to(dev), torch.from_numpy(idx[2:]).to(dev)], torch.ones(3, 1, 64, device=dev),
                       torch.eye(17, device=dev)[[3, 9, 12]], N)


# ---- the module with real networks ----------------------------------------------------------------------------------------------

def _module(dev, run_seg=True):
    from toothgroupnetwork_amd import nets
    net = nets.TSegNetModule({"run_tooth_segmentation_module": run_seg})
    seeded_fill(net, 1111)
    TC.set_heads(net)
    return net.to(dev)


def _by_hand(net, feats, labels, seed):
    from toothgroupnetwork_amd import tsegnet as T
    c = net.cent_module(feats)
    moved, counts = T.centroid_proposals(c[3], c[4], c[5])
    cents = T.cluster_centers(moved, counts)
    np.random.seed(seed)
    chosen = []
    for x in cents:
        pick = np.random.permutation(x.shape[0])[:8]
        chosen.append(x[torch.from_numpy(pick).to(x.device)])
    cropped, idx, lab = T.crop_features(feats, c[0], chosen, 3072, labels)
    # eval mode: the segmentation network sees one scan's crops at a time (TSegNetModule.segment), train mode all crops at once
    parts = [net.seg_module(x) for x in cropped.split([c_.shape[0] for c_ in chosen])] if not net.training else [net.seg_module(cropped)]
    seg = tuple(torch.cat(p) for p in zip(*parts))
    return c, counts, cents, chosen, cropped, idx, lab, seg


@pytest.fixture(scope="module")
def scans(dev):
    a, la = TC.clumped_scan(1121)
    b, lb = TC.clumped_scan(1122)
    feats = torch.from_numpy(np.stack([a, b])).to(dev)
    labels = torch.from_numpy(np.stack([la, lb]))[:, None, :].to(dev)
    return feats, labels


KEYS = ["l0_points", "l3_points", "l0_xyz", "l3_xyz", "offset_result", "dist_result", "pd_1", "weight_1", "pd_2", "id_pred",
        "center_points", "cluster_gt_seg_label", "cropped_feature_ls"]


@pytest.fixture(scope="module")
def module_runs(dev, scans):
    """{B: (the module's outputs, the composition by hand)} for B = 1 and 2, eval mode, the same np.random.seed in front of both."""
    net = _module(dev).eval()
    feats, labels = scans
    runs = {}
    for B in (1, 2):
        f, l = feats[:B].contiguous(), labels[:B].contiguous()
        with torch.no_grad():
            np.random.seed(77)
            o = net([f, l])
            runs[B] = (o, _by_hand(net, f, l, 77))
    return runs


@pytest.mark.parametrize("B", [1, 2])
def test_module_equals_the_composition_by_hand(module_runs, B):
    o, (c, counts, cents, chosen, cropped, idx, lab, seg) = module_runs[B]
    assert list(o) == KEYS
    assert counts == [TC.N_COARSE] * B, "every proposal passes the filter with the dist head's bias at 0.25"
    assert all(x.shape[0] >= 9 for x in cents), [x.shape[0] for x in cents]      # the 8-of-T choice drops some
    for name, want in zip(KEYS[:6], c):
        assert torch.equal(o[name], want), name
    assert torch.equal(o["cropped_feature_ls"], cropped) and tuple(cropped.shape) == (8 * B, 36, 3072)
    assert torch.equal(o["cluster_gt_seg_label"], lab)
    for name, want in zip(("pd_1", "weight_1", "pd_2", "id_pred"), seg):
        assert torch.equal(o[name], want), name
    cp = o["center_points"] if B > 1 else [o["center_points"]]
    assert isinstance(cp, list) and len(cp) == B
    for got, want in zip(cp, chosen):
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (1, 8, 3)
        assert np.array_equal(got[0].view(np.uint32), want.cpu().numpy().view(np.uint32))
    assert torch.isfinite(o["pd_2"]).all() and torch.isfinite(o["id_pred"]).all()


def test_the_join_of_scan_0_does_not_depend_on_the_batch(module_runs):
    """What the centroid network and the join produce for scan 0 -- its outputs, the centres, the crops' 36 channels, the crop labels --
    is bit-equal whether the scan runs alone or as the first of two."""
    one, two = module_runs[1][0], module_runs[2][0]
    assert np.array_equal(two["center_points"][0].view(np.uint32), one["center_points"].view(np.uint32))
    assert torch.equal(two["cluster_gt_seg_label"][:8], one["cluster_gt_seg_label"])
    for name, rows in (("l0_points", 1), ("l3_points", 1), ("l3_xyz", 1), ("offset_result", 1), ("dist_result", 1), ("cropped_feature_ls", 8)):
        assert torch.equal(two[name][:rows], one[name]), f"{name}: scan 0 of the B = 2 run differs from the B = 1 run"


def test_scan_0_of_a_batch_of_two_equals_the_single_scan_run(module_runs):
    """Every output of scan 0, the segmentation network's included, bit-equal between the B = 2 and the B = 1 run.  (nets.TsgSegNet on
    all 16 crops at once gives the first eight up to 2.6e-6 relative (pd_2) away from a batch of those eight alone, although its input
    is bit-equal: the module therefore runs it scan by scan in eval mode, TSegNetModule.segment.)"""
    one, two = module_runs[1][0], module_runs[2][0]
    worst = {}
    for name in ("pd_1", "weight_1", "pd_2", "id_pred"):
        a, b = two[name][:8].double(), one[name].double()
        worst[name] = float(((a - b).abs() / (1.0 + b.abs())).max())
    print(f"scan 0, B = 2 against B = 1, max |a - b| / (1 + |b|): {worst}")
    for name in ("pd_1", "weight_1", "pd_2", "id_pred"):
        assert torch.equal(two[name][:8], one[name]), f"{name}: scan 0 of the B = 2 run differs from the B = 1 run ({worst})"


def test_module_without_the_segmentation_stage(dev, scans):
    net = _module(dev, run_seg=False).eval()
    with torch.no_grad():
        o = net([scans[0][:1].contiguous(), scans[1][:1].contiguous()])
    assert list(o) == ["l0_points", "l3_points", "l0_xyz", "l3_xyz", "offset_result", "dist_result"]
    assert tuple(o["offset_result"].shape) == (1, 3, 256) and tuple(o["dist_result"].shape) == (1, 1, 256)


def test_module_get_ddf_has_the_reference_signature(dev, joined, fx):
    from toothgroupnetwork_amd import nets
    net = nets.TSegNetModule({"run_tooth_segmentation_module": True})
    cent = fx["mod_cent_bits"].view(np.float32)[fx["mod_perm"]][None]          # (1, T, 3) numpy, as the reference passes it
    ddf = net.get_ddf(joined["cropped"][:, :3].permute(0, 2, 1), cent)
    assert tuple(ddf.shape) == (TC.MAX_CROPS, 1, TC.CROP_K)
    idx = joined["idx"][0].cpu().numpy()
    within_reference_noise("get_ddf", R.sorted_columns(ddf.cpu().numpy(), idx)[:, 0, ::4], fx["mod_ddf32"], fx["mod_ddf64"])


def test_training_gradient_reaches_l0_points_through_the_crops(dev, scans):
    from toothgroupnetwork_amd import tsegnet as T
    net = _module(dev).train()
    feats, labels = scans[0][:1].contiguous(), scans[1][:1].contiguous()
    np.random.seed(78)
    o = net([feats, labels])
    cropped, l0 = o["cropped_feature_ls"], o["l0_points"]
    assert cropped.requires_grad and l0.requires_grad
    with torch.no_grad():
        fused, idx, _ = T.crop_features(feats, l0.detach(), [o["center_points"][0]], 3072)
    assert torch.equal(cropped.detach(), fused), "the differentiable path must give the fused launch's values"
    g = torch.Generator().manual_seed(5)
    w = torch.randint(-8, 9, (8, 32, 3072), generator=g).float().to(dev)        # small integers: every sum is exact in any order
    l0.retain_grad()
    (cropped[:, 3:35] * w).sum().backward()
    want = torch.zeros_like(l0)
    for t in range(8):
        want[0].index_add_(1, idx[0][t], w[t])
    assert torch.equal(l0.grad, want)
    assert net.cent_module.fp1.mlp_convs[0].weight.grad is not None, "the segmentation input reaches the centroid trunk"
