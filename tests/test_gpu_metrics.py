"""GPU: the scoring kernels (csrc/metrics.hip) and their host layer (metrics.py, eval_sharded's scored ModelStep) against the reference's
outputs (tests/golden/reference_cpu_r14_metrics.npz) and the numpy statement of the contract (tests/metrics_ref.py).  Counts are
integers and the scores float64 arithmetic in a fixed order: every comparison here is equality."""
import os

import numpy as np
import pytest
import torch

import metrics_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r14_metrics.npz")))


@pytest.fixture(scope="module")
def M(dev):
    from toothgroupnetwork_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def P(dev):
    from toothgroupnetwork_amd import _lib
    return _lib.lib().tgn_seg_confusion_chunk()


def _t(a, dev, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)


def _tables(M, dev, gt, sem, ins, nlab, offset=None):
    a, s = M.confusion(_t(gt, dev), _t(sem, dev), None if ins is None else _t(ins, dev), nlab, offset)
    return a.cpu().numpy(), s.cpu().numpy()


def _same_scores(sc, i, want):
    """a SegScores row against metrics_ref.scores_from_tables, bit for bit (NaN included)"""
    got = [float(v[i]) for v in (sc.iou, sc.f1, sc.acc, sc.sem_acc)]
    assert R.f64_bytes(got) == R.f64_bytes([want["iou"], want["f1"], want["acc"], want["sem_acc"]])
    assert int(sc.instances[i]) == want["instances"]
    assert sc.iou_per_instance[i].cpu().numpy().tobytes() == want["iou_per_instance"].tobytes()
    assert np.array_equal(sc.matched_gt[i].cpu().numpy(), want["matched_gt"])


@pytest.mark.parametrize("case", ["upper", "lower", "one"])
def test_fixture_cases_equal_the_reference_bit_for_bit(fx, M, dev, case):
    gt, sem, ins = (fx[f"{case}_{k}"].astype(np.int64) for k in ("gt", "sem", "ins"))
    for tag, half in (("none", None), ("half", True)):
        for as_tensor in (False, True):
            args = [_t(a, dev) for a in (gt, sem, ins)] if as_tensor else [gt, sem, ins]
            iou, f1, acc, sem_acc, arr = M.cal_metric(*args, is_half=half)
            assert all(type(v) is float for v in (iou, f1, acc, sem_acc))
            assert R.f64_bytes([iou, f1, acc, sem_acc]) == fx[f"{case}_{tag}_values"].tobytes()
            assert R.f64_bytes(arr) == fx[f"{case}_{tag}_iou_arr"].tobytes()
    A, S = R.tables(gt, sem, ins, 64)
    a, s = M.confusion(_t(gt, dev), _t(sem, dev), _t(ins, dev))
    assert a.dtype == torch.int32 and tuple(a.shape) == (1, 64, 64)
    assert np.array_equal(a[0].cpu().numpy(), A) and np.array_equal(s[0].cpu().numpy(), S)
    for half in (False, True):
        _same_scores(M.scores(a, s, is_half=half), 0, R.scores_from_tables(A, S, half))


@pytest.mark.parametrize("nlab", [2, 17, 64])
def test_edge_sizes_give_equal_tables(M, dev, P, nlab):
    rng = np.random.default_rng(1400 + nlab)
    for n in (1, 63, 64, 65, P - 1, P, P + 1, 2 * P + 1):
        gt = rng.integers(0, nlab, n)
        ins = np.where(rng.random(n) < 0.7, gt, rng.integers(0, nlab, n))
        sem = np.where(rng.random(n) < 0.5, ins, rng.integers(0, nlab, n))
        A, S = R.tables(gt, sem, ins, nlab)
        a, s = _tables(M, dev, gt, sem, ins, nlab)
        assert np.array_equal(a[0], A) and np.array_equal(s[0], S), n
        assert int(A.sum()) == n


def test_one_key_on_every_vertex_is_counted_exactly(M, dev, P):
    n = 2 * P + 1
    for nlab, key in ((64, (0, 0, 0)), (64, (63, 5, 62)), (2, (1, 1, 1))):
        ins, gt, sem = (np.full(n, v, np.int64) for v in key)
        a, s = _tables(M, dev, gt, sem, ins, nlab)
        A, S = np.zeros((nlab, nlab), np.int64), np.zeros((nlab, nlab), np.int64)
        A[key[0], key[1]] = n
        S[key[0], key[2]] = n
        assert np.array_equal(a[0], A) and np.array_equal(s[0], S)


def test_ragged_batch_equals_the_single_scan_calls(M, dev, P):
    rng = np.random.default_rng(1410)
    lens = [P + 37, 0, 301, 2 * P + 1, 77]                   # an empty scan; scans that start at odd positions inside a chunk
    scans = []
    for i, n in enumerate(lens):
        gt = rng.integers(0, 49, n)
        ins = np.where(rng.random(n) < 0.8, gt, rng.integers(0, 49, n))
        sem = np.where(rng.random(n) < 0.9, ins, rng.integers(0, 49, n))
        if i == 2:
            ins = np.zeros(n, np.int64)                       # no instance
        scans.append((gt, sem, ins))
    cat = [np.concatenate([sc[k] for sc in scans]) for k in range(3)]
    off = np.cumsum(lens).tolist()
    a, s = M.confusion(*(_t(c, dev) for c in cat), 64, off)
    a2, s2 = M.confusion(*(_t(c, dev) for c in cat), 64, torch.tensor(off, dtype=torch.int32, device=dev))     # a device offset
    assert torch.equal(a, a2) and torch.equal(s, s2)
    sc = M.scores(a, s)
    dicts = M.score_scans(*([sc_[k] for sc_ in scans] for k in range(3)))
    for i, (gt, sem, ins) in enumerate(scans):
        A, S = R.tables(gt, sem, ins, 64)
        assert np.array_equal(a[i].cpu().numpy(), A) and np.array_equal(s[i].cpu().numpy(), S), i
        want = R.scores_from_tables(A, S)
        _same_scores(sc, i, want)
        if lens[i]:
            a1, s1 = M.confusion(_t(gt, dev), _t(sem, dev), _t(ins, dev))
            assert torch.equal(a1[0], a[i]) and torch.equal(s1[0], s[i])
            _same_scores(M.scores(a1, s1), 0, want)
        d = dicts[i]
        assert R.f64_bytes([d["iou"], d["f1"], d["acc"], d["sem_acc"]]) == R.f64_bytes([want[k] for k in ("iou", "f1", "acc", "sem_acc")])
        assert d["instances"] == want["instances"] and d["matched_gt"] == want["matched_gt"][want["matched_gt"] >= 0].tolist()
    for i in (1, 2):
        assert int(sc.instances[i]) == 0 and all(np.isnan(float(v[i])) for v in (sc.iou, sc.f1, sc.acc, sc.sem_acc))
        assert dicts[i]["instances"] == 0 and np.isnan(dicts[i]["iou"]) and dicts[i]["iou_per_instance"] == []
    with pytest.raises(ZeroDivisionError):
        M.cal_metric(*scans[2])
    assert M.score_scans([], []) == []


def test_labels_outside_the_range_are_left_out_and_raise(M, dev):
    from toothgroupnetwork_amd import _lib
    rng = np.random.default_rng(1420)
    n, nlab = 1000, 17
    gt, sem, ins = (rng.integers(0, nlab, n) for _ in range(3))
    gt[3], sem[500], ins[999], ins[7] = -1, nlab, nlab, -1
    A, S = R.tables(gt, sem, ins, nlab)
    assert int(A.sum()) == n - 4
    st = _lib.stream()
    _lib.lib().tgn_clear_index_error(st)
    a, s = _tables(M, dev, gt, sem, ins, nlab)
    assert np.array_equal(a[0], A) and np.array_equal(s[0], S)
    assert _lib.lib().tgn_take_index_error(st) & _lib.INDEX_ERROR_CROP
    a, s = _tables(M, dev, np.clip(gt, 0, nlab - 1), np.clip(sem, 0, nlab - 1), np.clip(ins, 0, nlab - 1), nlab)
    assert not _lib.lib().tgn_take_index_error(st)
    big = rng.integers(0, 64, n)
    bad = big.copy()
    bad[11] = 64
    with pytest.raises(IndexError):
        M.cal_metric(big, big, bad)
    low = big.copy()
    low[11] = -1
    with pytest.raises(IndexError):
        M.cal_metric(low, big, big)
    with pytest.raises(IndexError):
        M.score_scans([big, big], [big, bad])
    got, want = M.cal_metric(big, big, big), R.cal_metric(big, big, big)       # the next clean call does not raise
    assert R.f64_bytes(got[:4]) == R.f64_bytes(want[:4]) and R.f64_bytes(got[4]) == R.f64_bytes(want[4])


def test_input_forms_give_the_packed_int64_result(M, dev, P):
    rng = np.random.default_rng(1430)
    B, N, nlab = 2, P // 2 + 33, 33
    gt, sem, ins = (rng.integers(0, nlab, (B, N)) for _ in range(3))
    want_a, want_s = M.confusion(_t(gt, dev), _t(sem, dev), _t(ins, dev), nlab)
    for b in range(B):
        A, S = R.tables(gt[b], sem[b], ins[b], nlab)
        assert np.array_equal(want_a[b].cpu().numpy(), A) and np.array_equal(want_s[b].cpu().numpy(), S)

    def strided(x):                                           # every second column of a wider tensor
        wide = torch.zeros(B, 2 * N, dtype=torch.int64, device=dev)
        wide[:, ::2] = _t(x, dev)
        return wide[:, ::2]

    def offset_view(x):                                       # a contiguous view that starts one element into its storage
        flat = torch.zeros(B * N + 1, dtype=torch.int64, device=dev)
        flat[1:] = _t(x, dev).reshape(-1)
        return flat[1:].view(B, N)

    forms = {"int32": lambda x: _t(x, dev, torch.int32), "strided": strided, "offset": offset_view,
             "transposed": lambda x: _t(x, dev).t().contiguous().t()}
    for name, f in forms.items():
        views = [f(x) for x in (gt, sem, ins)]
        if name == "strided":
            assert not views[0].is_contiguous()
        if name == "offset":
            assert views[0].storage_offset() == 1 and views[0].data_ptr() % 16 == 8
        a, s = M.confusion(*views, nlab)
        assert torch.equal(a, want_a) and torch.equal(s, want_s), name
    # mixed alignment: only gt off the 16-byte grid
    a, s = M.confusion(offset_view(gt), _t(sem, dev), _t(ins, dev), nlab)
    assert torch.equal(a, want_a) and torch.equal(s, want_s)
    # ins=None means ins = sem
    a, s = M.confusion(_t(gt, dev), _t(sem, dev), None, nlab)
    a2, s2 = M.confusion(_t(gt, dev), _t(sem, dev), _t(sem, dev), nlab)
    assert torch.equal(a, a2) and torch.equal(s, s2)
    # a non-default stream
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        a, s = M.confusion(_t(gt, dev), _t(sem, dev), _t(ins, dev), nlab)
        sc = M.scores(a, s)
    side.synchronize()
    assert torch.equal(a, want_a) and torch.equal(s, want_s)
    _same_scores(sc, 1, R.scores_from_tables(*R.tables(gt[1], sem[1], ins[1], nlab)))


def _planted_logits(rng, B, C, N):
    x = rng.standard_normal((B, C, N)).astype(np.float32)
    x[0, :, 0] = 0.25                                         # every channel equal: channel 0
    x[0, C - 1, 1] = x[0, 1, 1] = 9.0                         # two equal maxima: the lower channel
    x[0, C - 1, 2] = np.nan                                   # a NaN beats every number
    x[0, 1, 3] = x[0, C - 1, 3] = np.nan                      # two NaNs: the first
    x[0, 0, 3] = np.inf
    x[B - 1, :, N - 1] = -np.inf                              # nothing but -inf: channel 0
    x[B - 1, 0, N - 2] = np.nan                               # a NaN in channel 0 stays
    return x


@pytest.mark.parametrize("shape", ["2x17x(2P+1)", "1x2x65", "2x64x4100"])
def test_confusion_from_logits_equals_confusion_of_the_argmax(M, dev, P, shape):
    B, C, N = {"2x17x(2P+1)": (2, 17, 2 * P + 1), "1x2x65": (1, 2, 65), "2x64x4100": (2, 64, 4100)}[shape]    # 4100: the 16-byte loads
    rng = np.random.default_rng(1440 + C)
    x = _planted_logits(rng, B, C, N)
    gt = rng.integers(-1, C - 1, (B, N))
    logits, g = torch.from_numpy(x).to(dev), _t(gt, dev)
    pred = torch.argmax(logits, 1)
    assert pred[0, :4].tolist() == [0, 1, C - 1, 1] and pred[B - 1, N - 2:].tolist() == [0, 0]      # what torch does with the planted vertices
    want_a, want_s = M.confusion(g + 1, pred, pred, C)
    a, s = M.confusion_from_logits(logits, g)
    assert torch.equal(a, want_a) and torch.equal(s, want_s)
    A, S = R.tables(gt[0] + 1, pred[0].cpu().numpy(), pred[0].cpu().numpy(), C)
    assert np.array_equal(a[0].cpu().numpy(), A) and np.array_equal(s[0].cpu().numpy(), S)
    a, s = M.confusion_from_logits(logits, g[:, None, :].to(torch.int32), gt_shift=1)               # (B, 1, N), int32
    assert torch.equal(a, want_a) and torch.equal(s, want_s)
    a, s = M.confusion_from_logits(logits.transpose(1, 2).contiguous().transpose(1, 2), g)          # point-major storage
    assert torch.equal(a, want_a) and torch.equal(s, want_s)
    a, s = M.confusion_from_logits(logits, g - 1, gt_shift=2)
    assert torch.equal(a, want_a) and torch.equal(s, want_s)
    half = logits.half()                                                                            # f16: the packed-fp32 result of its values
    a, s = M.confusion_from_logits(half, g)
    a2, s2 = M.confusion_from_logits(half.float().contiguous(), g)
    assert torch.equal(a, a2) and torch.equal(s, s2)
    pred16 = torch.argmax(half.float(), 1)
    a3, s3 = M.confusion(g + 1, pred16, pred16, C)
    assert torch.equal(a, a3) and torch.equal(s, s3)


class _Stub(torch.nn.Module):
    """returns stored logits, whatever it is given (as "cls_pred")"""

    def __init__(self, table):
        super().__init__()
        self.table = table

    def forward(self, inputs):
        key = int(inputs[0][0, 0, 0].item())
        return {"cls_pred": self.table[key].to(inputs[0].device)}


def _items(rng, N=512, C=17):
    items, table = [], {}
    for k in range(3):
        gt = rng.integers(-1, 16, (1, 1, N))
        x = rng.standard_normal((1, C, N)).astype(np.float32)
        if k == 1:
            x[:, 0] = 50.0                                    # every vertex predicted gingiva: nothing to score
        else:
            x[0, gt[0, 0] + 1, np.arange(N)] += 3.0
        feat = np.zeros((1, 6, N), np.float32)
        feat[0, 0, 0] = k
        items.append({"feat": torch.from_numpy(feat), "gt_seg_label": torch.from_numpy(gt), "mesh_path": [f"item{k}"]})
        table[k] = torch.from_numpy(x)
    return items, table


def test_scored_class_step_and_eval_sharded(M, dev):
    from toothgroupnetwork_amd import eval_sharded as E, training
    items, table = _items(np.random.default_rng(1450))
    model = training.PointPpFirstModel({}, module=lambda config: _Stub(table), trainable=False)
    step = E.ModelStep(model, scored=True)
    plain = E.ModelStep(model)
    outs = []
    for k, item in enumerate(items):
        out = step(k, item)
        assert tuple(out) == step.keys
        base = plain(k, item)
        assert tuple(base) == plain.keys == ("tooth_class_loss_1_val", "total_val")
        assert out["tooth_class_loss_1_val"] == base["tooth_class_loss_1_val"] and out["total_val"] == base["total_val"]
        # torch itself, not the code under test
        labels = item["gt_seg_label"] + 1
        assert out["tooth_class_loss_1_val"] == torch.nn.functional.cross_entropy(table[k].float().to(dev), labels.view(1, -1).to(dev)).item()
        pred = torch.argmax(table[k], 1).reshape(-1).numpy()
        gt = item["gt_seg_label"].reshape(-1).numpy() + 1
        if k == 1:
            assert [out[key] for key in step.keys[2:]] == [0.0, 0.0, 0.0, 0.0, 1.0]
        else:
            want = M.cal_metric(gt, pred, pred)
            assert R.f64_bytes(want[:4]) == R.f64_bytes(R.cal_metric(gt, pred, pred, nlab=17)[:4])
            assert [out[key] for key in step.keys[2:]] == [want[0], want[1], want[2], want[3], 0.0]
        outs.append(out)
    res = E.eval_sharded(["a", "b", "c"], step, 0, 1, device=dev, load=lambda p: items["abc".index(p)])
    assert res["steps"] == 3
    for key in step.keys:
        assert res["avg"][key] == (outs[0][key] + outs[1][key] + outs[2][key]) / 3      # the meter's sum, in its order
        assert np.isfinite(res["avg"][key])
    assert res["avg"]["unscored_val"] == 1.0 / 3
