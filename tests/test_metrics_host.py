"""CPU: the scoring contract against the reference's own outputs, the result files against the reference writer's, and the argument
checks of the scoring layer that need no device (tests/golden/make_golden_r14_metrics.py made the fixture)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_ref as R
from conftest import GOLDEN, REPO


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r14_metrics.npz")))


@pytest.mark.parametrize("case", ["upper", "lower", "one"])
@pytest.mark.parametrize("tag,half", [("none", None), ("half", True)])
def test_table_contract_equals_the_reference_bit_for_bit(fx, case, tag, half):
    iou, f1, acc, sem_acc, arr = R.cal_metric(fx[f"{case}_gt"], fx[f"{case}_sem"], fx[f"{case}_ins"], half)
    assert R.f64_bytes([iou, f1, acc, sem_acc]) == fx[f"{case}_{tag}_values"].tobytes()
    assert R.f64_bytes(arr) == fx[f"{case}_{tag}_iou_arr"].tobytes()


def test_fixture_holds_the_planted_cases(fx):
    gt, sem, ins = (fx[f"upper_{k}"].astype(np.int64) for k in ("gt", "sem", "ins"))
    A, S = R.tables(gt, sem, ins, 64)
    r = R.scores_from_tables(A, S)
    m = r["matched_gt"]
    assert A[11, 11] > 0 and A[11, 12] > 0                                  # two teeth merged under one instance
    assert m[13] == 13 and m[19] == 13                                      # one tooth split, both halves vote for it
    assert m[29] == 0                                                       # a gingiva majority
    assert A[30, 15] == A[30, 16] == A[30].max() and m[30] == 15            # an exact gt tie goes to the smaller label
    assert S[21, 21] == S[21, 22] == S[21].max()                            # an exact sem tie
    assert int(np.argmax(S[23])) + 8 == m[23]                               # s + 8 == g
    assert A[40].sum() == 1 and A[63].sum() > 0                             # a single vertex; the largest label
    assert fx["upper_none_values"][3] < fx["upper_half_values"][3]
    assert fx["one_gt"].shape == (1,)
    with pytest.raises(ZeroDivisionError):
        R.cal_metric(np.zeros(5, np.int64), np.zeros(5, np.int64), np.zeros(5, np.int64))


@pytest.mark.parametrize("jaw", ["upper", "lower"])
def test_predict_and_write_output_reproduce_the_reference_file(fx, jaw, tmp_path):
    from toothgroupnetwork_amd import results
    want = json.loads(fx[f"json_{jaw}_bytes"].tobytes().decode())
    sem, ins = fx[f"json_{jaw}_sem"].astype(np.int64), fx[f"json_{jaw}_ins"].astype(np.int64)
    seen = []

    def pipeline(path):
        seen.append(path)
        return {"sem": sem.copy(), "ins": ins.copy()}

    out = tmp_path / "pred.json"
    results.process(pipeline, f"PATIENT_{jaw}.obj", str(out))
    got = json.loads(out.read_text())
    assert seen == [f"PATIENT_{jaw}.obj"]
    assert list(got) == list(want) == ["id_patient", "jaw", "labels", "instances"]
    assert got == want
    shift = 20 if jaw == "lower" else 0
    assert got["labels"] == np.where(sem > 0, sem + shift, sem).tolist() and got["instances"] == ins.tolist()
    assert out.read_bytes() == fx[f"json_{jaw}_bytes"].tobytes()
    labels, instances = results.read_labels(str(out), with_instances=True)
    assert labels.dtype == np.int64 and labels.tolist() == want["labels"] and instances.tolist() == want["instances"]
    assert results.read_labels(str(out)).tolist() == want["labels"]


def test_get_jaw_from_the_name_and_from_the_first_line(tmp_path):
    from toothgroupnetwork_amd import results
    assert results.get_jaw("/data/013FHA7K/013FHA7K_lower.obj") == "lower"
    assert results.get_jaw("013FHA7K_upper.obj") == "upper"
    for text, want in (("# upper\nv 0 0 0\n", "upper"), ("# lower\n", "lower"), ("# neither\n", None), ("", None)):
        p = tmp_path / "scan.obj"                                           # one part: the name says nothing
        p.write_text(text)
        assert results.get_jaw(str(p)) == want
    q = tmp_path / "a_b_upper.obj"                                          # three parts: the first line decides
    q.write_text("# lower\n")
    assert results.get_jaw(str(q)) == "lower"
    assert results.get_jaw(str(tmp_path / "missing.obj")) is None
    with pytest.raises(ValueError, match="jaw"):
        results.predict(lambda p: {"sem": np.zeros(3, np.int64), "ins": np.zeros(3, np.int64)}, str(tmp_path / "missing.obj"))


def test_confusion_refuses_label_counts_outside_2_to_64_before_any_launch():
    """The tables of a workgroup live in LDS, 64 x 64 at most, and there is no other kernel behind it; the check comes before the
    first HIP call (the buffers are never touched), so it holds without a device."""
    from toothgroupnetwork_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for nlab in (1, 65):
        assert L.tgn_seg_confusion(1, 1, p, p, p, p, nlab, p, p, None) == _lib.ERR_UNSUPPORTED
        assert L.tgn_last_error().decode() == (f"tgn_seg_confusion: nlab {nlab} unsupported (2 <= nlab <= 64: the tables of a "
                                               "workgroup live in LDS)")
    assert L.tgn_seg_confusion_logits(1, 65, 1, p, p, 1, p, p, None) == _lib.ERR_UNSUPPORTED
    assert L.tgn_last_error().decode() == ("tgn_seg_confusion_logits: 65 channels unsupported (2 <= C <= 64: the tables of a "
                                           "workgroup live in LDS)")
    assert L.tgn_seg_scores(1, 65, p, p, 0, p, p, p, p, None) == _lib.ERR_UNSUPPORTED
    assert L.tgn_seg_confusion_chunk() >= 64 and L.tgn_seg_confusion_chunk() % 2 == 0


def test_scoring_refuses_cpu_tensors_and_non_integer_labels():
    from toothgroupnetwork_amd import metrics
    lab = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.cal_metric(lab, lab, lab)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.confusion(lab[None], lab[None])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.confusion_from_logits(torch.zeros(1, 17, 8), lab[None])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.score_scans([lab], [lab])
    for bad in (lab.float(), lab.bool()):
        with pytest.raises(TypeError, match="^gt must"):
            metrics.confusion(bad, lab)
        with pytest.raises(TypeError, match="^sem must"):
            metrics.confusion(lab, bad)
        with pytest.raises(TypeError, match="^ins must"):
            metrics.confusion(lab, lab, bad)
        with pytest.raises(TypeError, match="^gt must"):
            metrics.confusion_from_logits(torch.zeros(1, 17, 8), bad[None])
        with pytest.raises(TypeError, match="^pred_sem_labels must"):
            metrics.cal_metric(lab, bad, lab)
    with pytest.raises(TypeError, match="^gt_labels must"):
        metrics.cal_metric(np.zeros(8, np.float32), np.zeros(8, np.int64), np.zeros(8, np.int64))
    with pytest.raises(TypeError, match="^logits must"):
        metrics.confusion_from_logits(lab[None, None], lab[None])
    assert metrics.MAX_LABELS == 64


def test_scored_steps_declare_their_schema():
    from toothgroupnetwork_amd import eval_sharded as E
    keys = ("tooth_class_loss_1_val", "total_val", "iou_val", "f1_val", "acc_val", "sem_acc_val", "unscored_val")
    fake = type("Fake", (), {"val_terms": ("tooth_class_loss_1",)})()
    assert E.ModelStep(fake, scored=True).keys == keys
    assert E.ModelStep(fake).keys == ("tooth_class_loss_1_val", "total_val")     # the unscored steps are as they were


def test_product_scoring_code_does_not_import_the_test_reference():
    for rel in ("toothgroupnetwork_amd/metrics.py", "toothgroupnetwork_amd/results.py", "tools/score_results.py", "tools/metrics_bench.py"):
        txt = open(os.path.join(REPO, rel)).read()
        assert "metrics_ref" not in txt and "import oracle" not in txt and "from oracle" not in txt


def test_score_results_tool_prints_its_help():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "score_results.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for opt in ("--gt_json_path", "--pred_json_path", "--gt_dir", "--pred_dir"):
        assert opt in r.stdout
