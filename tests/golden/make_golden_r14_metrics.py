#!/usr/bin/env python3
"""Fixtures of the segmentation scores and the result files (tests/golden/reference_cpu_r14_metrics.npz), produced by running the
REFERENCE's own cal_metric (eval_visualize_results.py:20-57) and ScanSegmentation (predict_utils.py) on CPU in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_r14_metrics.py

eval_visualize_results.py cannot be imported (it parses argv, imports trimesh and open3d and loads files at import time), so its
source is parsed with `ast` and only the cal_metric definition is executed, here, at generation time.  predict_utils.py imports as it is.

Cases (labels of synth.labelled_arch(3000, 14) mapped to FDI numbers; every case is scored with is_half None and True):
  upper   FDI 11..27, the prediction derived from the ground truth with these planted (plant_upper):
            instance 11   the ground-truth teeth 11 and 12 merged under one instance
            instances 13, 19   tooth 13 split into two instances that both vote for 13
            instance 29   30 gingiva vertices and 10 of tooth 14: its majority is gingiva (g = 0)
            instance 30   k vertices of tooth 15 and k of tooth 16: an exact tie in the gt vote (asserted), goes to 15
            instance 21   its sem labels are 21 and 22 in equal numbers: an exact tie in the sem vote (asserted), goes to 21
            instance 23   sem = 15 on all of it, so s + 8 == g: counted by is_half only
            instance 40   a single vertex
            instance 63   tooth 24 predicted as 63, the largest label
  lower   FDI 31..47, sem = ins = the ground truth with 5 % of the vertices relabelled at random
  one     a scan of one vertex
Stored per case: gt, sem, ins (int16), the four values (float64) and IOU_arr for both is_half settings; and the bytes the reference's
ScanSegmentation.process writes for an upper and a lower prediction (the pipeline's arrays are stored: classes 11..28 in both jaws, the
writer adds 20 to the lower jaw's)."""
import ast
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("TGN_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from toothgroupnetwork_amd import synth  # noqa: E402
from toothgroupnetwork_amd.inference import fdi_from_classes  # noqa: E402

OUT = os.path.join(HERE, "reference_cpu_r14_metrics.npz")
SEED = 1401


def reference_cal_metric():
    tree = ast.parse(open(os.path.join(REFERENCE, "eval_visualize_results.py")).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "cal_metric"][0]
    ns = {"np": np}
    exec(compile(ast.Module([fn], []), "eval_visualize_results.py", "exec"), ns)
    return ns["cal_metric"]


def fdi_labels(seed, lower):
    _, lab = synth.labelled_arch(3000, 14, seed=seed)
    fdi = fdi_from_classes(lab + 1)                          # -1 -> 0 gingiva, teeth 0..13 -> 11..18, 21..26
    if lower:
        fdi[fdi > 0] += 20
    return fdi


def plant_upper(gt):
    ins = gt.copy()
    ins[gt == 12] = 11
    t13 = np.flatnonzero(gt == 13)
    ins[t13[: len(t13) // 3]] = 19
    gum, t14 = np.flatnonzero(gt == 0), np.flatnonzero(gt == 14)
    ins[gum[:30]] = 29
    ins[t14[:10]] = 29
    t15, t16 = np.flatnonzero(gt == 15), np.flatnonzero(gt == 16)
    k = min(len(t15), len(t16)) // 4
    ins[t15[:k]] = 30
    ins[t16[:k]] = 30
    ins[gum[40]] = 40
    ins[gt == 24] = 63
    t21 = np.flatnonzero(ins == 21)
    if len(t21) % 2:
        ins[t21[-1]] = 0
        t21 = t21[:-1]
    sem = ins.copy()
    sem[t21[len(t21) // 2:]] = 22
    sem[ins == 23] = 15
    # the planted ties are exact, and the split halves both vote for 13
    assert np.count_nonzero((ins == 30) & (gt == 15)) == np.count_nonzero((ins == 30) & (gt == 16)) == k > 0
    assert np.count_nonzero((ins == 21) & (sem == 21)) == np.count_nonzero((ins == 21) & (sem == 22)) > 0
    assert set(np.unique(gt[ins == 19])) == set(np.unique(gt[ins == 13])) == {13}
    assert np.count_nonzero(ins == 40) == 1 and np.count_nonzero(ins == 63) > 0
    u, c = np.unique(gt[ins == 29], return_counts=True)
    assert u[np.argmax(c)] == 0
    return sem, ins


def main():
    cal = reference_cal_metric()
    rng = np.random.default_rng(SEED)
    cases = {}
    gt = fdi_labels(SEED, lower=False)
    cases["upper"] = (gt,) + plant_upper(gt)
    gt = fdi_labels(SEED + 1, lower=True)
    pred = gt.copy()
    flip = rng.random(gt.shape[0]) < 0.05
    pred[flip] = rng.choice(np.unique(gt), size=int(flip.sum()))
    cases["lower"] = (gt, pred, pred.copy())
    cases["one"] = tuple(np.array([11], np.int64) for _ in range(3))
    out = {"cases": np.array(sorted(cases))}
    for name, (g, s, p) in cases.items():
        assert 0 <= min(g.min(), s.min(), p.min()) and max(g.max(), s.max(), p.max()) <= 63
        out[f"{name}_gt"], out[f"{name}_sem"], out[f"{name}_ins"] = g.astype(np.int16), s.astype(np.int16), p.astype(np.int16)
        for tag, half in (("none", None), ("half", True)):
            iou, f1, acc, sem_acc, arr = cal(g, s, p, is_half=half)
            out[f"{name}_{tag}_values"] = np.array([iou, f1, acc, sem_acc], np.float64)
            out[f"{name}_{tag}_iou_arr"] = np.array(arr, np.float64)
    assert out["upper_none_values"][3] != out["upper_half_values"][3]            # the s + 8 == g instance counts under is_half only

    sys.path.insert(0, REFERENCE)
    import predict_utils                                                          # the reference's writer, as it is
    for jaw in ("upper", "lower"):
        g = fdi_labels(SEED + 2, lower=False)
        sem, ins = g.copy(), g.copy()
        ins[g == 11] = 12                                                         # sem and ins differ in the file
        out[f"json_{jaw}_sem"], out[f"json_{jaw}_ins"] = sem.astype(np.int16), ins.astype(np.int16)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "out.json")
            predict_utils.ScanSegmentation(lambda p: {"sem": sem.copy(), "ins": ins.copy()}).process(f"PATIENT_{jaw}.obj", path)
            out[f"json_{jaw}_bytes"] = np.frombuffer(open(path, "rb").read(), dtype=np.uint8)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
