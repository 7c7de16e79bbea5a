"""The scoring contract of include/tgn_pointops.h (tgn_seg_confusion, tgn_seg_scores) in numpy, independent of the kernels: two integer
tables per scan, then the reference's float64 arithmetic (eval_visualize_results.py:20-57) in its order.  tests/test_metrics_host.py
holds it to the reference's own outputs bit for bit; tests/test_gpu_metrics.py holds the kernels to it."""
import numpy as np


def tables(gt, sem, ins, nlab):
    """ins_gt[p][g], ins_sem[p][s] as int64; a vertex with any label outside [0, nlab) is left out of both"""
    gt, sem, ins = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (gt, sem, ins))
    ok = np.ones(gt.shape[0], dtype=bool)
    for a in (gt, sem, ins):
        ok &= (a >= 0) & (a < nlab)
    A = np.zeros((nlab, nlab), np.int64)
    S = np.zeros((nlab, nlab), np.int64)
    np.add.at(A, (ins[ok], gt[ok]), 1)
    np.add.at(S, (ins[ok], sem[ok]), 1)
    return A, S


def scores_from_tables(A, S, is_half=False):
    """-> dict: iou, f1, acc, sem_acc (np.float64; NaN without an instance), instances, iou_per_instance (nlab,) float64 with NaN where
    the label is absent or 0, matched_gt (nlab,) int64 with -1 there"""
    nlab = A.shape[0]
    n, insc, gtc = int(A.sum()), A.sum(1), A.sum(0)
    iou = f1 = acc = np.float64(0.0)
    hit = cnt = 0
    per = np.full(nlab, np.nan, np.float64)
    matched = np.full(nlab, -1, np.int64)
    for p in range(1, nlab):
        if insc[p] == 0:
            continue
        cnt += 1
        g, s = int(np.argmax(A[p])), int(np.argmax(S[p]))          # first maximum: np.unique + argmax
        TP = int(A[p, g])
        FP, FN = int(insc[p]) - TP, int(gtc[g]) - TP
        TN = n - TP - FP - FN
        acc = acc + np.float64(TP + TN) / np.float64(FP + TP + FN + TN)
        prec, rec = np.float64(TP) / np.float64(TP + FP), np.float64(TP) / np.float64(TP + FN)
        f1 = f1 + (np.float64(2.0) * (prec * rec)) / (prec + rec)
        per[p] = np.float64(TP) / np.float64(FP + TP + FN)
        iou = iou + per[p]
        matched[p] = g
        if s == g or (is_half and s + 8 == g):
            hit += 1
    nan = np.float64(np.nan)
    d = np.float64(cnt)
    return {"iou": iou / d if cnt else nan, "f1": f1 / d if cnt else nan, "acc": acc / d if cnt else nan,
            "sem_acc": np.float64(hit) / d if cnt else nan, "instances": cnt, "iou_per_instance": per, "matched_gt": matched}


def cal_metric(gt, sem, ins, is_half=None, nlab=64):
    """the reference's return value from the tables: (IoU, F1, ACC, SEM_ACC, IOU_arr); ZeroDivisionError without an instance"""
    A, S = tables(gt, sem, ins, nlab)
    r = scores_from_tables(A, S, bool(is_half))
    if r["instances"] == 0:
        raise ZeroDivisionError("division by zero")
    per = r["iou_per_instance"]
    return r["iou"], r["f1"], r["acc"], r["sem_acc"], per[r["matched_gt"] >= 0].tolist()


def f64_bytes(values):
    return np.asarray(values, dtype=np.float64).tobytes()
