#!/usr/bin/env python3
"""Score result files against ground-truth files on the GPU: what the reference's eval_visualize_results.py prints for one pair
(IoU, F1 = TSA, SEM_ACC = TIR; no visualisation), for any number of pairs in ONE ragged launch (metrics.score_scans).

    python tools/score_results.py --gt_json_path GT.json --pred_json_path PRED.json           # one pair, or repeat both options
    python tools/score_results.py --gt_dir ground-truth/ --pred_dir test_results/             # paired by file name

Both kinds of file hold {"labels": [...], "instances": [...]} per vertex (toothgroupnetwork_amd/results.py writes the predictions).
As the reference does, a prediction's "labels" serve as semantic and as instance labels; --use_instances takes its "instances" instead.
Prints one JSON line per scan and a final line with the means over the scans that have an instance.
"""
import argparse
import glob
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def pairs_from_dirs(gt_dir, pred_dir):
    """every *.json below pred_dir with a file of the same name below gt_dir (searched recursively: the challenge's ground truth
    lies in one folder per patient)"""
    gt = {os.path.basename(p): p for p in sorted(glob.glob(os.path.join(gt_dir, "**", "*.json"), recursive=True))}
    out = []
    for p in sorted(glob.glob(os.path.join(pred_dir, "**", "*.json"), recursive=True)):
        if os.path.basename(p) in gt:
            out.append((gt[os.path.basename(p)], p))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gt_json_path", action="append", default=[], help="a ground-truth file; may be given many times")
    ap.add_argument("--pred_json_path", action="append", default=[], help="the prediction for the gt file at the same position")
    ap.add_argument("--gt_dir", help="a directory of ground-truth files (searched recursively)")
    ap.add_argument("--pred_dir", help="a directory of predictions, paired with --gt_dir by file name")
    ap.add_argument("--is_half", action="store_true", help="cal_metric's is_half: a semantic label 8 below the matched tooth counts too")
    ap.add_argument("--use_instances", action="store_true", help="take the prediction's \"instances\" as instance labels")
    a = ap.parse_args(argv)
    if len(a.gt_json_path) != len(a.pred_json_path):
        ap.error("--gt_json_path and --pred_json_path must be given the same number of times")
    if (a.gt_dir is None) != (a.pred_dir is None):
        ap.error("--gt_dir and --pred_dir go together")
    pairs = list(zip(a.gt_json_path, a.pred_json_path)) + (pairs_from_dirs(a.gt_dir, a.pred_dir) if a.gt_dir else [])
    if not pairs:
        ap.error("nothing to score: give --gt_json_path/--pred_json_path or --gt_dir/--pred_dir")

    import numpy as np
    from toothgroupnetwork_amd import metrics, results
    gts, sems, inss = [], [], []
    for gt_path, pred_path in pairs:
        gts.append(results.read_labels(gt_path))
        sem, ins = results.read_labels(pred_path, with_instances=True)
        if gts[-1].shape != sem.shape:
            sys.exit(f"{pred_path}: {sem.shape[0]} labels, {gt_path} has {gts[-1].shape[0]}")
        sems.append(sem)
        inss.append(ins if a.use_instances else sem)
    scored = metrics.score_scans(gts, sems, inss, is_half=a.is_half)
    for (gt_path, pred_path), r in zip(pairs, scored):
        print(json.dumps({"gt": gt_path, "pred": pred_path, "IoU": r["iou"], "F1(TSA)": r["f1"], "ACC": r["acc"],
                          "SEM_ACC(TIR)": r["sem_acc"], "instances": r["instances"]}))
    have = [r for r in scored if r["instances"] > 0]
    mean = {k: (float(np.mean([r[s] for r in have])) if have else float("nan"))
            for k, s in (("IoU", "iou"), ("F1(TSA)", "f1"), ("ACC", "acc"), ("SEM_ACC(TIR)", "sem_acc"))}
    print(json.dumps({"scans": len(scored), "unscored": len(scored) - len(have), **mean}))


if __name__ == "__main__":
    main()
