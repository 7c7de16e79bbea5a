#!/usr/bin/env python3
"""start_inference.py over this package: every scan of a split through one of the reference's six models, one result file per scan.

    python tools/infer.py --input_dir_path 3D_scans_per_patient_obj_files --split_txt_path base_name_test_fold.txt \\
        --save_path test_results --model_name tgnet --checkpoint_path ckpts/tgnet_fps --checkpoint_path_bdl ckpts/tgnet_bdl
    python tools/infer.py ... --gpus 8 --seed 0 --gt_dir ground-truth_labels         (starts its 8 ranks itself, scores the results)

(both checkpoints come out of tools/train.py: --model_name tgnet_fps, then --model_name tgnet_bdl over the first one's file)

The six arguments of the first form are start_inference.py's, with its defaults for all but the input directory ('.h5' is appended
to both checkpoint paths, as there).  Added: --batch and --workers (inference.infer_paths), --seed (np.random.seed on every rank
before its scans: tgnet's boundary resampling draws from numpy's global generator, so its labels are a function of the seed, the
sorted list of scans and the number of ranks), --gt_dir (score the written files against ground-truth files of the same name:
metrics.score_scans), --gpus and --backend (one process per GPU, rank r takes every world-th scan of the sorted list; started and
checked as tools/preprocess_sharded.py's ranks are).

Two deliberate deviations from the reference: the scans are processed in sorted order, and --split_txt_path '' takes every
sub-directory.  A scan that fails -- a mesh one subdivision cannot lift above 24 000 points, a tgnet pass without foreground, a
file whose jaw is neither in its name nor in its first line -- is listed in the result line and the run goes on.

Rank 0 prints exactly one JSON line: metric, model_name, scans, written, failed (paths and messages), scans_per_s over the slowest
rank, mean stage times, the rank description and, with --gt_dir, the means of IoU, F1, accuracy and SEM_ACC with the share of
unscored scans.  A run that dies prints an error line instead (launch.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from toothgroupnetwork_amd import infer_run, launch  # noqa: E402


def main(argv=None, script=None, pipeline=None):
    return infer_run.main(argv, script=os.path.abspath(__file__) if script is None else script, pipeline=pipeline)


if __name__ == "__main__":
    launch.guard(main)
