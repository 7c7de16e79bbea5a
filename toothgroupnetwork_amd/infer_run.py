"""The reference's start_inference.py as a library: find the scans of a split, run them through one of the six pipelines
(inference.infer_paths), write one result file per scan (results.py), optionally score the files against ground truth, all of it
sharded over the GPUs of a node the way tools/preprocess_sharded.py is.  tools/infer.py is the command line.

  collect_scans  start_inference.py:18-32 -> the SORTED list of *.obj files
  parse_args     the reference's six flags with its names and meaning, plus --batch --workers --seed --gt_dir --gpus --backend
  output_path    save_path/<basename with .obj -> .json>  (start_inference.py:39)
  run_scans      infer_paths + results.predict + results.write_output over a list of paths; a failing scan is recorded, not fatal
  score_files    result files paired with ground-truth files by name, ONE ragged launch (metrics.score_scans) -> sums
  main           the sharded run; rank 0 prints exactly one JSON line

Deviations from start_inference.py, both deliberate: the list is sorted (the reference's order is the file system's; here the order
decides the draws of tgnet's boundary resampling, so it has to be a function of the names), and an empty --split_txt_path means every
sub-directory (the reference then matches nothing and does nothing)."""
import argparse
import glob
import os
import sys
import time

import numpy as np

from . import inference, results

METRIC = "inference scans/sec (OBJ -> result file per scan)"
BLOCK = 16          # infer_paths is called on 16 x batch paths at a time: the results of a block are written while the next one runs
STAGE_KEYS = ("load", "sample", "compute", "finish")
SCORE_KEYS = ("iou", "f1", "acc", "sem_acc")


def collect_scans(input_dir, split_txt):
    """The *.obj files of every sub-directory of input_dir, at any depth, whose base name is a line of the split file -- input_dir
    itself is not taken, as `os.walk(...)[1:]` -- sorted.  split_txt "" (or None): every sub-directory.  A split file that does not
    exist: FileNotFoundError naming it."""
    names = None
    if split_txt:
        if not os.path.isfile(split_txt):
            raise FileNotFoundError(f"the split file {split_txt!r} (--split_txt_path) does not exist")
        with open(split_txt, "r") as f:
            names = {line.strip() for line in f}
    found = []
    for dir_path in [x[0] for x in os.walk(input_dir)][1:]:
        if names is None or os.path.basename(dir_path) in names:
            found += glob.glob(os.path.join(dir_path, "*.obj"))
    return sorted(found)


def build_parser():
    ap = argparse.ArgumentParser(description="Inference models: start_inference.py over this package")
    ap.add_argument("--input_dir_path", default="3D_scans_per_patient_obj_files", type=str, help="input directory path that contain obj files.")
    ap.add_argument("--split_txt_path", default="base_name_test_fold.txt", type=str, help="split txt path; '' takes every sub-directory")
    ap.add_argument("--save_path", type=str, default="test_results", help="result save directory.")
    ap.add_argument("--model_name", type=str, default="tgnet", help="model name. list: " + " | ".join(inference.MODEL_NAMES))
    ap.add_argument("--checkpoint_path", default="ckpts/tgnet_fps", type=str, help="checkpoint path ('.h5' is appended).")
    ap.add_argument("--checkpoint_path_bdl", default="ckpts/tgnet_bdl", type=str, help="checkpoint path (for tgnet's boundary module).")
    ap.add_argument("--batch", type=int, default=8, help="scans per network call (single-network models) and a quarter of the scans per FPS launch")
    ap.add_argument("--workers", type=int, default=None, help="loader threads (default: this rank's share of the host's cores, at most 16)")
    ap.add_argument("--seed", type=int, default=None, help="np.random.seed before the run: tgnet's boundary resampling is otherwise not reproducible")
    ap.add_argument("--gt_dir", default=None, help="ground-truth *.json (searched recursively, paired by file name): score the results")
    ap.add_argument("--gpus", type=int, default=0, help="ranks of this run: without torchrun the script starts them itself")
    ap.add_argument("--backend", default=None, help="process-group backend (default: nccl = RCCL on GPUs)")
    return ap


def parse_args(argv=None):
    """-> the arguments; a --model_name that is none of the six is inference.inference_config's ValueError, before anything is started"""
    args = build_parser().parse_args(argv)
    inference.inference_config(args.model_name)
    return args


def output_path(save_path, scan_path):
    return os.path.join(save_path, os.path.basename(scan_path).replace(".obj", ".json"))


def run_scans(pipeline, paths, save_path, batch=8, workers=None):
    """Every path through infer_paths(on_error="skip"), block by block, each result written to output_path by results.predict (the jaw,
    the lower jaw's + 20) and results.write_output on a writer thread.  -> {"written": [output files], "failed": [{"path", "error"}],
    "stage_s": mean seconds per scan and stage}.  A scan whose jaw cannot be determined is a failed scan like any other."""
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(save_path, exist_ok=True)
    paths = list(paths)
    written, failed, stage_sums = [], [], {}

    def write(path, result):
        if "error" in result:
            return None, result["error"]
        try:
            labels, instances, jaw = results.predict(lambda _path: result, path)
            out = output_path(save_path, path)
            results.write_output(labels, instances, jaw, out)
            return out, None
        except Exception as e:  # noqa: BLE001
            return None, f"{type(e).__name__}: {e}"

    size = BLOCK * max(int(batch), 1)
    with ThreadPoolExecutor(max_workers=1, thread_name_prefix="tgn-write") as writer:
        writes = []
        for s in range(0, len(paths), size):
            block, stats = paths[s:s + size], {}
            answers = inference.infer_paths(pipeline, block, batch=batch, workers=workers, on_error="skip", stats=stats)
            for k, v in stats.items():
                stage_sums[k] = stage_sums.get(k, 0.0) + v * len(block)
            writes += [(p, writer.submit(write, p, r)) for p, r in zip(block, answers)]
            del answers
        for path, f in writes:
            out, error = f.result()
            if error is None:
                written.append(out)
            else:
                failed.append({"path": path, "error": error})
    return {"written": written, "failed": failed, "stage_s": {k: v / len(paths) for k, v in stage_sums.items()} if paths else {}}


def score_files(pred_paths, gt_dir):
    """Each result file with the ground-truth file of the same name below gt_dir (recursively), all pairs in one ragged launch.  As the
    reference's scoring script does, a prediction's "labels" serve as semantic and as instance labels.  -> [pairs, unscored, sums of iou,
    f1, acc, sem_acc]: a scan without an instance adds 0.0 to the four sums and 1 to `unscored`, as eval_sharded.ModelStep(scored=True) counts;
    a pair whose lengths differ is left out of `pairs`."""
    from . import metrics
    gt = {os.path.basename(p): p for p in sorted(glob.glob(os.path.join(gt_dir, "**", "*.json"), recursive=True))}
    gts, sems = [], []
    for p in pred_paths:
        if os.path.basename(p) not in gt:
            continue
        want, got = results.read_labels(gt[os.path.basename(p)]), results.read_labels(p)
        if want.shape == got.shape:
            gts.append(want)
            sems.append(got)
    scored = metrics.score_scans(gts, sems)
    have = [r for r in scored if r["instances"] > 0]
    return [float(len(scored)), float(len(scored) - len(have))] + [float(sum(r[k] for r in have)) for k in SCORE_KEYS]


def shard(paths, rank, world):
    """rank's share of the sorted list: every world-th scan (upper and lower jaws, large and small scans alternate in a sorted list)"""
    from . import sharding
    return [paths[i] for i in sharding.shard_indices(len(paths), rank, world, mode="round_robin")]


def main(argv=None, script=None, pipeline=None):
    """The run of tools/infer.py.  pipeline: a ready pipeline instead of make_inference_pipeline's (tests of the control flow)."""
    import torch.distributed as dist

    from . import launch, sharding
    args = parse_args(argv)
    if args.gpus and script is not False:
        launch.ensure_ranks(args.gpus, script or os.path.abspath(sys.argv[0]), sys.argv[1:] if argv is None else list(argv),
                            backend=args.backend, metric=METRIC)
    launch.begin(METRIC)
    if args.gpus:
        launch.require_world(args.gpus, sharding.env_rank_world()[2])
    rank, _, world, device = sharding.init_from_env(backend=args.backend)
    paths = collect_scans(args.input_dir_path, args.split_txt_path)
    mine = shard(paths, rank, world)
    launch.stage("calibrate")
    if pipeline is None:
        pipeline = inference.make_inference_pipeline(args.model_name, [args.checkpoint_path + ".h5", args.checkpoint_path_bdl + ".h5"])
    if args.seed is not None:
        np.random.seed(args.seed)
    launch.stage("timed")
    sharding.barrier()
    t0 = time.perf_counter()
    done = run_scans(pipeline, mine, args.save_path, batch=args.batch, workers=args.workers)
    seconds = time.perf_counter() - t0
    scores = score_files(done["written"], args.gt_dir) if args.gt_dir else [0.0] * (2 + len(SCORE_KEYS))
    launch.stage("gather")
    stage_sums = [done["stage_s"].get(k, 0.0) * len(mine) for k in STAGE_KEYS]
    vec = [float(len(mine)), float(len(done["written"])), float(len(done["failed"])), seconds] + stage_sums + scores
    mat = sharding.gather_metrics(vec, device=device).cpu()
    failed = [done["failed"]]
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        failed = [None] * dist.get_world_size()
        dist.all_gather_object(failed, done["failed"])
    launch.stage("report")
    who = launch.describe_ranks(device)
    if rank == 0:
        total = mat.sum(0).tolist()
        n, slowest = int(round(total[0])), float(mat[:, 3].max())
        line = {"metric": METRIC, "model_name": args.model_name, "scans": n, "written": int(round(total[1])),
                "failed": [f for part in failed for f in part], "scans_per_s": (n / slowest if slowest > 0 else float("nan")),
                "n_gpus": world, "per_rank_scans": [int(round(v)) for v in mat[:, 0].tolist()],
                "per_rank_seconds": [round(v, 6) for v in mat[:, 3].tolist()],
                # mean per scan over all ranks (thread time of a stage; null where the run has no such stage), and rank 0's own parts
                "stage_ms": {k: (round(total[4 + j] / n * 1e3, 3) if n and total[4 + j] > 0 else None) for j, k in enumerate(STAGE_KEYS)},
                "stage_ms_rank0": {k: round(v * 1e3, 3) for k, v in done["stage_s"].items()}}
        if args.gt_dir:
            base = 4 + len(STAGE_KEYS)
            pairs = int(round(total[base]))
            line.update({"scored": pairs, "unscored": (total[base + 1] / pairs if pairs else float("nan")),
                         **{k: (total[base + 2 + j] / pairs if pairs else float("nan")) for j, k in enumerate(SCORE_KEYS)}})
        launch.emit({**line, **who})
    launch.shutdown()
