"""Result files: what the reference's ScanSegmentation writes (predict_utils.py:44-61, 82-137; driven by start_inference.py) and
what its scoring script reads back (eval_visualize_results.py:59-63).

  get_jaw       "upper" / "lower" from the file name `<patient>_<jaw>.obj`, else from the first line of the OBJ file (`# upper`)
  write_output  the JSON object {"id_patient": "", "jaw", "labels", "instances"}
  predict       pipeline(scan_path) -> (labels, instances, jaw); a lower jaw's non-zero semantic labels get + 20 (FDI 11..28 -> 31..48)
  process       predict + write_output
  read_labels   the "labels" (and "instances") of such a file as int64 arrays, for metrics.cal_metric / metrics.score_scans

`pipeline` is inference.InferencePipeLine, inference.TSegNetInferencePipeLine or anything else that maps a path to
{"sem": (V,) array, "ins": (V,) array}.  Host code only.
"""
import json
import os

import numpy as np


class _NpEncoder(json.JSONEncoder):
    def default(self, obj):
        if isinstance(obj, np.integer):
            return int(obj)
        if isinstance(obj, np.floating):
            return float(obj)
        if isinstance(obj, np.ndarray):
            return obj.tolist()
        return super().default(obj)


def get_jaw(path):
    """predict_utils.py:63-80: the jaw from a name of exactly two '_'-separated parts in front of the first '.', else the first line
    of the file without its two leading characters and its newline; None when that is neither "upper" nor "lower" or the file cannot
    be read.  (As in the reference, a two-part name is taken as it is: `scan_left.obj` gives "left".)"""
    parts = os.path.basename(path).split(".")[0].split("_")
    if len(parts) == 2:
        return parts[1]
    try:
        with open(path, "r") as f:
            jaw = f.readline()[2:-1]
    except (OSError, UnicodeDecodeError):
        return None
    return jaw if jaw in ("upper", "lower") else None


def write_output(labels, instances, jaw, output_path):
    """predict_utils.py:44-61: one JSON object, keys in the reference's order"""
    with open(output_path, "w") as fp:
        json.dump({"id_patient": "", "jaw": jaw, "labels": labels, "instances": instances}, fp, cls=_NpEncoder)


def predict(pipeline, scan_path):
    """predict_utils.py:82-128 -> (labels, instances, jaw): lists of python ints, one per vertex.  As in the reference the + 20 is
    applied to result["sem"] in place, so a pipeline that returns one array under both keys gets it in "ins" too."""
    result = pipeline(scan_path)
    jaw = get_jaw(scan_path)
    if jaw == "lower":
        sem = result["sem"]
        sem[sem > 0] += 20
    elif jaw != "upper":
        raise ValueError(f"{scan_path}: the jaw is neither in the file name (<patient>_upper.obj / <patient>_lower.obj) nor in the "
                         f"file's first line (got {jaw!r})")
    instances = np.asarray(result["ins"]).astype(int).tolist()
    labels = np.asarray(result["sem"]).astype(int).tolist()
    if len(labels) != len(instances):
        raise ValueError(f"{scan_path}: {len(labels)} labels and {len(instances)} instances; the pipeline must return one of each per vertex")
    return labels, instances, jaw


def process(pipeline, input_path, output_path):
    """predict_utils.py:130-137"""
    labels, instances, jaw = predict(pipeline, input_path)
    write_output(labels, instances, jaw, output_path)


def read_labels(json_path, with_instances=False):
    """The "labels" of a result or ground-truth file as a flat int64 array (eval_visualize_results.py:59-63); with_instances: also its
    "instances" (the labels again where the file has none)."""
    with open(json_path, "r") as f:
        loaded = json.load(f)
    labels = np.array(loaded["labels"], dtype=np.int64).reshape(-1)
    if not with_instances:
        return labels
    return labels, np.array(loaded.get("instances", loaded["labels"]), dtype=np.int64).reshape(-1)
