"""The reference's per-scan evaluation loop, sharded over the GPUs of one node.

Reference: ``Trainer.test`` (trainer.py:49-54) -- one ``model.step(batch_idx, batch_item, "test")`` per scan of the
validation loader (batch size 1), each step's ``LossMap.get_loss_dict_for_print("val")`` folded into a ``LossMeter``
(loss_meter.py:2-23), ``get_avg_results()`` at the end.  Scans are independent, so rank r of `world` takes every
world-th scan (round robin over the sorted file list), nothing is exchanged while computing, and ONE
``all_gather_into_tensor`` of a small fp64 vector -- step count, seconds, the meter's sums -- combines the ranks
(sharding.gather_metrics: RCCL over xGMI on GPUs, gloo on CPU).  The averages every rank ends up with are the serial
loop's: sum over all scans / number of scans.

The model side is a *step object*: ``step(batch_idx, batch_item) -> {name_val: float, ..., total_val: float}`` with a
fixed ``keys`` tuple (the metric schema must be the same on every rank, also on a rank whose shard is empty).
``ModelStep`` makes one of a trainer's model (training.TrainingModel.evaluate, phase "test") and, with ``scored=True``, adds
the segmentation scores of every scan (metrics.py: IoU, F1, accuracy, SEM_ACC of the predicted classes) to the same meter.
Tests of the control flow hand in their own step object.
"""
import glob
import os
import time

import numpy as np
import torch

from . import launch, metrics, sharding
from .training import LossMeter, load_item


def list_preprocessed(data_dir):
    """the files DentalModelGenerator reads (generator.py:13), sorted so that every rank sees the same order"""
    return sorted(glob.glob(os.path.join(data_dir, "*_sampled_points.npy")))


class ModelStep:
    """The step object of `model`: anything with training.TrainingModel's `evaluate(batch_item, phase) -> (output, LossMap)` and a
    `val_terms` tuple, the names of its test-phase terms (training._ClassModel).  __call__ is Trainer.test's loop body:
    evaluate(batch_item, "test") and the LossMap's get_loss_dict_for_print("val").

    scored=True adds the scores of the step's prediction (metrics.confusion_from_logits on output[model.output_key] and gt_seg_label,
    then metrics.scores): iou_val, f1_val, acc_val, sem_acc_val as cal_metric gives them for torch.argmax of the logits, with the classes
    1..C-1 as instances and gingiva -1 counted as class 0.  The scores stay out of total_val, which remains the reference's sum of
    losses.  A scan with no predicted instance (every vertex gingiva) contributes 0.0 to the four scores and 1.0 to unscored_val, so
    the averages stay finite and the share of such scans is visible.  They ride in the LossMap (add_value): ONE host read per step
    fetches the loss and the scores."""
    SCORES = ("iou", "f1", "acc", "sem_acc", "unscored")

    def __init__(self, model, scored=False, is_half=False):
        if not hasattr(model, "val_terms"):
            raise TypeError(f"{type(model).__name__} declares no val_terms: every rank of a sharded validation, also one whose shard is "
                            "empty, needs the names of the step's terms before the first step, and this model does not name them")
        self.model, self.scored, self.is_half = model, scored, is_half
        self.keys = tuple(f"{t}_val" for t in model.val_terms) + ("total_val",) + (tuple(f"{n}_val" for n in self.SCORES) if scored else ())

    def __call__(self, batch_idx, batch_item):
        output, loss_map = self.model.evaluate(batch_item, "test")
        if self.scored:
            logits = output[self.model.output_key]
            sc = metrics.scores(*metrics.confusion_from_logits(logits, batch_item["gt_seg_label"].to(logits.device), gt_shift=1),
                                is_half=self.is_half)
            per_scan = torch.stack([sc.iou, sc.f1, sc.acc, sc.sem_acc])                                # (4, B) float64
            scored = sc.instances > 0
            means = torch.where(scored[None], per_scan, torch.zeros_like(per_scan)).mean(1)
            for name, value in zip(self.SCORES, [*means, (~scored).double().mean()]):
                loss_map.add_value(name, value)
        return loss_map.get_loss_dict_for_print("val")


def reference_state_dict(state):
    """A checkpoint the reference wrote holds `self.module.state_dict()` of its wrapper module (base_model.py:33-37), whose
    network sits under `first_sem_model.` (pointnet_pp.py:78) or `first_ins_cent_model.` (point_transformer.py:9) next to the
    loss's `criterion.*` entries; the network mirrors here (nets.py) are the bare networks.  Strips that prefix and drops the
    criterion entries; a state_dict of a bare network passes through unchanged."""
    prefixes = ("first_sem_model.", "first_ins_cent_model.")
    if not any(k.startswith(prefixes) for k in state):
        return state
    out = {}
    for k, v in state.items():
        if k.startswith("criterion."):
            continue
        for p in prefixes:
            if k.startswith(p):
                k = k[len(p):]
                break
        out[k] = v
    return out


def eval_sharded(paths, step, rank, world, device=None, load=load_item):
    """Trainer.test's loop over this rank's share of `paths` and the one gather.  Returns, on every rank,
    {"avg": LossMeter averages over ALL scans, "steps": scans evaluated, "per_rank_steps", "per_rank_seconds",
     "scans_per_s": steps / slowest rank's seconds}.
    A scan that fails on one rank (a load error, a step whose keys differ from its schema, a gather index out of range)
    does not leave the other ranks waiting in the collective: the rank stops its loop, carries an error flag in the
    gathered vector, and EVERY rank raises after the gather, naming the ranks that failed."""
    keys = tuple(step.keys)
    meter = LossMeter()
    mine = sharding.shard_indices(len(paths), rank, world, "round_robin")
    sharding.barrier()
    t0 = time.perf_counter()
    failure = None
    for i in mine:
        try:
            loss_map = step(i, load(paths[i]))
            if tuple(sorted(loss_map)) != tuple(sorted(keys)):
                raise KeyError(f"step returned keys {sorted(loss_map)}, its schema says {sorted(keys)}")
        except Exception as e:  # noqa: BLE001
            failure = (i, e)
            launch.note(scan_error=f"scan {i} ({os.path.basename(str(paths[i]))}): {type(e).__name__}: {str(e)[:200]}")
            break
        meter.aggr(loss_map)
    if device is not None and device.type == "cuda":
        try:
            torch.cuda.synchronize(device)
        except Exception as e:  # noqa: BLE001
            failure = failure or (-1, e)
    seconds = time.perf_counter() - t0
    vec = [float(meter.step_num), seconds, 0.0 if failure is None else 1.0] + [float(meter.loss_meter_dict.get(k, 0.0)) for k in keys]
    launch.stage("gather")
    mat = sharding.gather_metrics(vec, device=device).cpu()           # the one collective of the run
    failed = [r for r in range(mat.shape[0]) if float(mat[r, 2]) != 0.0]
    if failed:
        mine_txt = f"; here: scan {failure[0]}: {type(failure[1]).__name__}: {failure[1]}" if failure is not None else ""
        raise RuntimeError(f"evaluation failed on rank(s) {failed}{mine_txt}") from (failure[1] if failure is not None else None)
    steps = int(round(float(mat[:, 0].sum())))
    sums = mat[:, 3:].sum(0).tolist()
    slowest = float(mat[:, 1].max())
    return {"avg": {k: (s / steps if steps else float("nan")) for k, s in zip(keys, sums)}, "steps": steps,
            "per_rank_steps": [int(round(v)) for v in mat[:, 0].tolist()],
            "per_rank_seconds": [round(v, 6) for v in mat[:, 1].tolist()],
            "scans_per_s": steps / slowest if slowest > 0 else float("nan")}


def write_synthetic_preprocessed(root, n, rank=0, world=1, n_points=24000, seed=0):
    """`n` synthetic preprocessed scans in the format preprocess_data.py:52-58 writes -- (n_points, 7) float64:
    xyz, unit normal, FDI-derived label 0..16 -- for runs without the dataset.  Rank r writes every world-th file."""
    from . import synth
    os.makedirs(root, exist_ok=True)
    for i in range(rank, n, world):
        path = os.path.join(root, f"SYN{i:05d}_{'upper' if i % 2 == 0 else 'lower'}_sampled_points.npy")
        if os.path.exists(path):
            continue
        cloud = synth.arch_cloud(n_points, seed=seed + i, with_normals=True).astype(np.float64)
        # labels: 16 teeth as angular sectors of the arch + gingiva (0) below the crown line -- any fixed function of position
        ang = np.arctan2(cloud[:, 1], cloud[:, 0])
        tooth = np.clip(((ang - ang.min()) / max(float(np.ptp(ang)), 1e-9) * 16).astype(np.int64), 0, 15) + 1
        tooth[cloud[:, 2] < np.median(cloud[:, 2])] = 0
        tmp = path + f".tmp{os.getpid()}"
        with open(tmp, "wb") as f:
            np.save(f, np.concatenate([cloud[:, :6], tooth[:, None].astype(np.float64)], axis=1))
        os.replace(tmp, path)
