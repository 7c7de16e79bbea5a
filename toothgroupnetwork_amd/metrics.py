"""Scoring a predicted segmentation against its ground truth on the GPU: the reference's cal_metric
(eval_visualize_results.py:20-57) -- per predicted instance the majority ground-truth tooth, then IoU, F1 (the challenge's TSA),
accuracy and the label-agreement rate SEM_ACC (TIR) -- which the reference computes with about ten full-length numpy passes per
instance on the host.  Here the vertices are read once (csrc/metrics.hip, include/tgn_pointops.h):

  confusion              two integer tables per scan: vertices per (instance, ground-truth label) and per (instance, semantic label)
  confusion_from_logits  the same tables from a semantic network's (B, C, N) logits, torch.argmax fused in
  scores                 the four values, the instance count, per-instance IoU and matched tooth, from the tables, on the device
  cal_metric             the reference's function: same signature, same return value, bit for bit
  score_scans            many scans of different lengths in one ragged launch

The tables are integer counts and the scores float64 arithmetic in the reference's order, so nothing here has a tolerance.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib

MAX_LABELS = 64          # tgn_seg_confusion's label limit; FDI numbers reach 48

SegScores = namedtuple("SegScores", "iou f1 acc sem_acc instances iou_per_instance matched_gt")


def _label_tensor(t, name):
    """The dtype and kind check of a label argument, before the library is touched: an integer torch tensor or it is a TypeError."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor of an integer dtype, got {type(t).__name__}")
    if t.dtype == torch.bool or t.is_floating_point() or t.is_complex():
        raise TypeError(f"{name} must hold integer labels (int32 or int64), got {t.dtype}")
    return t


def _packed(t):
    return t.detach().to(torch.int64).contiguous()


def _nlab(nlab):
    nlab = int(nlab)
    if not 2 <= nlab <= MAX_LABELS:
        raise ValueError(f"nlab = {nlab} must satisfy 2 <= nlab <= {MAX_LABELS}")
    return nlab


def confusion(gt, sem, ins=None, nlab=MAX_LABELS, offset=None):
    """gt, sem, ins: integer label tensors on the GPU, all (B, N), or all flat (n,) with `offset` = pointops-style cumulative scan ends
    (a list, or an integer tensor of (b,); None: one scan).  ins=None means ins = sem.  int32 or int64, any stride or storage offset:
    they are cast and packed here.  -> (ins_gt, ins_sem), each (b, nlab, nlab) int32: ins_gt[i, p, g] = the vertices of scan i with
    ins == p and gt == g, ins_sem[i, p, s] those with ins == p and sem == s.  A vertex with a label outside [0, nlab) is left out of
    both and latches _lib.INDEX_ERROR_CROP on the stream, which is neither cleared nor read here.  No host synchronisation."""
    _label_tensor(gt, "gt"), _label_tensor(sem, "sem")
    if ins is not None:
        _label_tensor(ins, "ins")
    nlab = _nlab(nlab)
    _lib.require_cuda(gt, sem, ins, offset if isinstance(offset, torch.Tensor) else None)
    if gt.shape != sem.shape or (ins is not None and ins.shape != gt.shape):
        raise ValueError(f"gt, sem and ins must have one shape, got {tuple(gt.shape)}, {tuple(sem.shape)}"
                         + (f", {tuple(ins.shape)}" if ins is not None else ""))
    dev = gt.device
    if gt.dim() == 2 and offset is None:
        B, N = gt.shape
        n = B * N
        off = torch.arange(1, B + 1, dtype=torch.int64, device=dev).mul_(N).to(torch.int32)
    elif gt.dim() == 1:
        n = gt.shape[0]
        if offset is None:
            offset = [n]
        if isinstance(offset, torch.Tensor):
            _label_tensor(offset, "offset")
            off = offset.detach().reshape(-1).to(torch.int32).contiguous()          # (its values are the caller's: no host read)
        else:
            ends = [int(v) for v in offset]
            if any(b < a for a, b in zip([0] + ends, ends)) or (ends and ends[-1] != n):
                raise ValueError(f"offset must be non-decreasing cumulative scan ends ending at n = {n}, got {ends}")
            off = torch.tensor(ends, dtype=torch.int32).to(dev, non_blocking=True)
    else:
        raise ValueError(f"labels must be (B, N), or flat (n,) with offset; got {tuple(gt.shape)}"
                         + (" with offset" if offset is not None else ""))
    if n >= 2 ** 31:
        raise ValueError(f"{n} vertices in one launch: the limit is 2^31 - 1")
    b = int(off.shape[0])
    g, s = _packed(gt).reshape(-1), _packed(sem).reshape(-1)
    p = s if ins is None else _packed(ins).reshape(-1)
    ins_gt = torch.empty(b, nlab, nlab, dtype=torch.int32, device=dev)
    ins_sem = torch.empty(b, nlab, nlab, dtype=torch.int32, device=dev)
    _lib.ops().tgn_seg_confusion(b, n, off, g, s, p, nlab, ins_gt, ins_sem, _lib.stream())
    return ins_gt, ins_sem


def confusion_from_logits(logits, gt, gt_shift=1):
    """logits (B, C, N) of a float dtype, any layout (cast to float32 and packed here), 2 <= C <= 64; gt (B, N) or (B, 1, N) integer,
    counted as gt + gt_shift (the loaders hand gingiva as -1).  -> (ins_gt, ins_sem), each (B, C, C) int32, equal to
    confusion(gt + gt_shift, pred, pred, nlab=C) with pred = torch.argmax(logits, 1).  No host synchronisation."""
    _label_tensor(gt, "gt")
    if not isinstance(logits, torch.Tensor) or not logits.is_floating_point():
        raise TypeError(f"logits must be a floating-point torch tensor, got {getattr(logits, 'dtype', type(logits).__name__)}")
    _lib.require_cuda(logits, gt)
    if logits.dim() != 3:
        raise ValueError(f"logits must be (B, C, N), got {tuple(logits.shape)}")
    B, C, N = logits.shape
    if not 2 <= C <= MAX_LABELS:
        raise ValueError(f"{C} channels: 2 <= C <= {MAX_LABELS}")
    if gt.dim() == 3 and gt.shape[1] == 1:
        gt = gt[:, 0]
    if tuple(gt.shape) != (B, N):
        raise ValueError(f"gt must be (B, N) or (B, 1, N) = ({B}, {N}), got {tuple(gt.shape)}")
    x, g = logits.detach().to(torch.float32).contiguous(), _packed(gt)
    ins_gt = torch.empty(B, C, C, dtype=torch.int32, device=x.device)
    ins_sem = torch.empty(B, C, C, dtype=torch.int32, device=x.device)
    _lib.ops().tgn_seg_confusion_logits(B, C, N, x, g, int(gt_shift), ins_gt, ins_sem, _lib.stream())
    return ins_gt, ins_sem


def _scores_raw(ins_gt, ins_sem, is_half):
    for t, name in ((ins_gt, "ins_gt"), (ins_sem, "ins_sem")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise TypeError(f"{name} must be an int32 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    _lib.require_cuda(ins_gt, ins_sem)
    if ins_gt.dim() != 3 or ins_gt.shape[1] != ins_gt.shape[2] or ins_sem.shape != ins_gt.shape:
        raise ValueError(f"ins_gt and ins_sem must both be (b, nlab, nlab), got {tuple(ins_gt.shape)} and {tuple(ins_sem.shape)}")
    b, nlab = int(ins_gt.shape[0]), _nlab(ins_gt.shape[1])
    a, s, dev = ins_gt.contiguous(), ins_sem.contiguous(), ins_gt.device
    sc = torch.empty(b, 4, dtype=torch.float64, device=dev)
    inst = torch.empty(b, dtype=torch.int32, device=dev)
    iou_pi = torch.empty(b, nlab, dtype=torch.float64, device=dev)
    matched = torch.empty(b, nlab, dtype=torch.int32, device=dev)
    _lib.ops().tgn_seg_scores(b, nlab, a, s, 1 if is_half else 0, sc, inst, iou_pi, matched, _lib.stream())
    return sc, inst, iou_pi, matched


def scores(ins_gt, ins_sem, is_half=False):
    """The tables of confusion / confusion_from_logits -> SegScores of device tensors: iou, f1, acc, sem_acc (b,) float64 (NaN for a scan
    without an instance), instances (b,) int32, iou_per_instance (b, nlab) float64 (NaN where the label is absent or 0), matched_gt
    (b, nlab) int32 (-1 there).  The arithmetic is the reference's, value for value (include/tgn_pointops.h).  No host synchronisation."""
    sc, inst, iou_pi, matched = _scores_raw(ins_gt, ins_sem, is_half)
    return SegScores(sc[:, 0], sc[:, 1], sc[:, 2], sc[:, 3], inst, iou_pi, matched)


def _check_labels(a, name):
    """a label argument of cal_metric / score_scans: an integer tensor or an integer numpy array, or it is a TypeError"""
    if isinstance(a, torch.Tensor):
        _label_tensor(a, name)
    elif np.asarray(a).dtype.kind not in "iu":
        raise TypeError(f"{name} must hold integer labels, got {np.asarray(a).dtype}")


def _to_device(a, dev):
    """checked numpy array or tensor -> flat integer tensor on the GPU.  A tensor must already be there (no CPU fallback)."""
    if isinstance(a, torch.Tensor):
        _lib.require_cuda(a)
        return a.reshape(-1)
    arr = np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int64)
    return torch.from_numpy(arr).to(dev if dev is not None else _current_device())


def _current_device():
    if not torch.cuda.is_available():
        raise RuntimeError("toothgroupnetwork_amd operators run only on a ROCm GPU (none is visible); there is deliberately no CPU "
                           "fallback -- the CPU restatement lives in oracle/ and is test-only.")
    return torch.device("cuda", torch.cuda.current_device())


def _device_of(*arrays):
    """the device of the first GPU tensor among the arguments; None: numpy arrays go to the current GPU"""
    for a in arrays:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    return None


def _scan_dicts(host, nlab):
    """rows of [iou, f1, acc, sem_acc, instances, iou_per_instance (nlab), matched_gt (nlab)] -> one dict per scan"""
    out = []
    for row in host:
        matched = row[5 + nlab:5 + 2 * nlab].astype(np.int64)
        keep = matched >= 0
        out.append({"iou": float(row[0]), "f1": float(row[1]), "acc": float(row[2]), "sem_acc": float(row[3]), "instances": int(row[4]),
                    "iou_per_instance": row[5:5 + nlab][keep].tolist(), "instance_labels": np.flatnonzero(keep).tolist(),
                    "matched_gt": matched[keep].tolist()})
    return out


def _score_packed(g, s, p, offset, is_half, what):
    """one checked ragged launch and ONE host read of everything the callers return"""
    _lib.begin_index_check()
    a, m = confusion(g, s, p, MAX_LABELS, offset)
    sc, inst, iou_pi, matched = _scores_raw(a, m, is_half)
    packed = torch.cat([sc, inst.to(torch.float64)[:, None], iou_pi, matched.to(torch.float64)], dim=1)
    _lib.raise_on_index_error(what)
    return _scan_dicts(packed.cpu().numpy(), MAX_LABELS)


def cal_metric(gt_labels, pred_sem_labels, pred_ins_labels, is_half=None, vertices=None):
    """eval_visualize_results.py:20-57, same signature and return value: (IoU, F1, ACC, SEM_ACC, IOU_arr), four floats and the list of
    per-instance IoUs in ascending instance label, equal to the reference's as float64 bit patterns.  numpy arrays (uploaded to the
    current GPU) or GPU tensors of integer labels in [0, 64); `vertices` is unused, as in the reference.  Raises ZeroDivisionError when
    no instance is predicted, as the reference does, and IndexError for a label outside [0, 64) (through the stream's error word:
    TGN_INDEX_CHECK=off drops that check and its synchronisation).  One host read."""
    for a, name in ((gt_labels, "gt_labels"), (pred_sem_labels, "pred_sem_labels"), (pred_ins_labels, "pred_ins_labels")):
        _check_labels(a, name)
    dev = _device_of(gt_labels, pred_sem_labels, pred_ins_labels)
    g, s = _to_device(gt_labels, dev), _to_device(pred_sem_labels, dev)
    p = s if pred_ins_labels is pred_sem_labels else _to_device(pred_ins_labels, dev)
    if not (g.shape == s.shape == p.shape):
        raise ValueError(f"one label per vertex in each array: got {g.shape[0]}, {s.shape[0]} and {p.shape[0]}")
    r = _score_packed(g, s, p, None, bool(is_half), "cal_metric: a label outside [0, 64)")[0]
    if r["instances"] == 0:
        raise ZeroDivisionError("division by zero (cal_metric: no instance is predicted, every pred_ins_labels value is 0)")
    return r["iou"], r["f1"], r["acc"], r["sem_acc"], r["iou_per_instance"]


def score_scans(gt_list, sem_list, ins_list=None, is_half=False):
    """Many scans of different lengths in one ragged launch: lists of per-scan label arrays (numpy or GPU tensors), ins_list=None
    meaning ins = sem.  -> one dict per scan: iou, f1, acc, sem_acc (NaN for a scan without an instance, not an exception), instances,
    iou_per_instance / instance_labels / matched_gt (lists over the instances that occur, ascending).  IndexError for a label outside
    [0, 64).  One host read for all scans."""
    if len(gt_list) != len(sem_list) or (ins_list is not None and len(ins_list) != len(gt_list)):
        raise ValueError("gt_list, sem_list and ins_list must hold one entry per scan")
    if not len(gt_list):
        return []
    lists = [(name, arrays) for name, arrays in (("gt_list", gt_list), ("sem_list", sem_list), ("ins_list", ins_list)) if arrays is not None]
    for name, arrays in lists:
        for i, a in enumerate(arrays):
            _check_labels(a, f"{name}[{i}]")
    dev = _device_of(*gt_list, *sem_list, *(ins_list or []))
    parts = {name: [_to_device(a, dev).to(torch.int64) for a in arrays] for name, arrays in lists}
    lens = [int(t.shape[0]) for t in parts["gt_list"]]
    for name, ts in parts.items():
        if [int(t.shape[0]) for t in ts] != lens:
            raise ValueError(f"{name}: every scan needs one label per vertex, as in gt_list")
    g, s = torch.cat(parts["gt_list"]), torch.cat(parts["sem_list"])
    p = torch.cat(parts["ins_list"]) if ins_list is not None else None
    return _score_packed(g, s, p, np.cumsum(lens).tolist(), bool(is_half), "score_scans: a label outside [0, 64)")
