"""A float64 torch restatement of tsegnet's training criterion (losses.tsegnet_loss_terms), independent of the package's compositions and
of the reference's code: dense arithmetic on probabilities and logits, logaddexp / logsumexp instead of the loss modules, autograd for
the gradients; the three centroid terms come from losses_ref.centroid_terms.  tests/test_training_host.py holds it to the reference's
float64 values (tests/golden/reference_cpu_r17_training.npz) before anything is compared with it.

Also here: the criterion case's inputs rebuilt on the CPU from the r11 fixture (the crops' index sets, the chosen centres), the forward
bounds of the three segmentation terms, and the helpers the host and GPU tests share."""
import math
import os
import sys

import numpy as np
import torch

import losses_ref
from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import training_cases as C  # noqa: E402
from crop_cases import unpack_sets  # noqa: E402

U = 2.0 ** -24                      # the unit roundoff of float32
NAMES = ("dist_loss", "cent_loss", "chamf_loss", "seg_1_loss", "seg_2_loss", "id_pred_loss")


def fixture():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r17_training.npz")))


def label_centroids(xyz, labels):
    """xyz (3, N) float64, labels (N,) -> (centroid (3, 16) float64 with zero columns for absent teeth, exists (16,) bool)"""
    cent, exists = np.zeros((3, 16)), np.zeros(16, bool)
    for t in range(16):
        m = labels == t
        if m.any():
            cent[:, t], exists[t] = xyz[:, m].mean(axis=1), True
    return cent, exists


def crop_targets(centres, cent16, exists, crop_labels):
    """centres (T, 3), cent16 (3, 16), exists (16,), crop_labels (T, 1, k) numpy -> (ids (T,), bins (T, 1, k), smallest relative gap
    between the two nearest existing centroids of a centre)"""
    d = ((centres.astype(np.float64)[:, None, :] - cent16.astype(np.float64).T[None]) ** 2).sum(-1)
    d[:, ~exists] = np.inf
    ids = d.argmin(1) + 1
    two = np.sort(d, axis=1)[:, :2]
    return ids, (crop_labels + 1 == ids[:, None, None]).astype(np.int64), float(((two[:, 1] - two[:, 0]) / two[:, 1]).min())


def seg_terms(pd_1, weight_1, pd_2, id_pred, ids, bins):
    """float64 tensors (pd_1 (T, 2, k), weight_1 and pd_2 (T, 1, k), id_pred (T, 17)), ids (T,) int64 in 1..16, bins (T, 1, k) 0 / 1 ->
    (seg_1_loss, seg_2_loss, id_pred_loss, kappa): kappa = mean(lse + |x_true|) / mean(lse - x_true), the factor by which the
    cross entropy's last subtraction amplifies the relative error of its operands."""
    T = pd_1.shape[0]
    y = bins.reshape(T, -1).to(pd_1.dtype)
    p_true = pd_1[:, 1] * y + pd_1[:, 0] * (1 - y)
    w = 1 / (1 + torch.exp(-weight_1.reshape(T, -1)))
    seg_1 = ((p_true * w) ** 2 + (1 - w) ** 2).mean()
    x = pd_2.reshape(T, -1)
    bce = torch.logaddexp(torch.zeros_like(x), x) - x * y
    seg_2 = ((2 - w) * bce).mean()
    lse = torch.logsumexp(id_pred, dim=1)
    x_true = id_pred[torch.arange(T), ids]
    kappa = float((lse + x_true.abs()).mean() / (lse - x_true).mean())
    return seg_1, seg_2, (lse - x_true).mean(), kappa


def criterion_inputs(fx11):
    """The criterion case on the CPU, from the r11 fixture's crop index sets and centres: dict of float32 / int64 numpy arrays.  The
    crop columns are in ascending point order, not the kNN's: every term is a mean over them."""
    case = C.criterion_case()
    idx = unpack_sets(fx11["mod_idxset"]).astype(np.int64)                               # (T, k), ascending
    centres = fx11["mod_cent_bits"].view(np.float32)[fx11["mod_perm"].astype(np.int64)]  # (T, 3)
    crop_xyz = np.ascontiguousarray(case["feats"][0, :3][:, idx].transpose(1, 0, 2))     # (T, 3, k)
    crop_labels = case["labels"][0, 0][idx][:, None, :]
    pd_1, weight_1, pd_2, id_pred = (t.numpy() for t in C.train_seg(torch.from_numpy(crop_xyz)))
    return dict(case=case, centres=centres, crop_labels=crop_labels, pd_1=pd_1, weight_1=weight_1, pd_2=pd_2, id_pred=id_pred)


def six_terms_64(inp):
    """All six terms of the criterion case in float64 -> (dict name -> float, ids, bins, kappa)"""
    case = inp["case"]
    cent16, exists = label_centroids(case["feats"][0, :3].astype(np.float64), case["labels"][0, 0])
    ids, bins, gap = crop_targets(inp["centres"], cent16, exists, inp["crop_labels"])
    assert gap > 1e-6, "a crop centre is equidistant from two centroids"
    d = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    cent = losses_ref.centroid_terms(d(case["offset"]), d(case["l3_xyz"]), d(case["dist"]).reshape(1, -1), d(cent16)[None],
                                     torch.from_numpy(exists)[None])
    seg = seg_terms(d(inp["pd_1"]), d(inp["weight_1"]), d(inp["pd_2"]), d(inp["id_pred"]), torch.from_numpy(ids), torch.from_numpy(bins))
    return dict(zip(NAMES, [float(v) for v in cent + seg[:3]])), ids, bins, seg[3]


def forward_bound(name, n, kappa=1.0):
    """The relative forward bound (log2(n) + c) * 2^-24 of a float32 mean of n elements whose value takes c rounded operations each
    (a library function counts as 2), times kappa where the last operation subtracts."""
    # seg_1: sigmoid 2, nll * w 1, square 1, 1 - w 1, square 1, add 1, the mean's division 1
    # seg_2: exp 2, log1p 2, two additions of the cross entropy 2, sigmoid 2, 2 - w 1, product 1, the mean's division 1
    # id:    x - max 1, exp 2, the sum of 17 as ceil(log2 17) = 5, log 2, + max 1, - x_true 1, the mean's division 1
    c = {"seg_1_loss": 8, "seg_2_loss": 11, "id_pred_loss": 13}[name]
    return (math.log2(n) + c) * U * kappa


def check_grad(name, got, exact):
    """The gradient rule of tests/test_gpu_losses.py without a reference float32 run: e = |got - exact| / max|exact|, rms(e) <= 1e-6 and
    max(e) <= 1e-5."""
    got, exact = np.asarray(got, np.float64), np.asarray(exact, np.float64)
    assert got.shape == exact.shape, (name, got.shape, exact.shape)
    scale = float(np.max(np.abs(exact)))
    assert scale > 0, name
    e = np.abs(got - exact) / scale
    e_rms, e_max = float(np.sqrt(np.mean(e ** 2))), float(e.max())
    print(f"  grad {name}: rms {e_rms:.3e} max {e_max:.3e}")
    assert e_rms <= 1e-6 and e_max <= 1e-5, (name, e_rms, e_max)


def within_one_ulp(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    return bool(np.all((got == want) | (np.nextafter(want, got) == got)))
