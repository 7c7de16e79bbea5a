#!/usr/bin/env python3
"""The geometric loss terms of a tgnet_fps training step (offset, direction, chamfer: models/tgn_loss.py:6-61, 263-302) on one
24 000-point scan with 14 teeth (synth.labelled_arch), forward plus backward to the gradient of the offsets, in three forms timed in
one process:

  loop     the reference's formulation: a python loop over the teeth with boolean-mask indexing (one host round trip per tooth) and a
           sort of the (N, T) distance matrix for the chamfer term;
  static   the static-shape torch composition: train_step_bench.losses' index_add_ terms (without its cross entropy) plus a torch
           chamfer term (two smallest of the distances to the valid centroids by topk), no host round trip;
  fused    toothgroupnetwork_amd.losses.tgn_offset_losses (csrc/loss.hip).

and tsegnet's centroid_loss (models/tsg_loss.py:57-61) at the M = 256 coarse points TsgCentroidNet produces, B = 1, 14 centroids:
a torch restatement (sorts as the reference) against losses.centroid_loss.  The forms alternate inside every repetition; a repetition
times `--inner` calls between two device events; the figure is the median over `--reps` repetitions after `--warmup`, in microseconds
per call, with the spread (min .. max).  Values of the forms are printed next to each other.  One JSON line.

    python tools/loss_bench.py [--points 24000] [--reps 20] [--inner 10] [--warmup 3] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import train_step_bench as TSB  # noqa: E402
from toothgroupnetwork_amd import losses, pointnet2_utils as U, synth  # noqa: E402

WEIGHTS = (0.03, 0.03, 0.15)      # offset_1_loss, offset_1_dir_loss, chamf_1_loss (train_configs/tgnet_fps.py)


def loop_terms(offset, xyz, label):
    """offset, xyz (N, 3), label (N,) in -1..15: the reference's loop (clamped around 0 / 0 as train_step_bench.losses_loop)."""
    cen = dirl = 0.0
    n_cen = n_dir = 0
    cents = []
    for t in range(16):
        m = label == t
        if int(m.sum()) < 5:
            continue
        n_cen += 1
        pts, off = xyz[m][None], offset[m][None]
        c = pts.mean(1, keepdim=True)
        cents.append(c.view(3))
        cen = cen + U.square_distance(pts + off, c).sum() / pts.shape[1]
        on = off.norm(dim=2, keepdim=True)
        d = (c - pts) / (c - pts).norm(dim=2, keepdim=True).clamp_min(1e-12)
        keep = on[0, :, 0] > 2e-4
        if bool(keep.any()):
            n_dir += 1
            dot = ((off / on.clamp_min(1e-12))[0][keep] * d[0][keep]).sum(1) - 1.0
            dirl = dirl + (dot * dot).mean()
    moved = (xyz + offset)[label != -1]
    two = U.square_distance(moved[None], torch.stack(cents)[None]).sort(dim=-1)[0][:, :, :2]
    return cen / n_cen, dirl / n_dir, (two[:, :, 0] / two[:, :, 1]).sum() / moved.shape[0]


def static_geo(offset, xyz, label1, teeth=17):
    """The two geometric terms of train_step_bench.losses without its cross entropy (the same lines; main() checks them against it):
    offset, xyz (N, 3), label1 (N,) = label + 1 in 0..16, 0 = gingiva -> cen / cnt + dir / cnt, and the per-tooth statistics."""
    ones = torch.ones_like(label1, dtype=torch.float32)
    n_t = torch.zeros(teeth, device=xyz.device).index_add_(0, label1, ones)
    c_t = torch.zeros(teeth, 3, device=xyz.device).index_add_(0, label1, xyz) / n_t.clamp_min(1.0)[:, None]
    valid = ((n_t >= 5) & (torch.arange(teeth, device=xyz.device) >= 1)).float()
    dist = U.square_distance((xyz + offset)[None], c_t[None])[0]
    d2 = dist.gather(1, label1[:, None])[:, 0]
    cen_t = torch.zeros(teeth, device=xyz.device).index_add_(0, label1, d2) / n_t.clamp_min(1.0)
    to_c = c_t[label1] - xyz
    d = to_c / to_c.norm(dim=1, keepdim=True).clamp_min(1e-12)
    on = offset.norm(dim=1, keepdim=True)
    keep = (on[:, 0] > 2e-4).float()
    dot = ((offset / on.clamp_min(1e-12)) * d).sum(1) - 1.0
    k_t = torch.zeros(teeth, device=xyz.device).index_add_(0, label1, keep)
    dir_t = torch.zeros(teeth, device=xyz.device).index_add_(0, label1, dot * dot * keep) / k_t.clamp_min(1.0)
    cnt = valid.sum().clamp_min(1.0)
    return (cen_t * valid).sum() / cnt + (dir_t * valid).sum() / cnt, dist, valid


def static_terms(offset, xyz, label1):
    """static_geo plus a static chamfer term on the distance matrix it already has: the two smallest distances to the valid centroids by
    topk.  No host round trip."""
    geo, dist, valid = static_geo(offset, xyz, label1)
    two = torch.where(valid[None, :] > 0, dist, torch.full_like(dist, float("inf"))).topk(2, dim=1, largest=False)[0]
    fg = (label1 != 0).float()
    return geo, ((two[:, 0] / two[:, 1]) * fg).sum() / fg.sum()


def centroid_terms_torch(offset, xyz, distance, centroid):
    """models/tsg_loss.py:4-61 restated on (B, 3, M) / (B, 3, C) tensors."""
    B, _, M = offset.shape
    x, c = xyz.permute(0, 2, 1), centroid.permute(0, 2, 1)
    near = U.square_distance(x, c).sort(dim=-1)[0][:, :, 0].sqrt()
    dist_loss = torch.nn.functional.smooth_l1_loss(distance.view(-1, M), near)
    m = x + offset.permute(0, 2, 1)
    two = U.square_distance(m, c).sort(dim=-1)[0][:, :, :2]
    mask = distance.view(-1, M) <= 0.2
    cent = (two[:, :, 0] * mask).sum() / mask.sum()
    g = U.square_distance(c, m).sort(dim=-1)[0][:, :, 0]
    cmask = g <= 0.2
    cent = cent + (g * cmask).sum() / cmask.sum()
    rmask = two[:, :, 0] <= 0.2
    return dist_loss, cent, ((two[:, :, 0] / two[:, :, 1]) * rmask).sum() / rmask.sum()


def bench(forms, reps, inner, warmup):
    """forms: {name: fn}; the forms alternate inside a repetition.  -> {name: {us, min_us, max_us}}"""
    times = {n: [] for n in forms}
    for r in range(warmup + reps):
        for n, fn in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[n].append(a.elapsed_time(b) * 1000.0 / inner)
    return {n: dict(us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v))) for n, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=24000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    dev = torch.device("cuda")
    N = args.points
    rows, lab = synth.labelled_arch(N, 14, seed=3)
    xyz_cf = torch.from_numpy(np.ascontiguousarray(rows[:, :3].T))[None].to(dev)            # (1, 3, N)
    label = torch.from_numpy(lab).to(dev)
    torch.manual_seed(0)
    offset_cf = (0.05 * torch.randn(1, 3, N, device=dev)).requires_grad_()
    xyz, label1 = xyz_cf[0].t().contiguous(), label + 1
    offset_rows = offset_cf.detach()[0].t().contiguous().requires_grad_()                   # (N, 3), as a network head emits it

    def total(terms):
        return sum(w * t for w, t in zip(WEIGHTS, terms))

    def run_loop():
        offset_rows.grad = None
        t = loop_terms(offset_rows, xyz, label)
        total(t).backward()
        return t

    def run_static():
        offset_rows.grad = None
        geo, chamf = static_terms(offset_rows, xyz, label1)
        (0.03 * geo + 0.15 * chamf).backward()
        return geo, chamf

    def run_fused():
        offset_cf.grad = None
        t = losses.tgn_offset_losses(offset_cf, xyz_cf, label[None])
        total(t).backward()
        return t
    tl, ts, tf = run_loop(), run_static(), run_fused()
    with torch.no_grad():                       # static_geo restates train_step_bench.losses' geometric lines: the same value
        both, ce = TSB.losses(offset_rows, torch.zeros(N, 17, device=dev), xyz, label1)
        assert abs(float((both - ce) / 0.03) - float(ts[0])) <= 1e-4 * abs(float(ts[0])), (float(both - ce) / 0.03, float(ts[0]))
    values = {"loop": [float(v) for v in tl], "static": [float(ts[0]), float(ts[1])], "fused": [float(v) for v in tf],
              "note": "loop / fused: offset, dir, chamf; static: offset + dir (over one count, as train_step_bench.losses), chamf"}
    tgn = bench({"loop": run_loop, "static": run_static, "fused": run_fused}, args.reps, args.inner, args.warmup)

    M, C = 256, 14
    cent = torch.stack([xyz[label == t].mean(0) for t in range(C)], dim=1)[None].contiguous()   # (1, 3, C)
    pick = torch.randperm(N, device=dev)[:M]
    x3 = xyz_cf[:, :, pick].contiguous()
    near = U.square_distance(x3.permute(0, 2, 1), cent.permute(0, 2, 1)).min(-1)
    off3 = (0.8 * (cent[0][:, near[1][0]] - x3[0]) + 0.03 * torch.randn(3, M, device=dev))[None].requires_grad_()
    dist3 = (near[0].sqrt() + 0.05 * torch.randn(1, M, device=dev)).view(1, 1, M).requires_grad_()

    def run_tsg(fn):
        def go():
            off3.grad = dist3.grad = None
            t = fn(off3, x3, dist3, cent)
            (t[0] + t[1] + 0.1 * t[2]).backward()
            return t
        return go
    forms = {"torch": run_tsg(centroid_terms_torch), "fused": run_tsg(losses.centroid_loss)}
    tsg_values = {n: [float(v) for v in fn()] for n, fn in forms.items()}
    tsg = bench(forms, args.reps, args.inner, args.warmup)
    res = {"workload": f"geometric loss terms, forward + backward, 1 x {N} points, 14 teeth; centroid_loss at 1 x {M} points, {C} centroids",
           "reps": args.reps, "inner": args.inner, "tgn_us_per_call": tgn, "tgn_values": values,
           "fused_faster_than_static": tgn["fused"]["us"] < tgn["static"]["us"],
           "centroid_us_per_call": tsg, "centroid_values": tsg_values}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
