#!/usr/bin/env python3
"""The contrastive-boundary criterion (losses.contrast_boundary_loss) at the sizes tgnet_fps trains with: forward plus backward with
respect to the latent features, time and peak memory, against the reference's formulation in the same process.

  workloads   scan:  ONE 24 000-point scan, five decoder stages (stride 1, 4, 4, 4, 4; nsample 36, 24, 24, 24, 24), 10 classes
              crops: 14 crops of 3072 points as one batch, the same five stages, 2 classes (12 points per crop at the last stage,
                     against nsample 24: the padded lists are the workload)
              Stage i holds every 4th point of stage i-1 of every cloud; the latent features are (m_i, 32) normal draws with
              requires_grad; labels run along the arch (synth.labelled_arch).
  ours        losses.contrast_boundary_loss: integer votes, torch.where, pointops.subtraction for the (m, K-1, 32) differences
  fused       losses.contrast_boundary_loss(fused=True): the same votes and lists, every stage's distances, soft-NN sums and gradient
              in the two kernels of csrc/cbl.hip (losses.contrast_boundary_stage_fused), without the (m, K-1, 32) tensor
  reference   the reference's steps over this package's pointops: one-hot targets averaged over the kr nearest stage-0 points, labels
              and features gathered with advanced indexing to (m, K-1, ncls) and (m, K-1, 32), arg-max, boolean-mask indexing of the
              contributing rows (a host synchronisation per stage), the broadcast difference, soft nearest neighbours, mean
  difference  the part a fused distance kernel would replace, alone: pointops.subtraction, the squared sum over the 32 channels, and
              their backward -- the time, and the bytes of the (m, K-1, 32) tensors it writes (from the shapes: the difference, its
              square in the forward; the square's and the difference's gradients in the backward)
  knn         the nine neighbour searches of a step alone (five stage lists, four vote lists), through pointops.knn_indices

Every variant is timed twice: `cold`, with pointops' neighbour-list memo cleared before EVERY timed call, so each call runs all of
its searches (what the criterion costs on its own), and `memo`, with the lists of the unchanged points served from the memo (inside a
network the five stage lists are the Point-Transformer blocks' own, already in the memo; the four vote lists are the criterion's).
The reference variant's knnquery also clones the list and takes a square root of the distances, on a hit as well.

The variants alternate step by step; wall clock around a synchronised step, medians of --steps after --warmup with the quartiles as the
spread; peak memory is torch's max_memory_allocated over one step minus what was allocated before it.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

STRIDE, NSAMPLE, C = (1, 4, 4, 4, 4), (36, 24, 24, 24, 24), 32
WORKLOADS = {"scan": (1, 24000, 10), "crops": (14, 3072, 2)}


def quartiles(ms):
    q1, q2, q3 = np.percentile(ms, [25, 50, 75])
    return {"median_ms": round(float(q2), 3), "q1_ms": round(float(q1), 3), "q3_ms": round(float(q3), 3)}


def make_workload(name, dev):
    from toothgroupnetwork_amd import pointops, synth
    B, N, ncls = WORKLOADS[name]
    clouds, labels = zip(*(synth.labelled_arch(N, 14, seed=30 + b) for b in range(B)))
    target = np.stack(labels) + 1                                                   # 0 = gingiva, teeth 1..14
    target = np.where(target > 9, target - 8, target) if ncls == 10 else np.minimum(target, 1)
    xyz = torch.from_numpy(np.stack(clouds)[:, :, :3].copy()).to(dev)               # (B, N, 3)
    g = torch.Generator().manual_seed(5)
    points, latents, n = [], [], N
    for i, s in enumerate(STRIDE):
        if i:
            xyz, n = xyz[:, ::s].contiguous(), xyz[:, ::s].shape[1]
        o = pointops.register_offsets(torch.arange(1, B + 1, dtype=torch.int32, device=dev) * n, [n * (b + 1) for b in range(B)])
        points.append([xyz.reshape(-1, 3).contiguous(), o])
        latents.append((torch.randn(B * n, C, generator=g) * 0.5).to(dev).requires_grad_())
    return points, latents, torch.from_numpy(target.reshape(-1)).to(dev), ncls


def ours(points, latents, target, ncls):
    from toothgroupnetwork_amd import losses
    loss, counts = losses.contrast_boundary_loss(points, latents, target, NSAMPLE, STRIDE)
    return loss, torch.autograd.grad(loss.sum(), latents)


def fused(points, latents, target, ncls):
    from toothgroupnetwork_amd import losses
    loss, counts = losses.contrast_boundary_loss(points, latents, target, NSAMPLE, STRIDE, fused=True)
    return loss, torch.autograd.grad(loss.sum(), latents)


def reference_formulation(points, latents, target, ncls):
    from toothgroupnetwork_amd import pointops
    onehot = F.one_hot(target, ncls)
    p0, o0 = points[0]
    out = []
    for i, ((p, o), f) in enumerate(zip(points, latents)):
        if i == 0:
            labels = onehot.float()
        else:
            kr = int(np.prod(STRIDE[:i]))
            idx, _ = pointops.knnquery(kr, p0, p, o0, o)
            labels = onehot[idx.view(-1).long(), :].view(p.shape[0], kr, ncls).float().mean(-2)
        idx, _ = pointops.knnquery(NSAMPLE[i], p, p, o, o)
        idx = idx[..., 1:].contiguous()
        m, k1 = idx.shape
        neighbor_label = labels[idx.view(-1).long(), :].view(m, k1, ncls)
        neighbor_feature = f[idx.view(-1).long(), :].view(m, k1, C)
        posmask = torch.argmax(labels.unsqueeze(-2), -1) == torch.argmax(neighbor_label, -1)
        npos = posmask.int().sum(-1)
        point_mask = torch.logical_and(0 < npos, npos < k1)
        if not torch.any(point_mask):                                                 # (a host synchronisation)
            out.append(f.sum() * 0)
            continue
        posmask, feats, neigh = posmask[point_mask], f[point_mask], neighbor_feature[point_mask]
        dist = torch.sqrt(torch.sum((feats.unsqueeze(-2) - neigh) ** 2, -1) + 1e-12)
        z = -dist
        e = torch.exp(z - torch.max(z, -1, keepdim=True)[0])
        per_point = -torch.log(torch.sum(e * posmask, -1) / torch.sum(e, -1) + 1e-12)
        out.append(per_point.mean() * 0.1)
    loss = torch.stack(out)
    return loss, torch.autograd.grad(loss.sum(), latents)


def difference_only(points, latents, target, ncls):
    from toothgroupnetwork_amd import pointops
    total = 0
    for (p, o), f, k in zip(points, latents, NSAMPLE):
        idx = pointops.knn_indices(k, p, p, o, o)[:, 1:].contiguous()
        diff = pointops.subtraction(f, f, idx)
        total = total + (diff * diff).sum(2).sum()
    return total, torch.autograd.grad(total, latents)


def knn_only(points, latents, target, ncls):
    from toothgroupnetwork_amd import pointops
    p0, o0 = points[0]
    for i, ((p, o), k) in enumerate(zip(points, NSAMPLE)):
        pointops.knn_indices(k, p, p, o, o)
        if i:
            pointops.knn_indices(int(np.prod(STRIDE[:i])), p0, p, o0, o)


def peak_bytes(fn, args):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn(*args)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def run(name, steps, warmup, dev):
    args = make_workload(name, dev)
    from toothgroupnetwork_amd import pointops
    variants = (("ours", ours), ("fused", fused), ("reference", reference_formulation), ("difference", difference_only), ("knn", knn_only))
    ms = {mode: {tag: [] for tag, _ in variants} for mode in ("cold", "memo")}
    for i in range(warmup + steps):
        for mode in ("cold", "memo"):
            for tag, fn in variants:
                if mode == "cold":
                    pointops.knn_cache_clear()        # time the searches, not the memo
                else:
                    knn_only(*args)                   # (the cold calls before it left the memo in whatever state)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(*args)
                torch.cuda.synchronize()
                if i >= warmup:
                    ms[mode][tag].append((time.perf_counter() - t0) * 1e3)
    a, b, fu = ours(*args)[0], reference_formulation(*args)[0], fused(*args)[0]
    sizes = [(lat.shape[0], k - 1) for lat, k in zip(args[1], NSAMPLE)]
    diff_bytes = sum(m * k1 * C * 4 for m, k1 in sizes)
    res = {mode: {tag: quartiles(v) for tag, v in by_tag.items()} for mode, by_tag in ms.items()}
    peak = {}
    for tag, fn in variants[:4]:
        pointops.knn_cache_clear()
        peak[tag] = round(peak_bytes(fn, args) / 2 ** 20, 1)
    res["peak_MiB"] = peak
    # the difference part with its own list searches taken out: it is timed with them in `cold`
    stage_knn = _stage_knn_ms(args, steps)
    diff_cold = res["cold"]["difference"]["median_ms"] - stage_knn
    res.update(stage_points=[m for m, _ in sizes], loss_ours=[round(v, 7) for v in a.tolist()], loss_reference=[round(v, 7) for v in b.tolist()],
               loss_fused=[round(v, 7) for v in fu.tolist()],
               difference_tensor_MiB=round(diff_bytes / 2 ** 20, 1), stage_list_searches_cold_ms=round(stage_knn, 3), difference_without_its_searches_cold_ms=round(diff_cold, 3),
               difference_share_of_ours_time={"cold": round(diff_cold / res["cold"]["ours"]["median_ms"], 3),
                                              "memo": round(res["memo"]["difference"]["median_ms"] / res["memo"]["ours"]["median_ms"], 3)},
               difference_share_of_ours_peak=round(peak["difference"] / peak["ours"], 3),
               fused_over_ours_time={mode: round(res[mode]["fused"]["median_ms"] / res[mode]["ours"]["median_ms"], 3) for mode in ("cold", "memo")},
               fused_over_ours_peak=round(peak["fused"] / peak["ours"], 3),
               speedup_over_reference={mode: round(res[mode]["reference"]["median_ms"] / res[mode]["ours"]["median_ms"], 3) for mode in res if mode in ("cold", "memo")})
    return res


def _stage_knn_ms(args, steps):
    """median ms of the five stage-list searches alone, memo cleared before each call: what `difference` spends on them when cold"""
    from toothgroupnetwork_amd import pointops
    points = args[0]
    out = []
    for _ in range(steps):
        pointops.knn_cache_clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for (p, o), k in zip(points, NSAMPLE):
            pointops.knn_indices(k, p, p, o, o)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cbl_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda")
    res = {name: run(name, args.steps, args.warmup, dev) for name in args.workloads}
    print(json.dumps({"workload": "contrastive-boundary criterion, forward + backward to the latents, fp32", **res}))


if __name__ == "__main__":
    main()
