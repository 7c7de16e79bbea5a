#!/usr/bin/env python3
"""GPU time of scoring (toothgroupnetwork_amd/metrics.py: confusion + scores, confusion_from_logits + scores) against the two ways it
could be done without the kernels: the reference-style numpy loop on this host (eval_visualize_results.py:20-57: about ten full-length
passes per instance) and the torch composition on the same GPU (torch.bincount(ins * L + gt, minlength=L * L) twice plus the score
arithmetic in torch; argmax first for the logits case).  One process; device-event medians after warm-up, every timed call checked to
give the same values as the others first.  Prints one JSON line per shape; times in ms.

    python tools/metrics_bench.py [--reps 50] [--cpu-reps 3]

Shapes: one scan of 200 000 vertices with FDI labels, one of 24 000, 64 ragged scans of 100 000 - 250 000, logits (8, 17, 24000).
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from toothgroupnetwork_amd import metrics, synth  # noqa: E402
from toothgroupnetwork_amd.inference import fdi_from_classes  # noqa: E402

L = metrics.MAX_LABELS


def event_ms(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return float(np.median(t))


def host_ms(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def numpy_loop(gt, sem, ins):
    """the reference's loop, restated: per instance the masks, two np.unique and four count_nonzero"""
    names = np.unique(ins)
    names = names[names != 0]
    iou = f1 = acc = hit = 0
    for name in names:
        im = ins == int(name)
        u, c = np.unique(gt[im], return_counts=True)
        g = u[np.argmax(c)]
        gm = gt == g
        TP, FN = np.count_nonzero(gm * im), np.count_nonzero(gm * np.invert(im))
        FP, TN = np.count_nonzero(np.invert(gm) * im), np.count_nonzero(np.invert(gm) * np.invert(im))
        acc += (TP + TN) / (FP + TP + FN + TN)
        prec, rec = TP / (TP + FP), TP / (TP + FN)
        f1 += 2 * (prec * rec) / (prec + rec)
        iou += TP / (FP + TP + FN)
        u, c = np.unique(sem[im], return_counts=True)
        hit += u[np.argmax(c)] == g
    k = len(names)
    return iou / k, f1 / k, acc / k, hit / k


def torch_scores(A, S):
    """the four values of every scan from (b, L, L) tables with torch operators (float64, vectorised over the instances)"""
    A, S = A.double(), S.double()
    n, insc, gtc = A.sum((1, 2)), A.sum(2), A.sum(1)
    tp, g = A.max(2)
    s = S.argmax(2)
    fp, fn = insc - tp, torch.gather(gtc, 1, g) - tp
    tn = n[:, None] - tp - fp - fn
    present = insc > 0
    present[:, 0] = False
    prec, rec = tp / (tp + fp), tp / (tp + fn)
    terms = torch.stack([tp / (fp + tp + fn), 2 * (prec * rec) / (prec + rec), (tp + tn) / (fp + tp + fn + tn), (s == g).double()])
    k = present.sum(1)
    return torch.where(present[None], terms, torch.zeros_like(terms)).sum(2) / k


def torch_tables(gt, sem, ins, scan, b):
    base = scan * (L * L) + ins * L
    return (torch.bincount(base + gt, minlength=b * L * L).view(b, L, L), torch.bincount(base + sem, minlength=b * L * L).view(b, L, L))


def fdi_scan(n, seed, rng):
    _, lab = synth.labelled_arch(n, 14, seed=seed)
    gt = fdi_from_classes(lab + 1)
    pred = gt.copy()
    flip = rng.random(n) < 0.05
    pred[flip] = rng.choice(np.unique(gt), size=int(flip.sum()))
    return gt, pred


def labels_case(name, lens, a, dev, rng):
    base = [fdi_scan(max(lens), 1400 + i, rng) for i in range(min(4, len(lens)))]           # (a scan is a prefix of one of four arches)
    scans = [tuple(arr[:n] for arr in base[i % len(base)]) for i, n in enumerate(lens)]
    gt, pred = (torch.from_numpy(np.concatenate([s[k] for s in scans])).to(dev) for k in (0, 1))
    off = np.cumsum(lens).tolist()
    scan = torch.from_numpy(np.repeat(np.arange(len(lens)), lens)).to(dev)
    b = len(lens)

    def fused():
        return metrics.scores(*metrics.confusion(gt, pred, None, L, off))

    def composed():
        return torch_scores(*torch_tables(gt, pred, pred, scan, b))

    f, c = fused(), composed()
    ta, ts = torch_tables(gt, pred, pred, scan, b)
    fa, fs = metrics.confusion(gt, pred, None, L, off)
    assert torch.equal(fa.long(), ta) and torch.equal(fs.long(), ts), "tables differ from torch.bincount's"
    assert torch.allclose(torch.stack([f.iou, f.f1, f.acc, f.sem_acc]), c, rtol=1e-12, atol=0), "scores differ from the torch composition"
    ref = numpy_loop(*(scans[0][k] for k in (0, 1, 1)))
    assert [float(v[0]) for v in (f.iou, f.f1, f.acc, f.sem_acc)] == [float(v) for v in ref], "scores differ from the numpy loop"
    res = {"metric": "metrics_bench", "case": name, "scans": b, "vertices": int(sum(lens)),
           "fused_ms": event_ms(fused, a.reps), "torch_bincount_ms": event_ms(composed, a.reps),
           "numpy_loop_ms": host_ms(lambda: [numpy_loop(s[0], s[1], s[1]) for s in scans[:a.cpu_scans]], a.cpu_reps) * b / min(b, a.cpu_scans)}
    res["numpy_loop_scans_timed"] = min(b, a.cpu_scans)
    return res


def logits_case(a, dev, rng, B=8, C=17, N=24000):
    gt = torch.from_numpy(np.stack([synth.labelled_arch(N, 14, seed=1500 + i)[1] for i in range(B)])).to(dev)          # -1 .. 13
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(B, C, N, generator=g) + 4.0 * torch.nn.functional.one_hot(gt.cpu() + 1, C).permute(0, 2, 1)).to(dev)
    scan = torch.arange(B, device=dev).repeat_interleave(N)

    def fused():
        return metrics.scores(*metrics.confusion_from_logits(logits, gt, 1))

    def composed():
        pred = logits.argmax(1).reshape(-1)
        base = scan * (C * C) + pred * C
        return torch_scores(torch.bincount(base + gt.reshape(-1) + 1, minlength=B * C * C).view(B, C, C),
                            torch.bincount(base + pred, minlength=B * C * C).view(B, C, C))

    f, c = fused(), composed()
    assert torch.allclose(torch.stack([f.iou, f.f1, f.acc, f.sem_acc]), c, rtol=1e-12, atol=0), "scores differ from the torch composition"
    pred = logits.argmax(1).cpu().numpy()
    gts = gt.cpu().numpy() + 1
    return {"metric": "metrics_bench", "case": "logits_8x17x24000", "scans": B, "vertices": B * N,
            "fused_ms": event_ms(fused, a.reps), "torch_bincount_ms": event_ms(composed, a.reps),
            "numpy_loop_ms": host_ms(lambda: [numpy_loop(gts[i], pred[i], pred[i]) for i in range(B)], a.cpu_reps),
            "numpy_loop_scans_timed": B}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--cpu-scans", type=int, default=4, help="scans of the ragged case the numpy loop is timed on (scaled to all)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "metrics_bench needs a GPU"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(14)
    print(json.dumps({"metric": "metrics_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "labels": L}), flush=True)
    print(json.dumps(labels_case("one_scan_200000", [200000], a, dev, rng)), flush=True)
    print(json.dumps(labels_case("one_scan_24000", [24000], a, dev, rng)), flush=True)
    print(json.dumps(labels_case("ragged_64_scans", rng.integers(100000, 250001, size=64).tolist(), a, dev, rng)), flush=True)
    print(json.dumps(logits_case(a, dev, rng)), flush=True)


if __name__ == "__main__":
    main()
