#!/usr/bin/env python3
"""What the atomic-free backward of the gather family costs (config.cfg.ordered_backward, ordered.py, csrc/scatter_ordered.hip).

The baseline is the atomic path exactly as the operators run it with the switch off (the pre-zeroed gradient included) and, for the
lists, the stable torch sort below (sorted_reverse_lists); never the new code against itself.  On one 24 000-point synthetic arch scan with its real k-NN lists:

  grouping backward            (24 000, 16, 32) and (24 000, 36, 32)      zeros + tgn_grouping_backward  |  tgn_scatter_ordered
  interpolation backward       6 000 -> 24 000 rows, k = 3, c = 64        zeros + tgn_interpolation_backward  |  tgn_scatter_ordered, query rows
  Point-Transformer tail       (24 000, 16, 32, g = 4)                    zeros + the kernel with its scatter  |  the kernel without + tgn_scatter_ordered
  list build                   (24 000, 16) and (24 000, 36)              sorted_reverse_lists (torch)  |  tgn_reverse_lists

Every ordered figure comes twice: `lists cached` (the memo hit every block of a stage after the first sees) and `lists built` (the
list build in the timed window).  The variants of a row alternate call by call in one process; device events around each call;
medians of --reps after --warmup, quartiles as the spread.

--train N runs tools/training_bench.py (its own loop, tgnet_fps, one 24 000-point scan) in N fresh processes per setting,
TGN_ORDERED_BACKWARD=0 and =1 alternating, and reports the trainer step's median per process and the spread between processes.

Prints a text table and one JSON line."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def quartiles(ms):
    q1, q2, q3 = np.percentile(ms, [25, 50, 75])
    return {"median_us": round(float(q2) * 1e3, 1), "q1_us": round(float(q1) * 1e3, 1), "q3_us": round(float(q3) * 1e3, 1)}


def alternate(variants, reps, warmup):
    """variants: {tag: fn}; the fns run in turn, each call between two device events -> {tag: quartiles}"""
    ms = {tag: [] for tag in variants}
    for i in range(warmup + reps):
        for tag, fn in variants.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            end.synchronize()
            if i >= warmup:
                ms[tag].append(start.elapsed_time(end))
    return {tag: quartiles(v) for tag, v in ms.items()}


def sorted_reverse_lists(idx):
    """The lists of ordered.reverse_lists(idx, m) for square idx (m, k1) as plain torch: a stable sort of the flattened lists and a
    searchsorted over the sorted keys (tests/ordered_ref.reverse_lists_torch).  The baseline of the `list build` rows."""
    m = idx.shape[0]
    flat = idx.reshape(-1)
    flat = torch.where((flat < 0) | (flat >= m), torch.zeros_like(flat), flat)
    keys, order = torch.sort(flat, stable=True)
    rev_start = torch.searchsorted(keys, torch.arange(m + 1, dtype=keys.dtype, device=keys.device), out_int32=True)
    return rev_start, order.to(torch.int32)


def micro(points, reps, warmup, dev):
    from toothgroupnetwork_amd import _lib, config, ordered, pointops as P, synth
    O, st = _lib.ops(), _lib.stream
    rows, _ = synth.labelled_arch(points, 14, seed=3)
    xyz = torch.from_numpy(np.ascontiguousarray(rows[:, :3])).to(dev)
    off = P.register_offsets(torch.tensor([points], dtype=torch.int32, device=dev), [points])
    g = torch.Generator().manual_seed(0)
    out = {}

    def built(fn, idx, n):
        """fn(lists) with the lists built inside the timed window"""
        def run():
            ordered.lists_cache_clear()
            fn(ordered.reverse_lists(idx, n))
        return run

    for k in (16, 36):
        idx = P.knn_indices(k, xyz, None, off, off)
        go = torch.randn(points, k, 32, generator=g).to(dev)
        flat = go.view(points * k, 32)

        def atomic(go=go, idx=idx, k=k):
            grad = torch.zeros(points, 32, device=dev)
            O.tgn_grouping_backward(points, k, 32, go, idx, grad, st())
        lists = ordered.reverse_lists(idx, points)
        out[f"grouping backward ({points}, {k}, 32)"] = alternate(
            {"atomic": atomic, "ordered, lists cached": lambda: ordered.scatter(flat, points, lists),
             "ordered, lists built": built(lambda l: ordered.scatter(flat, points, l), idx, points)}, reps, warmup)
        out[f"list build ({points}, {k})"] = alternate(
            {"sorted_reverse_lists": lambda: sorted_reverse_lists(idx), "tgn_reverse_lists": built(lambda l: None, idx, points)}, reps, warmup)

    # interpolation: a quarter of the points as the coarse cloud, every point interpolates from its 3 nearest coarse points
    coarse = points // 4
    sub = xyz[torch.randperm(points, generator=g)[:coarse].to(dev)].contiguous()
    coff = P.register_offsets(torch.tensor([coarse], dtype=torch.int32, device=dev), [coarse])
    idx3, dist2 = P._knn_raw(3, sub, xyz, coff, off)
    w = P._inverse_distance_weights(torch.sqrt(dist2)).contiguous()
    go = torch.randn(points, 64, generator=g).to(dev)

    def interp_atomic():
        grad = torch.zeros(coarse, 64, device=dev)
        O.tgn_interpolation_backward(points, 64, 3, go, idx3, w, grad, st())
    lists3 = ordered.reverse_lists(idx3, coarse)
    coef = w.view(points * 3, 1)
    out[f"interpolation backward {coarse} -> {points}, c = 64"] = alternate(
        {"atomic": interp_atomic, "ordered, lists cached": lambda: ordered.scatter(go, coarse, lists3, coef=coef, k=3),
         "ordered, lists built": built(lambda l: ordered.scatter(go, coarse, l, coef=coef, k=3), idx3, coarse)}, reps, warmup)

    # the Point-Transformer tail's backward
    k, c, g_ = 16, 32, 4
    idx = P.knn_indices(k, xyz, None, off, off)
    xv, pr = torch.randn(points, c, generator=g).to(dev), torch.randn(points, k, c, generator=g).to(dev)
    sm = torch.softmax(torch.randn(points, k, g_, generator=g), 1).to(dev)
    go = torch.randn(points, c, generator=g).to(dev)

    def tail_atomic():
        g_xv, g_pr, g_lg = torch.zeros_like(xv), torch.empty_like(pr), torch.empty_like(sm)
        O.tgn_pt_softmax_aggregate_backward(points, k, c, g_, xv, pr, sm, idx, go, g_xv, g_pr, g_lg, st())

    def tail_built():
        ordered.lists_cache_clear()
        ordered.softmax_aggregate_backward(xv, pr, sm, idx, go)
    ordered.reverse_lists(idx, points)
    with config.override(ordered_backward=True):        # ordered.softmax_aggregate_backward reads the switch; tail_atomic is the raw kernel
        out[f"tail backward ({points}, {k}, {c}, g = {g_})"] = alternate(
            {"atomic": tail_atomic, "ordered, lists cached": lambda: ordered.softmax_aggregate_backward(xv, pr, sm, idx, go),
             "ordered, lists built": tail_built}, reps, warmup)
    return out


def train_steps(processes, steps, warmup):
    """tools/training_bench.py's loop in fresh processes, the switch off and on in turn -> per setting the trainer medians (ms)"""
    tool = os.path.join(os.path.dirname(os.path.abspath(__file__)), "training_bench.py")
    res = {"0": [], "1": []}
    for _ in range(processes):
        for flag in ("0", "1"):
            env = dict(os.environ, TGN_ORDERED_BACKWARD=flag)
            done = subprocess.run([sys.executable, tool, "--models", "tgnet_fps", "--steps", str(steps), "--warmup", str(warmup)], env=env,
                                  capture_output=True, text=True, timeout=600)
            if done.returncode:
                raise RuntimeError(f"training_bench.py failed (TGN_ORDERED_BACKWARD={flag}):\n{done.stderr[-2000:]}")
            line = [ln for ln in done.stdout.splitlines() if ln.startswith("{")][-1]
            res[flag].append(json.loads(line)["tgnet_fps"]["trainer"]["median_ms"])
    return {("ordered" if flag == "1" else "atomic"): {"per_process_median_ms": v, "median_ms": round(float(np.median(v)), 3),
                                                       "min_ms": min(v), "max_ms": max(v)} for flag, v in res.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--points", type=int, default=24000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--train", type=int, default=0, help="fresh processes per setting for the tgnet_fps train step (0: leave it out)")
    ap.add_argument("--train_steps", type=int, default=20)
    ap.add_argument("--train_warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ordered_backward_bench.py needs a GPU: there is nothing to measure without one")
    res = {"micro": micro(args.points, args.reps, args.warmup, torch.device("cuda"))}
    print(f"medians of {args.reps} after {args.warmup}, variants alternating call by call, device events; microseconds (q1 .. q3)")
    for row, variants in res["micro"].items():
        base = next(iter(variants.values()))["median_us"]
        print(row)
        for tag, q in variants.items():
            print(f"    {tag:24s} {q['median_us']:9.1f}  ({q['q1_us']:.1f} .. {q['q3_us']:.1f})   x{q['median_us'] / base:.2f}")
    if args.train:
        torch.cuda.synchronize()
        res["train_step"] = train_steps(args.train, args.train_steps, args.train_warmup)
        print(f"tgnet_fps train step, 1 x 24 000 points, tools/training_bench.py's trainer loop: median of {args.train_steps} steps per process, "
              f"{args.train} fresh processes per setting, settings alternating; milliseconds")
        for tag, v in res["train_step"].items():
            print(f"    {tag:10s} median {v['median_ms']:.3f}  (processes: {v['min_ms']:.3f} .. {v['max_ms']:.3f})  {v['per_process_median_ms']}")
    print(json.dumps({"workload": f"ordered backward against the atomic path, 1 x {args.points} points, fp32", **res}))


if __name__ == "__main__":
    main()
