#!/usr/bin/env python3
"""The fused BatchNorm over rows with atomic and with ordered column sums (config.cfg.ordered_bn), forward + backward through
point_transformer.bn_rows, at the row shapes a 24 000-point tgnet_fps step has: the widest (24 000 * 36, 32), a mid stage
(1 500 * 24, 128) and a deep one (94 * 24, 512).

The two forms alternate call by call in one process, so both see the same clocks and allocator; device time between two events
around one forward + backward, medians of --reps after --warmup, with the quartiles as the spread.  `reduce_blocks` and
`workspace_bytes` are what the ordered form's finishing launch reads per column and in all.  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

SHAPES = {"widest": (24000 * 36, 32), "mid": (1500 * 24, 128), "deep": (94 * 24, 512)}


def run(rows, C, reps, warmup, dev):
    from toothgroupnetwork_amd import _lib, config, point_transformer as PT
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, C, generator=g).to(dev).requires_grad_(True)
    dy = torch.randn(rows, C, generator=g).to(dev)
    bns = {form: torch.nn.BatchNorm1d(C).to(dev).train() for form in ("atomic", "ordered")}
    us = {form: [] for form in bns}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(warmup + reps):
        for form, bn in bns.items():
            with config.override(ordered_bn=form == "ordered"):
                start.record()
                y = PT.bn_rows(bn, x, relu=True)
                torch.autograd.grad(y, [x, bn.weight, bn.bias], dy)
                stop.record()
            stop.synchronize()
            if i >= warmup:
                us[form].append(start.elapsed_time(stop) * 1e3)
    out = {}
    for form, v in us.items():
        q1, q2, q3 = np.percentile(v, [25, 50, 75])
        out[form] = {"median_us": round(float(q2), 1), "q1_us": round(float(q1), 1), "q3_us": round(float(q3), 1)}
    nbytes = int(_lib.lib().tgn_bn_rows_ordered_workspace_bytes(rows, C))
    out.update(ordered_over_atomic=round(out["ordered"]["median_us"] / out["atomic"]["median_us"], 3), reduce_blocks=nbytes // (2 * C * 8),
               workspace_bytes=nbytes)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda")
    res = {f"{tag} {shape}": run(*shape, args.reps, args.warmup, dev) for tag, shape in SHAPES.items()}
    print(json.dumps({"workload": "bn_rows forward + backward, relu, fp32: atomic against ordered column sums", **res}))


if __name__ == "__main__":
    main()
