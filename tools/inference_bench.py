#!/usr/bin/env python3
"""One scan through the semantic inference pipeline (toothgroupnetwork_amd/inference.py = inference_pipeline_sem.py): OBJ of ~108 000
vertices -> labels per vertex, with a seeded Point-Transformer network; stage times, with and without the FPS-of-an-FPS-result
shortcut between the resampling and the network's first level.

    python tools/inference_bench.py                                    the semantic pipeline and infer_scans (above)
    python tools/inference_bench.py --model_name tsegnet|tgnet [--out F]  a two-stage pipeline over 48 scans: the loop [pipe(p) for p in
        paths] against the staged inference.infer_paths(pipe, paths, batch=8) in one process, alternated --repeats times after one warm-up
        of each, by the wall clock around runs that end in a device synchronise; medians, the spread of the repeats, and the mean stage
        times of both.  Randomly initialised modules under a fixed seed; a scan on which they find nothing to crop fails alike in both
        runs and is counted ("answered").  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from toothgroupnetwork_amd import inference, nets, pointops, synth

dev = torch.device("cuda")


def synthetic_scans(n=48):
    paths = []
    for i in range(n):
        pth = os.path.join(tempfile.gettempdir(), f"tgn_infer_scan_{i}.obj")
        if not os.path.exists(pth):
            with open(pth, "w") as f:
                f.write(synth.obj_text(330 + (i % 7) * 10, 300, 100 + i, "plain", with_tail=False))
        paths.append(pth)
    return paths


def two_stage_pipeline(name):
    if name == "tgnet":
        torch.manual_seed(0)                                # tests/test_gpu_tgnet_pipeline.py's REAL_SEED
        config = inference.inference_config("tgnet")
        first = nets.GroupingNetworkModule({"model_parameter": config["fps_model_info"]["model_parameter"]})
        bdl = nets.GroupingNetworkModule({"model_parameter": config["boundary_model_info"]["model_parameter"]})
        return inference.TgnInferencePipeLine(first.to(dev).eval(), bdl.to(dev).eval())
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import tsegnet_cases as SC
    from seeded import seeded_fill
    import types
    net = nets.TSegNetModule({"run_tooth_segmentation_module": True})
    seeded_fill(net, 1111)                                  # tools/tsegnet_bench.py's weights
    net = SC.set_heads(net).to(dev).eval()

    class SnappedCentroids(torch.nn.Module):
        """The seeded centroid network at its real cost, with the two heads' outputs replaced: untrained heads move the 256 coarse points
        of a whole arch nowhere near each other, DBSCAN then finds no cluster and the scan ends before the join.  As tsegnet_cases.fixed_cent
        does, the offsets snap the coarse points to a 0.25 lattice (one cluster per occupied cell, about as many as a jaw has teeth) and
        every distance passes the 0.3 filter."""

        def forward(self, inp):
            l0_points, l1, l0_xyz, l3_xyz, _, dist = net.cent_module(inp)
            return l0_points, l1, l0_xyz, l3_xyz, torch.floor(l3_xyz * 4.0 + 0.5) * 0.25 - l3_xyz, torch.zeros_like(dist)

    def seg_module(cropped):
        CROPS.append(int(cropped.shape[0]))
        return net.seg_module(cropped)

    return inference.TSegNetInferencePipeLine(types.SimpleNamespace(cent_module=SnappedCentroids(), seg_module=seg_module, get_ddf=None))


CROPS = []                                                  # crops per tsegnet scan, every run


def two_stage(a):
    pipe, paths = two_stage_pipeline(a.model_name), synthetic_scans(a.scans)

    def run(staged):
        np.random.seed(0)
        stats = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = inference.infer_paths(pipe, paths, batch=a.batch, workers=a.workers, on_error="skip", stats=stats, staged=staged)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, stats, out

    warm = {staged: run(staged) for staged in (False, True)}
    answered = [sum("error" not in r for r in warm[staged][2]) for staged in (False, True)]
    same = all(("error" in x) == ("error" in y) and ("error" in x or (np.array_equal(x["sem"], y["sem"]) and np.array_equal(x["ins"], y["ins"])))
               for x, y in zip(warm[False][2], warm[True][2]))
    errors = sorted({r["error"].split(": ", 2)[-1][:120] for r in warm[False][2] if "error" in r})
    runs = {False: [], True: []}
    for _ in range(a.repeats):                              # alternating: both see the same machine state
        for staged in (False, True):
            runs[staged].append(run(staged)[:2])
    res = {"what": f"{a.model_name}: sequential loop against staged infer_paths", "device": torch.cuda.get_device_name(0), "scans": len(paths),
           "batch": a.batch, "workers": a.workers or inference.default_workers(), "repeats": a.repeats, "answered": answered, "same_labels": bool(same),
           "errors": errors}
    if CROPS:
        res["crops_per_scan_mean"] = round(float(np.mean(CROPS)), 2)
    for staged, key in ((False, "sequential"), (True, "staged")):
        ms = [t * 1e3 / len(paths) for t, _ in runs[staged]]
        stages = {k: round(float(np.mean([s.get(k, 0.0) for _, s in runs[staged]])) * 1e3, 3) for k in runs[staged][0][1]}
        res[key] = {"ms_per_scan_median": round(float(np.median(ms)), 3), "ms_per_scan_runs": [round(m, 3) for m in ms],
                    "spread_ms": round(max(ms) - min(ms), 3), "scans_per_s": round(1e3 / float(np.median(ms)), 2), "stage_ms": stages}
    gain = res["sequential"]["ms_per_scan_median"] - res["staged"]["ms_per_scan_median"]
    res["gain_ms_per_scan"] = round(gain, 3)
    res["staged_is_faster_by_more_than_the_spread"] = bool(gain > max(res["sequential"]["spread_ms"], res["staged"]["spread_ms"]))
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(res) + "\n")


ap = argparse.ArgumentParser()
ap.add_argument("--model_name", choices=("tsegnet", "tgnet"), default=None, help="measure a two-stage pipeline instead of the semantic one")
ap.add_argument("--scans", type=int, default=48)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--workers", type=int, default=None, help="loader threads of the staged run (default: inference.default_workers())")
ap.add_argument("--out", default=None, help="append the JSON line to this file")
args = ap.parse_args()
if args.model_name:
    two_stage(args)
    sys.exit(0)

torch.manual_seed(0)
path = os.path.join(tempfile.gettempdir(), "tgn_infer_scan.obj")
with open(path, "w") as f:
    f.write(synth.obj_text(360, 300, 7, "plain", with_tail=False))
net = nets.PointTransformerSeg().to(dev).eval()
pipe = inference.InferencePipeLine(net)
for shortcut in (True, False):
    pointops.FPS_PREFIX = None if shortcut else False
    pointops.fps_prefix_clear()
    out = pipe(path)                                    # warm-up (code objects, fold memo, allocator)
    runs = []
    for _ in range(5):
        t0 = time.perf_counter()
        out = pipe(path)
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0, dict(pipe.times)))
    best = min(runs, key=lambda r: r[0])
    print(f"FPS identity between resampling and the network {'on ' if shortcut else 'off'}: {best[0] * 1e3:7.1f} ms per scan  "
          + "  ".join(f"{k} {v * 1e3:.1f}" for k, v in best[1].items()) + f"   ({out['sem'].shape[0]} vertices, {len(np.unique(out['sem']))} labels)")

# throughput form: many scans, overlapped stages
paths = synthetic_scans(48)
pointops.FPS_PREFIX = None
inference.infer_scans(paths[:8], net, batch=8)
for b in (8, 16):
    t0 = time.perf_counter()
    res = inference.infer_scans(paths, net, batch=b)
    dt = time.perf_counter() - t0
    print(f"infer_scans, {len(paths)} scans, batch {b}: {dt * 1e3 / len(paths):6.1f} ms per scan = {len(paths) / dt:6.1f} scans/s")
