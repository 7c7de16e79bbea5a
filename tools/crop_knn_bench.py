#!/usr/bin/env python3
"""GPU time of tgn_crop_knn (csrc/crop.hip) in its two regimes, for one build or for several builds alternated in one process:

  crops   16 centres with k = 3072 over one 24 000-point scan   (tooth_crops, tsegnet's join: few workgroups, long sort)
  vote    5000 centres with k = 10 over 15 000 candidates        (cluster.py's noise vote: thousands of workgroups, short sort)

Every repeat times `--launches` back-to-back launches between two device events and reports the time of one; with several
libraries the repeats alternate between them (a, b, a, b, ...), so that drift of the machine lands on all of them alike.  The outputs
of all libraries are compared bit for bit.  Prints one JSON line; times in microseconds per launch.

    python tools/crop_knn_bench.py [--repeats 7] [--launches 20] [--libs parent=path/to/libtgn_parent.so new=path/to/libtgn_new.so]

(tools/ab_build.sh builds such libraries from one translation unit.)
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from toothgroupnetwork_amd import _lib, synth  # noqa: E402

_P = ctypes.c_void_p


def load(path):
    fn = ctypes.CDLL(os.path.abspath(path)).tgn_crop_knn
    fn.restype, fn.argtypes = _lib.SIGNATURES["tgn_crop_knn"]
    return fn


def regimes(dev):
    rows, lab = synth.labelled_arch(24000, 16, seed=912)
    xyz = rows[:, :3]
    cent = np.stack([xyz[lab == t].mean(0) for t in range(16)]).astype(np.float32)
    crops = (torch.from_numpy(np.ascontiguousarray(xyz.T))[None].to(dev), torch.from_numpy(cent).to(dev), 3072)
    rng = np.random.default_rng(913)
    cand = torch.from_numpy(np.ascontiguousarray(xyz[rng.permutation(24000)[:15000]].T))[None].to(dev)
    query = torch.from_numpy(xyz[rng.permutation(24000)[:5000]].copy()).to(dev)
    return {"crops": crops, "vote": (cand, query, 10)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--libs", nargs="*", default=[], help="name=path ...; default: the package's library alone")
    a = ap.parse_args()
    libs = dict(s.split("=", 1) for s in a.libs) or {"built": _lib.LIB_PATH}
    fns = {name: load(path) for name, path in libs.items()}
    dev = torch.device("cuda", 0)
    st = _lib.stream()
    res = {"metric": "crop_knn_bench", "device": torch.cuda.get_device_name(0), "unit": "us per launch", "repeats": a.repeats,
           "launches": a.launches}
    for tag, (feats, cent, k) in regimes(dev).items():
        B, C, N = feats.shape
        T = cent.shape[0]
        scan = torch.zeros(T, dtype=torch.int32, device=dev)
        out = {name: torch.empty(T, k, dtype=torch.int64, device=dev) for name in fns}

        def launch(name):
            rc = fns[name](B, N, C, _P(feats.data_ptr()), T, _P(scan.data_ptr()), _P(cent.data_ptr()), k, _P(out[name].data_ptr()), st)
            if rc:
                raise RuntimeError(f"tgn_crop_knn of {name} returned {rc}")

        for name in fns:                                 # warm-up: code object load, first launch
            launch(name), launch(name)
        torch.cuda.synchronize()
        first = next(iter(out.values()))
        res[f"{tag}_outputs_bit_equal"] = all(torch.equal(first, o) for o in out.values())
        times = {name: [] for name in fns}
        for _ in range(a.repeats):
            for name in fns:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    launch(name)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
        for name, t in times.items():
            res[f"{tag}_{name}"] = {"min": round(min(t), 2), "median": round(float(np.median(t)), 2), "max": round(max(t), 2),
                                    "all": [round(x, 2) for x in t]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
