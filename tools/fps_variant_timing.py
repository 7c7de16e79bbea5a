#!/usr/bin/env python3
"""Interleaved timing of the two FPS launches that carry the headline step, across several builds of the library in ONE process.

  python tools/fps_variant_timing.py parent=tools/_bin/ab/libtgn_parent.so new=toothgroupnetwork_amd/csrc/libtgn_pointops.so

L1 = 256 x 24 000 -> 4096 (fps_bucket_kernel<512,48>), L2 = 256 x 4096 -> 1024 on level 1's output with TGN_FPS_LOW_VALU
(<512,16>), on the benchmark's own scans; 4w = 256 x 2048 -> 512 with TGN_FPS_LOW_VALU on the first 2048 points of level 1's
output (<256,8>, the four-wave form; not part of the headline).  Results are compared across the libraries first (indices and
coordinates, bit for bit).  Then ROUNDS rounds; in every round every library in turn times LAUNCHES launches of L1, of L1 with one sample (zero iterations:
the set-up alone), and the same pairs for L2 and 4w.  Printed: ms per launch, median [min .. max] over the rounds, and
us per iteration = (launch - set-up) / (samples - 1).  Build the variants with tools/ab_build.sh."""
import ctypes
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from toothgroupnetwork_amd import synth  # noqa: E402

ROUNDS, LAUNCHES = 7, 3
B, N, S1, S2 = 256, 24000, 4096, 1024
N4, S4 = 2048, 512
FPS_LOCAL_INDEX, FPS_LOW_VALU = 2, 16      # include/tgn_pointops.h


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    f = lib.tgn_furthestsampling_dense
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_void_p]
    return f


def main(argv):
    builds = [a.split("=", 1) for a in argv]
    if not builds:
        raise SystemExit(__doc__)
    fns = {name: load(path) for name, path in builds}
    dev = torch.device("cuda", 0)
    xyz1 = torch.from_numpy(np.ascontiguousarray(synth.scan_batch(B, N, "arch", seed=100)[:, :, :3])).to(dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(fn, xyz, n, s, flags, idx, out):
        rc = fn(B, n, s, xyz.data_ptr(), None, idx.data_ptr(), out.data_ptr(), flags, stream)
        if rc != 0:
            raise RuntimeError(f"tgn_furthestsampling_dense failed with status {rc}")

    # results first: every library against the first one
    ref = None
    for name, fn in fns.items():
        i1 = torch.full((B, S1), -7, dtype=torch.int32, device=dev)
        o1 = torch.full((B, S1, 3), -7.0, device=dev)
        launch(fn, xyz1, N, S1, FPS_LOCAL_INDEX, i1, o1)
        i2 = torch.full((B, S2), -7, dtype=torch.int32, device=dev)
        o2 = torch.full((B, S2, 3), -7.0, device=dev)
        launch(fn, o1, S1, S2, FPS_LOCAL_INDEX | FPS_LOW_VALU, i2, o2)
        torch.cuda.synchronize()
        got = (i1, o1.view(torch.int32), i2, o2.view(torch.int32))
        if ref is None:
            ref = got
        elif not all(torch.equal(a, b) for a, b in zip(ref, got)):
            raise SystemExit(f"{name}: results differ from {builds[0][0]}")
    print(f"# results of {len(fns)} libraries: identical (indices and coordinate bits, both levels)")
    xyz2 = ref[1].view(torch.float32).clone()
    idx = torch.empty((B, S1), dtype=torch.int32, device=dev)
    out = torch.empty((B, S1, 3), device=dev)
    xyz4 = xyz2[:, :N4].contiguous()
    cases = [("L1 launch", xyz1, N, S1, FPS_LOCAL_INDEX), ("L1 set-up", xyz1, N, 1, FPS_LOCAL_INDEX),
             ("L2 launch", xyz2, S1, S2, FPS_LOCAL_INDEX | FPS_LOW_VALU), ("L2 set-up", xyz2, S1, 1, FPS_LOCAL_INDEX | FPS_LOW_VALU),
             ("4w launch", xyz4, N4, S4, FPS_LOCAL_INDEX | FPS_LOW_VALU), ("4w set-up", xyz4, N4, 1, FPS_LOCAL_INDEX | FPS_LOW_VALU)]
    for fn in fns.values():     # code objects loaded, clocks up
        for _, x, n, s, fl in cases:
            launch(fn, x, n, s, fl, idx, out)
    torch.cuda.synchronize()
    ms = {name: {c[0]: [] for c in cases} for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            for tag, x, n, s, fl in cases:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(LAUNCHES):
                    launch(fn, x, n, s, fl, idx, out)
                e1.record()
                e1.synchronize()
                ms[name][tag].append(e0.elapsed_time(e1) / LAUNCHES)
    print(f"# {torch.cuda.get_device_name(0)}; {ROUNDS} interleaved rounds, {LAUNCHES} launches per timing; ms: median [min .. max]")
    print(f"{'build':>10s} | " + " | ".join(f"{t + ' launch':>27s} {t + ' set-up':>27s} {t + ' us/it':>9s}" for t in ("L1", "L2", "4w")))

    def cell(v):
        return f"{np.median(v):7.4f} [{min(v):7.4f}..{max(v):7.4f}]"

    for name in fns:
        m = ms[name]
        cols = []
        for t, s in (("L1", S1), ("L2", S2), ("4w", S4)):
            it = (np.median(m[t + " launch"]) - np.median(m[t + " set-up"])) / (s - 1) * 1e3
            cols.append(f"{cell(m[t + ' launch'])} {cell(m[t + ' set-up'])} {it:9.4f}")
        print(f"{name:>10s} | " + " | ".join(cols))
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
