#!/usr/bin/env python3
"""Host time per call of the FPS front end (toothgroupnetwork_amd/fps.py): `farthest_point_sample` on (1, 64, 3) -> 8 and
`furthestsampling` on one cloud of 64 -> 8 with registered offsets (no host copy).  At this size the kernel is negligible and the
number is the Python path.  One repeat per process: 200 warm-up calls, 2000 timed calls, one synchronise at the end.
`--tree DIR` imports the package from another checkout (a built one), to alternate two commits: profiles/fps_front_end_before_after.txt."""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import torch

from toothgroupnetwork_amd import pointnet2_utils as U, pointops as P

assert os.path.abspath(U.__file__).startswith(os.path.abspath(args.tree)), U.__file__
dev = torch.device("cuda")
torch.manual_seed(0)
x = torch.rand(1, 64, 3, device=dev)
p = x[0].contiguous()
o = P.register_offsets(torch.tensor([64], dtype=torch.int32, device=dev), [64])
no = P.register_offsets(torch.tensor([8], dtype=torch.int32, device=dev), [8])
for name, fn in (("dense farthest_point_sample (1,64,3)->8", lambda: U.farthest_point_sample(x, 8)),
                 ("packed furthestsampling 64->8", lambda: P.furthestsampling(p, o, no))):
    for _ in range(200):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(2000):
        fn()
    torch.cuda.synchronize()
    print(f"{args.label:6s} {name}: {(time.perf_counter() - t0) / 2000 * 1e6:.2f} us per call", flush=True)
