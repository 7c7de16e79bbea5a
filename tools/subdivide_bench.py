#!/usr/bin/env python3
"""One pass of midpoint subdivision (csrc/subdivide.hip, preprocess.subdivide_midpoint) on synthetic arch meshes of 7 000 and 15 000
vertices (synth.obj_text(100, 70) and (150, 100), the triangles in a seeded random order), four figures per mesh, in one process:

  device   the launch sequence of tgn_subdivide_midpoint alone, between two events on the stream (inputs, outputs and workspace
           already on the device, `--inner` calls per repetition);
  wrapper  the wall time of preprocess.subdivide_midpoint: host checks, three copies to the device, the launches, the one
           synchronisation for the new-vertex count, three copies back;
  numpy    the vectorised CPU form (np.unique, first-occurrence ranks), on the same host;
  loop     the dictionary loop as open3d writes it, on the same host (`--loop-reps` repetitions: it is slow).

The two CPU forms are copies of tests/subdivide_ref.py's (product code imports nothing from tests/).  The forms alternate inside every
repetition; medians over `--reps` repetitions after `--warmup`, with the spread (min .. max), in microseconds.  The wrapper's result is
checked against the numpy form bit for bit before anything is timed.  One JSON line.

    python tools/subdivide_bench.py [--reps 30] [--inner 20] [--warmup 5] [--loop-reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from toothgroupnetwork_amd import _lib, preprocess, synth  # noqa: E402

MESHES = ((100, 70, 61), (150, 100, 64))


def numpy_once(v, n, t):
    nv, nf = v.shape[0], t.shape[0]
    p, q = t.reshape(-1), t[:, [1, 2, 0]].reshape(-1)
    lo, hi = np.minimum(p, q), np.maximum(p, q)
    _, first, inverse = np.unique(lo * np.int64(max(nv, 1)) + hi, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    mid = (nv + rank[inverse.reshape(-1)]).reshape(nf, 3)
    h0 = first[order]
    new_v = np.concatenate([v, 0.5 * (v[lo[h0]] + v[hi[h0]])])
    new_n = np.concatenate([n, 0.5 * (n[lo[h0]] + n[hi[h0]])])
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    ab, bc, ca = mid[:, 0], mid[:, 1], mid[:, 2]
    return new_v, new_n, np.ascontiguousarray(np.stack([a, ab, ca, ab, b, bc, bc, c, ca, ab, bc, ca], axis=1).reshape(-1, 3))


def loop_once(v, n, t):
    verts, norms, new_index, tris = [row for row in v], [row for row in n], {}, []

    def edge(p, q):
        key = (min(p, q), max(p, q))
        if key not in new_index:
            new_index[key] = len(verts)
            verts.append(0.5 * (v[key[0]] + v[key[1]]))
            norms.append(0.5 * (n[key[0]] + n[key[1]]))
        return new_index[key]

    for a, b, c in t.tolist():
        ab, bc, ca = edge(a, b), edge(b, c), edge(c, a)
        tris += [(a, ab, ca), (ab, b, bc), (bc, c, ca), (ab, bc, ca)]
    return np.array(verts), np.array(norms), np.array(tris, dtype=np.int64)


def load_mesh(n_u, n_v, seed):
    with tempfile.TemporaryDirectory(prefix="tgn_subdivide_bench_") as d:
        path = os.path.join(d, "scan.obj")
        with open(path, "w") as f:
            f.write(synth.obj_text(n_u, n_v, seed, "plain", with_tail=False))
        mesh = preprocess.read_txt_obj_ls(path, ret_mesh=True)[1]
    order = np.random.default_rng(seed).permutation(mesh["triangles"].shape[0])
    return dict(mesh, triangles=np.ascontiguousarray(mesh["triangles"][order]))


def stats(us):
    return dict(us=float(np.median(us)), min_us=float(min(us)), max_us=float(max(us)))


def bench_mesh(mesh, args):
    dev = torch.device("cuda")
    L = _lib.lib()
    v, n, t = mesh["vertices"], mesh["vertex_normals"], mesh["triangles"]
    nv, nf = v.shape[0], t.shape[0]
    want = numpy_once(v, n, t)
    got = preprocess.subdivide_midpoint(mesh)
    for a, b in zip(want, (got["vertices"], got["vertex_normals"], got["triangles"])):
        assert a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64)), "the kernel and the numpy form disagree"
    dv, dn, dt = (torch.from_numpy(x).to(dev) for x in (v, n, t))
    need = L.tgn_subdivide_midpoint_workspace_bytes(nf)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out_v = torch.empty((nv + 3 * nf, 3), dtype=torch.float64, device=dev)
    out_n, out_t = torch.empty_like(out_v), torch.empty((4 * nf, 3), dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)

    def launch():
        _lib.check(L.tgn_subdivide_midpoint(nv, nf, _lib.ptr(dv), _lib.ptr(dn), _lib.ptr(dt), _lib.ptr(out_v), _lib.ptr(out_n), _lib.ptr(out_t),
                                            _lib.ptr(count), _lib.ptr(ws), need, _lib.stream()), "tgn_subdivide_midpoint")

    times = {"device": [], "wrapper": [], "numpy": []}
    for r in range(args.warmup + args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            launch()
        b.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        preprocess.subdivide_midpoint(mesh)
        t1 = time.perf_counter()
        numpy_once(v, n, t)
        t2 = time.perf_counter()
        if r >= args.warmup:
            times["device"].append(a.elapsed_time(b) * 1000.0 / args.inner)
            times["wrapper"].append((t1 - t0) * 1e6)
            times["numpy"].append((t2 - t1) * 1e6)
    loop = []
    for _ in range(args.loop_reps):
        t0 = time.perf_counter()
        loop_once(v, n, t)
        loop.append((time.perf_counter() - t0) * 1e6)
    assert int(count.item()) == want[0].shape[0] - nv
    out = {k: stats(x) for k, x in times.items()}
    out["loop"] = stats(loop)
    out.update(vertices=nv, triangles=nf, new_vertices=int(want[0].shape[0] - nv), workspace_bytes=int(need))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("subdivide_bench needs a GPU: there is nothing to measure without one")
    res = {"workload": "one pass of midpoint subdivision, vertices + normals + triangles, microseconds",
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner,
           "meshes": [bench_mesh(load_mesh(*m), args) for m in MESHES]}
    res["wrapper_beats_numpy_at_15000"] = res["meshes"][1]["wrapper"]["us"] < res["meshes"][1]["numpy"]["us"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
