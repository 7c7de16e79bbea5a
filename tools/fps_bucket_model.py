#!/usr/bin/env python3
"""CPU model of the bookkeeping of fps_bucket_kernel (csrc/fps_bucket.hip): how many buckets does one sample touch?

The kernel's iteration time follows the busiest wave: every bucket a new sample's box test cannot rule out costs that
wave one 64-point update, and every update that lowers the bucket's maximum costs it a 64-lane refresh.  Which buckets are
touched depends only on how the cloud was dealt out to the buckets, so it can be counted without a GPU.  This tool restates

  * the set-up: bounding box, clamped cell coordinates, the cell code (`z`: Morton code, `hilbert`: Hilbert index of the
    cell, `kd`: no cells at all -- balanced kd leaves of 64 points, longest-axis median, splits at multiples of 64),
    the counting sort (stable here; arbitrary inside a cell on the device) and the bucket -> (wave, slot) map;
  * one iteration: the box test `!(L >= bmax)` with the kernel's fp32 operation order, the update, the refresh-skip rule
    (a refresh only when a point that HELD the bucket's maximum came closer) and the arg-max with first-index ties;

and prints, per cloud, the mean number of touched buckets per iteration, how many of those changed any point, how many
were refreshed, the same two counts on the busiest wave (the one the others wait for at the barrier), how often the wave that
wins an iteration did not have to search its candidate in it (`winner: clean`: its own-candidate mask is ready and the box test
leaves its chain), how often it is the previous winner's wave, the extra buckets a reused mask walks per iteration, and the
histogram of the busiest wave's touched count.  `kd` is the yardstick of what a better partition than any curve over cells could give.

The samples it picks on the way are farthest point sampling itself; --check compares them with a plain numpy FPS, and the
`hilbert` mapping with the table the library exports (tgn_fps_bucket_order).  numpy only, no GPU.

  python tools/fps_bucket_model.py --synthetic arch --order hilbert          # the benchmark's level 1: 24 000 -> 4096
  python tools/fps_bucket_model.py --synthetic arch --n 4096 --m 1024 --nt 512 --p 16 --order z --perm 1,3
  python tools/fps_bucket_model.py --cloud scan.npy --m 4096 --order kd
"""
import argparse
import ctypes
import importlib.util
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE = 64
F32 = np.float32


# ---- cell codes ---------------------------------------------------------------------------------------------------------
def morton3(cx, cy, cz, bits):
    """x bit b -> code bit 3 b, y -> 3 b + 1, z -> 3 b + 2 (spread5 of the kernel's large-cloud path)."""
    code = np.zeros_like(cx, dtype=np.uint32)
    for b in range(bits):
        code |= ((cx >> b) & 1).astype(np.uint32) << (3 * b)
        code |= ((cy >> b) & 1).astype(np.uint32) << (3 * b + 1)
        code |= ((cz >> b) & 1).astype(np.uint32) << (3 * b + 2)
    return code


def hilbert3(cx, cy, cz, bits):
    """fps_hilbert3 of csrc/fps_common.h, vectorised: Hilbert index of cell (cx, cy, cz) of a (2^bits)^3 grid."""
    X = [np.asarray(c).astype(np.uint32).copy() for c in (cx, cy, cz)]
    M = 1 << (bits - 1)
    Q = M
    while Q > 1:
        P = np.uint32(Q - 1)
        for i in range(3):
            hit = (X[i] & np.uint32(Q)) != 0
            t = np.where(hit, np.uint32(0), (X[0] ^ X[i]) & P)
            X[0] = np.where(hit, X[0] ^ P, X[0] ^ t)
            X[i] = X[i] ^ t if i else X[0]
        Q >>= 1
    X[1] = X[1] ^ X[0]
    X[2] = X[2] ^ X[1]
    t = np.zeros_like(X[0])
    Q = M
    while Q > 1:
        t = np.where((X[2] & np.uint32(Q)) != 0, t ^ np.uint32(Q - 1), t)
        Q >>= 1
    h = np.zeros_like(X[0])
    for b in range(bits - 1, -1, -1):
        for i in range(3):
            h = (h << np.uint32(1)) | (((X[i] ^ t) >> np.uint32(b)) & np.uint32(1))
    return h


def hilbert_table(bits):
    """The mapping in the layout of tgn_fps_bucket_order: entry x | y << bits | z << 2 bits."""
    c = np.arange(1 << (3 * bits), dtype=np.uint32)
    mask = (1 << bits) - 1
    return hilbert3(c & mask, (c >> bits) & mask, c >> (2 * bits), bits).astype(np.uint16)


def library_table(bits=4, path=None):
    """The table the kernel itself reads, through the C API (host side; the library is loaded, no device is opened)."""
    path = path or os.environ.get("TGN_LIB_PATH") or os.path.join(REPO, "toothgroupnetwork_amd", "csrc", "libtgn_pointops.so")
    lib = ctypes.CDLL(path)
    out = np.zeros(1 << (3 * bits), dtype=np.uint16)
    lib.tgn_fps_bucket_order.restype = ctypes.c_int
    lib.tgn_fps_bucket_order.argtypes = [ctypes.c_int, ctypes.c_void_p]
    rc = lib.tgn_fps_bucket_order(bits, out.ctypes.data_as(ctypes.c_void_p))
    if rc != 0:
        raise RuntimeError(f"tgn_fps_bucket_order({bits}) failed with status {rc}")
    return out


def cell_coords(xyz, bits):
    """Step 1 and `cell_of` of the kernel: fp32 throughout; non-finite coordinates stay out of the box and land in cell 0."""
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        finite = np.abs(xyz) <= F32(3.0e38)
        lo = np.where(finite, xyz, F32(np.inf)).min(axis=0)
        hi = np.where(finite, xyz, F32(-np.inf)).max(axis=0)
        ext = (hi - lo).astype(F32)
        ok = (ext > 0) & (ext < F32(3.0e38))
        scale = np.where(ok, F32(1 << bits) / np.where(ok, ext, F32(1)), F32(0)).astype(F32)
        t = ((xyz - lo).astype(F32) * scale).astype(F32)
        t = np.fmin(np.fmax(t, F32(0)), F32((1 << bits) - 1))      # fmaxf / fminf: NaN -> 0
        t = np.where(np.isnan(t), F32(0), t)
    return t.astype(np.int64)


def kd_order(xyz):
    """Sorted position -> point index for balanced kd leaves of 64: split along the longest axis at the multiple of 64
    nearest the median (the last, partial leaf ends up on the right)."""
    pts = np.nan_to_num(np.asarray(xyz, dtype=np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    out = []
    stack = [np.arange(pts.shape[0])]
    while stack:
        idx = stack.pop()
        if idx.size <= WAVE:
            out.append(idx)
            continue
        p = pts[idx]
        ax = int(np.argmax(p.max(axis=0) - p.min(axis=0)))
        idx = idx[np.argsort(p[:, ax], kind="stable")]
        nb = -(-idx.size // WAVE)
        left = WAVE * ((nb + 1) // 2)
        stack.append(idx[left:])      # popped after the left half: depth-first, left to right
        stack.append(idx[:left])
    return np.concatenate(out)


def sorted_order(xyz, order, bits):
    """Sorted position -> original point index (what tab[] holds before the wave permutation)."""
    if order == "kd":
        return kd_order(xyz)
    cc = cell_coords(xyz, bits)
    if order == "z":
        code = morton3(cc[:, 0], cc[:, 1], cc[:, 2], bits)
    elif order == "hilbert":
        code = hilbert3(cc[:, 0], cc[:, 1], cc[:, 2], bits)
    else:
        raise ValueError(f"order {order!r}: expected z, hilbert or kd")
    return np.argsort(code, kind="stable")


# ---- bucket -> wave ------------------------------------------------------------------------------------------------------
def bucket_wave(nb, nw, perm):
    """fps_bucket_slot of the kernel: bucket b sits in register slot b / NW of wave perm(b % NW, slot).
    3 is what the kernel does (rotation by the slot); 0 is plain round robin, 1 the XOR fold that served the Z-order curve,
    2, 4 and 5 other rotations that were tried."""
    b = np.arange(nb)
    sl, i = b // nw, b % nw
    if perm == 0:
        w = i
    elif perm == 1:
        w = i ^ ((sl ^ (sl >> 3)) & (nw - 1))
    elif perm == 2:
        w = (i + 3 * sl + (sl >> 3)) & (nw - 1)
    elif perm == 3:
        w = (i + sl) & (nw - 1)
    elif perm == 4:
        w = (i + 3 * sl) & (nw - 1)
    elif perm == 5:
        w = (i + 5 * sl + (sl >> 3)) & (nw - 1)
    else:
        raise ValueError(f"perm {perm}: expected 0 .. 5")
    return w


# ---- the iteration --------------------------------------------------------------------------------------------------------
def _dist(dx, dy, dz):
    return ((dx * dx).astype(F32) + (dy * dy).astype(F32)).astype(F32) + (dz * dz).astype(F32)   # dist_direct_nofma


def _box_test(blo, bhi, bmax, q):
    """fps_box_mask of the kernel: True where a sample at q may change a bucket (fp32, the update's operation order)."""
    e = np.fmax(np.fmax(blo - q, q - bhi), F32(0)).astype(F32)
    return ~(_dist(e[:, 0], e[:, 1], e[:, 2]) >= bmax)


def simulate(xyz, m, order="hilbert", bits=4, perm=3, nt=512, p=48, own_rule="b", trace=None):
    """Run the kernel's bookkeeping for m samples.  Returns (indices, stats).

    Every wave's candidate is tracked as the kernel tracks it: searched again only when the bucket that holds it is refreshed.  A
    wave that did not search in an iteration takes the box test of its own buckets against its own candidate before the barrier
    (`own mask`), and the wave that wins uses that mask for the next iteration instead of the test at the hand-off.  own_rule "a"
    drops the own mask whenever a bucket of the wave is refreshed (it is then the mask of the hand-off, bit for bit); "b" keeps it
    until the wave searches again (bucket maxima only shrink, so it contains the mask of the hand-off).  `trace`, if a list, gets
    one (j, winning wave, reused, mask used for the wave's buckets, mask of the hand-off for them) per iteration."""
    if own_rule not in ("a", "b"):
        raise ValueError(f"own_rule {own_rule!r}: expected a or b")
    xyz = np.ascontiguousarray(xyz, dtype=F32)[:, :3]
    n = xyz.shape[0]
    nw = nt // WAVE
    if n > nt * p:
        raise ValueError(f"{n} points do not fit <{nt},{p}> ({nt * p})")
    pos2pt = sorted_order(xyz, order, bits)
    nb = -(-n // WAVE)
    pad = nb * WAVE - n
    owner = np.concatenate([pos2pt, np.full(pad, -1, dtype=pos2pt.dtype)]).reshape(nb, WAVE)
    valid = owner >= 0
    pts = np.where(valid[:, :, None], xyz[np.maximum(owner, 0)], F32(0)).astype(F32)       # padding sits at the origin
    key = np.where(valid, owner, np.iinfo(np.int64).max).astype(np.int64)                   # tie key = original index
    d = np.where(valid, F32(1e10), F32(-1)).astype(F32)
    with np.errstate(invalid="ignore"):
        blo = np.fmin.reduce(np.where(valid[:, :, None], pts, F32(np.inf)), axis=1).astype(F32)    # NaN stays out of the box
        bhi = np.fmax.reduce(np.where(valid[:, :, None], pts, F32(-np.inf)), axis=1).astype(F32)
    bmax = d.max(axis=1)
    barg = key.min(axis=1)                        # all real points start at 1e10: the smallest index wins
    wave_of = bucket_wave(nb, nw, perm)

    idx = np.zeros(m, dtype=np.int64)
    touched = np.zeros(m, dtype=np.int64)
    changed = np.zeros(m, dtype=np.int64)
    refreshed = np.zeros(m, dtype=np.int64)
    busy_t = np.zeros(m, dtype=np.int64)
    busy_r = np.zeros(m, dtype=np.int64)
    q = xyz[0] if n else np.zeros(3, dtype=F32)
    # per wave: the bucket of its candidate (-1: to be searched), the candidate point, and the mask taken against it
    wave_buckets = [np.nonzero(wave_of == w)[0] for w in range(nw)]
    cand_bucket = np.full(nw, -1, dtype=np.int64)
    cand_pt = np.zeros(nw, dtype=np.int64)
    dirty = np.ones(nw, dtype=bool)
    own_ok = np.zeros(nw, dtype=bool)
    own_mask = [np.zeros(b.size, dtype=bool) for b in wave_buckets]
    extra = np.zeros(m, dtype=np.int64)         # buckets walked only because a reused mask was older than the hand-off's
    clean = same = 0
    prev_wl = -1
    with np.errstate(invalid="ignore", over="ignore"):
        exact = _box_test(blo, bhi, bmax, q)    # the mask of iteration 1, taken in front of the loop from point 0
        used = exact.copy()
        for j in range(1, m):
            extra[j] = int((used & ~exact).sum())
            U = np.nonzero(used & ~exact)[0]
            if U.size:                          # a bucket of a stale mask: its update is a no-op, and nothing is refreshed
                du = (pts[U] - q).astype(F32)
                assert not (_dist(du[:, :, 0], du[:, :, 1], du[:, :, 2]) < d[U]).any()
            T = np.nonzero(exact)[0]
            if T.size:
                dT = d[T]
                diff = (pts[T] - q).astype(F32)
                dd = _dist(diff[:, :, 0], diff[:, :, 1], diff[:, :, 2])
                closer = dd < dT
                hold = ((dT == bmax[T][:, None]) & closer).any(axis=1)
                nd = np.fmin(dd, dT)                                   # vmin_f32: NaN never lowers a distance
                d[T] = nd
                R = T[hold]
                if R.size:
                    ndr = nd[hold]
                    mx = ndr.max(axis=1)
                    bmax[R] = mx
                    barg[R] = np.where(ndr == mx[:, None], key[R], np.iinfo(np.int64).max).min(axis=1)
                    dirty[wave_of[R[R == cand_bucket[wave_of[R]]]]] = True
                    if own_rule == "a":
                        own_ok[wave_of[R]] = False
                touched[j] = T.size
                changed[j] = int(closer.any(axis=1).sum())
                refreshed[j] = R.size
                busy_t[j] = np.bincount(wave_of[T], minlength=nw).max()
                if R.size:
                    busy_r[j] = np.bincount(wave_of[R], minlength=nw).max()
            searched = dirty.copy()
            for w in np.nonzero(dirty)[0]:      # section B: the wave's candidate, first index on ties
                wb = wave_buckets[w]
                if wb.size and bmax[wb].max() >= 0:
                    at = wb[bmax[wb] == bmax[wb].max()]
                    cand_bucket[w] = at[np.argmin(barg[at])]
                    cand_pt[w] = barg[cand_bucket[w]]
                dirty[w] = False
                own_ok[w] = False
            for w in np.nonzero(~searched & ~own_ok)[0]:    # off the chain, before the barrier
                wb = wave_buckets[w]
                own_mask[w] = _box_test(blo[wb], bhi[wb], bmax[wb], xyz[cand_pt[w]] if cand_bucket[w] >= 0 else np.zeros(3, dtype=F32))
                own_ok[w] = True
            top = bmax.max()
            k = int(barg[bmax == top].min()) if top >= 0 else 0
            idx[j] = k
            q = xyz[k]
            exact = _box_test(blo, bhi, bmax, q)            # the hand-off: the mask of iteration j + 1
            used = exact.copy()
            if top >= 0:
                live = cand_bucket >= 0
                wl = int(np.nonzero(live)[0][np.lexsort((cand_pt[live], -bmax[cand_bucket[live]]))[0]])
                assert cand_pt[wl] == k, "the winning wave's candidate is not the block's arg-max"
                reused = bool(own_ok[wl])
                wb = wave_buckets[wl]
                if reused:
                    used[wb] = own_mask[wl]
                if trace is not None:
                    trace.append((j, wl, reused, used[wb].copy(), exact[wb].copy()))
                clean += not searched[wl]
                same += wl == prev_wl
                prev_wl = wl
    it = max(m - 1, 1)
    stats = {
        "n": n, "m": m, "buckets": nb, "order": order, "bits": bits, "perm": perm, "nt": nt, "p": p,
        "touched": touched.sum() / it, "changed": changed.sum() / it, "refreshed": refreshed.sum() / it,
        "busiest_touched": busy_t.sum() / it, "busiest_refreshed": busy_r.sum() / it,
        "busiest_hist": np.bincount(busy_t[1:]).tolist(),
        # the winning wave: did not search in the iteration it wins (its own mask can be ready); is the previous winner's wave
        "winner_clean": clean / it, "winner_same_wave": same / it, "own_rule": own_rule, "extra_touched": extra.sum() / it,
    }
    return idx, stats


def plain_fps(xyz, m):
    """Farthest point sampling as the reference states it (fp32, ((dx^2 + dy^2) + dz^2), first index on ties)."""
    xyz = np.ascontiguousarray(xyz, dtype=F32)[:, :3]
    d = np.full(xyz.shape[0], F32(1e10), dtype=F32)
    idx = np.zeros(m, dtype=np.int64)
    k = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(1, m):
            diff = (xyz - xyz[k]).astype(F32)
            d = np.fmin(_dist(diff[:, 0], diff[:, 1], diff[:, 2]), d)
            k = int(np.argmax(d))
            idx[j] = k
    return idx


def _synth():
    spec = importlib.util.spec_from_file_location("_tgn_synth", os.path.join(REPO, "toothgroupnetwork_amd", "synth.py"))
    mod = importlib.util.module_from_spec(spec)        # by file: the package itself would import torch
    spec.loader.exec_module(mod)
    return mod


HEADER = (f"{'cloud':>6s} {'order':>8s} {'bits':>4s} {'perm':>4s} {'kernel':>9s} {'buckets':>7s} | {'touched':>8s} {'changed':>8s} "
          f"{'refreshed':>9s} | {'busiest wave: touched':>21s} {'refreshed':>9s} | {'winner: clean':>13s} {'same wave':>9s} {'extra':>6s} | "
          f"histogram of the busiest wave's touched count")


def row(name, s):
    kernel = f"<{s['nt']},{s['p']}>"
    hist = " ".join(f"{i}:{c}" for i, c in enumerate(s["busiest_hist"]) if c)
    return (f"{name:>6s} {s['order']:>8s} {s['bits']:4d} {s['perm']:4d} {kernel:>9s} {s['buckets']:7d} | {s['touched']:8.2f} "
            f"{s['changed']:8.2f} {s['refreshed']:9.2f} | {s['busiest_touched']:21.3f} {s['busiest_refreshed']:9.3f} | "
            f"{s['winner_clean']:13.3f} {s['winner_same_wave']:9.3f} {s['extra_touched']:6.3f} | {hist}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--cloud", help=".npy file, (n, >=3) or (b, n, >=3): xyz in the first three columns")
    src.add_argument("--synthetic", choices=["arch", "uniform"], help="synth.scan_batch clouds (the benchmark uses arch, seed 100)")
    ap.add_argument("--n", type=int, default=24000)
    ap.add_argument("--scans", type=int, default=2)
    ap.add_argument("--seed", type=int, default=100)
    ap.add_argument("--m", type=int, default=4096, help="samples per cloud")
    ap.add_argument("--order", default="hilbert", help="comma-separated: z, hilbert, kd")
    ap.add_argument("--bits", default="4", help="comma-separated cell bits per axis (the kernel: 4)")
    ap.add_argument("--perm", default="3", help="comma-separated bucket -> wave permutations: 3 the kernel's (i + slot) % NW, 0 round robin, "
                    "1 XOR fold, 2 / 4 / 5 other rotations (bucket_wave)")
    ap.add_argument("--nt", type=int, default=512, help="threads of the kernel instance")
    ap.add_argument("--p", type=int, default=48, help="points per thread = register slots = buckets per wave")
    ap.add_argument("--check", action="store_true", help="compare the samples with a plain FPS and the mapping with the library's table")
    args = ap.parse_args(argv)

    if args.cloud:
        clouds = np.load(args.cloud)
        clouds = clouds[None] if clouds.ndim == 2 else clouds
    else:
        clouds = _synth().scan_batch(args.scans, args.n, args.synthetic, seed=args.seed)
    if args.check:
        assert np.array_equal(hilbert_table(4), library_table(4)), "the tool's Hilbert mapping differs from the kernel's table"
        print("# hilbert mapping == tgn_fps_bucket_order(4)")
    print(HEADER)
    for order in args.order.split(","):
        for bits in [int(b) for b in args.bits.split(",")] if order != "kd" else [0]:
            for perm in [int(x) for x in args.perm.split(",")]:
                for c, cloud in enumerate(clouds):
                    idx, st = simulate(cloud, args.m, order, bits, perm, args.nt, args.p)
                    if args.check:
                        assert np.array_equal(idx, plain_fps(cloud, args.m)), "the model's samples are not farthest point sampling"
                    print(row(str(c), st), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
