"""The table behind tests/test_gpu_containment.py and tests/test_containment_host.py: one row per C-ABI entry point of
include/tgn_pointops.h that takes device pointers, in the style of tests/operator_forms.py.

A row names the C functions it covers (keys of _lib.SIGNATURES) and holds
  shapes    the cases, the smallest that reach every tile edge and every launch variant behind the entry point;
  tunings   optionally a list of _lib.tuning(...) settings every shape is run under;
  build     build(shape) -> the operands as (name, role, tensor-or-(shape, dtype)), CPU tensors, roles of tests/arena.py;
  call      call(shape) -> the function (L, views, stream) -> status that makes the raw _lib.lib() call on the views of those operands;
  sizes     {workspace operand: the *_workspace_bytes function (or the header sentence) its size comes from};
  after     optionally after(views, what): what the header promises beyond the outputs (a workspace left zeroed).

Conventions.  Float values are operator_forms.q16 (multiples of 1/16 in [-4, 4]) wherever the operator only moves or adds values:
sums of such values, and of products of two of them, are exact in float32 in any order, so results are bit-comparable even where
float atomics decide the order.  Coordinates of the searches are torch.rand (no ties to speak of; the searches are deterministic
anyway).  Index operands hold valid indices only, labels and offsets are valid: the sweep never passes a bad argument.  A workspace is
exactly what its size function returns; an output is exactly what the header states.  Where the contract leaves part of an
output alone, or accumulates into it, the row pre-fills the whole buffer with zeros (`Z`) and says so.

compare="bound" is allowed for tgn_pt_softmax_aggregate_backward and tgn_aggregation_backward only (BOUND_ALLOWED).  Neither row
needs it: their atomic sums add products of two q16 factors (the softmax weights handed to the backward are multiples of 1/16
too), which are exact in any order, so both rows compare bytes like every other.

EXEMPT lists the entry points without a row and why; tests/test_containment_host.py fails for an entry point with a pointer
argument that is neither covered nor listed.
"""
import numpy as np
import torch

from operator_forms import gen_for, q16

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
BOUND_ALLOWED = ("tgn_pt_softmax_aggregate_backward", "tgn_aggregation_backward")

ROWS = []


def row(name, covers, shapes, build, call, tunings=None, sizes=None, compare="bytes", after=None):
    ROWS.append(dict(name=name, covers=list(covers), shapes=shapes if isinstance(shapes, _Late) else list(shapes), build=build, call=call,
                     tunings=tunings or [{}], sizes=sizes or {}, compare=compare, after=after))


class _Late:
    """a list of `count` shapes worked out when it is first read: it needs a constant of the built library (tgn_fps_resident_capacity(),
    tgn_seg_confusion_chunk()), which collecting the tests must not"""

    def __init__(self, make, count):
        self.make, self.count, self.v = make, count, None

    def __len__(self):
        return self.count

    def __getitem__(self, i):
        if self.v is None:
            self.v = self.make()
            assert len(self.v) == self.count
        return self.v[i]


def _L():
    from toothgroupnetwork_amd import _lib
    return _lib.lib()


def P(t):
    """device pointer of a view; NULL for None and for an empty buffer"""
    import ctypes
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


def I(name, t):
    return (name, "in", t.contiguous())


def O(name, shape, dtype=F32):
    """an output every element of which the call writes: starts as the arena's fill"""
    return (name, "out", (tuple(shape), dtype))


def Z(name, shape, dtype=F32):
    """an output the call accumulates into, or writes only in part: starts as zeros"""
    return (name, "out", torch.zeros(tuple(shape), dtype=dtype))


def W(name, nbytes):
    return (name, "ws", ((int(nbytes),), U8))


def rnd(g, *shape):
    return torch.rand(*shape, generator=g) * 2 - 1


def ridx(g, hi, shape, dtype=I32):
    return torch.randint(0, hi, tuple(shape), generator=g).to(dtype)


def cum(sizes):
    return torch.tensor(np.cumsum(sizes), dtype=I32)


# ---------------------------------------------------------------------------------------------------------------------------
# farthest point sampling
# ---------------------------------------------------------------------------------------------------------------------------
FPS_LOCAL_INDEX, FPS_INDEX64, FPS_THROUGHPUT = 2, 4, 32
FPS_SMALL = [{"fps_lean": 0, "fps_bucket_min": 1000000}, {"fps_lean": 2, "fps_bucket_min": 1000000}]
FPS_BUCKET = [{"fps_bucket_min": 2048}]
RAGGED = ([1, 65, 433, 1025, 2049], [1, 17, 433, 256, 512])       # the 433-point cloud is sampled to exhaustion
BUCKETED = ([2049, 4097, 8193], [128, 128, 128])


def _cap():
    return int(_L().tgn_fps_resident_capacity())


def _fps_ws_bytes(kind, b, n_max):
    L = _L()
    return int(L.tgn_fps_throughput_workspace_bytes(b, n_max) if kind == "throughput" else L.tgn_fps_workspace_bytes(b, n_max))


def _fps_packed_build(fn, shape):
    """shape = (clouds, samples, optional outputs given, int64 indices, workspace kind)"""
    clouds, samples, opt, i64, kind = shape
    g = gen_for("fps" + str(clouds))
    n, m, b = sum(clouds), sum(samples), len(clouds)
    ops = [I("xyz", rnd(g, n, 3)), I("offset", cum(clouds)), I("new_offset", cum(samples)), O("idx", (m,), I64 if i64 else I32)]
    if opt:
        ops.append(O("new_xyz", (m, 3)))
    if fn == "tgn_furthestsampling":
        if opt or max(clouds) > _cap():
            ops.append(("tmp", "ws", ((n,), F32)))
    else:
        ops.append(W("ws", _fps_ws_bytes(kind, b, max(clouds))))
    if fn == "tgn_furthestsampling_prefix" and opt:
        ops.append(O("prefix_out", (b,), I32))
    return ops


def _fps_flags(i64, kind, local):
    return (FPS_LOCAL_INDEX if local else 0) | (FPS_INDEX64 if i64 else 0) | (FPS_THROUGHPUT if kind == "throughput" else 0)


def _fps_packed_call(fn, shape):
    clouds, samples = shape[0], shape[1]
    b, n_max, flags = len(clouds), max(clouds), _fps_flags(shape[3], shape[4], False)

    def call(L, v, st):
        head = (b, n_max, P(v["xyz"]), P(v["offset"]), P(v["new_offset"]))
        if fn == "tgn_furthestsampling":
            return L.tgn_furthestsampling(*head, P(v.get("tmp")), P(v["idx"]), P(v.get("new_xyz")), flags, st)
        ws = (P(v["ws"]), v["ws"].numel())
        if fn == "tgn_furthestsampling_ws":
            return L.tgn_furthestsampling_ws(*head, *ws, P(v["idx"]), P(v.get("new_xyz")), flags, st)
        return L.tgn_furthestsampling_prefix(*head, *ws, P(v["idx"]), P(v.get("new_xyz")), None, None, P(v.get("prefix_out")), flags, st)
    return call


def _fps_dense_build(fn, shape):
    """shape = (B, N, S, optional outputs given, int64 indices, workspace kind)"""
    B, N, S, opt, i64, kind = shape
    g = gen_for(f"fpsd{N}")
    ops = [I("xyz", rnd(g, B, N, 3)), O("idx", (B, S), I64 if i64 else I32)]
    if opt:
        ops.append(O("new_xyz", (B, S, 3)))
    if fn == "tgn_furthestsampling_dense":
        if opt or N > _cap():
            ops.append(("tmp", "ws", ((B * N,), F32)))
    else:
        ops.append(W("ws", _fps_ws_bytes(kind, B, N)))
    if fn == "tgn_furthestsampling_dense_prefix" and opt:
        ops.append(O("prefix_out", (B,), I32))
    return ops


def _fps_dense_call(fn, shape):
    B, N, S = shape[:3]
    flags = _fps_flags(shape[4], shape[5], True)

    def call(L, v, st):
        if fn == "tgn_furthestsampling_dense":
            return L.tgn_furthestsampling_dense(B, N, S, P(v["xyz"]), P(v.get("tmp")), P(v["idx"]), P(v.get("new_xyz")), flags, st)
        ws = (P(v["ws"]), v["ws"].numel())
        if fn == "tgn_furthestsampling_dense_ws":
            return L.tgn_furthestsampling_dense_ws(B, N, S, P(v["xyz"]), *ws, P(v["idx"]), P(v.get("new_xyz")), flags, st)
        return L.tgn_furthestsampling_dense_prefix(B, N, S, P(v["xyz"]), *ws, P(v["idx"]), P(v.get("new_xyz")), None, None,
                                                   P(v.get("prefix_out")), flags, st)
    return call


_OPT_I64 = [(True, False), (False, False), (True, True), (False, True)]
for _fn in ("tgn_furthestsampling", "tgn_furthestsampling_ws", "tgn_furthestsampling_prefix"):
    _sz = {"tmp": "header: offset[b-1] floats"} if _fn == "tgn_furthestsampling" else {"ws": "tgn_fps_workspace_bytes"}
    row(_fn + "[ragged]", [_fn], [RAGGED + oi + ("plain",) for oi in _OPT_I64],
        lambda s, fn=_fn: _fps_packed_build(fn, s), lambda s, fn=_fn: _fps_packed_call(fn, s),
        tunings=FPS_SMALL, sizes=_sz)
    row(_fn + "[bucket]", [_fn], [BUCKETED + oi + ("plain",) for oi in _OPT_I64[:2]],
        lambda s, fn=_fn: _fps_packed_build(fn, s), lambda s, fn=_fn: _fps_packed_call(fn, s),
        tunings=FPS_BUCKET, sizes=_sz)
    # one cloud past the register-resident capacity: the workspace kernel (the streaming kernel through tmp without a workspace)
    row(_fn + "[capacity+1]", [_fn], _Late(lambda: [([_cap() + 1], [64], True, False, "plain")], 1),
        lambda s, fn=_fn: _fps_packed_build(fn, s), lambda s, fn=_fn: _fps_packed_call(fn, s), sizes=_sz)
    if _fn != "tgn_furthestsampling":
        row(_fn + "[throughput]", [_fn], [([4097, 4097], [64, 64], True, False, "throughput")],
            lambda s, fn=_fn: _fps_packed_build(fn, s), lambda s, fn=_fn: _fps_packed_call(fn, s),
            sizes={"ws": "tgn_fps_throughput_workspace_bytes"})

_DENSE_SMALL = [(2, 1, 1), (2, 65, 17), (1, 433, 433), (2, 1025, 256), (2, 2049, 512)]
for _fn in ("tgn_furthestsampling_dense", "tgn_furthestsampling_dense_ws", "tgn_furthestsampling_dense_prefix"):
    _sz = {"tmp": "header: the dense form: B * N floats"} if _fn == "tgn_furthestsampling_dense" else {"ws": "tgn_fps_workspace_bytes"}
    row(_fn + "[small]", [_fn], [s + oi + ("plain",) for s in _DENSE_SMALL for oi in _OPT_I64[:2]] + [(2, 1025, 256, True, True, "plain")],
        lambda s, fn=_fn: _fps_dense_build(fn, s), lambda s, fn=_fn: _fps_dense_call(fn, s),
        tunings=FPS_SMALL, sizes=_sz)
    row(_fn + "[bucket]", [_fn], [(2, 2049, 128, True, False, "plain"), (1, 4097, 128, False, False, "plain"), (1, 8193, 128, True, True, "plain")],
        lambda s, fn=_fn: _fps_dense_build(fn, s), lambda s, fn=_fn: _fps_dense_call(fn, s),
        tunings=FPS_BUCKET, sizes=_sz)
    row(_fn + "[capacity+1]", [_fn], _Late(lambda: [(1, _cap() + 1, 64, True, False, "plain")], 1),
        lambda s, fn=_fn: _fps_dense_build(fn, s), lambda s, fn=_fn: _fps_dense_call(fn, s), sizes=_sz)
    if _fn != "tgn_furthestsampling_dense":
        row(_fn + "[throughput]", [_fn], [(2, 4097, 64, True, False, "throughput")],
            lambda s, fn=_fn: _fps_dense_build(fn, s), lambda s, fn=_fn: _fps_dense_call(fn, s),
            sizes={"ws": "tgn_fps_throughput_workspace_bytes"})


def _fps_identity_build(shape):
    """tests/test_gpu_fps_prefix.py's second call: the cloud IS an FPS sequence (the CPU oracle's, canonical tie order), handed back
    with prefix_in = its length and prefix_ref = its own coordinates, and a workspace of tgn_fps_workspace_bytes(B, N) bytes as that
    test passes it (0 at this size).  The kernel is PRESUMED to take the identity shortcut on the device: nothing here asserts which
    path ran, only that whichever ran stays inside its operands and gives the same bytes in the three runs."""
    from oracle import cpu
    B, N0, N, S = shape
    cloud = rnd(gen_for("fps_identity"), B, N0, 3).numpy()
    seq = cpu.index_points(cloud, cpu.farthest_point_sample(cloud, N))
    xyz = torch.from_numpy(np.ascontiguousarray(seq, dtype=np.float32))
    return [I("xyz", xyz), I("prefix_ref", xyz.clone()), I("prefix_in", torch.full((B,), N, dtype=I32)), I("offset", cum([N] * B)),
            I("new_offset", cum([S] * B)), O("idx", (B, S), I32), O("new_xyz", (B, S, 3)), O("prefix_out", (B,), I32),
            W("ws", _fps_ws_bytes("plain", B, N))]


row("tgn_furthestsampling_dense_prefix[identity]", ["tgn_furthestsampling_dense_prefix"], [(2, 300, 128, 64)], _fps_identity_build,
    lambda s: lambda L, v, st: L.tgn_furthestsampling_dense_prefix(s[0], s[2], s[3], P(v["xyz"]), P(v["ws"]), v["ws"].numel(), P(v["idx"]),
                                                                   P(v["new_xyz"]), P(v["prefix_in"]), P(v["prefix_ref"]), P(v["prefix_out"]),
                                                                   FPS_LOCAL_INDEX, st),
    sizes={"ws": "tgn_fps_workspace_bytes"})
row("tgn_furthestsampling_prefix[identity]", ["tgn_furthestsampling_prefix"], [(2, 300, 128, 64)], _fps_identity_build,
    lambda s: lambda L, v, st: L.tgn_furthestsampling_prefix(s[0], s[2], P(v["xyz"]), P(v["offset"]), P(v["new_offset"]), P(v["ws"]),
                                                             v["ws"].numel(), P(v["idx"]), P(v["new_xyz"]), P(v["prefix_in"]), P(v["prefix_ref"]),
                                                             P(v["prefix_out"]), 0, st),
    sizes={"ws": "tgn_fps_workspace_bytes"})


# ---------------------------------------------------------------------------------------------------------------------------
# neighbour searches
# ---------------------------------------------------------------------------------------------------------------------------
def _ball_r2(N, K):
    """a radius that holds about K of N uniform points of [-1, 1]^3: rows that are padded and rows that overflow"""
    return float((1.9 * K / N) ** (2.0 / 3.0))


def _ball_build(shape, with_idx=True):
    B, N, S, K, i64 = shape
    g = gen_for(f"ball{N}")
    xyz = rnd(g, B, N, 3)
    ops = [I("xyz", xyz), W("ws", _L().tgn_ball_query_workspace_bytes(B, N, S))]
    if with_idx:
        ops += [I("new_xyz", xyz[:, :S].clone()), O("idx", (B, S, K), I64 if i64 else I32)]
    return ops


def _ball_call(which):
    def factory(s):
        B, N, S, K, i64 = s
        r2 = _ball_r2(N, K)

        def call(L, v, st):
            ws = (P(v["ws"]), v["ws"].numel())
            if which == "build":
                return L.tgn_ball_query_build(B, N, S, K, r2, P(v["xyz"]), *ws, st)
            if which == "prebuilt":      # answered from the workspace tgn_ball_query_build filled in the same buffer just before
                rc = L.tgn_ball_query_build(B, N, S, K, r2, P(v["xyz"]), *ws, st)
                return rc or L.tgn_ball_query_prebuilt(B, N, S, K, r2, P(v["xyz"]), P(v["new_xyz"]), P(v["idx"]), int(i64), *ws, st)
            return L.tgn_ball_query(B, N, S, K, r2, P(v["xyz"]), P(v["new_xyz"]), P(v["idx"]), int(i64), *ws, st)
        return call
    return factory


# (1, 32769, 17, 16) is one past kBmMaxN / kGridPermCap but has too few queries for the grid (S * 8 < N / 64): the scan kernel.
# (1, 32769, 130, 16) is the same cloud with enough queries: the grid without the LDS permutation, the rank-select kernel whatever
# ball_bitmap says.  (2, 300, 37, 7): below 2048 points, the scan kernel.  (1, 4097, 130, 33): grid + chunked bitmap kernel.
_BALL = [(2, 300, 37, 7), (1, 4097, 130, 33), (1, 32769, 17, 16), (1, 32769, 130, 16)]
_BALL_SHAPES = [s + (i64,) for s in _BALL for i64 in (False, True)]
_BALL_TUNE = [{"ball_bitmap": 0}, {"ball_bitmap": 1}, {"ball_bitmap": 2}]
row("tgn_ball_query", ["tgn_ball_query"], _BALL_SHAPES, _ball_build, _ball_call("query"), tunings=_BALL_TUNE,
    sizes={"ws": "tgn_ball_query_workspace_bytes"})
# tgn_ball_query_build writes its workspace only: the row has no `out` operand, so its A against B comparison is empty by design and what is
# checked is the status, the guard bands, the cloud and the error word.  What it built is consumed, and compared, in the prebuilt row.
row("tgn_ball_query_build", ["tgn_ball_query_build"], [s + (False,) for s in _BALL], lambda s: _ball_build(s, False), _ball_call("build"),
    tunings=_BALL_TUNE, sizes={"ws": "tgn_ball_query_workspace_bytes"})
row("tgn_ball_query_prebuilt", ["tgn_ball_query_prebuilt"], _BALL_SHAPES, _ball_build, _ball_call("prebuilt"), tunings=_BALL_TUNE,
    sizes={"ws": "tgn_ball_query_workspace_bytes"})


def _knn_build(which, shape):
    segs, qs, k = shape
    g = gen_for(f"knn{sum(segs)}")
    n, m, b = sum(segs), sum(qs), len(segs)
    xyz = rnd(g, n, 3)
    starts = np.concatenate([[0], np.cumsum(segs)[:-1]])
    new_xyz = torch.cat([xyz[s0:s0 + q] for s0, q in zip(starts, qs)])      # the first points of every segment are its queries
    ops = [I("xyz", xyz), I("new_xyz", new_xyz), I("offset", cum(segs)), I("new_offset", cum(qs)), O("idx", (m, k), I32), O("dist2", (m, k))]
    if which == "ws":
        ops.append(W("ws", _L().tgn_knnquery_workspace_bytes(m)))
    if which == "grid":
        ops.append(W("ws", _L().tgn_knnquery_grid_workspace_bytes(b, n, m)))
    return ops


def _knn_call(which):
    def factory(s):
        segs, qs, k = s

        def call(L, v, st):
            a = (P(v["xyz"]), P(v["new_xyz"]), P(v["offset"]), P(v["new_offset"]), P(v["idx"]), P(v["dist2"]))
            if which == "plain":
                return L.tgn_knnquery(len(segs), sum(qs), k, *a, st)
            if which == "ws":
                return L.tgn_knnquery_ws(len(segs), sum(qs), k, *a, P(v["ws"]), v["ws"].numel(), st)
            return L.tgn_knnquery_grid(len(segs), sum(segs), sum(qs), k, *a, P(v["ws"]), v["ws"].numel(), st)
        return call
    return factory


# a segment shorter than k is padded by the kernels (index = segment start, distance 1e10): defined, not a bad argument
_KNN = [([1, 17, 300], [1, 3, 64], k) for k in (1, 16, 36)]
row("tgn_knnquery", ["tgn_knnquery"], _KNN, lambda s: _knn_build("plain", s), _knn_call("plain"))
row("tgn_knnquery_ws", ["tgn_knnquery_ws"], _KNN, lambda s: _knn_build("ws", s), _knn_call("ws"), sizes={"ws": "tgn_knnquery_workspace_bytes"})
row("tgn_knnquery_grid", ["tgn_knnquery_grid"], _KNN + [([5000], [130], 63)], lambda s: _knn_build("grid", s), _knn_call("grid"),
    sizes={"ws": "tgn_knnquery_grid_workspace_bytes"})


def _tnn_build(shape):
    B, N, S, i64 = shape
    g = gen_for(f"three_nn{N}")
    return [I("xyz1", rnd(g, B, N, 3)), I("xyz2", rnd(g, B, S, 3)), O("dist", (B, N, 3)), O("idx", (B, N, 3), I64 if i64 else I32)]


# S < 16 and S > kTnnTile = 1024: three_nn_kernel; 16 <= S <= 1024: three_nn_split_kernel
row("tgn_three_nn", ["tgn_three_nn"], [s + (i,) for s in [(1, 1, 3), (2, 70, 3), (2, 70, 16), (1, 65, 1024), (1, 333, 1025)] for i in (False, True)],
    _tnn_build, lambda s: lambda L, v, st: L.tgn_three_nn(s[0], s[1], s[2], P(v["xyz1"]), P(v["xyz2"]), P(v["dist"]), P(v["idx"]), int(s[3]), st))


def _sqd_build(shape):
    B, N, M = shape
    g = gen_for("sqd")
    return [I("src", q16(g, B, N, 3)), I("dst", q16(g, B, M, 3)), O("out", (B, N, M))]


row("tgn_square_distance", ["tgn_square_distance"], [(1, 1, 1), (2, 17, 33), (1, 300, 257)], _sqd_build,
    lambda s: lambda L, v, st: L.tgn_square_distance(*s, P(v["src"]), P(v["dst"]), P(v["out"]), st))

# rows 4 and 1025 with (6, 0, 3): the four-rows-per-lane kernel alone and with a one-row tail; rows 3: below it; (7, 2, 4): the plain kernel
row("tgn_slice_columns", ["tgn_slice_columns"], [(r,) + c for r in (3, 4, 7, 1025) for c in ((6, 0, 3), (7, 2, 4))],
    lambda s: [I("in", q16(gen_for("slice"), s[0], s[1])), O("out", (s[0], s[3]))],
    lambda s: lambda L, v, st: L.tgn_slice_columns(s[0], s[1], s[2], s[3], P(v["in"]), P(v["out"]), st))


# ---------------------------------------------------------------------------------------------------------------------------
# the dense gather family
# ---------------------------------------------------------------------------------------------------------------------------
_DENSE = [(1, 1, 1, 1, 0), (2, 200, 37, 8, 5), (2, 300, 61, 33, 64), (1, 777, 99, 64, 253)]
_IMPLS = [(1, -1), (2, 0), (2, 2), (2, 16), (2, 17), (2, 18), (7, 16), (7, 0), (7, 2), (10, -1), (0, -1)]     # test_group_points_every_kernel_variant


def _group_build(shape):
    B, N, S, K, D = shape[:5]
    i64, first = shape[5], shape[6]
    g = gen_for(f"group{N}")
    xyz = q16(g, B, N, 3)
    ops = [I("xyz", xyz), I("new_xyz", xyz[:, :S].clone()), I("idx", ridx(g, N, (B, S, K), I64 if i64 else I32)), O("out", (B, S, K, 3 + D))]
    if D:
        ops.append(I("points", q16(g, B, N, D)))
    return ops


def _group_head(v, s):
    return (s[0], s[1], s[2], s[3], s[4], P(v["xyz"]), P(v["new_xyz"]), P(v.get("points")), P(v["idx"]), int(s[5]), int(s[6]), P(v["out"]))


# (2, 192, 32, 8, 3): the only shape here the pairs kernel takes (D in {0, 3, 6}, K a power of two, S * K % 64 == 0); (2, 300, 64, 32, 61)
# the row-piece kernel (3 + D >= 64, K % 4 == 0).  A kernel that does not take a shape falls back to the next one down, as the header says.
_GROUP = _DENSE + [(2, 192, 32, 8, 3), (2, 300, 64, 32, 61)]
row("tgn_group_points", ["tgn_group_points"], [s + (i64, first) for s in _GROUP for i64, first in ((False, True), (True, False))], _group_build,
    lambda s: lambda L, v, st: L.tgn_group_points(*_group_head(v, s), st))
row("tgn_group_points_ex", ["tgn_group_points_ex"],
    [s + (False, True) + ip + (mb,) for s in _GROUP[1:] for ip in _IMPLS for mb in (0,)] + [s + (True, True, 0, -1, 64) for s in _GROUP[1:]],
    _group_build, lambda s: lambda L, v, st: L.tgn_group_points_ex(*_group_head(v, s), s[7], s[8], s[9], st))


def _gather_build(scatter):
    def build(shape):
        B, N, S, K, D, i64 = shape
        C, M = max(D, 1), S * K
        g = gen_for(f"gather{N}")
        idx = I("idx", ridx(g, N, (B, M), I64 if i64 else I32))
        if scatter:     # grad_points is accumulated into: pre-filled with zeros
            return [I("grad_out", q16(g, B, M, C)), idx, Z("grad_points", (B, N, C))]
        return [I("points", q16(g, B, N, C)), idx, O("out", (B, M, C))]
    return build


_DENSE_I = [s + (i,) for s in _DENSE for i in (False, True)]
row("tgn_gather_points", ["tgn_gather_points"], _DENSE_I, _gather_build(False),
    lambda s: lambda L, v, st: L.tgn_gather_points(s[0], s[1], s[2] * s[3], max(s[4], 1), P(v["points"]), P(v["idx"]), int(s[5]), P(v["out"]), st))
row("tgn_scatter_add_points", ["tgn_scatter_add_points"], _DENSE_I, _gather_build(True),
    lambda s: lambda L, v, st: L.tgn_scatter_add_points(s[0], s[1], s[2] * s[3], max(s[4], 1), P(v["grad_out"]), P(v["idx"]), int(s[5]),
                                                 P(v["grad_points"]), st))


def _interp3_build(ex):
    def build(shape):
        B, N, S, C, i64, weight = shape
        g = gen_for(f"three_interpolate{N}{C}")
        ops = [I("points2", q16(g, B, S, C)), I("dist", q16(g, B, N, 3).abs() + 1.0 / 16), I("idx", ridx(g, S, (B, N, 3), I64 if i64 else I32)),
               O("out", (B, N, C))]
        if weight:
            ops.append(O("weight", (B, N, 3)))
        if ex:
            ops.append(I("add", q16(g, B, N, C)))
        return ops
    return build


# C = 8: the 16-byte kernel; C = 5: the per-element one
_INTERP3 = [(s[0], s[1], s[2], C, i64, w) for s in _DENSE for C in (5, 8) for i64, w in ((False, True), (True, False))]
row("tgn_three_interpolate", ["tgn_three_interpolate"], _INTERP3, _interp3_build(False),
    lambda s: lambda L, v, st: L.tgn_three_interpolate(s[0], s[1], s[2], s[3], P(v["points2"]), P(v["dist"]), P(v["idx"]), int(s[4]), P(v["out"]),
                                                P(v.get("weight")), st))
row("tgn_three_interpolate_ex", ["tgn_three_interpolate_ex"], _INTERP3, _interp3_build(True),
    lambda s: lambda L, v, st: L.tgn_three_interpolate_ex(s[0], s[1], s[2], s[3], P(v["points2"]), P(v["dist"]), P(v["idx"]), int(s[4]), P(v["add"]), 1,
                                                   P(v["out"]), P(v.get("weight")), st))


# ---------------------------------------------------------------------------------------------------------------------------
# the packed gather family: (n, m, ns, c, w_c) = source rows, queries, neighbours, channels, weight channels
# ---------------------------------------------------------------------------------------------------------------------------
_PACKED = [(1, 1, 1, 1, 1), (33, 7, 3, 5, 1), (257, 61, 16, 32, 4), (250, 64, 17, 36, 4)]
_V4 = [{"gather_v4": 0}, {"gather_v4": 5}]


def _pk(name, covers, build, call):
    row(name, covers, _PACKED, build, call, tunings=_V4)


def _g(s, tag):
    return gen_for(tag + str(s[0]))


_pk("tgn_grouping_forward", ["tgn_grouping_forward"],
    lambda s: (lambda g: [I("input", q16(g, s[0], s[3])), I("idx", ridx(g, s[0], (s[1], s[2]))), O("output", (s[1], s[2], s[3]))])(_g(s, "grouping")),
    lambda s: lambda L, v, st: L.tgn_grouping_forward(s[1], s[2], s[3], P(v["input"]), P(v["idx"]), P(v["output"]), st))
# grad_input is accumulated into (float atomics on exact q16 sums): pre-filled with zeros
_pk("tgn_grouping_backward", ["tgn_grouping_backward"],
    lambda s: (lambda g: [I("grad_output", q16(g, s[1], s[2], s[3])), I("idx", ridx(g, s[0], (s[1], s[2]))), Z("grad_input", (s[0], s[3]))])(_g(s, "grouping_b")),
    lambda s: lambda L, v, st: L.tgn_grouping_backward(s[1], s[2], s[3], P(v["grad_output"]), P(v["idx"]), P(v["grad_input"]), st))
# interpolation: input (m, c) on the coarse cloud, idx / weight (n, k) with k = ns, output (n, c); the header: output / grad_input
# pre-zeroed, accumulated into
_pk("tgn_interpolation_forward", ["tgn_interpolation_forward"],
    lambda s: (lambda g: [I("input", q16(g, s[1], s[3])), I("idx", ridx(g, s[1], (s[0], s[2]))), I("weight", q16(g, s[0], s[2])),
                          Z("output", (s[0], s[3]))])(_g(s, "interpolation")),
    lambda s: lambda L, v, st: L.tgn_interpolation_forward(s[0], s[3], s[2], P(v["input"]), P(v["idx"]), P(v["weight"]), P(v["output"]), st))
_pk("tgn_interpolation_backward", ["tgn_interpolation_backward"],
    lambda s: (lambda g: [I("grad_output", q16(g, s[0], s[3])), I("idx", ridx(g, s[1], (s[0], s[2]))), I("weight", q16(g, s[0], s[2])),
                          Z("grad_input", (s[1], s[3]))])(_g(s, "interpolation_b")),
    lambda s: lambda L, v, st: L.tgn_interpolation_backward(s[0], s[3], s[2], P(v["grad_output"]), P(v["idx"]), P(v["weight"]), P(v["grad_input"]), st))
_pk("tgn_subtraction_forward", ["tgn_subtraction_forward"],
    lambda s: (lambda g: [I("input1", q16(g, s[0], s[3])), I("input2", q16(g, s[0], s[3])), I("idx", ridx(g, s[0], (s[0], s[2]))),
                          O("output", (s[0], s[2], s[3]))])(_g(s, "subtraction")),
    lambda s: lambda L, v, st: L.tgn_subtraction_forward(s[0], s[2], s[3], P(v["input1"]), P(v["input2"]), P(v["idx"]), P(v["output"]), st))
# both gradients are accumulated into (the reference's kernel adds with atomics): pre-filled with zeros
_pk("tgn_subtraction_backward", ["tgn_subtraction_backward"],
    lambda s: (lambda g: [I("idx", ridx(g, s[0], (s[0], s[2]))), I("grad_output", q16(g, s[0], s[2], s[3])), Z("grad_input1", (s[0], s[3])),
                          Z("grad_input2", (s[0], s[3]))])(_g(s, "subtraction_b")),
    lambda s: lambda L, v, st: L.tgn_subtraction_backward(s[0], s[2], s[3], P(v["idx"]), P(v["grad_output"]), P(v["grad_input1"]), P(v["grad_input2"]), st))


def _agg_build(backward):
    def build(s):
        n, _, ns, c, w_c = s
        g = _g(s, "aggregation")
        ops = [I("input", q16(g, n, c)), I("position", q16(g, n, ns, c)), I("weight", q16(g, n, ns, w_c)), I("idx", ridx(g, n, (n, ns)))]
        if not backward:    # the kernels add to what they find in output, as the reference's do: pre-filled with zeros
            return ops + [Z("output", (n, c))]
        # grad_input is accumulated into with atomics (sums of products of two q16 factors: exact); all three pre-filled with zeros
        return ops + [I("grad_output", q16(g, n, c)), Z("grad_input", (n, c)), Z("grad_position", (n, ns, c)), Z("grad_weight", (n, ns, w_c))]
    return build


_pk("tgn_aggregation_forward", ["tgn_aggregation_forward"], _agg_build(False),
    lambda s: lambda L, v, st: L.tgn_aggregation_forward(s[0], s[2], v["input"].shape[1], s[4], P(v["input"]), P(v["position"]), P(v["weight"]),
                                                  P(v["idx"]), P(v["output"]), st))
_pk("tgn_aggregation_backward", ["tgn_aggregation_backward"], _agg_build(True),
    lambda s: lambda L, v, st: L.tgn_aggregation_backward(s[0], s[2], v["input"].shape[1], s[4], P(v["input"]), P(v["position"]), P(v["weight"]),
                                                   P(v["idx"]), P(v["grad_output"]), P(v["grad_input"]), P(v["grad_position"]),
                                                   P(v["grad_weight"]), st))


# ---------------------------------------------------------------------------------------------------------------------------
# Point-Transformer attention, linear_wgrad, bn_rows
# ---------------------------------------------------------------------------------------------------------------------------
_PT_KEYS = ("Wp1", "bp1", "Wp2", "bp2", "a1", "t1", "Ww1", "bw1", "Ww2", "bw2")


def _attn_build(shape):
    n, ns, c, g_, post = shape
    g = gen_for(f"pt_attention{c}")
    r = lambda *s: torch.randn(*s, generator=g)
    par = dict(Wp1=r(3, 3) * 0.8, bp1=r(3) * 0.2, Wp2=r(c, 3) * 0.8, bp2=r(c) * 0.2, a1=1.0 + 0.1 * r(c), t1=r(c) * 0.2,
               Ww1=r(g_, c) / c ** 0.5, bw1=r(g_) * 0.2, Ww2=r(g_, g_) / g_ ** 0.5, bw2=r(g_) * 0.2)
    ops = [I("p", q16(g, n, 3)), I("xq", q16(g, n, c)), I("xk", q16(g, n, c)), I("xv", q16(g, n, c)), I("idx", ridx(g, n, (n, ns)))]
    ops += [I(k, par[k]) for k in _PT_KEYS]
    if post:
        ops += [I("post_scale", 1.0 + 0.1 * r(c)), I("post_shift", 0.2 * r(c))]
    return ops + [O("out", (n, c))]


# the five widths of tests/test_gpu_pt_attention_bounds.py (one kernel instantiation per weight-channel count), n = 257: 64 full
# blocks of four queries and one query over
row("tgn_pt_attention_forward", ["tgn_pt_attention_forward"],
    [(257, ns, c, g_, post) for c, g_ in ((32, 4), (64, 8), (128, 16), (256, 32), (512, 64)) for ns, post in ((8, False), (16, True))] + [(1, 1, 4, 4, False)],
    _attn_build,
    lambda s: lambda L, v, st: L.tgn_pt_attention_forward(s[0], s[1], s[2], s[3], P(v["p"]), P(v["xq"]), P(v["xk"]), P(v["xv"]), P(v["idx"]),
                                                   *[P(v[k]) for k in _PT_KEYS], P(v.get("post_scale")), P(v.get("post_shift")), P(v["out"]), st))

_SMA = [(300, 65, 32, 4), (257, 8, 48, 6), (257, 8, 64, 8), (1, 1, 4, 1)]


def _sma_build(backward):
    def build(shape):
        n, ns, c, g_ = shape
        g = gen_for(f"pt_sma{c}")
        ops = [I("xv", q16(g, n, c)), I("pr", q16(g, n, ns, c)), I("idx", ridx(g, n, (n, ns)))]
        if not backward:
            return ops + [I("logit", q16(g, n, ns, g_)), O("sm", (n, ns, g_)), O("out", (n, c))]
        # sm is an INPUT of the backward: multiples of 1/64 in [0, 1], so that the atomic sums of grad_out * sm into grad_xv (which is
        # accumulated into: pre-filled with zeros) are exact in any order
        return ops + [I("sm", q16(g, n, ns, g_).abs() / 4), I("grad_out", q16(g, n, c)), Z("grad_xv", (n, c)), O("grad_pr", (n, ns, c)),
                      O("grad_logit", (n, ns, g_))]
    return build


row("tgn_pt_softmax_aggregate_forward", ["tgn_pt_softmax_aggregate_forward"], _SMA, _sma_build(False),
    lambda s: lambda L, v, st: L.tgn_pt_softmax_aggregate_forward(*s, P(v["xv"]), P(v["pr"]), P(v["logit"]), P(v["idx"]), P(v["sm"]), P(v["out"]), st))
row("tgn_pt_softmax_aggregate_backward", ["tgn_pt_softmax_aggregate_backward"], _SMA, _sma_build(True),
    lambda s: lambda L, v, st: L.tgn_pt_softmax_aggregate_backward(*s, P(v["xv"]), P(v["pr"]), P(v["sm"]), P(v["idx"]), P(v["grad_out"]), P(v["grad_xv"]),
                                                            P(v["grad_pr"]), P(v["grad_logit"]), st))


def _wgrad_build(shape):
    rows, cin, cout, bias = shape
    g = gen_for(f"wgrad{rows}")
    ops = [I("x", q16(g, rows, cin)), I("gy", q16(g, rows, cout)), O("dW", (cout, cin)), W("ws", _L().tgn_linear_wgrad_workspace_bytes(rows, cin, cout))]
    return ops + ([O("db", (cout,))] if bias else [])


row("tgn_linear_wgrad", ["tgn_linear_wgrad"],
    [(r, ci, co, b) for r in (2, 257, 4099) for (ci, co), b in (((3, 3), True), ((13, 70), False), ((32, 32), True))] + [(1, 1, 1, True)],
    _wgrad_build,
    lambda s: lambda L, v, st: L.tgn_linear_wgrad(s[0], s[1], s[2], P(v["x"]), P(v["gy"]), P(v["dW"]), P(v.get("db")), P(v["ws"]), v["ws"].numel(), st),
    sizes={"ws": "tgn_linear_wgrad_workspace_bytes"})


def _bn_ws(C):
    """the header: ZERO before the first use"""
    return ("ws", "ws", torch.zeros(int(_L().tgn_bn_rows_workspace_bytes(C)), dtype=U8))


def _bn_zero_after(v, what):
    assert not bool(v["ws"].any()), f"{what}: tgn_bn_rows left a non-zero byte in its workspace (the header: the kernels leave it zeroed)"


def _bn_fwd_build(shape):
    rows, C, running, relu = shape
    g = gen_for(f"bn{rows}{C}")
    ops = [I("x", q16(g, rows, C)), I("gamma", q16(g, C)), I("beta", q16(g, C)), O("y", (rows, C)), O("save_mean", (C,)), O("save_invstd", (C,)),
           _bn_ws(C)]
    if running:     # updated in place: they start with contents
        ops += [("running_mean", "out", q16(g, C)), ("running_var", "out", q16(g, C).abs() + 0.5), ("nbt", "out", torch.tensor([3], dtype=I64))]
    return ops


def _bn_bwd_build(shape):
    rows, C, _, relu = shape
    g = gen_for(f"bnb{rows}{C}")
    # save_mean on the 1/16 grid and save_invstd = 1/2: (x - mean) * invstd * dy is then exact, and so are the double atomic sums
    return [I("x", q16(g, rows, C)), I("y", q16(g, rows, C)), I("dy", q16(g, rows, C)), I("gamma", q16(g, C)), I("save_mean", q16(g, C)),
            I("save_invstd", torch.full((C,), 0.5)), O("dx", (rows, C)), O("dgamma", (C,)), O("dbeta", (C,)), _bn_ws(C)]


_BN = [(rows, C, flag, flag) for rows in (2, 257, 4099) for C, flag in ((1, True), (20, False), (1024, True))] + [(257, 20, True, False), (257, 1024, False, True)]
row("tgn_bn_rows_forward", ["tgn_bn_rows_forward"], _BN, _bn_fwd_build,
    lambda s: lambda L, v, st: L.tgn_bn_rows_forward(s[0], s[1], P(v["x"]), P(v["gamma"]), P(v["beta"]), 1e-5, 0.1, P(v.get("running_mean")),
                                              P(v.get("running_var")), P(v.get("nbt")), int(s[3]), P(v["y"]), P(v["save_mean"]),
                                              P(v["save_invstd"]), P(v["ws"]), st),
    sizes={"ws": "tgn_bn_rows_workspace_bytes"}, after=_bn_zero_after)
row("tgn_bn_rows_backward", ["tgn_bn_rows_backward"], _BN, _bn_bwd_build,
    lambda s: lambda L, v, st: L.tgn_bn_rows_backward(s[0], s[1], P(v["x"]), P(v["y"]), P(v["dy"]), P(v["gamma"]), P(v["save_mean"]), P(v["save_invstd"]),
                                               int(s[3]), P(v["dx"]), P(v["dgamma"]), P(v["dbeta"]), P(v["ws"]), st),
    sizes={"ws": "tgn_bn_rows_workspace_bytes"}, after=_bn_zero_after)


# ---------------------------------------------------------------------------------------------------------------------------
# crops, clustering, tsegnet
# ---------------------------------------------------------------------------------------------------------------------------
_CROP = [(1, 1, 2), (2, 600, 17), (1, 1025, 64)]


def _feats(g, b, c, n):
    return q16(g, b, c, n)


def _centroid_build(shape):
    b, n, nlab = shape
    g = gen_for(f"label_centroids{n}")
    return [I("feats", _feats(g, b, 6, n)), I("labels", torch.randint(-1, nlab, (b, n), generator=g)), O("counts", (b, nlab), I32), O("cent", (b, nlab, 3))]


row("tgn_label_centroids", ["tgn_label_centroids"], _CROP, _centroid_build,
    lambda s: lambda L, v, st: L.tgn_label_centroids(s[0], s[1], 6, P(v["feats"]), P(v["labels"]), s[2], P(v["counts"]), P(v["cent"]), st))
row("tgn_label_centroids_f64", ["tgn_label_centroids_f64"], _CROP, _centroid_build,
    lambda s: lambda L, v, st: L.tgn_label_centroids_f64(s[0], s[1], 6, P(v["feats"]), P(v["labels"]), s[2], P(v["counts"]), P(v["cent"]), st))


def _crop_common(g, b, n, t):
    return [I("feats", _feats(g, b, 6, n)), I("crop_scan", ridx(g, b, (t,)))]


def _crop_knn_build(shape):
    b, n, t, k = shape
    g = gen_for(f"crop_knn{n}")
    return _crop_common(g, b, n, t) + [I("cent", q16(g, t, 3)), O("idx_out", (t, k), I64)]


# k = 4096 = kKnnMaxK at n = 4097
row("tgn_crop_knn", ["tgn_crop_knn"], [(1, 1, 2, 1), (2, 600, 17, 1), (2, 600, 17, 64), (1, 1025, 64, 64), (1, 4097, 3, 4096)], _crop_knn_build,
    lambda s: lambda L, v, st: L.tgn_crop_knn(s[0], s[1], 6, P(v["feats"]), s[2], P(v["crop_scan"]), P(v["cent"]), s[3], P(v["idx_out"]), st))


def _crop_gather_build(shape):
    b, n, t, k, with_labels = shape
    g = gen_for(f"crop_gather{n}")
    ops = _crop_common(g, b, n, t) + [I("idx", ridx(g, n, (t, k), I64)), O("out", (t, 6, k))]
    return ops + ([I("labels", torch.randint(-1, 17, (b, n), generator=g)), O("out_labels", (t, 1, k), I64)] if with_labels else [])


row("tgn_crop_gather_center", ["tgn_crop_gather_center"],
    [(1, 1, 2, 1, True), (2, 600, 17, 64, True), (2, 600, 17, 1, False), (1, 1025, 64, 64, False), (1, 4097, 3, 4096, True)], _crop_gather_build,
    lambda s: lambda L, v, st: L.tgn_crop_gather_center(s[0], s[1], 6, s[2], s[3], P(v["feats"]), P(v["crop_scan"]), P(v["idx"]), P(v.get("labels")),
                                                 P(v["out"]), P(v.get("out_labels")), st))


def _blobs(name, n, spread=2):
    """n points in three blobs on the 1/16 grid (as tests/operator_forms.py)"""
    g = gen_for(name)
    centres = torch.tensor([[-2.0, -2.0, 0.0], [0.0, 2.0, 1.0], [2.0, -1.0, -1.0]])
    return centres[torch.arange(n) % 3] + torch.randint(-spread, spread + 1, (n, 3), generator=g).float() / 16, g


def _dbscan_build(shape):
    sizes = shape
    n, b = sum(sizes), len(sizes)
    return [I("xyz", _blobs("dbscan", n)[0]), I("offset", cum(sizes)), O("labels", (n,), I64), O("core", (n,), U8), O("nclusters", (b,), I32),
            W("ws", _L().tgn_dbscan_workspace_bytes(b, n))]


row("tgn_dbscan", ["tgn_dbscan"], [(1,), (257,), (1025,), (1, 100, 156)], _dbscan_build,
    lambda s: lambda L, v, st: L.tgn_dbscan(len(s), sum(s), P(v["xyz"]), P(v["offset"]), 0.2, 5, P(v["labels"]), P(v["core"]), P(v["nclusters"]),
                                     P(v["ws"]), v["ws"].numel(), st),
    sizes={"ws": "tgn_dbscan_workspace_bytes"})
_CLN = [(1,), (257,), (1025,)]
row("tgn_mean_shift", ["tgn_mean_shift"], _CLN,
    lambda s: [I("xyz", _blobs("mean_shift", s[0])[0].double()), O("means", (s[0], 3), F64), O("counts", (s[0],), I32)],
    lambda s: lambda L, v, st: L.tgn_mean_shift(s[0], P(v["xyz"]), 0.5, 300, P(v["means"]), P(v["counts"]), st))
row("tgn_nearest_center", ["tgn_nearest_center"], [(1, 1), (257, 3), (1025, 17)],
    lambda s: (lambda pts_g: [I("xyz", pts_g[0].double()), I("centers", q16(pts_g[1], s[1], 3).double()), O("labels", (s[0],), I64)])(_blobs("nearest", s[0])),
    lambda s: lambda L, v, st: L.tgn_nearest_center(s[0], P(v["xyz"]), s[1], P(v["centers"]), P(v["labels"]), st))


def _moments_build(shape):
    n, nlab, masked = shape
    pts, g = _blobs("moments", n)
    ops = [I("xyz", pts), I("labels", torch.randint(0, nlab, (n,), generator=g)), O("counts", (nlab,), I32), O("mean", (nlab, 3), F64),
           O("cov", (nlab, 3, 3), F64)]
    return ops + ([I("mask", ridx(g, 2, (n,), U8))] if masked else [])


row("tgn_cluster_moments", ["tgn_cluster_moments"], [(1, 1, False), (257, 3, True), (1025, 17, False)], _moments_build,
    lambda s: lambda L, v, st: L.tgn_cluster_moments(s[0], P(v["xyz"]), P(v["labels"]), P(v.get("mask")), s[1], P(v["counts"]), P(v["mean"]), P(v["cov"]), st))


def _vote_build(shape):
    m, k, n_cand = shape
    g = gen_for(f"vote{m}")
    return [I("nn_idx", ridx(g, n_cand, (m, k), I64)), I("cand_labels", ridx(g, 5, (n_cand,), I64)), O("out", (m,), I64)]


row("tgn_cluster_vote", ["tgn_cluster_vote"], [(1, 1, 1), (257, 10, 100), (1025, 32, 300)], _vote_build,
    lambda s: lambda L, v, st: L.tgn_cluster_vote(s[0], s[1], P(v["nn_idx"]), s[2], P(v["cand_labels"]), P(v["out"]), st))


def _prop_build(shape):
    b, m = shape
    g = gen_for(f"proposals{m}")
    # moved: the kept points are packed into the first sum(counts) rows and the rest is left alone: pre-filled with zeros
    return [I("l3_xyz", q16(g, b, 3, m)), I("offset", q16(g, b, 3, m)), I("dist", q16(g, b, 1, m) / 8 + 0.25), Z("moved", (b * m, 3)),
            O("counts", (b,), I32)]


row("tgn_tsg_proposals", ["tgn_tsg_proposals"], [(1, 1), (2, 64), (3, 1000), (2, 1024)], _prop_build,       # 1024 = kPropMaxM
    lambda s: lambda L, v, st: L.tgn_tsg_proposals(s[0], s[1], P(v["l3_xyz"]), P(v["offset"]), P(v["dist"]), 0.3, P(v["moved"]), P(v["counts"]), st))


def _cropf_build(shape):
    b, n, cf, t, k, with_labels = shape
    g = gen_for(f"crop_features{n}{cf}")
    ops = _crop_common(g, b, n, t) + [I("cent", q16(g, t, 3)), I("idx", ridx(g, n, (t, k), I64)), O("out", (t, 3 + cf + 1, k))]
    if cf:
        ops.append(I("l0_points", q16(g, b, cf, n)))
    return ops + ([I("labels", torch.randint(-1, 17, (b, n), generator=g)), O("out_labels", (t, 1, k), I64)] if with_labels else [])


row("tgn_tsg_crop_features", ["tgn_tsg_crop_features"],
    [(1, 1, 0, 1, 1, False), (2, 600, 5, 5, 100, True), (2, 600, 32, 5, 1, False), (1, 1025, 32, 3, 100, True), (1, 1025, 0, 3, 257, True)], _cropf_build,
    lambda s: lambda L, v, st: L.tgn_tsg_crop_features(s[0], s[1], 6, s[2], s[3], s[4], P(v["feats"]), P(v.get("l0_points")), P(v["crop_scan"]), P(v["cent"]),
                                                P(v["idx"]), P(v.get("labels")), P(v["out"]), P(v.get("out_labels")), st))


def _paint_build(shape):
    b, n, t, k = shape
    g = gen_for(f"paint{n}")
    return [I("crop_scan", ridx(g, b, (t,))), I("idx", ridx(g, n, (t, k), I64)), I("mask", ridx(g, 2, (t, k), U8)), I("ids", ridx(g, 48, (t,), I64)),
            O("out", (b, n), I64)]


row("tgn_tsg_paint", ["tgn_tsg_paint"], [(1, 1, 1, 1), (2, 600, 5, 100), (1, 1025, 3, 1), (2, 257, 7, 257)], _paint_build,
    lambda s: lambda L, v, st: L.tgn_tsg_paint(s[0], s[1], s[2], s[3], P(v["crop_scan"]), P(v["idx"]), P(v["mask"]), P(v["ids"]), P(v["out"]), st))


# ---------------------------------------------------------------------------------------------------------------------------
# the training losses
# ---------------------------------------------------------------------------------------------------------------------------
def _offset_loss_inputs(b, n):
    g = gen_for(f"offset_loss{n}")
    xyz, labels = q16(g, b, 3, n), torch.randint(-1, 16, (b, n), generator=g)
    counts = torch.stack([torch.bincount(labels[i][labels[i] >= 0], minlength=16) for i in range(b)]).to(I32)
    cent = torch.zeros(b, 16, 3)
    for i in range(b):
        for t in range(16):
            if counts[i, t]:
                cent[i, t] = xyz[i][:, labels[i] == t].mean(1)
    return g, [I("offset", q16(g, b, 3, n) / 8), I("xyz", xyz), I("labels", labels), I("counts", counts), I("cent", cent)]


def _offl_fwd_build(shape):
    b, n = shape
    return _offset_loss_inputs(b, n)[1] + [O("losses", (3,)), O("scales", (b, 33)), W("ws", _L().tgn_offset_loss_workspace_bytes(b, n))]


def _offl_bwd_build(shape):
    b, n = shape
    g, ops = _offset_loss_inputs(b, n)
    return ops + [I("scales", q16(g, b, 33).abs() / 64), I("grad_losses", q16(g, 3)), O("grad_offset", (b, 3, n))]


# (2, 32769): one point past kLossMaxBlocks * kLossThreads, the grid-stride path
_LOSS_BN = [(1, 1), (3, 65), (1, 257), (2, 32769)]
_OFFL = ("offset", "xyz", "labels", "counts", "cent")
row("tgn_offset_loss_forward", ["tgn_offset_loss_forward"], _LOSS_BN, _offl_fwd_build,
    lambda s: lambda L, v, st: L.tgn_offset_loss_forward(s[0], s[1], *[P(v[k]) for k in _OFFL], P(v["losses"]), P(v["scales"]), P(v["ws"]),
                                                  v["ws"].numel(), st),
    sizes={"ws": "tgn_offset_loss_workspace_bytes"})
row("tgn_offset_loss_backward", ["tgn_offset_loss_backward"], _LOSS_BN, _offl_bwd_build,
    lambda s: lambda L, v, st: L.tgn_offset_loss_backward(s[0], s[1], *[P(v[k]) for k in _OFFL], P(v["scales"]), P(v["grad_losses"]), P(v["grad_offset"]), st))


def _centl_inputs(shape):
    b, m, c, with_exists = shape
    g = gen_for(f"centroid_loss{m}")
    ops = [I("offset", q16(g, b, 3, m) / 8), I("xyz", q16(g, b, 3, m)), I("distance", q16(g, b, m).abs() / 8), I("centroid", q16(g, b, 3, c))]
    if with_exists:
        ex = ridx(g, 2, (b, c), U8)
        ex[:, 0] = 1
        ops.append(I("exists", ex))
    return g, ops


def _centl_fwd_build(shape):
    b = shape[0]
    return _centl_inputs(shape)[1] + [O("losses", (3,)), O("scales", (4,)), O("rev_arg", (b, 16), I32), W("ws", _L().tgn_centroid_loss_workspace_bytes(b))]


def _centl_bwd_build(shape):
    b, m = shape[:2]
    g, ops = _centl_inputs(shape)
    rev = torch.where(torch.rand(b, 16, generator=g) < 0.5, ridx(g, m, (b, 16)), torch.full((b, 16), -1, dtype=I32))
    return ops + [I("scales", q16(g, 4).abs() / 64), I("rev_arg", rev), I("grad_losses", q16(g, 3)), O("grad_offset", (b, 3, m)),
                  O("grad_distance", (b, m))]


_CENTL = [(1, 1, 2, False), (3, 63, 16, True), (2, 1025, 16, False), (2, 1025, 16, True)]
_CENTK = ("offset", "xyz", "distance", "centroid")
row("tgn_centroid_loss_forward", ["tgn_centroid_loss_forward"], _CENTL, _centl_fwd_build,
    lambda s: lambda L, v, st: L.tgn_centroid_loss_forward(s[0], s[1], s[2], *[P(v[k]) for k in _CENTK], P(v.get("exists")), P(v["losses"]), P(v["scales"]),
                                                    P(v["rev_arg"]), P(v["ws"]), v["ws"].numel(), st),
    sizes={"ws": "tgn_centroid_loss_workspace_bytes"})
row("tgn_centroid_loss_backward", ["tgn_centroid_loss_backward"], _CENTL, _centl_bwd_build,
    lambda s: lambda L, v, st: L.tgn_centroid_loss_backward(s[0], s[1], s[2], *[P(v[k]) for k in _CENTK], P(v.get("exists")), P(v["scales"]), P(v["rev_arg"]),
                                                     P(v["grad_losses"]), P(v["grad_offset"]), P(v["grad_distance"]), st))


# ---------------------------------------------------------------------------------------------------------------------------
# DGCNN, PointNet
# ---------------------------------------------------------------------------------------------------------------------------
def _fknn_build(shape):
    B, N, D, k, with_dist = shape
    g = gen_for(f"feature_knn{N}")
    ops = [I("x", rnd(g, B, D, N)), O("idx", (B, N, k), I64), W("ws", _L().tgn_feature_knn_workspace_bytes(B, N, k))]
    return ops + ([O("dist2", (B, N, k))] if with_dist else [])


# one and several candidate splits, every DP / KP instantiation class, an odd N at a split boundary
row("tgn_feature_knn", ["tgn_feature_knn"],
    [s + (d,) for s in [(1, 32, 3, 32), (2, 257, 6, 20), (1, 1025, 64, 9), (1, 1537, 17, 1)] for d in (True, False)] + [(1, 300, 30, 8, True)], _fknn_build,
    lambda s: lambda L, v, st: L.tgn_feature_knn(s[0], s[1], s[2], s[3], P(v["x"]), P(v["idx"]), P(v.get("dist2")), P(v["ws"]), v["ws"].numel(), st),
    sizes={"ws": "tgn_feature_knn_workspace_bytes"})


def _edge_sizes(B, N):
    """into channels 64..127 of a 192-channel buffer with 8 floats between the scans: the buffer holds (B - 1) * ostride + (coff + 64) * N
    floats (include/tgn_pointops.h) -- to its last element"""
    ostride, coff = 192 * N + 8, 64
    return ostride, coff, (B - 1) * ostride + (coff + 64) * N


def _edge_build(two):
    def build(shape):
        B, N, K = shape
        g = gen_for(f"edgeconv{N}")
        # the call writes channels coff .. coff + 63 of every scan and leaves the rest alone: the whole buffer is pre-filled with zeros
        ops = [I("P", q16(g, B, N, 64)), I("Q", q16(g, B, N, 64)), I("idx", ridx(g, N, (B, N, K), I64)), Z("out", (_edge_sizes(B, N)[2],))]
        return ops + ([I("W2", q16(g, 64, 64) / 8), I("b2", q16(g, 64))] if two else [])
    return build


# (1, 8195, 20): the grid-stride loop starts above 8192 queries
_EDGE = [(1, 1, 1), (2, 5, 32), (1, 8195, 20)]
row("tgn_edgeconv1_max", ["tgn_edgeconv1_max"], _EDGE, _edge_build(False),
    lambda s: lambda L, v, st: L.tgn_edgeconv1_max(s[0], s[1], s[2], P(v["P"]), P(v["Q"]), P(v["idx"]), P(v["out"]), *_edge_sizes(s[0], s[1])[:2], st))
row("tgn_edgeconv2_max", ["tgn_edgeconv2_max"], _EDGE, _edge_build(True),
    lambda s: lambda L, v, st: L.tgn_edgeconv2_max(s[0], s[1], s[2], P(v["P"]), P(v["Q"]), P(v["idx"]), P(v["W2"]), P(v["b2"]), P(v["out"]),
                                            *_edge_sizes(s[0], s[1])[:2], st))


def _lmax_build(shape):
    B, K, C, N, act = shape
    g = gen_for(f"linear_act_max{N}")
    return [I("x", q16(g, B, K, N)), I("Wt", q16(g, K, C)), I("shift", q16(g, C)), O("out", (B, C)),
            W("ws", _L().tgn_linear_act_max_workspace_bytes(B, N, K, C))]


# (B, K, C, N); N = 1000 / 1001: rows of x that are / are not 16-byte aligned, the vector and the scalar staging
row("tgn_linear_act_max", ["tgn_linear_act_max"],
    [s + (act,) for s, acts in (((1, 1, 1, 1), (0,)), ((1, 16, 128, 128), (0, 1, 2)), ((2, 17, 130, 129), (1,)), ((3, 33, 257, 1000), (2,)),
                                ((3, 33, 257, 1001), (0, 1, 2))) for act in acts], _lmax_build,
    lambda s: lambda L, v, st: L.tgn_linear_act_max(s[0], s[3], s[1], s[2], P(v["x"]), P(v["Wt"]), P(v["shift"]), s[4], 0.2, P(v["out"]), P(v["ws"]),
                                             v["ws"].numel(), st),
    sizes={"ws": "tgn_linear_act_max_workspace_bytes"})


# ---------------------------------------------------------------------------------------------------------------------------
# metrics, subdivision
# ---------------------------------------------------------------------------------------------------------------------------
def _chunk():
    return int(_L().tgn_seg_confusion_chunk())


def _conf_build(shape):
    sizes, nlab = shape
    n, b = sum(sizes), len(sizes)
    g = gen_for(f"seg_confusion{n}")
    return [I("offset", cum(sizes)), I("gt", ridx(g, nlab, (n,), I64)), I("sem", ridx(g, nlab, (n,), I64)), I("ins", ridx(g, nlab, (n,), I64)),
            O("ins_gt", (b, nlab, nlab), I32), O("ins_sem", (b, nlab, nlab), I32)]


row("tgn_seg_confusion", ["tgn_seg_confusion"],
    _Late(lambda: [((1,), 2), ((_chunk(),), 17), ((_chunk() + 1,), 64), ((300, 0, _chunk() + 1, 1), 17)], 4), _conf_build,
    lambda s: lambda L, v, st: L.tgn_seg_confusion(len(s[0]), sum(s[0]), P(v["offset"]), P(v["gt"]), P(v["sem"]), P(v["ins"]), s[1], P(v["ins_gt"]),
                                            P(v["ins_sem"]), st))


def _logits_build(shape):
    B, C, N = shape
    g = gen_for(f"seg_logits{N}")
    return [I("logits", q16(g, B, C, N)), I("gt", torch.randint(-1, C - 1, (B, N), generator=g)), O("ins_gt", (B, C, C), I32), O("ins_sem", (B, C, C), I32)]


row("tgn_seg_confusion_logits", ["tgn_seg_confusion_logits"], [(1, 2, 1), (2, 17, 2049), (1, 64, 2048)], _logits_build,
    lambda s: lambda L, v, st: L.tgn_seg_confusion_logits(s[0], s[1], s[2], P(v["logits"]), P(v["gt"]), 1, P(v["ins_gt"]), P(v["ins_sem"]), st))


def _scores_build(shape):
    b, nlab, _ = shape
    g = gen_for(f"seg_scores{nlab}")
    return [I("ins_gt", ridx(g, 50, (b, nlab, nlab)) * ridx(g, 2, (b, nlab, 1))), I("ins_sem", ridx(g, 50, (b, nlab, nlab))), O("scores", (b, 4), F64),
            O("instances", (b,), I32), O("iou", (b, nlab), F64), O("matched_gt", (b, nlab), I32)]


row("tgn_seg_scores", ["tgn_seg_scores"], [(1, 2, 0), (3, 17, 1), (2, 64, 0)], _scores_build,
    lambda s: lambda L, v, st: L.tgn_seg_scores(s[0], s[1], P(v["ins_gt"]), P(v["ins_sem"]), s[2], P(v["scores"]), P(v["instances"]), P(v["iou"]),
                                         P(v["matched_gt"]), st))


def _subdivide_build(shape):
    nv, nf, with_normals = shape
    g = gen_for(f"subdivide{nf}")
    if nf == 4:
        tri = torch.tensor([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], dtype=I64)      # the tetrahedron
    else:
        tri = ridx(g, nv, (nf, 3), I64)
    # rows [0, nv + *n_new) of out_vertices / out_normals are written, the rest of the upper bound is left alone: pre-filled with zeros
    ops = [I("vertices", q16(g, nv, 3).double()), I("triangles", tri), Z("out_vertices", (nv + 3 * nf, 3), F64), O("out_triangles", (4 * nf, 3), I64),
           O("n_new", (1,), I32), W("ws", _L().tgn_subdivide_midpoint_workspace_bytes(nf))]
    return ops + ([I("normals", q16(g, nv, 3).double()), Z("out_normals", (nv + 3 * nf, 3), F64)] if with_normals else [])


# 1366 triangles = 4098 half-edges: one scan chunk and two over
row("tgn_subdivide_midpoint", ["tgn_subdivide_midpoint"],
    [(4, 4, True), (4, 4, False), (700, 1366, True), (700, 1366, False), (5, 0, True)], _subdivide_build,
    lambda s: lambda L, v, st: L.tgn_subdivide_midpoint(s[0], s[1], P(v["vertices"]), P(v.get("normals")), P(v["triangles"]), P(v["out_vertices"]),
                                                 P(v.get("out_normals")), P(v["out_triangles"]), P(v["n_new"]), P(v["ws"]), v["ws"].numel(), st),
    sizes={"ws": "tgn_subdivide_midpoint_workspace_bytes"})


# ---------------------------------------------------------------------------------------------------------------------------
# the two members of the fused set-abstraction family that group c of tests/test_gpu_hotpath_overlap.py does not launch
# ---------------------------------------------------------------------------------------------------------------------------
def _gather_act_build(shape):
    B, N, S, K, C1, i64, relu = shape
    g = gen_for(f"sa_gather_act{N}")
    return [I("A", q16(g, B, N, C1)), I("new_xyz", q16(g, B, S, 3)), I("Wxs", q16(g, 3, C1)), I("b2", q16(g, C1)),
            I("idx", ridx(g, N, (B, S, K), I64 if i64 else I32)), O("out", (B, S, K, C1))]


row("tgn_sa_gather_act", ["tgn_sa_gather_act"],
    [(1, 1, 1, 1, 4, False, 0), (2, 200, 37, 8, 20, False, 1), (2, 300, 61, 33, 64, True, 1), (1, 777, 99, 64, 252, False, 1)], _gather_act_build,
    lambda s: lambda L, v, st: L.tgn_sa_gather_act(s[0], s[1], s[2], s[3], s[4], P(v["A"]), P(v["new_xyz"]), P(v["Wxs"]), P(v["b2"]), P(v["idx"]),
                                            int(s[5]), s[6], P(v["out"]), st))
# the image is a whole number of (128-column, 16-row) tiles: C2 = 1, 130 and 260 leave a ragged last tile, which the call must fill too
row("tgn_sa_mlp2_split_weights", ["tgn_sa_mlp2_split_weights"], [(16, 1), (32, 130), (64, 128), (208, 260)],
    lambda s: [I("W2f", q16(gen_for("split_weights"), s[0] // 8, s[1], 8)), O("W2s", (int(_L().tgn_sa_mlp2_split_bytes(s[0], s[1])),), U8)],
    lambda s: lambda L, v, st: L.tgn_sa_mlp2_split_weights(s[0], s[1], P(v["W2f"]), P(v["W2s"]), st))


# ---------------------------------------------------------------------------------------------------------------------------
# entry points without a row
# ---------------------------------------------------------------------------------------------------------------------------
_HOST = "host memory or no launch: "
_FWD = "forwards to its tgn_* twin, which has a row; tests/test_gpu_parity.py::test_all_ten_verbatim_launchers_on_a_side_stream runs it"
_SA = "fused set-abstraction family: write containment and the two-fill comparison are group c of tests/test_gpu_hotpath_overlap.py"
EXEMPT = {
    "tgn_obj_count": _HOST + "reads a file, host pointers",
    "tgn_obj_read": _HOST + "reads a file into host arrays",
    "tgn_vertex_normals": _HOST + "CPU code over host arrays",
    "tgn_scan_open": _HOST + "the preprocess loader, host memory",
    "tgn_scan_take": _HOST + "copies host rows out of a handle",
    "tgn_fps_bucket_order": _HOST + "fills a host table, no device needed",
    "tgn_set_default_stream": _HOST + "stores a stream handle",
    "tgn_stream_delay": _HOST + "its pointer is the stream; the kernel touches no memory",
    "tgn_take_index_error": _HOST + "its pointer is the stream; reads the library's own error word",
    "tgn_clear_index_error": _HOST + "its pointer is the stream; clears the library's own error word",
    **{n: _FWD for n in ("furthestsampling_cuda_launcher", "knnquery_cuda_launcher", "grouping_forward_cuda_launcher",
                         "grouping_backward_cuda_launcher", "interpolation_forward_cuda_launcher", "interpolation_backward_cuda_launcher",
                         "subtraction_forward_cuda_launcher", "subtraction_backward_cuda_launcher", "aggregation_forward_cuda_launcher",
                         "aggregation_backward_cuda_launcher")},
    **{n: _SA for n in ("tgn_sa_point_transform", "tgn_sa_point_transform_bf16x3", "tgn_sa_gather_max", "tgn_sa_direct_max", "tgn_sa_mlp2_max",
                        "tgn_sa_mlp2_max_bf16x3", "tgn_sa_all_mlp2_max")},
}
EXEMPT_HOST = ("tgn_obj_count", "tgn_obj_read", "tgn_vertex_normals", "tgn_scan_open", "tgn_scan_take", "tgn_fps_bucket_order",
               "tgn_set_default_stream", "tgn_stream_delay", "tgn_take_index_error", "tgn_clear_index_error")


def covered():
    return {n for r in ROWS for n in r["covers"]}
