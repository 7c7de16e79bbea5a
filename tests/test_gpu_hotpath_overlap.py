"""GPU: what the pipelined fused HotPath computes while two steps overlap, and what its kernels write.

bench.py --fused 1 runs FPS and the ball queries of step k+1 on one stream over the set-abstraction kernels of step k on another.
FPS indices are a pure function of the coordinates, so every level of every step has exactly one right answer whatever runs beside
it.  Three groups of tests:

  a  the schedule itself at the benchmark's shapes (B = 8, both parity sets, two alternating batches, no host synchronisation
     between steps), every level against the CPU oracle applied to the GPU's OWN input of that level -- the first wrong level
     names itself -- and every output against the one-stream HotPath, bit for bit;
  b  one FPS launch beside one set-abstraction launch, all operands carved from one canary-filled arena with 64-KiB guard bands:
     no byte outside the declared outputs may change, the FPS result is the oracle's, the level's output is that of the same
     launch run alone;
  c  the fused set-abstraction family alone in the same arena, at shapes that are no multiple of any tile and at Shape A's levels.

No float atomics anywhere on these paths: equality is the bar for everything but the oracle's float64 MLP (not compared here)."""
import hashlib
import time

import numpy as np
import pytest
import torch

from arena import CANARY, CANARY_B, GUARD, Arena  # noqa: F401  (tests/arena.py)

pytestmark = pytest.mark.gpu

T_STEPS = 6        # steps issued back to back per round (both parity sets are inspected: steps T-2 and T-1)
ROUNDS = 5         # fresh HotPath objects per case: fixed, never "until it fails"
SEEDS = (5, 105)   # synth.scan_batch seeds scan i with seed + i: two disjoint batches of 8
PAIRS = 4          # (FPS, set-abstraction) launch pairs per case of group b, every one checked.  The first pair on two new streams
#                    starts its kernels too far apart to overlap (measured: never wrong before the fix, profiles/fps_overlap_before_after.txt);
#                    of the later ones four in five were wrong at 1024 points before the fix.  Fixed, never "until it fails".


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---------------------------------------------------------------------------------------------------------------------------
# a. the pipelined fused schedule at the shapes bench.py --fused 1 times
# ---------------------------------------------------------------------------------------------------------------------------
_ORACLE_MEMO = {}


def _memo(oracle, what, arrays, fn):
    """The oracle applied to the GPU's own intermediate results: a correct run feeds it the same bytes in every round and in both
    parity sets, so each distinct input is computed once."""
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    key = (what, h.hexdigest())
    if key not in _ORACLE_MEMO:
        _ORACLE_MEMO[key] = fn()
    return _ORACLE_MEMO[key]


_ONE_STREAM = {}


def _one_stream_outputs(dev, name, shape, B, seed):
    """HotPath(fused=True) on one stream: the level outputs the pipelined schedule has to reproduce bit for bit."""
    from toothgroupnetwork_amd import hotpath, synth
    key = (name, B, seed)
    if key not in _ONE_STREAM:
        pts = T(synth.scan_batch(B, shape["n"], "arch", seed), dev)
        levels = hotpath.HotPath(B, dev, shape=shape, fused=True).run(pts[:, :, :3].contiguous(), [pts])
        torch.cuda.synchronize()
        _ONE_STREAM[key] = [lv["out"].clone() for lv in levels]
    return _ONE_STREAM[key]


def _diff(got, want):
    """'<count> of <size> entries, scans [...], first differing row per scan {...}' for two (B, S, ...) arrays"""
    ne = (got != want).reshape(got.shape[0], got.shape[1], -1).any(2)
    scans = [int(b) for b in np.nonzero(ne.any(1))[0]]
    return (f"{int((got != want).sum())} of {got.size} entries differ, in scans {scans}, first differing row per scan "
            f"{ {b: int(np.argmax(ne[b])) for b in scans} }")


@pytest.mark.parametrize("name", ["A", "B"])
def test_pipelined_fused_hotpath_overlapping_steps_vs_oracle(dev, oracle, name):
    """HotPath(fused=True, pipeline=True), bf16x3 kernels (the default), Shape A and Shape B at B = 8: six steps back to back with
    no host synchronisation between them, alternating two batches, five rounds on fresh objects; then both parity sets, per level:
    FPS indices = the oracle's on the level's own input cloud, new_xyz = those rows of it bit for bit, every branch's ball query =
    the oracle's, the level's output = the one-stream HotPath's, bit for bit.

    Shape A level 3 (1024 -> 256) and Shape B level 2 (1024 -> 512) are the levels whose FPS runs as fps_lean_kernel<256, 4> beside
    the previous step's bf16x3 kernels.  Before the fix this test failed there and only there (profiles/fps_overlap_before_after.txt)."""
    from toothgroupnetwork_amd import config, hotpath, synth
    assert config.cfg.sa_bf16x3, "the case under test is the default bf16x3 path"
    shape = hotpath.SHAPE_A if name == "A" else hotpath.SHAPE_B
    B = 8
    t0 = time.time()
    batches = [synth.scan_batch(B, shape["n"], "arch", s) for s in SEEDS]
    dpts = [T(b, dev) for b in batches]
    dxyz = [p[:, :, :3].contiguous() for p in dpts]
    want_out = [_one_stream_outputs(dev, name, shape, B, s) for s in SEEDS]
    failures = []
    for rnd in range(ROUNDS):
        hp = hotpath.HotPath(B, dev, shape=shape, pipeline=True, fused=True)
        for k in range(T_STEPS):
            hp.run(dxyz[k & 1], [dpts[k & 1]], inputs_on_current_stream=False)
        torch.cuda.synchronize()
        for k in (T_STEPS - 2, T_STEPS - 1):
            levels, cur = hp.sets[k & 1], np.ascontiguousarray(batches[k & 1][:, :, :3])
            for li, lv in enumerate(levels):
                tag = f"round {rnd} step {k} level {li + 1} (FPS {lv['N']} -> {lv['S']})"
                fidx = _memo(oracle, ("fps", lv["S"]), [cur], lambda: oracle.farthest_point_sample(cur, lv["S"]))
                got_idx = lv["fps_idx"].cpu().numpy()
                if not np.array_equal(got_idx, fidx):
                    failures.append(f"{tag}: fps_idx != oracle: {_diff(got_idx, fidx)}")
                got_xyz = lv["new_xyz"].cpu().numpy()
                rows = oracle.index_points(cur, np.clip(got_idx, 0, lv["N"] - 1))      # (a wild index is reported by the line above)
                if not np.array_equal(got_xyz.view(np.uint32), rows.view(np.uint32)):
                    failures.append(f"{tag}: new_xyz is not cloud[fps_idx]: {_diff(got_xyz, rows)}")
                for bi, (br, (r, K)) in enumerate(zip(lv["branches"], hotpath._branches(shape["radius"][li], shape["nsample"][li]))):
                    gidx = _memo(oracle, ("ball", r, K), [cur, got_xyz], lambda: oracle.query_ball_point(r, K, cur, got_xyz))
                    got_g = br["group_idx"].cpu().numpy()
                    if not np.array_equal(got_g, gidx):
                        failures.append(f"{tag} branch {bi}: group_idx != oracle: {_diff(got_g, gidx)}")
                if not torch.equal(lv["out"], want_out[k & 1][li]):
                    failures.append(f"{tag}: out != one-stream HotPath: {_diff(lv['out'].cpu().numpy(), want_out[k & 1][li].cpu().numpy())}")
                cur = got_xyz          # the next level is judged on what the GPU handed it
        del hp
    print(f"\nshape {name}: {ROUNDS} rounds x {T_STEPS} steps, {len(failures)} failed comparisons, {time.time() - t0:.1f} s")
    for f in failures:
        print("   ", f)
    assert not failures, f"{len(failures)} comparisons failed; the first: {failures[0]}"


# ---------------------------------------------------------------------------------------------------------------------------
# b / c. single launches in the arena
# ---------------------------------------------------------------------------------------------------------------------------
def _branch_operands(N, S, K, D, widths, B, seed, bf16x3, dev, xyz_first=True):
    """plan_branch of a seeded one- or two-layer shared MLP plus seeded inputs of a level: dict(plan, xyz, new_xyz, points, idx)."""
    from toothgroupnetwork_amd import sa_fused as F
    g = torch.Generator().manual_seed(seed)
    C1 = widths[0]
    W1 = torch.randn(C1, 3 + D, generator=g) / float(D + 3) ** 0.5
    first = {k: v.to(dev) if torch.is_tensor(v) else v for k, v in F.pack_first_layer(W1, 0.1 * torch.randn(C1, generator=g), None, None, D,
                                                                                    xyz_first).items()}
    second = None
    if len(widths) == 2:
        W2 = torch.randn(widths[1], C1, generator=g) / float(C1) ** 0.5
        second = tuple(t.to(dev) for t in F.pack_second_layer(W2, 0.1 * torch.randn(widths[1], generator=g), None, None, F.pad16(C1)))
    plan = F.plan_branch(first, second, K, D, bf16x3=bf16x3)
    xyz = torch.rand(B, N, 3, generator=g) * 2 - 1
    return dict(plan=plan, B=B, N=N, S=S, xyz=xyz.to(dev), new_xyz=xyz[:, torch.randperm(N, generator=g)[:S]].contiguous().to(dev),
                points=torch.randn(B, N, D, generator=g).to(dev) if D else None,
                idx=torch.randint(0, N, (B, S, K), generator=g, dtype=torch.int32).to(dev))


def _branch_into_arena(ar, ops, tag=""):
    """Every operand of launch_branch as an arena buffer: inputs and weight images copied in, `out` and `A` left as canary."""
    plan, h = ops["plan"], {}
    for k in ("xyz", "new_xyz", "points", "idx"):
        h[k] = None if ops[k] is None else ar.add(tag + k, like=ops[k])
    for k in ("W1", "b1", "Wt", "W2f", "b2", "W2s"):
        h[k] = ar.add(tag + k, like=plan[k]) if plan.get(k) is not None else None
    h["Wts"] = ar.add(tag + "Wts", like=plan["Wts"][0]) if plan.get("Wts") is not None else None
    h["out"] = ar.add(tag + "out", shape=(ops["B"], ops["S"], plan["C_out"]), dtype=torch.float32, out=True)
    h["A"] = None if plan["direct"] else ar.add(tag + "A", shape=(ops["B"], ops["N"], plan["C1p"]), dtype=torch.float32, out=True)
    return h


def _arena_launcher(ops, h, views):
    """launch(stream) -> launch_branch on the arena's views, with the arena's copy of the plan"""
    from toothgroupnetwork_amd import sa_fused as F
    v = {k: (None if i is None else views[i]) for k, i in h.items()}
    plan = dict(ops["plan"])
    for k in ("W1", "b1", "Wt", "W2f", "b2", "W2s"):
        if k in plan:
            plan[k] = v[k]
    if plan.get("Wts") is not None:
        plan["Wts"] = (v["Wts"], plan["Wts"][1])

    def launch(st):
        F.launch_branch(plan, ops["B"], ops["N"], ops["S"], v["xyz"], v["new_xyz"], v["points"], v["idx"], 0, v["out"], v["A"], st)
    return launch, v


def _unguarded(ops):
    """the same launch on ordinary allocations: (out, A)"""
    from toothgroupnetwork_amd import _lib, sa_fused as F
    plan = ops["plan"]
    out = torch.empty(ops["B"], ops["S"], plan["C_out"], dtype=torch.float32, device=ops["xyz"].device)
    A = None if plan["direct"] else torch.empty(ops["B"], ops["N"], plan["C1p"], dtype=torch.float32, device=ops["xyz"].device)
    F.launch_branch(plan, ops["B"], ops["N"], ops["S"], ops["xyz"], ops["new_xyz"], ops["points"], ops["idx"], 0, out, A, _lib.stream())
    torch.cuda.synchronize()
    return out, A


def _kernels_of(plan):
    return ((("" if plan["direct"] else "point_transform" + ("_bf16x3" if plan["Wts"] is not None else "") + " + ")) +
            ("mlp2_max" + ("_bf16x3" if plan["W2s"] is not None else "") if plan["nlayers"] == 2 else
             ("direct_max" if plan["direct"] else "gather_max")))


# Shape A's levels 2 and 3 (hotpath.SHAPE_A): the set-abstraction launches that are resident while the next step samples
SA_BESIDE = {2: dict(N=4096, S=1024, K=32, D=128, widths=[256, 512]), 3: dict(N=1024, S=256, K=32, D=512, widths=[512, 1024])}


@pytest.mark.parametrize("n_fps", [512, 1024, 2048])       # fps_lean_kernel<64, 8>, <256, 4>, <256, 8>
@pytest.mark.parametrize("level", [2, 3])
@pytest.mark.parametrize("bf16x3", [True, False])
def test_fps_beside_one_sa_launch_in_a_guarded_arena(dev, oracle, n_fps, level, bf16x3):
    """tgn_furthestsampling_dense (B = 8, n_fps -> n_fps / 4, FPS_LOCAL_INDEX) on a high-priority stream beside ONE launch_branch of
    Shape A's level-2 / level-3 plan (bf16x3 and fp32 MFMA) on a second stream, the set-abstraction launch first and no dependency
    between the two.  Every operand of both lives in one arena: no byte outside fps_idx / new_xyz / out / A may change (guard bands,
    the FPS input cloud, the weights); fps_idx is the oracle's; new_xyz those rows; out is what the same launch wrote when alone."""
    from toothgroupnetwork_amd import _lib, synth
    B, S_fps = 8, n_fps // 4
    cloud = np.ascontiguousarray(synth.scan_batch(B, n_fps, "arch", 7)[:, :, :3])
    ops = _branch_operands(B=B, seed=100 + level, bf16x3=bf16x3, dev=dev, **SA_BESIDE[level])
    assert not ops["plan"]["direct"] and (ops["plan"]["W2s"] is not None) == bf16x3
    ar = Arena()
    h_idx = ar.add("fps_idx", shape=(B, S_fps), dtype=torch.int32, out=True)      # a guard band, then an output, at the front
    h = _branch_into_arena(ar, ops, "sa.")
    h_cloud = ar.add("fps_cloud", like=T(cloud, dev))
    h_nxyz = ar.add("fps_new_xyz", shape=(B, S_fps, 3), dtype=torch.float32, out=True)   # ... and an output, then a guard band, at the end
    views = ar.build(dev)
    launch, v = _arena_launcher(ops, h, views)
    s_sa, s_fps = torch.cuda.Stream(device=dev, priority=0), torch.cuda.Stream(device=dev, priority=-1)
    L = _lib.lib()

    launch(_lib.stream())                       # alone
    torch.cuda.synchronize()
    ar.check("set-abstraction launch alone")
    alone = v["out"].clone()
    ar.reset_outputs()
    torch.cuda.synchronize()

    want = oracle.farthest_point_sample(cloud, S_fps)
    for rep in range(PAIRS):
        launch(_lib.c_void_p(s_sa.cuda_stream))     # beside FPS: enqueued first, FPS right behind it on the other stream
        _lib.check(L.tgn_furthestsampling_dense(B, n_fps, S_fps, _lib.ptr(views[h_cloud]), None, _lib.ptr(views[h_idx]), _lib.ptr(views[h_nxyz]),
                                                _lib.FPS_LOCAL_INDEX, _lib.c_void_p(s_fps.cuda_stream)), "fps")
        torch.cuda.synchronize()
        what = f"FPS {n_fps} -> {S_fps} beside level {level} {_kernels_of(ops['plan'])}, pair {rep}"
        ar.check(what)
        got = views[h_idx].cpu().numpy()
        assert np.array_equal(got, want), f"{what}: fps_idx != oracle: {_diff(got, want)}"
        assert np.array_equal(views[h_nxyz].cpu().numpy().view(np.uint32), oracle.index_points(cloud, want).view(np.uint32)), what + ": new_xyz"
        assert torch.equal(v["out"], alone), f"{what}: the level's output differs from the same launch alone"
        ar.reset_outputs()
        torch.cuda.synchronize()


# (N, S, K, D, widths): the odd cases of test_gpu_sa_forward_bounds / test_gpu_sa_fused -- rows, queries and widths that are no
# multiple of a tile, K below 32 and between 32 and 64, a single query, one K tile -- for each kernel launch_branch can pick
ALONE_SHAPES = [(700, 50, 7, 13, [20, 36]), (640, 33, 36, 200, [72, 100]), (300, 1, 48, 0, [16, 4]), (900, 77, 17, 61, [100, 260]),
                (400, 20, 32, 40, [16, 48]), (512, 256, 64, 256, [196, 256]), (3000, 1024, 32, 36, [32, 32]),
                (900, 100, 16, 6, [64]), (700, 50, 64, 13, [256]), (500, 60, 7, 61, [100]), (4099, 129, 32, 125, [208])]


def _same_bytes(got, want, what):
    """a run under CANARY against the same run under CANARY_B: a guard value that reached an output, or an element nobody wrote,
    differs between the two"""
    for name in got:
        assert torch.equal(got[name], want[name]), f"{what}: {name} differs between the arena fills {CANARY:#x} and {CANARY_B:#x}"


def _run_alone_in_arena(dev, ops, what):
    by_fill = {}
    for fill in (CANARY, CANARY_B):
        ar = Arena(fill)
        h = _branch_into_arena(ar, ops)
        views = ar.build(dev)
        launch, v = _arena_launcher(ops, h, views)
        from toothgroupnetwork_amd import _lib
        launch(_lib.stream())
        torch.cuda.synchronize()
        ar.check(what)
        out, A = _unguarded(ops)
        assert torch.equal(v["out"], out), what + ": out differs from the unguarded call"
        assert A is None or torch.equal(v["A"], A), what + ": A differs from the unguarded call"
        by_fill[fill] = ar.out_bytes()
    _same_bytes(by_fill[CANARY], by_fill[CANARY_B], what)


# (one-layer plans have no bf16x3 form)
ALONE_CASES = [s + (bf,) for s in ALONE_SHAPES for bf in ((True, False) if len(s[4]) == 2 else (False,))]


@pytest.mark.parametrize("N,S,K,D,widths,bf16x3", ALONE_CASES)
def test_sa_family_writes_only_its_outputs_odd_shapes(dev, N, S, K, D, widths, bf16x3):
    """launch_branch at odd shapes, B = 3, every operand in the arena: tgn_sa_point_transform[_bf16x3], tgn_sa_direct_max,
    tgn_sa_gather_max, tgn_sa_mlp2_max[_bf16x3] (direct and commuted) write `out` and `A` and nothing else, and write there what the
    same call writes into ordinary allocations."""
    ops = _branch_operands(N, S, K, D, widths, 3, N + K + D, bf16x3, dev, xyz_first=bool(N & 1))
    _run_alone_in_arena(dev, ops, f"({N},{S},{K},{D},{widths}) {_kernels_of(ops['plan'])}")


@pytest.mark.parametrize("level", [1, 2, 3])
@pytest.mark.parametrize("bf16x3", [True, False])
def test_sa_family_writes_only_its_outputs_shape_a(dev, level, bf16x3):
    """the same for Shape A's three levels at B = 8 (level 1: the direct two-layer form; levels 2, 3: transform + chained kernel,
    level 3 on the 256 x 256 tile)"""
    from toothgroupnetwork_amd import hotpath
    sh = hotpath.SHAPE_A
    N = sh["n"] if level == 1 else sh["npoint"][level - 2]
    ops = _branch_operands(N, sh["npoint"][level - 1], sh["nsample"][level - 1], sh["d"][level - 1], sh["mlp"][level - 1], 8, 200 + level,
                           bf16x3, dev)
    _run_alone_in_arena(dev, ops, f"Shape A level {level} {_kernels_of(ops['plan'])}")


@pytest.mark.parametrize("M,D,C1", [(4099, 1024, 784), (1000, 61, 100), (300, 13, 208), (129, 0, 16)])
@pytest.mark.parametrize("bf16x3", [True, False])
def test_point_transform_writes_only_A(dev, M, D, C1, bf16x3):
    """tgn_sa_point_transform / _bf16x3 at the odd shapes of test_point_transform_bf16x3_vs_float64 (row counts that are no multiple
    of 128, widths that are no multiple of 128 or 16, D = 0): A in the arena equals sa_point_transform's own allocation."""
    from toothgroupnetwork_amd import _lib, sa_fused as F
    g = torch.Generator().manual_seed(M + D)
    xyz = (torch.rand(1, M, 3, generator=g) * 2 - 1).to(dev)
    pts = torch.randn(1, M, D, generator=g).to(dev) if D else None
    Wt = (torch.randn(D + 3, C1, generator=g) / (D + 3) ** 0.5).to(dev)
    Wts = F.split_point_transform(Wt) if bf16x3 else None
    by_fill = {}
    for fill in (CANARY, CANARY_B):
        ar = Arena(fill)
        hA = ar.add("A", shape=(1, M, C1), dtype=torch.float32, out=True)
        hx, hW = ar.add("xyz", like=xyz), ar.add("Wt", like=Wt)
        hp = ar.add("points", like=pts) if D else None
        hs = ar.add("Wts", like=Wts[0]) if bf16x3 else None
        views = ar.build(dev)
        F._launch_point_transform(M, D, C1, views[hx], views[hp] if D else None, views[hW], (views[hs], Wts[1]) if bf16x3 else None,
                                  views[hA], _lib.stream())
        torch.cuda.synchronize()
        ar.check(f"point transform ({M},{D},{C1}) bf16x3={bf16x3}")
        assert torch.equal(views[hA], F.sa_point_transform(xyz, pts, Wt, Wts))
        by_fill[fill] = ar.out_bytes()
    _same_bytes(by_fill[CANARY], by_fill[CANARY_B], f"point transform ({M},{D},{C1}) bf16x3={bf16x3}")


@pytest.mark.parametrize("N", [33, 65, 257, 1000])
@pytest.mark.parametrize("D,C1,C2", [(6, 64, 128), (125, 100, 260)])
def test_group_all_writes_only_its_outputs(dev, N, D, C1, C2):
    """tgn_sa_all_mlp2_max (direct and commuted first layer; one chunk, a ragged last chunk, many chunks) with its chunk workspace and
    its output in the arena, against sa_all_mlp2_max's own allocations."""
    from toothgroupnetwork_amd import _lib, sa_fused as F
    from toothgroupnetwork_amd._lib import ptr
    torch.manual_seed(N + D)
    B = 3
    xyz, pts = torch.rand(B, N, 3, device=dev), torch.randn(B, N, D, device=dev)
    convs = [torch.nn.Conv2d(3 + D, C1, 1).to(dev), torch.nn.Conv2d(C1, C2, 1).to(dev)]
    bns = [torch.nn.BatchNorm2d(C1).to(dev).eval(), torch.nn.BatchNorm2d(C2).to(dev).eval()]
    with torch.no_grad():
        want = F.sa_all_mlp2_max(xyz, pts, convs, bns)
        plan = F._module_plan(convs, bns, 64, D, True, False)
        L = _lib.lib()
        chunks = int(L.tgn_sa_all_chunks(N))
        A1 = None if plan["direct"] else F.sa_point_transform(xyz, pts, plan["Wt"])
        by_fill = {}
        for fill in (CANARY, CANARY_B):
            ar = Arena(fill)
            h_out = ar.add("out", shape=(B, C2), dtype=torch.float32, out=True)
            h_in = {k: ar.add(k, like=t) for k, t in (("xyz", xyz), ("points", pts), ("b1", plan["b1"]), ("W2f", plan["W2f"]),
                                                      ("b2", plan["b2"]))}
            h_w = ar.add("A1", like=A1) if A1 is not None else ar.add("Wd", like=plan["W1"])
            h_part = ar.add("part", shape=(B, chunks, C2), dtype=torch.float32, out=True) if chunks > 1 else None
            v = ar.build(dev)
            _lib.check(L.tgn_sa_all_mlp2_max(B, N, D, plan["C1p"], C2, ptr(v[h_w]) if A1 is not None else None, ptr(v[h_in["xyz"]]),
                                             ptr(v[h_in["points"]]), None if A1 is not None else ptr(v[h_w]), ptr(v[h_in["b1"]]),
                                             ptr(v[h_in["W2f"]]), ptr(v[h_in["b2"]]), ptr(v[h_part]) if chunks > 1 else None,
                                             ptr(v[h_out]), C2, _lib.stream()), "sa_all_mlp2_max")
            torch.cuda.synchronize()
            ar.check(f"group_all N={N} D={D} [{C1}, {C2}]")
            assert torch.equal(v[h_out], want)
            by_fill[fill] = ar.out_bytes()
    _same_bytes(by_fill[CANARY], by_fill[CANARY_B], f"group_all N={N} D={D} [{C1}, {C2}]")
