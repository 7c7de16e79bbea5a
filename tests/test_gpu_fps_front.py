"""The Python front end of farthest-point sampling (toothgroupnetwork_amd/fps.py): one book and one switch behind the packed
(pointops) and the dense (pointnet2_utils) operators.  Expected indices come from the CPU oracle.  The shapes are the smallest that
reach each branch the front end chooses between: at most 256 points, 257 - 2048 points, and one point above
tgn_fps_resident_capacity() (the workspace branch)."""
import numpy as np
import pytest
import torch

from toothgroupnetwork_amd import synth

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def i32(*values):
    return np.asarray(values, dtype=np.int32)


def _oracle_mode():
    """The oracle's mode bits (bit 0: FMA, bit 1: tree ties) for the process-wide _lib.set_fps_mode() setting."""
    from toothgroupnetwork_amd import _lib
    ties, fma = _lib.get_fps_mode()
    return (2 if ties == "tree" else 0) | (1 if fma else 0)


def _dense_chain(dev, oracle, x, sizes, first_with_coords=True):
    """x (B,N,3) sampled to sizes[0] (coordinates from the kernel, or the reference's index_points idiom), then
    farthest_point_sample of every result to the next size; each level is compared with the oracle.  Returns the index arrays."""
    from toothgroupnetwork_amd import pointnet2_utils as U
    mode, out, cur, ref = _oracle_mode(), [], T(x, dev), x
    for level, S in enumerate(sizes):
        if level == 0 and first_with_coords:
            idx, nxt = U._fps_dense(cur, S, want_coords=True)
        else:
            idx = U.farthest_point_sample(cur, S)
            nxt = U.index_points(cur, idx)
        want = oracle.farthest_point_sample(ref, S, mode=mode)
        assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), want), (level, S)
        ref = oracle.index_points(ref, want)
        assert np.array_equal(nxt.cpu().numpy(), ref), (level, S)
        out.append(want)
        cur = nxt
    return out


def _packed_chain(dev, oracle, clouds, levels, stride=4):
    """The Point-Transformer idiom (blocks.py:62-74): idx = furthestsampling(p, o, n_o); n_p = p[idx]; the next level samples n_p."""
    from toothgroupnetwork_amd import pointops as P
    mode, out = _oracle_mode(), []
    p_np = np.concatenate(clouds).astype(np.float32)
    o_np = np.cumsum([c.shape[0] for c in clouds]).astype(np.int32)
    p, o = T(p_np, dev), T(o_np, dev)
    for level in range(levels):
        n_o_np = np.cumsum(np.diff(np.concatenate([[0], o_np])) // stride).astype(np.int32)
        n_o = T(n_o_np, dev)
        idx = P.furthestsampling(p, o, n_o)
        want = oracle.furthestsampling(p_np, o_np, n_o_np, mode=mode)
        assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), want), level
        p, o, p_np, o_np = p[idx.long(), :], n_o, p_np[want.astype(np.int64)], n_o_np       # the model's own gather: a new tensor
        out.append(want)
    return out


def _packed_then_dense(dev, oracle, cloud):
    from toothgroupnetwork_amd import pointnet2_utils as U, pointops as P
    idx, n_p = P.fps_with_coords(T(cloud, dev), T(i32(600), dev), T(i32(150), dev))
    want = oracle.furthestsampling(cloud, i32(600), i32(150))
    assert np.array_equal(idx.cpu().numpy(), want) and np.array_equal(n_p.cpu().numpy(), cloud[want])
    got = U.farthest_point_sample(n_p[None], 40)
    want2 = oracle.farthest_point_sample(cloud[want][None], 40)
    assert np.array_equal(got.cpu().numpy(), want2)
    return [want, want2]


def _dense_then_packed(dev, oracle, cloud):
    from toothgroupnetwork_amd import pointnet2_utils as U, pointops as P
    idx, nx = U._fps_dense(T(cloud[None], dev), 150, want_coords=True)
    want = oracle.farthest_point_sample(cloud[None], 150)
    assert np.array_equal(idx.cpu().numpy(), want) and np.array_equal(nx.cpu().numpy()[0], cloud[want[0]])
    got = P.furthestsampling(nx[0], T(i32(150), dev), T(i32(40), dev))
    want2 = oracle.furthestsampling(cloud[want[0]], i32(150), i32(40))
    assert np.array_equal(got.cpu().numpy(), want2)
    return [want, want2]


def test_one_book_serves_both_layouts_and_never_crosses_them(dev, oracle):
    """With the switch forced on, a dense chain and a packed chain are offered their own earlier results out of the ONE book; a
    packed result is never offered to a dense call on the same points, nor a dense result to a packed call.  The offered counts are
    cumulative.  Every index is the oracle's and the one the same sequence gives with the switch forced off.

    The book is cleared in front of the last step: the step before it leaves a PACKED result with one segment of 150 points behind,
    which the packed call of the last step would rightly be offered (same layout) -- the count is to show the dense one is not."""
    from toothgroupnetwork_amd import config, fps
    dense = np.stack([synth.uniform_cloud(600, 31), synth.uniform_cloud(600, 32)])
    clouds = [synth.uniform_cloud(500, 33), synth.uniform_cloud(37, 34), synth.uniform_cloud(300, 35)]
    single_a, single_b = synth.uniform_cloud(600, 36), synth.uniform_cloud(600, 37)

    def sequence(offered):
        fps.clear()
        fps.stats["offered"] = 0
        got = _dense_chain(dev, oracle, dense, (150, 40))
        assert np.array_equal(got[1], np.tile(np.arange(40), (2, 1)))
        assert fps.stats["offered"] == offered[0]
        got += _packed_chain(dev, oracle, clouds, levels=3)
        assert fps.stats["offered"] == offered[1]
        got += _packed_then_dense(dev, oracle, single_a)
        assert fps.stats["offered"] == offered[2]
        fps.clear()
        got += _dense_then_packed(dev, oracle, single_b)
        assert fps.stats["offered"] == offered[3]
        return got

    with config.override(fps_prefix=True):
        fast = sequence((1, 3, 3, 3))
    with config.override(fps_prefix=False):
        plain = sequence((0, 0, 0, 0))
    fps.clear()
    assert len(fast) == len(plain) == 9
    for a, b in zip(fast, plain):
        assert np.array_equal(a, b)


def test_workspace_branch_in_both_layouts_with_the_shortcut_on(dev, oracle):
    """one cloud of one point more than the register-resident kernels hold, sampled to 8 out of the workspace; the 8 samples
    sampled to 4 are offered that result and give 0..3"""
    from toothgroupnetwork_amd import _lib, config, fps, pointnet2_utils as U, pointops as P
    n = int(_lib.ops().tgn_fps_resident_capacity()) + 1
    cloud = synth.arch_cloud(n, 41, False)
    assert fps.workspace(1, n - 1, n - 1, dev)[1] == 0 and fps.workspace(1, n, n, dev)[1] > 0
    want = oracle.farthest_point_sample(cloud[None], 8)
    with config.override(fps_prefix=True):
        fps.clear()
        fps.stats["offered"] = 0
        idx, nx = U._fps_dense(T(cloud[None], dev), 8, want_coords=True)
        assert np.array_equal(idx.cpu().numpy(), want) and np.array_equal(nx.cpu().numpy()[0], cloud[want[0]])
        assert torch.equal(U.farthest_point_sample(nx, 4), torch.arange(4, device=dev)[None])
        assert fps.stats["offered"] == 1
        idx, n_p = P.fps_with_coords(T(cloud, dev), T(i32(n), dev), T(i32(8), dev))
        assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(n_p.cpu().numpy(), cloud[want[0]])
        assert torch.equal(P.furthestsampling(n_p, T(i32(8), dev), T(i32(4), dev)), torch.arange(4, dtype=torch.int32, device=dev))
        assert fps.stats["offered"] == 2
    fps.clear()


def test_clear_and_adopt_reach_both_layouts(dev, oracle):
    """pointops' clear drops a dense result and pointnet2_utils' a packed one; pointops' adopt carries a dense result from the
    stream that made it to a stream that waited for it"""
    from toothgroupnetwork_amd import config, fps, pointnet2_utils as U, pointops as P
    cloud = synth.uniform_cloud(600, 51)
    x = T(cloud[None], dev)
    want = oracle.farthest_point_sample(cloud[None], 150)
    want2 = oracle.farthest_point_sample(cloud[want[0]][None], 40)
    assert np.array_equal(want2[0], np.arange(40))
    with config.override(fps_prefix=True):
        fps.clear()
        fps.stats["offered"] = 0
        _, nx = U._fps_dense(x, 150, want_coords=True)
        P.fps_prefix_clear()
        assert np.array_equal(U.farthest_point_sample(nx, 40).cpu().numpy(), want2) and fps.stats["offered"] == 0
        _, n_p = P.fps_with_coords(x[0], T(i32(600), dev), T(i32(150), dev))
        U.fps_prefix_clear()
        got = P.furthestsampling(n_p, T(i32(150), dev), T(i32(40), dev))
        assert np.array_equal(got.cpu().numpy(), want2[0]) and fps.stats["offered"] == 0
        fps.clear()
        s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        s1.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s1):
            idx, nx = U._fps_dense(x, 150, want_coords=True)
        s2.wait_stream(s1)
        nx.record_stream(s2)
        with torch.cuda.stream(s2):
            alone = U.farthest_point_sample(nx, 40)
        assert fps.stats["offered"] == 0                       # recorded on s1: not offered on s2 ...
        s2.wait_stream(s1)
        P.fps_prefix_adopt(s1, s2)
        with torch.cuda.stream(s2):
            adopted = U.farthest_point_sample(nx, 40)
        assert fps.stats["offered"] == 1                       # ... until s2 has adopted what s1 recorded
        torch.cuda.synchronize(dev)
        assert np.array_equal(idx.cpu().numpy(), want)
        assert np.array_equal(alone.cpu().numpy(), want2) and np.array_equal(adopted.cpu().numpy(), want2)
    fps.clear()


def test_tree_ties_never_take_part_through_the_front_end(dev, oracle):
    """lattice points (many equal distances) under the tree tie order: with the switch forced on no call is offered anything, and the
    chains are what the oracle samples in its tree-tie mode -- where FPS of an FPS result is not the identity"""
    from toothgroupnetwork_amd import _lib, config, fps
    rng = np.random.default_rng(0)
    lattice = [(rng.integers(-6, 7, size=(n, 3)) / 8).astype(np.float32) for n in (600, 500, 37, 300)]
    prev = _lib.set_fps_mode(ties="tree")
    try:
        assert _oracle_mode() & 2
        with config.override(fps_prefix=True):
            fps.clear()
            fps.stats["offered"] = 0
            _dense_chain(dev, oracle, lattice[0][None], (150, 40))
            _dense_chain(dev, oracle, lattice[0][None], (150, 40), first_with_coords=False)
            _packed_chain(dev, oracle, lattice[1:], levels=3)
            assert fps.stats["offered"] == 0 and fps.book.entries == []
    finally:
        _lib.set_fps_mode(ties=prev[0], fma=prev[1])
        fps.clear()
