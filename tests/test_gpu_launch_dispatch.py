"""GPU: the instantiations a launcher picks from run-time values (csrc/dispatch.h) that the other tests reach with one index width
only.  Every case launches with int32 and with int64 indices and wants the same bytes from both; one of the two is then held to
the reference and the bound of the family's own test:

* tgn_sa_direct_max, every (k-step count, column-tile count): the float64 layer of oracle/cpu.py, elementwise 1e-5 * (1 + |want|)
  (test_gpu_sa_fused.py);
* tgn_group_points_ex with int64 indices, every kernel: the oracle's bytes (test_gpu_parity.py);
* tgn_ball_query, every bitmap size of the chunk kernel and the rank-select kernel: the oracle's rows;
* tgn_three_nn, tgn_gather_points: the oracle's bytes; tgn_scatter_add_points: float64, 8 u sum|terms| (test_gpu_training_backward.py);
* tgn_three_interpolate: the oracle within 1e-5 (tests/golden/make_golden.py), and byte for byte tgn_three_interpolate_ex without an
  epilogue, the weights included.
"""
import numpy as np
import pytest
import torch

from test_gpu_sa_fused import _layer, close
from test_gpu_training_backward import _within

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("C1", [32, 64, 96, 128, 160, 192, 224, 256])      # NT = 1 .. 8 column tiles
@pytest.mark.parametrize("D", [0, 3, 13])                                  # KS = 2, 5, 8 k-steps
def test_sa_direct_max_every_instantiation_both_index_widths(dev, oracle, D, C1):
    from toothgroupnetwork_amd import _lib, pointnet2_utils as U
    B, N, S, K = 2, 96, 8, 8
    assert _lib.lib().tgn_sa_direct_supported(K, D, C1) == 1
    rng = np.random.default_rng(100 * D + C1)
    xyz = rng.normal(size=(B, N, 3)).astype(np.float32)
    feat = rng.normal(size=(B, N, D)).astype(np.float32) if D else None
    new_xyz = np.ascontiguousarray(xyz[:, :S])
    idx = rng.integers(0, N, size=(B, S, K))
    conv, bn = _layer(dev, D, C1, 7, True)
    tx, tn, tf, ti = T(xyz, dev), T(new_xyz, dev), (T(feat, dev) if D else None), T(idx, dev)
    with torch.no_grad():
        got64 = U.sa_level_max(tx, tn, tf, ti, conv, bn, True)
        got32 = U.sa_level_max(tx, tn, tf, ti.to(torch.int32), conv, bn, True)
    assert torch.equal(got32, got64)
    want = oracle.set_abstraction_first_layer(xyz, new_xyz, feat, idx, conv.weight.detach().reshape(C1, -1).cpu().numpy(),
                                              conv.bias.detach().cpu().numpy(), bn.weight.detach().cpu().numpy(),
                                              bn.bias.detach().cpu().numpy(), bn.running_mean.cpu().numpy(), bn.running_var.cpu().numpy(),
                                              bn.eps, True, reduce_max=True)
    close(got64.cpu().numpy(), want, f"direct level D={D} C1={C1}")


# (impl, policy, K, D): pairs (rows of 9 floats, S*K a multiple of 64); row pieces with 16-byte and with 4-byte LDS-DMA pieces
# (C >= 64, K = 8, D a multiple of 4 or not); staged 16-byte stores with narrow and with wide rows; K*C no multiple of 4, which only
# the per-element kernel takes (asked for as 2 and as 1)
@pytest.mark.parametrize("impl,policy,K,D", [(10, -1, 8, 6), (10, 0, 8, 6), (10, 16, 8, 6), (7, -1, 8, 64), (7, 0, 8, 64), (7, 16, 8, 64),
                                             (7, -1, 8, 61), (2, 17, 8, 5), (2, -1, 8, 61), (2, -1, 5, 4), (1, -1, 5, 4)])
def test_group_points_ex_int64_indices_every_kernel(dev, oracle, impl, policy, K, D):
    from toothgroupnetwork_amd import _lib
    B, N, S = 2, 256, 64
    rng = np.random.default_rng(impl * 1000 + K + D)
    xyz = rng.normal(size=(B, N, 3)).astype(np.float32)
    pts = rng.normal(size=(B, N, D)).astype(np.float32)
    new_xyz = np.ascontiguousarray(xyz[:, :S])
    idx = rng.integers(0, N, size=(B, S, K))
    want = oracle.group_points(xyz, new_xyz, pts, idx, True)
    L = _lib.lib()
    tx, tn, tp = T(xyz, dev), T(new_xyz, dev), T(pts, dev)
    got = {}
    for dt in (torch.int64, torch.int32):
        ti = T(idx, dev).to(dt)
        out = torch.full((B, S, K, 3 + D), float("nan"), device=dev)
        _lib.check(L.tgn_group_points_ex(B, N, S, K, D, _lib.ptr(tx), _lib.ptr(tn), _lib.ptr(tp), _lib.ptr(ti), int(dt == torch.int64), 1,
                                         _lib.ptr(out), impl, policy, 0, _lib.stream()))
        got[dt] = out
    assert torch.equal(got[torch.int32].view(torch.int32), got[torch.int64].view(torch.int32))
    assert np.array_equal(got[torch.int64].cpu().numpy(), want), (impl, policy)
    assert L.tgn_take_index_error(_lib.stream()) == 0


@pytest.mark.parametrize("variant", [2, 0])                                  # chunk kernel (a bitmap of 1 .. 4 quads per lane), rank-select
@pytest.mark.parametrize("N,S,radius", [(4096, 37, 0.1), (9000, 100, 0.08), (20000, 64, 0.06), (32768, 130, 0.05)])
def test_ball_query_every_bitmap_size_both_index_widths(dev, oracle, variant, N, S, radius):
    from toothgroupnetwork_amd import _lib, synth
    B, K = 1, 16
    L = _lib.lib()
    xyz = synth.arch_cloud(N, 40, False)[None]
    q = np.ascontiguousarray(xyz[:, :: N // S][:, :S])
    assert q.shape[1] == S
    tx, tq = T(xyz, dev), T(q, dev)
    r2 = float(torch.tensor(radius ** 2, dtype=torch.float32).item())
    nbytes = int(L.tgn_ball_query_workspace_bytes(B, N, S))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    got = {}
    with _lib.tuning(ball_bitmap=variant):
        for dt in (torch.int64, torch.int32):
            out = torch.full((B, S, K), -7, dtype=dt, device=dev)
            _lib.check(L.tgn_ball_query(B, N, S, K, r2, _lib.ptr(tx), _lib.ptr(tq), _lib.ptr(out), int(dt == torch.int64), _lib.ptr(ws),
                                        nbytes, _lib.stream()), "tgn_ball_query")
            got[dt] = out
    assert torch.equal(got[torch.int32].long(), got[torch.int64])
    assert np.array_equal(got[torch.int64].cpu().numpy(), oracle.query_ball_point(radius, K, xyz, q))


def test_three_nn_both_index_widths(dev, oracle):
    from toothgroupnetwork_amd import _lib
    B, N, S = 1, 70, 17
    rng = np.random.default_rng(B * 1000 + S)
    xyz2 = (rng.integers(-4, 5, size=(B, S, 3)) * 0.125).astype(np.float32)          # coarse lattice: ties and duplicates
    xyz1 = (rng.integers(-8, 9, size=(B, N, 3)) * 0.0625).astype(np.float32)
    t1, t2 = T(xyz1, dev), T(xyz2, dev)
    got = {}
    for dt in (torch.int64, torch.int32):
        dist = torch.full((B, N, 3), float("nan"), device=dev)
        idx = torch.full((B, N, 3), -7, dtype=dt, device=dev)
        _lib.check(_lib.lib().tgn_three_nn(B, N, S, _lib.ptr(t1), _lib.ptr(t2), _lib.ptr(dist), _lib.ptr(idx), int(dt == torch.int64),
                                           _lib.stream()), "three_nn")
        got[dt] = (dist, idx)
    assert torch.equal(got[torch.int32][0].view(torch.int32), got[torch.int64][0].view(torch.int32))
    assert torch.equal(got[torch.int32][1].long(), got[torch.int64][1])
    od, oi = oracle.three_nn(xyz1, xyz2)
    assert np.array_equal(got[torch.int64][0].cpu().numpy(), od) and np.array_equal(got[torch.int64][1].cpu().numpy(), oi)


def test_gather_and_scatter_add_points_both_index_widths(dev, oracle):
    """Every target row receives at most two contributions, whose fp32 sum does not depend on their order: the atomic scatter is
    reproducible and the two launches can be compared byte for byte.  A third of the indices are negative (they wrap)."""
    from toothgroupnetwork_amd import _lib, pointnet2_utils as U
    B, N, M, C = 2, 50, 9, 5
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(B, N, C)).astype(np.float32)
    idx = np.stack([rng.permutation(N)[:M] for _ in range(B)])
    idx[:, 7:] = idx[:, :2]                                                    # two rows hit twice
    wrapped = np.where(rng.random((B, M)) < 0.33, idx - N, idx)
    go = rng.normal(size=(B, M, C)).astype(np.float32)
    out, grad = {}, {}
    for dt in (torch.int64, torch.int32):
        p = T(pts, dev).requires_grad_(True)
        out[dt] = U.index_points(p, T(wrapped, dev).to(dt))
        out[dt].backward(T(go, dev))
        grad[dt] = p.grad
    assert torch.equal(out[torch.int32].detach().view(torch.int32), out[torch.int64].detach().view(torch.int32))
    assert torch.equal(grad[torch.int32].view(torch.int32), grad[torch.int64].view(torch.int32))
    assert np.array_equal(out[torch.int64].detach().cpu().numpy(), oracle.index_points(pts, idx))
    flat = torch.from_numpy((idx + np.arange(B)[:, None] * N).reshape(-1))
    g64 = torch.from_numpy(go).double().reshape(-1, C)
    exact = torch.zeros(B * N, C, dtype=torch.float64).index_add_(0, flat, g64).view(B, N, C)
    ab = torch.zeros(B * N, C, dtype=torch.float64).index_add_(0, flat, g64.abs()).view(B, N, C)
    _within(grad[torch.int64].cpu(), exact, ab, "d_points")


@pytest.mark.parametrize("C", [5, 8])                                       # dword lanes, 16-byte lanes
def test_three_interpolate_is_the_fused_form_without_an_epilogue(dev, oracle, C):
    from toothgroupnetwork_amd import _lib, pointnet2_utils as U
    B, N, S = 2, 40, 6
    rng = np.random.default_rng(C)
    xyz1 = rng.normal(size=(B, N, 3)).astype(np.float32)
    xyz2 = rng.normal(size=(B, S, 3)).astype(np.float32)
    f2 = rng.normal(size=(B, S, C)).astype(np.float32)
    dist, idx = U.three_nn(T(xyz1, dev), T(xyz2, dev))
    tf = T(f2, dev)
    L = _lib.lib()
    got = {}
    for dt in (torch.int64, torch.int32):
        ti = idx.to(dt)
        for ex in (False, True):
            out = torch.full((B, N, C), float("nan"), device=dev)
            w = torch.full((B, N, 3), float("nan"), device=dev)
            if ex:
                rc = L.tgn_three_interpolate_ex(B, N, S, C, _lib.ptr(tf), _lib.ptr(dist), _lib.ptr(ti), int(dt == torch.int64), None, 0,
                                                _lib.ptr(out), _lib.ptr(w), _lib.stream())
            else:
                rc = L.tgn_three_interpolate(B, N, S, C, _lib.ptr(tf), _lib.ptr(dist), _lib.ptr(ti), int(dt == torch.int64), _lib.ptr(out),
                                             _lib.ptr(w), _lib.stream())
            _lib.check(rc, "three_interpolate")
            got[dt, ex] = (out, w)
    first = got[torch.int64, False]
    for key, (out, w) in got.items():
        assert torch.equal(out.view(torch.int32), first[0].view(torch.int32)), key
        assert torch.equal(w.view(torch.int32), first[1].view(torch.int32)), key
    assert torch.equal(U.three_interpolate(tf, dist, idx), first[0])
    np.testing.assert_allclose(first[0].cpu().numpy(), oracle.three_interpolate(f2, dist.cpu().numpy(), idx.cpu().numpy()), rtol=0, atol=1e-5)
