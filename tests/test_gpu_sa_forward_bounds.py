"""GPU: the fused set-abstraction forward kernels (csrc/sa.hip, csrc/sa_mlp.hip) held to a float64 error bound scaled by their terms.

The kernels do not compute what the reference computes: they fold BatchNorm into the weights (sa_fused.pack_first_layer /
pack_second_layer), commute the first layer for wide inputs (A1 = [f, x] . W1t per point, cst = b - Wxs . centre per query) and by
default run the commuted first layer and the second layer as six bf16 MFMAs per fp32 product (bf16x3).  Each test restates the
algorithm the kernel documents in float64 and returns, for every output, the value `want` and the magnitude M, the sum of the absolute
values of the terms that algorithm adds:
  folded bias         |beta| + |s mu| + |s bias|,  s = gamma / sqrt(var + eps), W' = s W
  first layer         M1 = sum_j |W'[c,j]| |row_j| + |b' terms|; commuted form: row = [f, x] of the POINT plus sum_a |Wx'[c,a]| |centre_a|
                      (cancelling the centre term is part of that algorithm); direct form (3 + D <= 16): row = [x - c, f]
  second layer        M2 = sum_j |W2'[c,j]| (|h1_j| + M1_j) + |b2' terms|   (layer 1's bound through the 1-Lipschitz ReLU)
  max over neighbours M_out = max_k M2 (also for the max over a whole cloud), |max a - max b| <= max |a - b|
and asserts |got - want| <= C u M elementwise, u = 2^-24.

The constant.  C = 8 max(1, sqrt(n / 16)), n the length of the longest fp32 accumulation chain an output goes through: 3 + D + 4 for a
first layer (the row, the centre's three terms and the bias), C1p for a second layer.  8 u M covers the fold (s = gamma / sqrt(var + eps)
and W s: 3.5 u per weight, 5 u on the folded bias, both times their own terms) and a chain of up to 16 fp32 additions.  Each addition of
a chain rounds by at most u times a partial sum no larger than M; the roundings are independent, so a chain of n of them grows like
sqrt(n) (a standard deviation below u M sqrt(n / 3)), which 8 sqrt(n / 16) = 2 sqrt(n) bounds with room.  (The worst case is n u M;
no kernel comes near it, and the tests print the worst ratio |got - want| / (u M) of every case.)

bf16x3 against fp32-MFMA.  Dropping one of the six products costs a few hundred u per TERM, which averages down to a few u of M over a
long chain and can hide under C u M.  So the bf16x3 result's max and rms of |got - want| / M must also stay within 2x those of the
fp32-MFMA form on the same inputs (with a floor of one final rounding, u for the max and u / sqrt(3) for the rms: an exact result
stored in fp32 is that far off).

Exact outputs.  Where every pre-activation of an output lies below -C u M the output is exactly 0; a max does not see duplicated
neighbours (ball-query rows padded with their first index give the same bits as rows padded with another member of the ball)."""
import math

import numpy as np
import pytest
import torch

from test_gpu_sa_fused import MLP2_SHAPES

pytestmark = pytest.mark.gpu

U_RND = 2.0 ** -24


def chain_const(n):
    """C for an output whose longest fp32 accumulation chain has n additions (module docstring)."""
    return 8.0 * max(1.0, math.sqrt(n / 16.0))


# ------------------------------------------------------------------------------------------------------------------------------
# float64 restatement: (value, magnitude)
# ------------------------------------------------------------------------------------------------------------------------------
def fold64(conv, bn=None):
    """(W' (C_out, C_in), b', |b' terms|) of Conv2d(1x1) + eval-mode BatchNorm2d in float64; bn None: the convolution alone."""
    C = conv.out_channels
    W = conv.weight.detach().double().reshape(C, -1)
    bias = conv.bias.detach().double() if conv.bias is not None else torch.zeros_like(W[:, 0])
    if bn is None:
        return W, bias, bias.abs()
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    mu, beta = bn.running_mean.double(), bn.bias.detach().double()
    return W * s[:, None], beta - s * mu + s * bias, beta.abs() + (s * mu).abs() + (s * bias).abs()


def plain64(W, b, dev):
    """A layer without BatchNorm (HotPath's identity-folded levels) from numpy (W (C_out, C_in), b)."""
    W = torch.as_tensor(np.asarray(W), dtype=torch.float64, device=dev)
    b = torch.as_tensor(np.asarray(b), dtype=torch.float64, device=dev)
    return W, b, b.abs()


def _gather(t, idx):
    """t (B, N, C), idx (B, S, K) -> (B, S, K, C)"""
    bi = torch.arange(t.shape[0], device=t.device)[:, None, None]
    return t[bi, idx.long()]


def first_layer64(xyz, new_xyz, points, idx, layer, xyz_first, commuted):
    """Pre-activation and M1 of a first layer over the grouped rows, (B, S, K, C1) each.  new_xyz None: group-all (raw rows)."""
    W, b, Mb = layer
    D = 0 if points is None else points.shape[-1]
    Wx, Wp = (W[:, :3], W[:, 3:]) if xyz_first else (W[:, D:], W[:, :D])
    gx = _gather(xyz.double(), idx)
    c = new_xyz.double()[:, :, None, :] if new_xyz is not None else torch.zeros_like(gx[:, :, :1])
    rel = gx - c                                   # exact: both are fp32
    pre = rel @ Wx.t() + b
    mag = Mb.expand_as(pre).clone()
    if D:
        f = points.double()
        pre += _gather(f @ Wp.t(), idx)
        mag += _gather(f.abs() @ Wp.abs().t(), idx)
    if commuted:
        mag += gx.abs() @ Wx.abs().t() + c.abs() @ Wx.abs().t()
    else:
        mag += rel.abs() @ Wx.abs().t()
    return pre, mag


def next_layer64(pre, mag, layer):
    W, b, Mb = layer
    h = pre.clamp_min(0.0)
    return h @ W.t() + b, (h.abs() + mag) @ W.abs().t() + Mb


def reduce_max64(pre, mag):
    """(want, M_out, largest pre-activation) over the neighbour axis 2"""
    return pre.clamp_min(0.0).amax(2), mag.amax(2), pre.amax(2)


def check_bound(got, want, M, C, what, premax=None):
    """|got - want| <= C u M elementwise; outputs whose pre-activations all lie below -C u M are exactly 0.
    Returns |got - want| / M (for the bf16x3 / fp32-MFMA comparison) and prints the worst ratio to u M."""
    got = got.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got - want).abs()
    rel = torch.where(M > 0, err / M.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = rel / U_RND
    worst = int(torch.argmax(ratio)) if ratio.numel() else 0
    w = float(ratio.flatten()[worst]) if ratio.numel() else 0.0
    zeros = ""
    if premax is not None:
        dead = premax < -C * U_RND * M
        nz = int((got[dead] != 0).sum())
        assert nz == 0, f"{what}: {nz} outputs with every pre-activation negative are not exactly 0"
        zeros = f", {int(dead.sum())} exact zeros"
    print(f"\n{what}: worst |got - want| / (u M) = {w:.3f} (bound {C:.1f}){zeros}")
    assert w <= C, (f"{what}: |got - want| = {float(err.flatten()[worst]):.3e} is {w:.2f} u M > {C:.1f} u M "
                    f"(got {float(got.flatten()[worst])!r}, want {float(want.flatten()[worst])!r}, M {float(M.flatten()[worst]):.3e})")
    return rel


def compare_split(rel_split, rel_exact, what):
    """bf16x3 may not be more than 2x worse than the fp32-MFMA form, in max and in rms of |got - want| / M."""
    mx_s, mx_e = float(rel_split.max()), float(rel_exact.max())
    rms_s, rms_e = float(rel_split.square().mean().sqrt()), float(rel_exact.square().mean().sqrt())
    print(f"\n{what}: max {mx_s / U_RND:.3f} u vs fp32-MFMA {mx_e / U_RND:.3f} u, rms {rms_s / U_RND:.4f} u vs {rms_e / U_RND:.4f} u")
    assert mx_s <= 2.0 * max(mx_e, U_RND), f"{what}: bf16x3 max {mx_s / U_RND:.3f} u > 2 x fp32-MFMA max {mx_e / U_RND:.3f} u"
    assert rms_s <= 2.0 * max(rms_e, U_RND / math.sqrt(3.0)), \
        f"{what}: bf16x3 rms {rms_s / U_RND:.4f} u > 2 x fp32-MFMA rms {rms_e / U_RND:.4f} u"


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
OFFSET = (7.0, -5.0, 5.0)      # |offset| ~ 9.9: centres about 10 from the origin

REGIMES = ["tiny", "feat1e3", "cancel", "offorigin", "dups", "negative", "pad"]


def make_cloud(B, N, D, seed, regime):
    """(xyz (B,N,3), feat (B,N,D) or None, radius) as numpy float32"""
    from toothgroupnetwork_amd import synth
    rng = np.random.default_rng(seed)
    xyz = np.ascontiguousarray(synth.scan_batch(B, N, "arch", seed=seed % 97)[:, :, :3])
    feat = rng.normal(size=(B, N, D)).astype(np.float32) if D else None
    if regime == "offorigin":
        xyz = (xyz + np.asarray(OFFSET, np.float32)).astype(np.float32)
    if regime == "feat1e3" and D:
        feat = (feat * 1e3).astype(np.float32)
    if regime == "dups":        # every vertex twice: coincident points in every ball
        src = rng.permutation(np.repeat(np.arange((N + 1) // 2), 2)[:N])
        xyz = np.ascontiguousarray(xyz[:, src])
        feat = None if feat is None else np.ascontiguousarray(feat[:, src])
    radius = 0.02 if regime == "pad" else 0.3
    return xyz, feat, radius


def make_layer(dev, c_in, c_out, seed):
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(c_in, c_out, 1).to(dev)
    bn = torch.nn.BatchNorm2d(c_out).to(dev).eval()
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.3)
        bn.running_var.uniform_(0.4, 2.0)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.2)
    return conv, bn


def apply_regime(regime, convs, bns):
    """Per-regime changes of the layers that need no data (`cancel` is data-dependent: centre_means)."""
    with torch.no_grad():
        if regime == "tiny":            # outputs of about 1e-3 .. 1e-4: a large running_var, then a small gamma
            if len(bns) == 1:
                bns[0].weight.mul_(1e-3)
                bns[0].bias.mul_(1e-3)
            else:
                bns[0].running_var.mul_(1e4)
                bns[0].bias.mul_(1e-2)
                bns[1].weight.mul_(1e-1)
                bns[1].bias.mul_(1e-3)
        if regime == "negative":        # whole channels with every pre-activation negative, in every layer
            for bn in bns:
                bn.bias[1::4] = -50.0


def centre_means(pres, bns):
    """`cancel`: each BatchNorm's running mean := the median of its convolution's output over the rows, so that many pre-activations
    are near zero through cancellation.  pres: callables giving layer l's convolution output (rows, C) once layers < l are set."""
    with torch.no_grad():
        for pre, bn in zip(pres, bns):
            bn.running_mean.copy_(pre().reshape(-1, bn.num_features).median(0).values.float())


def T(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _fps_ball(U, tx, S, radius, K):
    new_xyz = U.index_points(tx, U.farthest_point_sample(tx, S))
    return new_xyz, U.query_ball_point(radius, K, tx, new_xyz)


def repad(idx):
    """The same neighbour SETS with the padding changed: ball-query rows are padded with their first index; pad with the last
    found neighbour instead (rows without padding are unchanged)."""
    i = idx.long()
    pad = torch.zeros_like(i, dtype=torch.bool)
    pad[..., 1:] = i[..., 1:] == i[..., :1]
    cnt = (~pad).sum(-1, keepdim=True)
    last = torch.gather(i, -1, cnt - 1)
    return torch.where(pad, last, i).to(idx.dtype), int(pad.sum())


# ------------------------------------------------------------------------------------------------------------------------------
# sa_point_transform: A = [points, xyz] @ Wt, fp32 MFMA and bf16x3
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D,C1", [(6000, 256, 256), (4099, 1024, 784), (1000, 61, 100), (300, 13, 208), (129, 0, 16), (2048, 128, 272)])
@pytest.mark.parametrize("regime", ["plain", "feat1e3", "offorigin"])
def test_point_transform_bound(dev, M, D, C1, regime):
    from toothgroupnetwork_amd import pointnet2_utils as U
    g = torch.Generator().manual_seed(M + D + C1)
    xyz = torch.rand(1, M, 3, generator=g) * 2 - 1
    if regime == "offorigin":
        xyz = xyz + torch.tensor(OFFSET)
    pts = torch.randn(1, M, D, generator=g) * (1e3 if regime == "feat1e3" else 1.0) if D else None
    Wt = torch.randn(D + 3, C1, generator=g) / (D + 3) ** 0.5
    xyz, pts, Wt = xyz.to(dev), (pts.to(dev) if D else None), Wt.to(dev)
    rows = xyz[0] if pts is None else torch.cat([pts[0], xyz[0]], 1)
    want = rows.double() @ Wt.double()
    mag = rows.double().abs() @ Wt.double().abs()
    C = chain_const(D + 3)
    exact = U.sa_point_transform(xyz, pts, Wt)[0]
    split = U.sa_point_transform(xyz, pts, Wt, U.split_point_transform(Wt))[0]
    what = f"point transform ({M},{D},{C1}) {regime}"
    r_exact = check_bound(exact, want, mag, C, what + " fp32-MFMA")
    r_split = check_bound(split, want, mag, C, what + " bf16x3")
    compare_split(r_split, r_exact, what)


# ------------------------------------------------------------------------------------------------------------------------------
# one-layer levels: sa_level_max (direct or transform + gather-max) and sa_first_layer (transform + gather-act)
# ------------------------------------------------------------------------------------------------------------------------------
ONE_LAYER_SHAPES = [(4096, 1024, 32, 128, 512), (6000, 1024, 32, 6, 128), (900, 100, 16, 6, 64), (700, 50, 64, 13, 256),
                    (500, 60, 7, 61, 100), (800, 90, 48, 0, 32), (640, 33, 36, 200, 784)]


def _one_layer_case(dev, N, S, K, D, C1, xyz_first, regime, idx_dtype):
    from toothgroupnetwork_amd import pointnet2_utils as U, _lib
    B = 2
    xyz, feat, radius = make_cloud(B, N, D, N + K + D, regime)
    tx, tf = T(xyz, dev), T(feat, dev)
    new_xyz, idx = _fps_ball(U, tx, S, radius, K)
    idx = idx.to(idx_dtype)
    conv, bn = make_layer(dev, 3 + D, C1, 7)
    apply_regime(regime, [conv], [bn])
    if regime == "cancel":
        centre_means([lambda: first_layer64(tx, new_xyz, tf, idx, fold64(conv), xyz_first, True)[0]], [bn])
    direct = bool(_lib.lib().tgn_sa_direct_supported(K, D, C1))
    layer = fold64(conv, bn)
    C = chain_const(3 + D + 4)
    tag = f"({N},{S},{K},{D},{C1}) xyz_first={xyz_first} {regime} {str(idx_dtype)[6:]}"
    with torch.no_grad():
        pre, mag = first_layer64(tx, new_xyz, tf, idx, layer, xyz_first, commuted=not direct)
        want, M, premax = reduce_max64(pre, mag)
        for reduce in (False, True):
            got = U.sa_first_layer(tx, new_xyz, tf, idx, conv, bn, xyz_first, reduce_max=reduce)
            if reduce:
                check_bound(got, want, M, C, f"sa_first_layer(reduce_max) {'direct' if direct else 'gather-max'} {tag}", premax)
            elif K <= 64 and C1 % 4 == 0:
                pre_c, mag_c = (pre, mag) if not direct else first_layer64(tx, new_xyz, tf, idx, layer, xyz_first, commuted=True)
                check_bound(got, pre_c.clamp_min(0.0), mag_c, C, f"sa_first_layer gather-act {tag}", pre_c)
        got = U.sa_level_max(tx, new_xyz, tf, idx, conv, bn, xyz_first)
        check_bound(got, want, M, C, f"sa_level_max {'direct' if direct else 'gather-max'} {tag}", premax)
        idx2, npad = repad(idx)
        if npad:
            assert torch.equal(U.sa_level_max(tx, new_xyz, tf, idx2, conv, bn, xyz_first), got), "a duplicated neighbour changed a max"
    return premax


@pytest.mark.parametrize("N,S,K,D,C1", ONE_LAYER_SHAPES)
@pytest.mark.parametrize("xyz_first", [True, False])
def test_one_layer_levels_bound(dev, N, S, K, D, C1, xyz_first):
    _one_layer_case(dev, N, S, K, D, C1, xyz_first, "plain", torch.int64 if xyz_first else torch.int32)


@pytest.mark.parametrize("N,S,K,D,C1", [(6000, 1024, 32, 6, 128), (4096, 1024, 32, 128, 512), (500, 60, 7, 61, 100)])
@pytest.mark.parametrize("regime", REGIMES)
def test_one_layer_levels_bound_hard_inputs(dev, N, S, K, D, C1, regime):
    premax = _one_layer_case(dev, N, S, K, D, C1, regime in ("cancel", "dups", "pad"), regime, torch.int32 if regime in ("tiny", "pad") else torch.int64)
    if regime == "negative":
        assert bool((premax[..., 1::4] < 0).all())


# ------------------------------------------------------------------------------------------------------------------------------
# two-layer levels: sa_level_mlp2_max, direct and commuted, fp32 MFMA and bf16x3 (both workgroup tiles)
# ------------------------------------------------------------------------------------------------------------------------------
MLP2_EXTRA = [(1500, 512, 32, 128, 128, 392),     # C2 past 256, no multiple of 128: the 256-wide tile's second half partly empty
              (2000, 300, 24, 9, 48, 200)]         # direct form, C2 no multiple of 128


def _mlp2_case(dev, monkeypatch, N, S, K, D, C1, C2, xyz_first, regime):
    from toothgroupnetwork_amd import pointnet2_utils as U, _lib, sa_fused
    B = 2
    xyz, feat, radius = make_cloud(B, N, D, N + K + D + C2, regime)
    tx, tf = T(xyz, dev), T(feat, dev)
    new_xyz, idx = _fps_ball(U, tx, S, radius, K)
    conv1, bn1 = make_layer(dev, 3 + D, C1, 11)
    conv2, bn2 = make_layer(dev, C1, C2, 12)
    apply_regime(regime, [conv1, conv2], [bn1, bn2])
    direct = bool(_lib.lib().tgn_sa_mlp2_direct_supported(K, D))
    if regime == "cancel":
        pre1 = lambda: first_layer64(tx, new_xyz, tf, idx, fold64(conv1), xyz_first, True)[0]
        pre2 = lambda: next_layer64(*first_layer64(tx, new_xyz, tf, idx, fold64(conv1, bn1), xyz_first, True), fold64(conv2))[0]
        centre_means([pre1, pre2], [bn1, bn2])
    pre, mag = first_layer64(tx, new_xyz, tf, idx, fold64(conv1, bn1), xyz_first, commuted=not direct)
    pre, mag = next_layer64(pre, mag, fold64(conv2, bn2))
    want, M, premax = reduce_max64(pre, mag)
    del pre, mag
    C1p = sa_fused.pad16(C1)
    C = chain_const(max(3 + D + 4, C1p))
    tag = f"({N},{S},{K},{D},{C1},{C2}) {'direct' if direct else 'commuted'} xyz_first={xyz_first} {regime}"
    rel = {}
    idx2, npad = repad(idx)
    with torch.no_grad():
        for form in ("fp32", 128, 256):
            monkeypatch.setattr(U, "SA_BF16X3", form != "fp32")
            prev = _lib.set_tuning("sa_tile", 0 if form == "fp32" else form)
            try:
                for index in (idx, idx.to(torch.int32)):
                    got = U.sa_level_mlp2_max(tx, new_xyz, tf, index, [conv1, conv2], [bn1, bn2], xyz_first)
                    r = check_bound(got, want, M, C, f"sa_level_mlp2_max {'fp32-MFMA' if form == 'fp32' else f'bf16x3 tile {form}'} "
                                    f"{str(index.dtype)[6:]} {tag}", premax)
                rel[form] = r
                if npad:
                    assert torch.equal(U.sa_level_mlp2_max(tx, new_xyz, tf, idx2, [conv1, conv2], [bn1, bn2], xyz_first), got), \
                        f"{tag} {form}: a duplicated neighbour changed a max"
            finally:
                _lib.set_tuning("sa_tile", prev)
    for form in (128, 256):
        compare_split(rel[form], rel["fp32"], f"sa_level_mlp2_max bf16x3 tile {form} {tag}")
    return premax, npad


@pytest.mark.parametrize("N,S,K,D,C1,C2", MLP2_SHAPES + MLP2_EXTRA)
@pytest.mark.parametrize("xyz_first", [True, False])
def test_two_layer_level_bound(dev, monkeypatch, N, S, K, D, C1, C2, xyz_first):
    _mlp2_case(dev, monkeypatch, N, S, K, D, C1, C2, xyz_first, "plain")


@pytest.mark.parametrize("N,S,K,D,C1,C2", [(6000, 1024, 32, 6, 128, 128), (1024, 512, 32, 256, 256, 512), (400, 20, 32, 40, 16, 48),
                                            (900, 77, 17, 61, 100, 260)])
@pytest.mark.parametrize("regime", REGIMES)
def test_two_layer_level_bound_hard_inputs(dev, monkeypatch, N, S, K, D, C1, C2, regime):
    premax, npad = _mlp2_case(dev, monkeypatch, N, S, K, D, C1, C2, regime not in ("cancel", "dups", "pad"), regime)
    if regime == "negative":
        assert bool((premax[..., 1::4] < 0).all())
    if regime == "pad":
        assert npad > 0, "the small radius left no ball-query row padded"


def test_commuted_bound_off_origin(dev):
    """What the commuted form's bound carries off the origin: M1 over [f, x] plus |centre| against M1 over [x - c, f]."""
    from toothgroupnetwork_amd import pointnet2_utils as U
    B, N, S, K, D, C1 = 2, 1024, 256, 32, 64, 128
    for regime in ("plain", "offorigin"):
        xyz, feat, radius = make_cloud(B, N, D, 5, regime)
        tx, tf = T(xyz, dev), T(feat, dev)
        new_xyz, idx = _fps_ball(U, tx, S, radius, K)
        conv, bn = make_layer(dev, 3 + D, C1, 3)
        layer = fold64(conv, bn)
        _, m_comm = first_layer64(tx, new_xyz, tf, idx, layer, True, commuted=True)
        _, m_dir = first_layer64(tx, new_xyz, tf, idx, layer, True, commuted=False)
        ratio = m_comm / m_dir
        print(f"\n{regime}: commuted / direct first-layer magnitude: mean {float(ratio.mean()):.2f} max {float(ratio.max()):.2f}")
        assert bool((ratio >= 1.0).all())
        if regime == "offorigin":
            assert float(ratio.mean()) > 1.5      # the cloud really sits away from the origin


# ------------------------------------------------------------------------------------------------------------------------------
# group-all: PointNetSetAbstraction(group_all=True) -> sa_all_mlp2_max
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 31, 32, 33, 64, 65, 257, 24000])
@pytest.mark.parametrize("D,C1,C2", [(6, 64, 128), (512, 256, 512)])
def test_group_all_bound(dev, monkeypatch, N, D, C1, C2):
    from toothgroupnetwork_amd import pointnet2_utils as U, _lib, sa_fused
    monkeypatch.setattr(U, "FUSED_SA", True)
    calls = []
    real = U.sa_all_mlp2_max
    monkeypatch.setattr(U, "sa_all_mlp2_max", lambda *a: calls.append(1) or real(*a))
    B = 2
    xyz, feat, _ = make_cloud(B, N, D, N + D, "offorigin" if N % 2 else "plain")
    tx, tf = T(xyz, dev), T(feat, dev)
    mod = U.PointNetSetAbstraction(None, None, None, 3 + D, [C1, C2], True).to(dev).eval()
    torch.manual_seed(N + D)
    with torch.no_grad():
        for bn in mod.mlp_bns:
            bn.running_mean.normal_(0, 0.3)
            bn.running_var.uniform_(0.4, 2.0)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0, 0.2)
        got = mod(tx.permute(0, 2, 1), tf.permute(0, 2, 1))[1][:, :, 0]
    assert calls, "group-all did not take the fused path"
    idx = torch.arange(N, device=dev).expand(B, 1, N)
    pre, mag = first_layer64(tx, None, tf, idx, fold64(mod.mlp_convs[0], mod.mlp_bns[0]), True, commuted=True)
    pre, mag = next_layer64(pre, mag, fold64(mod.mlp_convs[1], mod.mlp_bns[1]))
    want, M, premax = reduce_max64(pre, mag)
    direct = bool(_lib.lib().tgn_sa_mlp2_direct_supported(min(N, 64), D))
    check_bound(got, want[:, 0], M[:, 0], chain_const(max(3 + D + 4, sa_fused.pad16(C1))),
                f"group-all N={N} D={D} {'direct' if direct else 'commuted'}", premax[:, 0])


# ------------------------------------------------------------------------------------------------------------------------------
# bench.py --fused: HotPath(fused=True) at its own shape, each level against its own fp32 input
# ------------------------------------------------------------------------------------------------------------------------------
def test_hotpath_fused_bench_shape_bound(dev, monkeypatch):
    from toothgroupnetwork_amd import hotpath, synth, pointnet2_utils as U, sa_fused
    B = 2
    scans = synth.scan_batch(B, hotpath.SHAPE_A["n"], "arch", 17)
    pts = T(scans, dev)
    xyz = pts[:, :, :3].contiguous()
    rel = {}
    for bf16x3, index_dtype in ((False, torch.int64), (True, torch.int32)):
        monkeypatch.setattr(U, "SA_BF16X3", bf16x3)
        hp = hotpath.HotPath(B, dev, shape=hotpath.SHAPE_A, index_dtype=index_dtype, fused=True)
        levels = hp.run(xyz, [pts])
        torch.cuda.synchronize()
        cur, feat = xyz, pts
        for li, lv in enumerate(levels):
            D = feat.shape[2]
            new_xyz = U.index_points(cur, lv["fps_idx"].long())
            assert torch.equal(new_xyz, lv["new_xyz"])
            layers = [plain64(W, b, dev) for W, b in lv["layers"]]
            direct = bool(hp.L.tgn_sa_mlp2_direct_supported(lv["K"], D))
            pre, mag = first_layer64(cur, new_xyz, feat, lv["group_idx"], layers[0], True, commuted=not direct)
            for layer in layers[1:]:
                pre, mag = next_layer64(pre, mag, layer)
            want, M, premax = reduce_max64(pre, mag)
            del pre, mag
            C1p = sa_fused.pad16(lv["layers"][0][0].shape[0])
            form = "bf16x3" if bf16x3 else "fp32-MFMA"
            rel[bf16x3, li] = check_bound(lv["out"], want, M, chain_const(max(3 + D + 4, C1p)),
                                          f"HotPath fused level {li + 1} {form} ({'direct' if direct else 'commuted'}, D={D})", premax)
            cur, feat = lv["new_xyz"], lv["out"]      # the level's own fp32 output feeds the next one
    # (levels 2 and 3 of the two runs read their own form's level-1 output: inputs a few u apart, the same error statistics)
    for li in range(len(hotpath.SHAPE_A["npoint"])):
        compare_split(rel[True, li], rel[False, li], f"HotPath fused level {li + 1}")
