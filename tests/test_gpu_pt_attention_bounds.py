"""GPU: the fused eval-mode Point-Transformer attention kernel (tgn_pt_attention_forward, csrc/pt_attention.hip) at every one of
its five instantiations pt_attention_fwd_kernel<G>, G = c / share_planes in {4, 8, 16, 32, 64}, held to an element-wise float64
bound scaled by the terms of its output sum.

The direct cases call point_transformer.pt_attention with hand-made folded operands (the dict keys of _fold_pt_layer), so the
`deep` routing of PointTransformerLayer.forward -- which sends c * g >= 8192 below 4096 points to the torch composition -- cannot
step in: G = 32 and G = 64 run here.  Three more tests go through the layer where it does take the kernel at those widths (4096
points at c = 256; 64 packed scans at c = 512).

Reference.  restate64() restates include/tgn_pointops.h's description of the operator in float64 from the same fp32 operands and
returns, per output entry, the exact value `want` and M = sum_j sm_j (|x_v[idx_j, ch]| + |p_r_j[ch]|), the sum of the absolute terms
of the output stage (|post_scale| M + |post_shift| with the epilogue).  (An analytic worst case through all five nested layers is
50 - 4000 times |want|: looser than the max-norm test this file sits beside.)

Yardstick.  compose32() is the plain fp32 torch composition of the same folded operands on the CPU (gather, linear_p, x_k - x_q +
p_r, linear_w, torch.softmax, weighted sum): what careful fp32 arithmetic loses on these inputs.  It is never the kernel.

Bound.  With rho(x) = |x - want| / (u M), u = 2^-24, per case and for both the max and the rms of rho over the entries:
    rho(kernel) <= max(2 rho(compose32), C),   C = 8 max(1, sqrt(nsample / 16))
C is the chain constant of tests/test_gpu_sa_forward_bounds.py for the output sum over the neighbours.  The factor 2 over the
yardstick covers the kernel's DPP tree order, __expf (whose error grows with |argument|; torch uses libm) and the BatchNorm fold.
Outputs behind the epilogue whose pre-activation lies below -C u M must be exactly 0.

Measured on an MI355X, kernel / fp32 composition, in units of u M (the yardstick's figures are the CPU's and the same anywhere):

    case (n = 70, nsample = 24 unless said)     max rho plain      max rho post       rms plain        rms post
    c=32  G=4                                    2.84 /  6.75       2.72 /  5.02     0.583 / 0.960    0.360 / 0.574
    c=64  G=8                                    6.63 /  7.90       6.95 /  7.26     1.064 / 1.415    0.668 / 0.878
    c=128 G=16                                   3.22 /  6.98       3.02 /  5.43     0.687 / 1.092    0.448 / 0.672
    c=256 G=32                                   6.53 /  8.84       4.49 /  8.17     0.908 / 1.149    0.564 / 0.701
    c=512 G=64                                   9.93 / 10.66       9.24 / 10.11     1.274 / 1.345    0.796 / 0.848
    c=64  G=64 (share_planes 1)                  4.73 /  8.21       4.79 /  7.69     0.848 / 1.251    0.590 / 0.841
    c=4   G=4  (share_planes 1)                  2.96 /  4.08       1.82 /  3.50     0.622 / 1.014    0.382 / 0.676
    c=24  G=8  (share_planes 3)                  3.35 /  6.68       3.12 /  6.15     0.699 / 1.060    0.495 / 0.730

    neighbour counts, c=64 G=8                  max rho            rms
    nsample  1                                  11.16 /  9.27      0.696 / 0.658      (|out - fl(x_v + p_r)| = 0 in all three
    nsample 15                                   5.85 /  7.55      0.719 / 1.124       one-neighbour cases: the kernel's output IS
    nsample 16                                   6.22 /  9.00      0.935 / 1.221       the fp32 sum; what is left is p_r's own
    nsample 17                                   5.00 /  7.94      0.755 / 1.175       rounding where it cancels against x_v)
    nsample 32                                   3.52 / 10.87      0.707 / 1.393
    nsample 33                                   8.57 / 10.81      0.833 / 1.428
    nsample 63                                   2.78 / 14.51      0.601 / 2.139
    nsample 64                                   4.11 / 18.31      0.622 / 1.913
    c=256 G=32 nsample  1                       32.41 / 32.41      0.863 / 0.831
    c=256 G=32 nsample 64                        4.88 / 16.02      0.762 / 2.093
    c=512 G=64 nsample  1                       70.34 / 70.34      0.984 / 0.979
    c=512 G=64 nsample 64                        6.10 / 17.88      0.871 / 2.152

    wide logits (bias added last; spread)       max rho            rms
    c=32  G=4   (146.3)                        111.31 /  98.40    12.381 / 11.643
    c=256 G=32  (116.2)                        234.46 / 182.98    13.396 / 11.429     (724 before the bias went on last)
    c=512 G=64  (133.3)                        354.60 / 279.94    24.891 / 16.899

    grid stride, n=16389 c=32 G=4 nsample=8     17.32 / 13.29      0.868 / 0.972
    negative post scales, c=128 G=16             6.12 /  8.55      0.715 / 0.969      (4263 exact zeros)
    layer c=256 n=4096 (fused, G=32)             2.22 /  4.26      0.445 / 0.664
    layer c=256 n=4095 (composition)             4.70 /  4.62      0.708 / 0.666
    layer c=512 n=64x93 (fused, G=64)            2.81 /  4.36      0.458 / 0.708

The kernel is at or below the yardstick wherever many neighbours are summed (its DPP tree is a pairwise sum, torch's is not), and
within 1.3 times it in the wide-logit cases.

Teeth.  Three wrong-value mutations of the kernel, each built into a library of its own and run against this file on an MI355X:
    sm[(g + i + 1) % G] in pass 2 (the neighbouring weight channel): 32 of 45 tests fail -- all 16 of test_every_instantiation,
        every nsample > 1 case of test_neighbour_counts_at_the_dpp_row_boundaries (with one neighbour every weight is exactly 1,
        whichever channel), the three wide-logit cases, the grid stride, the negative post scales, and the two layer tests that
        take the kernel ([4096-fused] and the batched stage 5);
    mx = 0 in place of the wave maximum: exactly the three cases of test_wide_logits_need_the_maximum_subtracted fail
        (non-finite output) and nothing else does -- N(0, 1) logits do not need the maximum.
The third mutation (bnorm's sum of squares in float) is reported in tests/test_gpu_bn_rows_bounds.py.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U_RND = 2.0 ** -24
KEYS = ("Wp1", "bp1", "Wp2", "bp2", "a1", "t1", "Ww1", "bw1", "Ww2", "bw2")


def chain_const(n):
    """The project's chain constant (tests/test_gpu_sa_forward_bounds.py) for an fp32 sum of n terms."""
    return 8.0 * max(1.0, math.sqrt(n / 16.0))


# ------------------------------------------------------------------------------------------------------------------------------
# operands (CPU, fp32)
# ------------------------------------------------------------------------------------------------------------------------------
def make_params(c, g, seed):
    """Folded operands of one layer (the keys of point_transformer._fold_pt_layer) with seeded random values; the scales keep
    the logits a few units wide, like a trained layer's."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    return dict(Wp1=r(3, 3) * 0.8, bp1=r(3) * 0.2, Wp2=r(c, 3) * 0.8, bp2=r(c) * 0.2,
                a1=(torch.rand(c, generator=gen) + 0.5) * torch.where(r(c) < -1.0, -1.0, 1.0), t1=r(c) * 0.2,
                Ww1=r(g, c) / math.sqrt(c), bw1=r(g) * 0.2, Ww2=r(g, g) / math.sqrt(g), bw2=r(g) * 0.2)


def make_inputs(n, c, nsample, seed):
    """p (n,3), x_q / x_k / x_v (n,c), idx (n,nsample) int32 in [0, n): every third row holds the point itself, every fifth row a
    repeated neighbour (rows of a kNN over a cloud with fewer points than neighbours look like that)."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.rand(n, 3, generator=gen) * 2.0 - 1.0
    xq, xk, xv = (torch.randn(n, c, generator=gen) for _ in range(3))
    idx = torch.randint(0, n, (n, nsample), generator=gen, dtype=torch.int32)
    idx[::3, 0] = torch.arange(0, n, 3, dtype=torch.int32)
    idx[::5, nsample // 2:] = idx[::5, :1]
    assert int(idx.min()) >= 0 and int(idx.max()) < n
    return p, xq, xk, xv, idx


def make_post(c, seed, negative=False):
    gen = torch.Generator().manual_seed(seed)
    scale = torch.rand(c, generator=gen) + 0.5
    if negative:
        scale = scale * torch.where(torch.arange(c) % 2 == 0, -1.0, 1.0)
    return scale, torch.randn(c, generator=gen) * 0.3


# ------------------------------------------------------------------------------------------------------------------------------
# float64 restatement and fp32 yardstick (CPU)
# ------------------------------------------------------------------------------------------------------------------------------
def _compose(p, xq, xk, xv, idx, P, post, rows, dtype):
    """include/tgn_pointops.h:212-222 with plain torch operators in `dtype`; rows: the points to evaluate (None: all).
    Returns out, M (sum of the absolute terms of the output stage), the value before the epilogue's ReLU, the logits."""
    t = lambda a: a.to(dtype)
    P = {k: t(v) for k, v in P.items()}
    p, xq, xk, xv = t(p), t(xq), t(xk), t(xv)
    rows = torch.arange(xq.shape[0]) if rows is None else rows
    il = idx[rows].long()
    m, ns = il.shape
    c, g = xq.shape[1], P["Ww2"].shape[0]
    rel = p[il] - p[rows][:, None, :]
    h = torch.relu(torch.nn.functional.linear(rel, P["Wp1"], P["bp1"]))
    pr = torch.nn.functional.linear(h, P["Wp2"], P["bp2"])                          # (m, ns, c)
    w = xk[il] - xq[rows][:, None, :] + pr
    u = torch.relu(w * P["a1"] + P["t1"])
    hid = torch.relu(torch.nn.functional.linear(u, P["Ww1"], P["bw1"]))
    lg = torch.nn.functional.linear(hid, P["Ww2"], P["bw2"])                        # (m, ns, g)
    sm = torch.softmax(lg, dim=1)
    smb = sm[:, :, None, :]                                                         # channel ch takes weight channel ch % g
    out = ((xv[il] + pr).view(m, ns, c // g, g) * smb).sum(1).reshape(m, c)
    M = ((xv[il].abs() + pr.abs()).view(m, ns, c // g, g) * smb).sum(1).reshape(m, c)
    pre = out
    if post is not None:
        s, b = t(post[0]), t(post[1])
        pre = out * s + b
        M = M * s.abs() + b.abs()
        out = torch.relu(pre)
    return out, M, pre, lg


def restate64(p, xq, xk, xv, idx, P, post=None, rows=None):
    return _compose(p, xq, xk, xv, idx, P, post, rows, torch.float64)


def compose32(p, xq, xk, xv, idx, P, post=None, rows=None):
    return _compose(p, xq, xk, xv, idx, P, post, rows, torch.float32)[0]


def rho(x, want, M):
    err = (x.double() - want).abs()
    r = torch.where(M > 0, err / M.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return r / U_RND


def check_bound(got, yard, want, M, pre, nsample, what, epilogue=False):
    """max and rms of rho(got) within max(2 rho(yard), C); behind the epilogue, outputs with pre < -C u M are exactly 0.
    Prints both worst ratios; returns the number of exact zeros that were checked."""
    got = got.detach().cpu()
    C = chain_const(nsample)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    rk, ry = rho(got, want, M), rho(yard, want, M)
    k_max, y_max = float(rk.max()), float(ry.max())
    k_rms, y_rms = float(rk.square().mean().sqrt()), float(ry.square().mean().sqrt())
    dead = 0
    if epilogue:
        mask = pre < -C * U_RND * M
        dead = int(mask.sum())
        nz = int((got[mask] != 0).sum())
        assert nz == 0, f"{what}: {nz} outputs whose pre-activation lies below -C u M are not exactly 0"
    print(f"\n{what}: max rho kernel {k_max:.2f} / fp32 composition {y_max:.2f}; rms {k_rms:.3f} / {y_rms:.3f} (C = {C:.1f})"
          + (f"; {dead} exact zeros" if epilogue else ""))
    worst = int(torch.argmax(rk))
    assert k_max <= max(2.0 * y_max, C), (f"{what}: max rho {k_max:.2f} > max(2 * {y_max:.2f}, {C:.1f}) at entry {worst}: got "
                                          f"{float(got.flatten()[worst])!r}, want {float(want.flatten()[worst])!r}, "
                                          f"M {float(M.flatten()[worst]):.3e}")
    assert k_rms <= max(2.0 * y_rms, C), f"{what}: rms rho {k_rms:.3f} > max(2 * {y_rms:.3f}, {C:.1f})"
    return dead


def run_kernel(dev, p, xq, xk, xv, idx, P, post=None):
    from toothgroupnetwork_amd import point_transformer as PT
    d = lambda a: a.to(dev).contiguous()
    out = PT.pt_attention(d(p), d(xq), d(xk), d(xv), d(idx), {k: d(v) for k, v in P.items()},
                          None if post is None else (d(post[0]), d(post[1])))
    torch.cuda.synchronize()
    return out


def direct_case(dev, n, c, g, nsample, seed, post=None, P=None, what=""):
    inp = make_inputs(n, c, nsample, seed)
    P = make_params(c, g, seed + 1) if P is None else P
    got = run_kernel(dev, *inp, P, post)
    want, M, pre, _ = restate64(*inp, P, post)
    yard = compose32(*inp, P, post)
    dead = check_bound(got, yard, want, M, pre, nsample, what or f"c={c} G={g} n={n} nsample={nsample} post={post is not None}",
                       epilogue=post is not None)
    return inp, P, got, want, M, dead


# ------------------------------------------------------------------------------------------------------------------------------
# direct calls
# ------------------------------------------------------------------------------------------------------------------------------
WIDTHS = [(32, 4), (64, 8), (128, 16), (256, 32), (512, 64), (64, 64), (4, 4), (24, 8)]


@pytest.mark.parametrize("with_post", [False, True], ids=["plain", "post"])
@pytest.mark.parametrize("c,g", WIDTHS, ids=[f"c{c}-G{g}" for c, g in WIDTHS])
def test_every_instantiation(dev, c, g, with_post):
    """all five pt_attention_fwd_kernel<G>, share_planes 8, 1 and 3; n = 70: the last workgroup (4 points) holds two idle waves"""
    direct_case(dev, 70, c, g, 24, seed=c * 7 + g, post=make_post(c, c + g) if with_post else None)


NEIGHBOURS = [(64, 8, ns) for ns in (1, 15, 16, 17, 32, 33, 63, 64)] + [(256, 32, 1), (256, 32, 64), (512, 64, 1), (512, 64, 64)]


@pytest.mark.parametrize("c,g,nsample", NEIGHBOURS, ids=[f"c{c}-G{g}-ns{ns}" for c, g, ns in NEIGHBOURS])
def test_neighbour_counts_at_the_dpp_row_boundaries(dev, c, g, nsample):
    """the active lanes end just below, at and just above a DPP row (16 lanes) and a half wave, at one lane and at all 64.
    With one neighbour its softmax weight is exactly 1 (exp(0) / exp(0)), so the output is the fp32 sum x_v + p_r and nothing of
    the softmax or the lane reduction may show: |out - fl(x_v + p_r)| <= 2 u M, p_r evaluated in fp32 in the kernel's order."""
    (p, xq, xk, xv, idx), P, got, want, M, _ = direct_case(dev, 70, c, g, nsample, seed=nsample * 11 + g)
    if nsample == 1:
        nb = idx[:, 0].long()
        rel = p[nb] - p
        W1, W2 = P["Wp1"], P["Wp2"]
        h = torch.relu(((rel[:, None, 0] * W1[:, 0] + rel[:, None, 1] * W1[:, 1]) + rel[:, None, 2] * W1[:, 2]) + P["bp1"])
        pr = ((h[:, None, 0] * W2[:, 0] + h[:, None, 1] * W2[:, 1]) + h[:, None, 2] * W2[:, 2]) + P["bp2"]
        fl = (xv[nb] + pr).double()
        worst = float(((got.cpu().double() - fl).abs() / (U_RND * M)).max())
        print(f"nsample = 1: worst |out - fl(x_v + p_r)| / (u M) = {worst:.3f}")
        assert worst <= 2.0


@pytest.mark.parametrize("c,g", [(32, 4), (256, 32), (512, 64)], ids=["G4", "G32", "G64"])
def test_wide_logits_need_the_maximum_subtracted(dev, c, g):
    """Ww2 scaled until one point's float64 logits span more than 100.  Outputs finite and inside the bound.
    A spread of 100 alone can leave every logit within +-88, where exp() of the raw logit is still a finite fp32 number, so a
    softmax that does not subtract the maximum could pass.  The test therefore also shifts two weight channels as a whole,
    bw2[0] by +200 and bw2[1] by -200.  No trained layer has such a bias, and the softmax over the neighbours is exactly
    invariant to it (a channel's bias is the same for every neighbour): the shift is there only so that exp() of a raw logit
    overflows in channel 0 and underflows for every neighbour in channel 1, which turns a missing maximum into inf / inf and
    0 / 0.  Its price is rounding at magnitude 200 in those two logits: that rounding, not the spread, is what lifts the
    yardstick to about 100 - 240 u M here, so the bound of this case (twice the yardstick) is dominated by the bias's own
    rounding.
    The shift also showed an avoidable loss in the kernel: it used to start each logit's sum from its bias, so the channel with
    the bias of 200 rounded all G partial sums at that magnitude -- G = 32 came out at 724 u M where the fp32 composition is at
    183.  The bias now goes on last (one rounding at that magnitude, as in the composition); this case keeps it so."""
    n, nsample, seed = 70, 24, 5 * g
    inp = make_inputs(n, c, nsample, seed)
    P = make_params(c, g, seed + 1)
    def spread():
        lg = restate64(*inp, P)[3]
        return float((lg.amax(1) - lg.amin(1)).max()), lg
    while spread()[0] <= 100.0:
        P["Ww2"] = P["Ww2"] * 2.0
    P["bw2"][0] += 200.0
    P["bw2"][1] -= 200.0
    widest, lg = spread()
    assert widest > 100.0
    assert float(lg[:, :, 0].amax(1).max()) > 90.0 and float(lg[:, :, 1].amax(1).min()) < -105.0
    print(f"\nwidest float64 logit spread of a point: {widest:.1f}")
    direct_case(dev, n, c, g, nsample, seed, P=P, what=f"wide logits c={c} G={g}")


def test_grid_stride_second_trip(dev):
    """the grid is capped at 4096 workgroups of 4 points: points 16 384 and above are a workgroup's second trip"""
    n = 16389
    _, _, got, want, M, _ = direct_case(dev, n, 32, 4, 8, seed=3)
    tail = rho(got.cpu()[16384:], want[16384:], M[16384:])
    assert float(tail.max()) <= chain_const(8), float(tail.max())


def test_epilogue_with_negative_scales_gives_exact_zeros(dev):
    """relu(out * post_scale + post_shift) with every other scale negative: where the exact pre-activation lies below -C u M the
    output is exactly 0 (check_bound asserts it); the case must hold such entries, and live ones"""
    c, g = 128, 16
    _, _, got, _, _, dead = direct_case(dev, 70, c, g, 24, seed=77, post=make_post(c, 78, negative=True))
    assert 100 < dead < got.numel() - 100 and int((got > 0).sum()) > 100


def _raw_call(dev, n, nsample, c, g, xk_offset=0, post=(False, False)):
    """tgn_pt_attention_forward through the C ABI on buffers large enough for any of the argument cases (nothing may be launched,
    and nothing that were could leave them).  Returns (status, last error, out untouched)."""
    from toothgroupnetwork_amd._lib import lib, ptr, stream
    big = 16 * 65 * 64
    z = lambda m=big: torch.zeros(m, dtype=torch.float32, device=dev)
    p, xq, xv, xk = z(), z(), z(), z(big + 4)
    idx = torch.zeros(big, dtype=torch.int32, device=dev)
    par = [z() for _ in KEYS]
    ps, pt = z(), z()
    out = torch.full((big,), 7.0, dtype=torch.float32, device=dev)
    xk_arg = ctypes.c_void_p(xk.data_ptr() + 4 * xk_offset)
    rc = lib().tgn_pt_attention_forward(n, nsample, c, g, ptr(p), ptr(xq), xk_arg, ptr(xv), ptr(idx), *[ptr(t) for t in par],
                                        ptr(ps) if post[0] else None, ptr(pt) if post[1] else None, ptr(out), stream())
    msg = lib().tgn_last_error().decode("utf-8", "replace")
    torch.cuda.synchronize()
    return rc, msg, bool((out == 7.0).all())


@pytest.mark.parametrize("kw,status", [
    (dict(n=16, nsample=16, c=24, g=12), "unsupported"),                       # weight channels outside {4, 8, 16, 32, 64}
    (dict(n=16, nsample=16, c=30, g=6), "unsupported"),                        # c % 4 != 0
    (dict(n=16, nsample=16, c=40, g=16), "unsupported"),                       # c % g != 0
    (dict(n=16, nsample=65, c=32, g=4), "unsupported"),                        # more neighbours than a wave has lanes
    (dict(n=16, nsample=16, c=32, g=4, xk_offset=1), "unsupported"),           # x_k not 16-byte aligned
    (dict(n=16, nsample=16, c=32, g=4, post=(True, False)), "invalid"),        # post_scale without post_shift
    (dict(n=16, nsample=16, c=32, g=4, post=(False, True)), "invalid"),
], ids=["g12", "c30", "c40-g16", "ns65", "xk-misaligned", "scale-only", "shift-only"])
def test_argument_errors_are_returned_before_any_launch(dev, kw, status):
    from toothgroupnetwork_amd import _lib
    rc, msg, untouched = _raw_call(dev, **kw)
    assert rc == {"unsupported": _lib.ERR_UNSUPPORTED, "invalid": _lib.ERR_INVALID_ARGUMENT}[status], (rc, msg)
    assert msg and "tgn_pt_attention_forward" in msg, msg
    assert untouched


def test_zero_points_is_ok_and_writes_nothing(dev):
    rc, _, untouched = _raw_call(dev, n=0, nsample=16, c=32, g=4)
    assert rc == 0 and untouched


# ------------------------------------------------------------------------------------------------------------------------------
# through PointTransformerLayer, eval mode
# ------------------------------------------------------------------------------------------------------------------------------
def _randomise_bn(mod, seed):
    g = torch.Generator().manual_seed(seed)
    for m_ in mod.modules():
        if isinstance(m_, torch.nn.BatchNorm1d):
            m_.running_mean.copy_(torch.randn(m_.num_features, generator=g) * 0.2)
            m_.running_var.copy_(torch.rand(m_.num_features, generator=g) * 1.5 + 0.5)
            m_.weight.data.copy_(torch.rand(m_.num_features, generator=g) + 0.5)
            m_.bias.data.copy_(torch.randn(m_.num_features, generator=g) * 0.1)


def _layer(dev, c, nsample, seed):
    """a seeded PointTransformerLayer(c, c, 8, nsample) with random BatchNorm statistics, eval mode"""
    from toothgroupnetwork_amd import point_transformer as PT
    torch.manual_seed(seed)
    layer = PT.PointTransformerLayer(c, c, 8, nsample)
    _randomise_bn(layer, seed + 1)
    return layer.to(dev).eval()


def _spy(monkeypatch):
    """counts the calls of the fused kernel's wrapper from here on: returns the one-entry list that holds the count"""
    from toothgroupnetwork_amd import point_transformer as PT
    calls = [0]
    real = PT.pt_attention

    def spy(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(PT, "pt_attention", spy)
    return calls


def _layer_run(dev, monkeypatch, c, nsample, sizes, seed):
    """_layer(c, nsample, seed) on packed arch clouds of `sizes` points.
    Returns (output, number of fused-kernel calls, CPU operands (p, x_q, x_k, x_v, idx, folded params))."""
    from toothgroupnetwork_amd import point_transformer as PT, pointops as P, synth
    layer = _layer(dev, c, nsample, seed)
    xyz = np.concatenate([synth.arch_cloud(m, seed=seed + i, with_normals=False) for i, m in enumerate(sizes)])
    n = int(sum(sizes))
    p = torch.from_numpy(xyz).to(dev)
    o = torch.from_numpy(np.cumsum(sizes).astype(np.int32)).to(dev)
    x = torch.randn(n, c, generator=torch.Generator().manual_seed(seed + 2)).to(dev)
    calls = _spy(monkeypatch)
    with torch.no_grad():
        y = layer([p, x, o])
        count = calls[0]
        xq, xk, xv = layer.linear_q(x), layer.linear_k(x), layer.linear_v(x)
        idx = P.knn_indices(nsample, p, p, o, o)
        params = PT._fold_pt_layer(layer.linear_p[0], layer.linear_p[1], layer.linear_p[3], layer.linear_w[0], layer.linear_w[2],
                                   layer.linear_w[3], layer.linear_w[5])
    torch.cuda.synchronize()
    ops = tuple(t.cpu() for t in (p, xq, xk, xv, idx)) + ({k: v.cpu() for k, v in params.items()},)
    return y, count, ops


def _check_layer(y, ops, nsample, what, sample):
    """the layer's output against the restatement and the yardstick on a fixed sample of 256 points (seed `sample`)"""
    rows = torch.randperm(y.shape[0], generator=torch.Generator().manual_seed(sample))[:256].sort().values
    want, M, pre, _ = restate64(*ops, rows=rows)
    yard = compose32(*ops, rows=rows)
    check_bound(y.cpu()[rows], yard, want, M, pre, nsample, what)


@pytest.mark.parametrize("n,fused", [(4096, 1), (4095, 0)], ids=["4096-fused", "4095-composition"])
def test_layer_dispatch_at_the_deep_threshold(dev, monkeypatch, n, fused):
    """c = 256, share_planes 8 (c * g = 8192): the fused kernel (G = 32) from 4096 points on, the composition below; either output
    inside the bound, each on the same seeded sample of 256 point numbers"""
    y, count, ops = _layer_run(dev, monkeypatch, 256, 16, [n], seed=21)
    assert count == fused
    _check_layer(y, ops, 16, f"layer c=256 n={n} ({'fused' if fused else 'composition'})", sample=4)


def test_layer_packed_segments_equal_the_segments_alone(dev, monkeypatch):
    """two clouds packed with offsets [300, 700] against each run alone: a point's arithmetic depends only on the values of its
    rows, never on where they sit, so the outputs are the same bits.  (The neighbour search and the BLAS projections in front of
    the kernel are compared too, so that a failure names its stage.)"""
    from toothgroupnetwork_amd import pointops as P, synth
    layer = _layer(dev, 32, 16, seed=8)
    sizes = [300, 400]
    clouds = [torch.from_numpy(synth.arch_cloud(m, seed=40 + i, with_normals=False)).to(dev) for i, m in enumerate(sizes)]
    feats = [torch.randn(m, 32, generator=torch.Generator().manual_seed(50 + i)).to(dev) for i, m in enumerate(sizes)]
    calls = _spy(monkeypatch)
    with torch.no_grad():
        p, x = torch.cat(clouds), torch.cat(feats)
        o = torch.tensor([300, 700], dtype=torch.int32, device=dev)
        packed = layer([p, x, o])
        idx_packed = P.knn_indices(16, p, p, o, o).clone()
        alone, idx_alone = [], []
        for i, (pp, xx) in enumerate(zip(clouds, feats)):
            oo = torch.tensor([sizes[i]], dtype=torch.int32, device=dev)
            alone.append(layer([pp, xx, oo]))
            idx_alone.append(P.knn_indices(16, pp, pp, oo, oo) + (0 if i == 0 else sizes[0]))
        proj_same = all(torch.equal(lin(x), torch.cat([lin(f) for f in feats])) for lin in (layer.linear_q, layer.linear_k, layer.linear_v))
    assert calls[0] == 3
    assert torch.equal(idx_packed, torch.cat(idx_alone)), "the neighbour search differs between packed and alone"
    assert proj_same, "the input projections (BLAS) differ between packed and alone"
    assert torch.equal(packed, torch.cat(alone))


def test_layer_batched_stage5_takes_the_widest_kernel(dev, monkeypatch):
    """64 scans' stage 5 packed: 64 x 93 = 5952 points at c = 512 is not `deep`, the layer runs pt_attention_fwd_kernel<64>"""
    y, count, ops = _layer_run(dev, monkeypatch, 512, 24, [93] * 64, seed=33)
    assert count == 1 and y.shape == (5952, 512)
    _check_layer(y, ops, 24, "layer c=512 n=64x93 (fused)", sample=6)
