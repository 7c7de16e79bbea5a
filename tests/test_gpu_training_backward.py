"""GPU: the backward kernels the training step runs, against float64 torch at the shapes the networks train with.

* ``pt_softmax_aggregate`` (csrc/pt_attention.hip): forward and backward against float64 autograd, one case per code path of
  both kernels (merged / fallback backward, register / global neighbour indices in the forward, one or two lane trips of the
  softmax, the grid-stride second trip), plus duplicate-heavy indices, large and tied logits and the LDS limit.
* ``PointTransformerLayer`` + the block's ``bn2`` in training mode at the five U-Net stage shapes against a float64 restatement
  of blocks.py:34-43 (and the branch ``PointTransformerLayer.forward`` takes when nothing needs a gradient).
* The PointNet++ backward scatters: ``group_points`` and ``index_points`` (``tgn_scatter_add_points``) and
  ``three_interpolate`` (``tgn_interpolation_backward`` with the batch offset added in Python).

Element-wise bounds follow the condition of the sum being checked, not the size of its result: an entry that is a sum of
terms t_i must satisfy |got - exact| <= 8 u sum |t_i| + tiny (u = 2^-24, the fp32 unit roundoff), with ``exact`` and sum |t_i|
both evaluated in float64 from the same fp32 inputs.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
TINY = 1e-30          # below every fp32 normal: lets a weight that underflows to zero in fp32 (exp(-160)) pass
LDS_LIMIT = 64 * 1024


def _within(got, exact, absterms, what, k=8.0):
    """|got - exact| <= k u |terms| + TINY everywhere; the message names the worst entry in units of u |terms|."""
    assert got is not None, f"{what}: no gradient"
    got = got.detach().double()
    assert got.shape == exact.shape, (what, got.shape, exact.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite entries"
    err = (got - exact).abs()
    lim = k * U32 * absterms + TINY
    bad = err > lim
    ratio = err / (U32 * absterms + TINY)
    print(f"{what}: worst {float(ratio.max()):.2f} u sum|terms| (bound {k})")
    if bool(bad.any()):
        i = int(ratio.reshape(-1).argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} entries over {k} u sum|terms|; worst at flat index {i}: "
                             f"got {got.reshape(-1)[i].item():.9g}, exact {exact.reshape(-1)[i].item():.9g}, "
                             f"sum|terms| {absterms.reshape(-1)[i].item():.3g} ({ratio.reshape(-1)[i].item():.1f} u)")


# ---------------------------------------------------------------------------------------------------------------------------
# 1. pt_softmax_aggregate
# ---------------------------------------------------------------------------------------------------------------------------
def _sa_exact(xv, pr, lg, idx, go):
    """float64 autograd of out[n,ch] = sum_j (xv[idx[n,j],ch] + pr[n,j,ch]) softmax_j(lg)[n,j,ch % g] (blocks.py:41-43), and the
    float64 sums of absolute terms of every entry checked."""
    n, ns, c = pr.shape
    g = lg.shape[2]
    s = c // g
    x, p, l = (t.detach().double().requires_grad_(True) for t in (xv, pr, lg))
    G = go.double()
    il = idx.long()
    sm = torch.softmax(l, dim=1)
    v = x[il] + p                                                              # (n, ns, c)
    out = (v.view(n, ns, s, g) * sm.unsqueeze(2)).sum(1).view(n, c)
    out.backward(G)
    with torch.no_grad():
        # A softmax weight evaluated in fp32 is off from the exact one by a relative u (kappa_j + mean kappa + sqrt(nsample)) or so:
        # the argument l_j - max of its exponential is rounded (exp's own condition, kappa_j = |l_j - max|), the normaliser carries the
        # sm-weighted mean of those errors and the rounding of a sum of nsample positive terms (a random walk). The magnitudes below
        # count every weight as sm_j (1 + (that) / 8), so that 8 u of them covers it.
        smd = sm.detach()
        kap = (l.detach() - l.detach().amax(1, keepdim=True)).abs()
        smw = smd * (1.0 + (kap + (smd * kap).sum(1, keepdim=True) + ns ** 0.5) / 8.0)
        smc = smw.repeat(1, 1, s)                                              # smc[n, j, ch] = smw[n, j, ch % g]
        vd = v.detach()
        out_abs = (vd * smc).abs().sum(1)
        dpr_abs = (G.unsqueeze(1) * smc).abs()
        # d_xv rows are atomic sums of m terms in an order the hardware picks: their rounding walks like sqrt(m) u of the terms
        m_row = torch.bincount(il.reshape(-1), minlength=x.shape[0]).double().unsqueeze(1)
        dxv_abs = torch.zeros_like(x).index_add_(0, il.reshape(-1), dpr_abs.reshape(-1, c)) * (1.0 + m_row.sqrt() / 8.0)
        dsm_abs = (G.unsqueeze(1) * vd).abs().view(n, ns, s, g).sum(2)           # terms of d_sm[n, j, g]
        dlg_abs = smw * (dsm_abs + (smw * dsm_abs).sum(1, keepdim=True))
    return dict(out=out.detach(), out_abs=out_abs, d_xv=x.grad, dxv_abs=dxv_abs, d_pr=p.grad, dpr_abs=dpr_abs, d_lg=l.grad,
                dlg_abs=dlg_abs)


def _sa_check(xv, pr, lg, idx, go, tag=""):
    from toothgroupnetwork_amd import point_transformer as PT
    xv, pr, lg = (t.detach().clone().requires_grad_(True) for t in (xv, pr, lg))
    out = PT.pt_softmax_aggregate(xv, pr, lg, idx)
    out.backward(go)
    want = _sa_exact(xv, pr, lg, idx, go)
    _within(out, want["out"], want["out_abs"], f"{tag} out")
    _within(pr.grad, want["d_pr"], want["dpr_abs"], f"{tag} d_pr")
    _within(xv.grad, want["d_xv"], want["dxv_abs"], f"{tag} d_xv")
    _within(lg.grad, want["d_lg"], want["dlg_abs"], f"{tag} d_logit")
    return out


def _sa_inputs(dev, n, nv, ns, c, g, seed, idx=None):
    gen = torch.Generator(device=dev).manual_seed(seed)
    xv = torch.randn(nv, c, device=dev, generator=gen)
    pr = torch.randn(n, ns, c, device=dev, generator=gen)
    lg = torch.randn(n, ns, g, device=dev, generator=gen) * 2.0
    go = torch.randn(n, c, device=dev, generator=gen)
    if idx is None:
        idx = torch.randint(0, nv, (n, ns), device=dev, dtype=torch.int32, generator=gen)
    return xv, pr, lg, idx, go


def _knn_idx(dev, xyz, ns):
    from toothgroupnetwork_amd import pointops as P
    tp = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32)).to(dev)
    to = torch.tensor([tp.shape[0]], dtype=torch.int32, device=dev)
    idx, _ = P.knnquery(ns, tp, tp, to, to)
    return idx.to(torch.int32).contiguous()


# (n, nv, nsample, c, g); the id names the branches each case reaches
_SA_CASES = [
    pytest.param(24000, 24000, 36, 32, 4, id="stage1-merged-grid_stride_2nd_trip"),
    pytest.param(6000, 6000, 24, 64, 8, id="stage2-merged"),
    pytest.param(1500, 1500, 24, 128, 16, id="stage3-merged-two_chunks"),
    pytest.param(375, 375, 24, 256, 32, id="stage4-merged-four_chunks"),
    pytest.param(93, 93, 24, 512, 64, id="stage5-merged-g64_no_shuffle"),
    pytest.param(1000, 1100, 16, 32, 4, id="merged-c32_masked_upper_lanes"),
    pytest.param(777, 800, 13, 48, 8, id="merged-c48_masked_lanes-ns_tail"),
    pytest.param(500, 520, 20, 96, 16, id="merged-c96_partial_second_chunk"),
    pytest.param(300, 340, 11, 48, 6, id="fallback-g6"),
    pytest.param(400, 400, 16, 96, 12, id="fallback-g12"),
    pytest.param(200, 210, 9, 144, 48, id="fallback-g48"),
    pytest.param(300, 320, 65, 32, 4, id="ns65-fwd_global_idx-fallback"),
    pytest.param(150, 160, 100, 64, 8, id="ns100-fwd_global_idx-fallback"),
    pytest.param(64, 80, 8, 256, 128, id="g128-softmax_second_lane_trip-fallback"),
    pytest.param(1, 3, 1, 4, 1, id="small-n1_ns1-g1_full_wave_shuffle"),
    pytest.param(5, 5, 3, 4, 4, id="small-ns3_not_mult4-merged"),
    pytest.param(7, 9, 5, 8, 1, id="small-n7-g1_full_wave_shuffle"),
]


@pytest.mark.parametrize("n,nv,ns,c,g", _SA_CASES)
def test_softmax_aggregate_vs_float64(dev, n, nv, ns, c, g):
    from toothgroupnetwork_amd import synth
    assert 4 * ns * g * 4 <= LDS_LIMIT, "case exceeds the wrappers' LDS limit"
    idx = None
    if n == nv and n >= 93:                                  # the stage shapes: neighbour rows from the kNN of an arch scan
        idx = _knn_idx(dev, synth.arch_cloud(n, seed=n % 97, with_normals=False), ns)
    _sa_check(*_sa_inputs(dev, n, nv, ns, c, g, seed=n + c, idx=idx), tag=f"n={n} ns={ns} c={c} g={g}")


@pytest.mark.parametrize("c,g", [pytest.param(64, 8, id="merged"), pytest.param(48, 6, id="fallback")])
@pytest.mark.parametrize("kind", ["one_row_per_point", "ball_query_padding", "knn_duplicated_vertices"])
def test_softmax_aggregate_duplicate_heavy_indices(dev, kind, c, g):
    """many (point, neighbour) pairs scattering into the same row of d_xv: (a) every neighbour of a point is one row (4 points,
    96 terms per row), (b) the tail half of each row repeats its first index, as ball query pads short rows, (c) kNN over a scan whose vertices
    are duplicated up to 12 times."""
    from toothgroupnetwork_amd import synth
    ns = 24
    gen = torch.Generator(device=dev).manual_seed(11)
    if kind == "one_row_per_point":
        n, nv = 4000, 1000
        idx = torch.randint(0, nv, (n, 1), device=dev, dtype=torch.int32, generator=gen).expand(n, ns).contiguous()
    elif kind == "ball_query_padding":
        n, nv = 3000, 3000
        idx = torch.randint(0, nv, (n, ns), device=dev, dtype=torch.int32, generator=gen)
        idx[:, ns // 2:] = idx[:, :1]
    else:
        base = synth.arch_cloud(2000, seed=5, with_normals=False)
        rng = np.random.default_rng(5)
        rep = rng.integers(1, 13, size=base.shape[0])
        xyz = np.repeat(base, rep, axis=0)[rng.permutation(int(rep.sum()))]
        n = nv = xyz.shape[0]
        idx = _knn_idx(dev, xyz, ns)
    xv, pr, lg, _, go = _sa_inputs(dev, n, nv, ns, c, g, seed=17, idx=idx)
    _sa_check(xv, pr, lg, idx, go, tag=kind)


@pytest.mark.parametrize("c,g", [pytest.param(64, 8, id="merged"), pytest.param(48, 6, id="fallback"),
                                 pytest.param(256, 128, id="g128")])
@pytest.mark.parametrize("kind", ["pm80", "pm80_plus_1e3", "tied", "tied_max"])
def test_softmax_aggregate_large_and_tied_logits(dev, kind, c, g):
    """logits of +-80 (exp overflows fp32 from 88.7 on) with and without a common offset of 1e3, all logits of a (point, channel)
    equal, and half of them tied at the maximum: finite, and within the float64 bound (a softmax without the max subtraction
    returns inf / nan here)."""
    n, nv, ns = 600, 700, 16
    xv, pr, _, idx, go = _sa_inputs(dev, n, nv, ns, c, g, seed=23)
    gen = torch.Generator(device=dev).manual_seed(29)
    if kind.startswith("pm80"):
        lg = (torch.rand(n, ns, g, device=dev, generator=gen) * 2.0 - 1.0) * 80.0
        lg[:, 0] = 80.0 * torch.sign(lg[:, 0] + 1e-3)       # every (point, channel) has an entry at +-80 exactly
        if kind == "pm80_plus_1e3":
            lg = lg + 1e3
    elif kind == "tied":
        lg = torch.randn(n, 1, g, device=dev, generator=gen).expand(n, ns, g).contiguous() * 50.0
    else:
        lg = torch.randn(n, ns, g, device=dev, generator=gen)
        lg[:, ::2] = 7.5                                     # above every other entry with overwhelming probability: an 8-way tie
    out = _sa_check(xv, pr, lg, idx, go, tag=kind)
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("n,ns,c,g", [pytest.param(24000, 36, 32, 4, id="stage1-merged"), pytest.param(300, 65, 32, 4, id="ns65"),
                                      pytest.param(64, 8, 256, 128, id="g128")])
def test_softmax_aggregate_forward_is_deterministic(dev, n, ns, c, g):
    """the forward has no atomics: two runs give the same bits (d_xv is an atomic scatter and is not held to this)."""
    from toothgroupnetwork_amd import point_transformer as PT
    xv, pr, lg, idx, _ = _sa_inputs(dev, n, n + 7, ns, c, g, seed=31)
    with torch.no_grad():
        a = PT.pt_softmax_aggregate(xv, pr, lg, idx)
        b = PT.pt_softmax_aggregate(xv, pr, lg, idx)
    assert torch.equal(a, b)


def test_softmax_aggregate_over_the_lds_limit_raises(dev):
    """4 waves x nsample x g x 4 B of LDS: nsample 65 x g 64 is 66 560 B, over the 64 KB the wrappers allow. Both entry points must
    refuse before launching; the buffers are sized for the call all the same."""
    from toothgroupnetwork_amd import point_transformer as PT
    from toothgroupnetwork_amd._lib import lib, ptr, stream
    n, ns, c, g = 4, 65, 64, 64
    assert 4 * ns * g * 4 > LDS_LIMIT
    xv, pr, lg, idx, go = _sa_inputs(dev, n, n, ns, c, g, seed=37)
    with pytest.raises(RuntimeError, match="too large"):
        PT.pt_softmax_aggregate(xv, pr, lg, idx)
    sm = torch.softmax(lg, dim=1)
    gx, gp, gl = torch.zeros_like(xv), torch.empty_like(pr), torch.empty_like(lg)
    torch.cuda.synchronize()
    rc = lib().tgn_pt_softmax_aggregate_backward(n, ns, c, g, ptr(xv), ptr(pr), ptr(sm), ptr(idx), ptr(go), ptr(gx), ptr(gp), ptr(gl),
                                                 stream())
    assert rc != 0 and b"too large" in lib().tgn_last_error()
    torch.cuda.synchronize()
    assert not gx.any()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. PointTransformerLayer + the block's bn2 in training mode
# ---------------------------------------------------------------------------------------------------------------------------
def _pt_layer_torch(layer, post_bn, p, x, idx):
    """blocks.py:34-43 followed by the block's relu(bn2(.)) (blocks.py:151), plain torch in the dtype of the modules, BatchNorms in
    training mode on batch statistics over (n, c, nsample) like the reference's transposes."""
    n, ns = idx.shape
    il = idx.long()
    x_q, x_k, x_v = layer.linear_q(x), layer.linear_k(x), layer.linear_v(x)
    p_r = p[il] - p.unsqueeze(1)                                              # queryandgroup(use_xyz=True) coordinates
    x_k = x_k[il]
    x_v = x_v[il]
    for i, m in enumerate(layer.linear_p):
        p_r = m(p_r.transpose(1, 2).contiguous()).transpose(1, 2).contiguous() if i == 1 else m(p_r)
    w = x_k - x_q.unsqueeze(1) + p_r
    for i, m in enumerate(layer.linear_w):
        w = m(w.transpose(1, 2).contiguous()).transpose(1, 2).contiguous() if i % 3 == 0 else m(w)
    w = torch.softmax(w, dim=1)
    s = layer.share_planes
    c = x_v.shape[2]
    out = ((x_v + p_r).view(n, ns, s, c // s) * w.unsqueeze(2)).sum(1).view(n, c)
    return F.relu(post_bn(out))


def _randomise_bn(mod, seed):
    g = torch.Generator().manual_seed(seed)
    for m in mod.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) * 1.5 + 0.5)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)


def _stage(dev, n, c, ns, seed):
    from toothgroupnetwork_amd import point_transformer as PT, synth
    torch.manual_seed(seed)
    layer = PT.PointTransformerLayer(c, c, 8, ns)
    bn2 = torch.nn.BatchNorm1d(c)
    _randomise_bn(layer, seed)
    _randomise_bn(bn2, seed + 1)
    p = torch.from_numpy(synth.arch_cloud(n, seed=seed, with_normals=False)).to(dev)
    x = torch.from_numpy(np.random.default_rng(seed).normal(size=(n, c)).astype(np.float32)).to(dev)
    return layer, bn2, p, x


_STAGES = [pytest.param(24000, 32, 36, id="stage1-n24000-c32"), pytest.param(6000, 64, 24, id="stage2-n6000-c64"),
           pytest.param(1500, 128, 24, id="stage3-n1500-c128"), pytest.param(375, 256, 24, id="stage4-n375-c256"),
           pytest.param(93, 512, 24, id="stage5-n93-c512")]


@pytest.mark.parametrize("n,c,ns", _STAGES)
def test_pt_layer_training_step_vs_float64(dev, n, c, ns):
    """the mirror layer in training mode with the block's bn2 + ReLU (kNN, _QueryGroup, _mlp_rows = split-K linears + bn_rows, the
    fused softmax aggregation, bn_rows(post_bn)): output, dL/dx, every parameter gradient and the running statistics after the step
    against a float64 restatement of blocks.py:34-43 on the same parameters and neighbour rows. Per tensor, the drop-in's distance
    from float64 is held to twice that of an fp32 torch restatement of the same layer, or 2e-5 of the tensor's norm, or (Linear
    parameters) the fp32 floor below, whichever is largest."""
    from toothgroupnetwork_amd import pointops as P
    layer, bn2, p, x = _stage(dev, n, c, ns, seed=n % 101 + c)
    mods = {}
    for name, dt in (("got", torch.float32), ("f32", torch.float32), ("f64", torch.float64)):
        mods[name] = (copy.deepcopy(layer).to(dev, dt).train(), copy.deepcopy(bn2).to(dev, dt).train())
    o = torch.tensor([n], dtype=torch.int32, device=dev)
    idx, _ = P.knnquery(ns, p, p, o, o)
    gy = torch.randn(n, c, device=dev, generator=torch.Generator(device=dev).manual_seed(n))
    seen = []                                          # (linear, input, output) of every Linear of the float64 run

    def keep(m, inp, out):
        out.retain_grad()
        seen.append((m, inp[0].detach(), out))
    hooks = [m.register_forward_hook(keep) for m in mods["f64"][0].modules() if isinstance(m, torch.nn.Linear)]
    res = {}
    for name, (lay, bn) in mods.items():
        dt = torch.float64 if name == "f64" else torch.float32
        xx = x.to(dt).clone().requires_grad_(True)
        if name == "got":
            y = lay([p, xx, o], post_bn=bn)
        else:
            y = _pt_layer_torch(lay, bn, p.to(dt), xx, idx)
        y.backward(gy.to(dt))
        t = {"out": y.detach(), "d_x": xx.grad}
        for mod_name, m in (("layer", lay), ("bn2", bn)):
            for k, prm in m.named_parameters():
                t[f"{mod_name}.{k}.grad"] = prm.grad
            for k, b in m.named_buffers():
                if b.dtype.is_floating_point:
                    t[f"{mod_name}.{k}"] = b.detach()
        res[name] = t
    for h in hooks:
        h.remove()
    got, f32, f64 = res["got"], res["f32"], res["f64"]
    assert sorted(got) == sorted(f64)
    # fp32 floor of a Linear's parameter gradients, a sum over all rows (n or n * nsample): 8 u of the float64 sums of absolute terms,
    # sum_r |dz_r| for the bias and |dz|^T |x| for the weight. It matters where the exact gradient is zero -- a bias in front of a
    # BatchNorm -- and what either fp32 run holds is the rounding residue of that sum.
    names = {id(m): f"layer.{k}" for k, m in mods["f64"][0].named_modules()}
    floor = {}
    with torch.no_grad():
        for m, inp, out in seen:
            dz = out.grad.reshape(-1, m.out_features).abs()
            floor[names[id(m)] + ".bias.grad"] = 8 * U32 * float(dz.sum(0).norm())
            floor[names[id(m)] + ".weight.grad"] = 8 * U32 * float((dz.t() @ inp.reshape(-1, m.in_features).abs()).norm())
    assert len(floor) == 2 * 7, sorted(floor)
    rows = []
    for k in sorted(f64):
        e = f64[k]
        assert got[k] is not None and torch.isfinite(got[k]).all(), k
        d_got = float((got[k].double() - e).norm())
        d_own = float((f32[k].double() - e).norm())
        norm = float(e.norm())
        lim = max(2.0 * d_own, 2e-5 * norm, floor.get(k, 0.0))
        rows.append((k, d_got, d_own, norm, lim))
    print("\n" + "\n".join(f"{k:38s} |got-exact| {a:.3e}  |fp32-exact| {b:.3e}  |exact| {nm:.3e}  bound {l:.3e}"
                           for k, a, b, nm, l in rows))
    over = [r for r in rows if r[1] > r[4]]
    assert not over, over


@pytest.mark.parametrize("n,c,ns,fused", [pytest.param(6000, 64, 24, True, id="stage2-fused_eval_kernel"),
                                          pytest.param(1500, 128, 24, True, id="stage3-fused_eval_kernel"),
                                          pytest.param(375, 256, 24, False, id="stage4-deep-composition"),
                                          pytest.param(93, 512, 24, False, id="stage5-deep-composition")])
def test_block_without_parameter_gradients_takes_the_branch_frozen_selects(dev, monkeypatch, n, c, ns, fused):
    """a PointTransformerBlock in eval mode whose parameters do not require a gradient, run with grad enabled: _frozen holds, so the
    layer takes the fused eval kernel (tgn_pt_attention_forward) unless the stage is one of the deep ones, where it keeps the
    composition. Either way the output equals the same block's training composition (parameters requiring grad, BN in eval) to
    fp32 rounding."""
    from toothgroupnetwork_amd import fold, point_transformer as PT
    layer, bn2, p, x = _stage(dev, n, c, ns, seed=n % 53 + c)
    torch.manual_seed(n)
    blk = PT.PointTransformerBlock(c, c, 8, ns)
    blk.transformer2.load_state_dict(layer.state_dict())
    _randomise_bn(blk, n)
    blk = blk.to(dev).eval()
    o = torch.tensor([n], dtype=torch.int32, device=dev)
    calls = {"fused": 0, "tail": 0}
    real_fused, real_tail = PT.pt_attention, PT.pt_softmax_aggregate

    def fused_spy(*a, **k):
        calls["fused"] += 1
        return real_fused(*a, **k)

    def tail_spy(*a, **k):
        calls["tail"] += 1
        return real_tail(*a, **k)
    monkeypatch.setattr(PT, "pt_attention", fused_spy)
    monkeypatch.setattr(PT, "pt_softmax_aggregate", tail_spy)
    with torch.enable_grad():
        y_train = blk([p, x, o])[1]                                       # parameters require grad: the composition
        assert calls == {"fused": 0, "tail": 1} and y_train.requires_grad
        for q in blk.parameters():
            q.requires_grad_(False)
        assert fold.frozen(blk.transformer2, p, x)
        y_frozen = blk([p, x, o])[1]
    assert not y_frozen.requires_grad
    assert calls == ({"fused": 1, "tail": 1} if fused else {"fused": 0, "tail": 2}), calls
    want = y_train.detach().double()
    err = float((y_frozen.double() - want).abs().max())
    assert err <= 2e-5 * max(1.0, float(want.abs().max())), err


# ---------------------------------------------------------------------------------------------------------------------------
# 3. PointNet++ backward scatters
# ---------------------------------------------------------------------------------------------------------------------------
def _group_exact(xyz, new_xyz, points, idx, go, xyz_first):
    """float64 autograd of the two grouping lines (pointnet2_utils.py:162-169 / 281-285) by fancy indexing (negative indices wrap),
    and the sums of absolute terms of each gradient."""
    B, S, K = idx.shape
    il = idx.long()
    bi = torch.arange(B, device=idx.device).view(B, 1, 1)
    x, nx = xyz.detach().double().requires_grad_(True), new_xyz.detach().double().requires_grad_(True)
    pt = None if points is None else points.detach().double().requires_grad_(True)
    rel = x[bi, il] - nx.unsqueeze(2)
    parts = [rel] if pt is None else ([rel, pt[bi, il]] if xyz_first else [pt[bi, il], rel])
    out = torch.cat(parts, -1)
    G = go.double()
    out.backward(G)
    D = 0 if points is None else points.shape[2]
    g_rel = G[..., :3] if xyz_first else G[..., D:]
    N = xyz.shape[1]
    flat = (il % N + bi * N).reshape(-1)
    ab = {"xyz": torch.zeros(B * N, 3, dtype=torch.float64, device=go.device).index_add_(0, flat, g_rel.abs().reshape(-1, 3)).view(B, N, 3),
          "new_xyz": g_rel.abs().sum(2)}
    gr = {"xyz": x.grad, "new_xyz": nx.grad}
    if D:
        g_f = G[..., 3:] if xyz_first else G[..., :D]
        ab["points"] = torch.zeros(B * N, D, dtype=torch.float64, device=go.device).index_add_(0, flat, g_f.abs().reshape(-1, D)).view(B, N, D)
        gr["points"] = pt.grad
    return out.detach(), gr, ab


def _ball_query_setup(dev, B, N, S, K, D, seed):
    from toothgroupnetwork_amd import pointnet2_utils as U, synth
    rng = np.random.default_rng(seed)
    xyz = np.stack([synth.arch_cloud(N, seed=seed + b, with_normals=False) for b in range(B)])
    centres = np.stack([xyz[b, rng.choice(N, S, replace=False)] for b in range(B)])   # points of the cloud: every ball holds its centre
    radius = 0.05 * (6000.0 / N) ** 0.5                                              # ~12 points of 32: most rows padded
    xyz_t, new_t = torch.from_numpy(xyz).to(dev), torch.from_numpy(centres).to(dev)
    idx = U.query_ball_point(radius, K, xyz_t, new_t)
    padded = float((idx[..., -1] == idx[..., 0]).float().mean())
    assert padded > 0.5, padded
    pts = torch.from_numpy(rng.normal(size=(B, N, D)).astype(np.float32)).to(dev) if D else None
    return xyz_t, new_t, pts, idx


_GROUP_SHAPES = [pytest.param(2, 6000, 1024, 32, 0, id="B2-N6000-S1024-K32-D0"),
                 pytest.param(2, 6000, 1024, 32, 64, id="B2-N6000-S1024-K32-D64"),
                 pytest.param(1, 24000, 4096, 32, 6, id="B1-N24000-S4096-K32-D6")]


@pytest.mark.parametrize("B,N,S,K,D", _GROUP_SHAPES)
@pytest.mark.parametrize("xyz_first", [True, False], ids=["xyz_first", "points_first"])
@pytest.mark.parametrize("itype", [torch.int64, torch.int32], ids=["int64", "int32"])
@pytest.mark.parametrize("neg", [False, True], ids=["nonneg", "negative_idx"])
def test_group_points_backward_vs_float64(dev, B, N, S, K, D, xyz_first, itype, neg):
    """ball-query rows padded with their first neighbour (most rows of these balls), scattered back into xyz / points; with
    'negative_idx' a third of the entries is replaced by idx - N, which the forward wraps and so must the backward."""
    from toothgroupnetwork_amd import pointnet2_utils as U
    xyz, new_xyz, pts, idx = _ball_query_setup(dev, B, N, S, K, D, seed=B * 7 + D)
    if neg:
        sel = torch.rand(idx.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) < 0.33
        idx = torch.where(sel, idx - N, idx)
        assert bool((idx < 0).any())
    idx = idx.to(itype)
    x, nx = xyz.clone().requires_grad_(True), new_xyz.clone().requires_grad_(True)
    pt = None if pts is None else pts.clone().requires_grad_(True)
    out = U.group_points(x, nx, pt, idx, xyz_first=xyz_first)
    go = torch.randn(out.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(S))
    out.backward(go)
    want, grads, ab = _group_exact(xyz, new_xyz, pts, idx, go, xyz_first)
    _within(out, want, want.abs(), "out")                         # a gather, and one rounded subtraction for the coordinates
    _within(x.grad, grads["xyz"], ab["xyz"], "d_xyz")
    _within(nx.grad, grads["new_xyz"], ab["new_xyz"], "d_new_xyz")
    if D:
        _within(pt.grad, grads["points"], ab["points"], "d_points")


@pytest.mark.parametrize("want", ["all", "points_only", "new_xyz_only"])
@pytest.mark.parametrize("xyz_first", [True, False], ids=["xyz_first", "points_first"])
def test_group_points_backward_with_some_inputs_requiring_grad(dev, want, xyz_first):
    """gradients requested for a subset of the inputs: those get the float64 gradient, the others none."""
    from toothgroupnetwork_amd import pointnet2_utils as U
    B, N, S, K, D = 2, 6000, 1024, 32, 64
    xyz, new_xyz, pts, idx = _ball_query_setup(dev, B, N, S, K, D, seed=41)
    req = {"all": (True, True, True), "points_only": (False, False, True), "new_xyz_only": (False, True, False)}[want]
    x, nx, pt = (t.clone().requires_grad_(r) for t, r in zip((xyz, new_xyz, pts), req))
    out = U.group_points(x, nx, pt, idx, xyz_first=xyz_first)
    go = torch.randn(out.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(43))
    out.backward(go)
    _, grads, ab = _group_exact(xyz, new_xyz, pts, idx, go, xyz_first)
    for (name, t), r in zip((("xyz", x), ("new_xyz", nx), ("points", pt)), req):
        if r:
            _within(t.grad, grads[name], ab[name], f"d_{name}")
        else:
            assert t.grad is None, name


@pytest.mark.parametrize("shape", [pytest.param((2, 1500), id="idx_BS"), pytest.param((2, 1024, 16), id="idx_BSK")])
@pytest.mark.parametrize("itype", [torch.int64, torch.int32], ids=["int64", "int32"])
def test_index_points_backward_vs_float64(dev, shape, itype):
    """indices drawn from a tenth of the cloud (every row repeated ~5 - 50 times), a third of them negative (idx - N)."""
    from toothgroupnetwork_amd import pointnet2_utils as U
    B, N, C = shape[0], 3000, 67
    gen = torch.Generator(device=dev).manual_seed(len(shape))
    points = torch.randn(B, N, C, device=dev, generator=gen)
    idx = torch.randint(0, N // 10, shape, device=dev, generator=gen)
    idx = torch.where(torch.rand(shape, device=dev, generator=gen) < 0.33, idx - N, idx).to(itype)
    p = points.clone().requires_grad_(True)
    out = U.index_points(p, idx)
    go = torch.randn(out.shape, device=dev, generator=gen)
    out.backward(go)
    il = idx.long()
    bi = torch.arange(B, device=dev).view(B, *([1] * (len(shape) - 1)))
    p64 = points.double().requires_grad_(True)
    ref = p64[bi, il]
    ref.backward(go.double())
    assert torch.equal(out.detach().double(), ref.detach())
    flat = (il % N + bi * N).reshape(-1)
    ab = torch.zeros(B * N, C, dtype=torch.float64, device=dev).index_add_(0, flat, go.double().abs().reshape(-1, C)).view(B, N, C)
    _within(p.grad, p64.grad, ab, "d_points")


def _interp_setup(dev, B, N, S, C, seed):
    from toothgroupnetwork_amd import pointnet2_utils as U, synth
    xyz1 = torch.from_numpy(np.stack([synth.arch_cloud(N, seed=seed + b, with_normals=False) for b in range(B)])).to(dev)
    xyz2 = torch.from_numpy(np.stack([synth.arch_cloud(S, seed=seed + 100 + b, with_normals=False) for b in range(B)])).to(dev)
    dist, idx = U.three_nn(xyz1, xyz2)
    # the expanded-form distance of a query on top of a support point can come out a rounding below zero; the network feeds it as
    # it is, here it is clamped so that the weights stay positive and the bound below is about the scatter, not a cancelling norm
    dist = dist.clamp_min(0.0)
    feats = torch.randn(B, S, C, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
    return feats, dist, idx


@pytest.mark.parametrize("B,N,S,C", [pytest.param(2, 24000, 6000, 128, id="B2-N24000-S6000-C128"),
                                     pytest.param(3, 1500, 375, 256, id="B3-N1500-S375-C256"),
                                     pytest.param(2, 500, 2, 16, id="B2-S2-padded"),
                                     pytest.param(3, 300, 1, 8, id="B3-S1-padded")])
@pytest.mark.parametrize("itype", [torch.int64, torch.int32], ids=["int64", "int32"])
def test_three_interpolate_backward_vs_float64(dev, B, N, S, C, itype):
    """inverse-distance weights of the three nearest support points (S < 3: three_nn pads with index 0 at infinite distance, weight
    0); B > 1 checks the per-batch row offset of the backward's scatter."""
    from toothgroupnetwork_amd import pointnet2_utils as U
    feats, dist, idx = _interp_setup(dev, B, N, S, C, seed=B * 13 + S)
    if S < 3:
        assert bool((idx[..., S:] == 0).all()) and bool(torch.isinf(dist[..., S:]).all())
    idx = idx.to(itype)
    f = feats.clone().requires_grad_(True)
    out = U.three_interpolate(f, dist, idx)
    go = torch.randn(out.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(N))
    out.backward(go)
    f64 = feats.double().requires_grad_(True)
    r = 1.0 / (dist.double() + 1e-8)
    w = r / r.sum(-1, keepdim=True)                                              # pointnet2_utils.py:337-339
    bi = torch.arange(B, device=dev).view(B, 1, 1)
    il = idx.long()
    terms = f64[bi, il] * w.unsqueeze(-1)                                         # (B, N, 3, C)
    ref = terms.sum(2)
    ref.backward(go.double())
    _within(out, ref.detach(), terms.detach().abs().sum(2), "out")
    gterms = (go.double().unsqueeze(2) * w.unsqueeze(-1)).abs()                  # (B, N, 3, C)
    ab = torch.zeros(B * S, C, dtype=torch.float64, device=dev).index_add_(0, (il + bi * S).reshape(-1), gterms.reshape(-1, C))
    _within(f.grad, f64.grad, ab.view(B, S, C), "d_points2")
