"""toothgroupnetwork_amd.losses on the GPU: the fused offset / direction / chamfer terms of tgnet_fps and tsegnet's centroid_loss against
the reference's own float32 and float64 runs (tests/golden/reference_cpu_r12_losses.npz), against the float64 restatement
tests/losses_ref.py on inputs the fixture lacks, and the properties the kernels promise: defined edge cases, every input form,
bit-equal repeats, graph capture, and FpsGroupingNetworkModel.get_loss's terms on the reference module case.

Bounds.  A loss value g with float64 value a and reference float32 value b: |g - a| <= max(2 |b - a|, 2e-5 |a|), what
test_gpu_grouping_network.py holds loss terms to.  A gradient: e = |got - exact| / max|exact| (the largest magnitude normalises because
these gradients carry a 1 / n, which an absolute floor would hide); rms(e) <= max(2 rms(e_ref32), 1e-6) and max(e) <= max(4 max(e_ref32), 1e-5),
the factors and floors of _within_reference_noise there.  Without a reference float32 run (the sweep) the floors alone hold."""
import os
import sys

import numpy as np
import pytest
import torch

import losses_ref as R
from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
from seeded import seeded_fill  # noqa: E402

pytestmark = pytest.mark.gpu

TGN_NAMES = ("offset_loss", "dir_loss", "chamf_loss")
TSG_NAMES = ("dist_loss", "cent_loss", "chamf_loss")


@pytest.fixture(scope="module")
def golden_r12():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r12_losses.npz")))


@pytest.fixture(scope="module")
def golden_r7():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r7_grouping.npz")))


def _L():
    from toothgroupnetwork_amd import losses
    return losses


# ---- the bounds --------------------------------------------------------------------------------------------------------------

def _check_loss(name, got, exact, ref32=None):
    own = abs(ref32 - exact) if ref32 is not None else 0.0
    print(f"  {name}: got {got:.9g} exact {exact:.9g} |got - exact| {abs(got - exact):.3e} reference fp32's {own:.3e}")
    assert abs(got - exact) <= max(2.0 * own, 2e-5 * abs(exact)), (name, got, exact, ref32)


def _check_grad(name, got, exact, ref32=None):
    got, exact = np.asarray(got, np.float64), np.asarray(exact, np.float64)
    assert got.shape == exact.shape, (name, got.shape, exact.shape)
    scale = float(np.max(np.abs(exact)))
    if scale == 0.0:
        assert not got.any(), name
        return
    e = np.abs(got - exact) / scale
    own = np.abs(np.asarray(ref32, np.float64) - exact) / scale if ref32 is not None else np.zeros(1)
    e_rms, e_max, own_rms, own_max = float(np.sqrt(np.mean(e ** 2))), float(e.max()), float(np.sqrt(np.mean(own ** 2))), float(own.max())
    print(f"  grad {name}: rms {e_rms:.3e} max {e_max:.3e}   reference fp32: rms {own_rms:.3e} max {own_max:.3e}")
    assert e_rms <= max(2.0 * own_rms, 1e-6), (name, "rms", e_rms, own_rms)
    assert e_max <= max(4.0 * own_max, 1e-5), (name, "max", e_max, own_max)


def _term_grads(terms, wrt):
    """per term its gradient with respect to wrt (zeros where the term does not depend on it)"""
    out = []
    for t in terms:
        g = torch.autograd.grad(t, wrt, retain_graph=True, allow_unused=True)[0]
        out.append((torch.zeros_like(wrt) if g is None else g).detach().double().cpu().numpy())
    return np.stack(out)


# ---- inputs the fixture lacks ------------------------------------------------------------------------------------------------------

def tgn_inputs(B, N, seed):
    """Labelled arch scans (2 to 14 teeth, about 30 points a tooth at least) with offsets that point roughly at the tooth centroids and
    every fifth one scaled to norm 1e-4.  Whether norms, counts and ratios stay off the thresholds is for the caller to assert
    (losses_ref.tgn_margins)."""
    from toothgroupnetwork_amd import synth
    rng = np.random.default_rng(seed)
    xyz, lab = [], []
    for b in range(B):
        rows, labels = synth.labelled_arch(N, max(2, min(14, N // 100)), seed=seed + b)
        xyz.append(rows[:, :3].T.copy()), lab.append(labels)
    xyz, lab = np.stack(xyz).astype(np.float32), np.stack(lab).astype(np.int64)
    off = np.zeros_like(xyz)
    for b in range(B):
        for t in range(16):
            m = lab[b] == t
            if m.any():
                off[b][:, m] = 0.6 * (xyz[b][:, m].mean(1, keepdims=True) - xyz[b][:, m])
    off += rng.normal(scale=0.02, size=off.shape).astype(np.float32)
    small = np.arange(0, N, 5)
    v = off[:, :, small].astype(np.float64)
    off[:, :, small] = (v / np.linalg.norm(v, axis=1, keepdims=True) * 1e-4).astype(np.float32)
    return torch.from_numpy(off), torch.from_numpy(xyz), torch.from_numpy(lab)


def tsg_inputs(B, M, C, seed):
    gen = torch.Generator().manual_seed(seed)
    cent = torch.rand(B, 3, C, generator=gen) * 1.2 - 0.6
    pick = torch.randint(0, C, (B, M), generator=gen)
    xyz = torch.gather(cent, 2, pick[:, None, :].expand(B, 3, M)) + 0.25 * torch.randn(B, 3, M, generator=gen)
    near = ((xyz[:, :, :, None] - cent[:, :, None, :]) ** 2).sum(1).min(2)
    target = torch.gather(cent, 2, near[1][:, None, :].expand(B, 3, M))
    off = 0.7 * (target - xyz) + 0.03 * torch.randn(B, 3, M, generator=gen)
    dist = near[0].sqrt() + 0.08 * torch.randn(B, M, generator=gen)
    return off, xyz, dist.view(B, 1, M), cent


def _run_tgn(dev, off, xyz, lab):
    o = off.to(dev).requires_grad_()
    terms = _L().tgn_offset_losses(o, xyz.to(dev), lab.to(dev))
    return [float(t.detach()) for t in terms], _term_grads(terms, o)


def _run_tsg(dev, off, xyz, dist, cent, exists=None):
    o, d = off.to(dev).requires_grad_(), dist.to(dev).requires_grad_()
    terms = _L().centroid_loss(o, xyz.to(dev), d, cent.to(dev), None if exists is None else exists.to(dev))
    return [float(t.detach()) for t in terms], _term_grads(terms, o), _term_grads(terms, d)


# ---- 1. reference parity -------------------------------------------------------------------------------------------------------

def test_tgn_terms_match_the_reference(dev, golden_r12):
    g = golden_r12
    vals, grads = _run_tgn(dev, torch.from_numpy(g["tgn_offset"]), torch.from_numpy(g["tgn_xyz"]), torch.from_numpy(g["tgn_labels"]).long())
    print("\ntgn fixture (B = 2, N = 1500):")
    for i, n in enumerate(TGN_NAMES):
        _check_loss(n, vals[i], g["tgn_loss_64"][i], g["tgn_loss_32"][i])
    for i, n in enumerate(TGN_NAMES):
        _check_grad(n, grads[i], g["tgn_grad_64"][i], g["tgn_grad_32"][i])


@pytest.mark.parametrize("key", ["tsg", "tsx"])
def test_centroid_terms_match_the_reference(dev, golden_r12, key):
    g = golden_r12
    exists = torch.from_numpy(g[f"{key}_exists"]) if f"{key}_exists" in g else None
    vals, g_off, g_dist = _run_tsg(dev, *(torch.from_numpy(g[f"{key}_{n}"]) for n in ("offset", "xyz", "distance", "centroid")), exists)
    print(f"\n{key} fixture {g[f'{key}_offset'].shape}, C = {g[f'{key}_centroid'].shape[2]}:")
    for i, n in enumerate(TSG_NAMES):
        _check_loss(n, vals[i], g[f"{key}_loss_64"][i], g[f"{key}_loss_32"][i])
    for i, n in enumerate(TSG_NAMES):
        _check_grad(f"{n} / offset", g_off[i], g[f"{key}_grad_offset_64"][i], g[f"{key}_grad_offset_32"][i])
    _check_grad("dist_loss / distance", g_dist[0], g[f"{key}_grad_distance_64"], g[f"{key}_grad_distance_32"])
    assert not g_dist[1:].any()


# ---- 2. restatement sweep ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [64, 65, 1000, 6000])
def test_tgn_terms_match_the_restatement(dev, B, N):
    off, xyz, lab = tgn_inputs(B, N, seed=500 + N + B)
    mg = R.tgn_margins(off, xyz, lab)
    assert mg["norm"] >= 5e-5 and mg["ratio_gap"] >= 1e-4 and not bool(((mg["counts"] >= 4) & (mg["counts"] <= 6)).any()), mg
    vals, grads = _run_tgn(dev, off, xyz, lab)
    o64 = off.double().requires_grad_()
    exact = R.tgn_terms(o64, xyz.double(), lab)
    exact_g = _term_grads(exact, o64)
    print(f"\ntgn B = {B}, N = {N}:")
    for i, n in enumerate(TGN_NAMES):
        _check_loss(n, vals[i], float(exact[i].detach()))
        _check_grad(n, grads[i], exact_g[i])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [2, 16])
@pytest.mark.parametrize("M", [1, 63, 320])
def test_centroid_terms_match_the_restatement(dev, B, C, M):
    for seed in range(900 + 7 * M + C + B, 1000 + 7 * M + C + B):   # the first seed whose inputs keep their margins (host arithmetic only)
        off, xyz, dist, cent = tsg_inputs(B, M, C, seed)
        mg = R.centroid_margins(off, xyz, dist.view(B, M), cent)
        if mg["mask"] >= 1e-3 and mg["ratio_gap"] >= 1e-4 and mg["arg_gap"] >= 1e-4:
            break
    else:
        raise AssertionError("no seed keeps the margins")
    vals, g_off, g_dist = _run_tsg(dev, off, xyz, dist, cent)
    o64, d64 = off.double().requires_grad_(), dist.double().view(B, M).requires_grad_()
    exact = R.centroid_terms(o64, xyz.double(), d64, cent.double())
    print(f"\ntsg B = {B}, M = {M}, C = {C} (seed {seed}):")
    for i, n in enumerate(TSG_NAMES):
        a = float(exact[i].detach())
        if np.isnan(a):
            assert np.isnan(vals[i]), (n, vals[i])
            continue
        _check_loss(n, vals[i], a)
    eg = _term_grads(exact, o64)
    for i, n in enumerate(TSG_NAMES):
        _check_grad(f"{n} / offset", g_off[i], eg[i])
    _check_grad("dist_loss / distance", g_dist[0].reshape(B, M), _term_grads(exact[:1], d64)[0])


# ---- 3. edge cases -------------------------------------------------------------------------------------------------------------

def _take_error():
    from toothgroupnetwork_amd import _lib
    return _lib.lib().tgn_take_index_error(_lib.stream())


def test_all_gingiva_gives_nan_losses_and_a_zero_gradient(dev):
    off, xyz, lab = tgn_inputs(2, 300, seed=3)
    o = off.to(dev).requires_grad_()
    terms = _L().tgn_offset_losses(o, xyz.to(dev), torch.full_like(lab, -1).to(dev))
    assert all(bool(torch.isnan(t)) for t in terms)
    grads = _term_grads(terms, o)
    assert np.isfinite(grads).all() and not grads.any()


def test_one_valid_tooth_gives_a_nan_chamfer_term_only(dev):
    off, xyz, lab = tgn_inputs(1, 300, seed=4)
    lab = torch.where(lab == 1, lab, torch.full_like(lab, -1))
    assert int((lab == 1).sum()) >= 7
    o = off.to(dev).requires_grad_()
    terms = _L().tgn_offset_losses(o, xyz.to(dev), lab.to(dev))
    assert bool(torch.isfinite(terms[0])) and bool(torch.isfinite(terms[1])) and bool(torch.isnan(terms[2]))
    o64 = off.double().requires_grad_()
    exact = R.tgn_terms(o64, xyz.double(), lab)
    _check_loss("offset_loss", float(terms[0]), float(exact[0]))
    _check_loss("dir_loss", float(terms[1]), float(exact[1]))
    assert np.isfinite(_term_grads(terms, o)).all()


def test_zero_offsets_give_finite_gradients_without_a_direction_part(dev):
    """where the reference's autograd gives NaN (0 / 0 in the backward of the division of the rows it then drops)"""
    off, xyz, lab = tgn_inputs(2, 500, seed=5)
    off[:, :, ::3] = 0.0
    mg = R.tgn_margins(off, xyz, lab)
    assert mg["norm"] >= 5e-5 and mg["ratio_gap"] >= 1e-4 and not bool(((mg["counts"] >= 4) & (mg["counts"] <= 6)).any()), mg
    o = off.to(dev).requires_grad_()
    terms = _L().tgn_offset_losses(o, xyz.to(dev), lab.to(dev))
    grads = _term_grads(terms, o)
    assert np.isfinite(grads).all() and all(bool(torch.isfinite(t)) for t in terms)
    assert not grads[1][:, :, ::3].any() and grads[1].any() and grads[0][:, :, ::3].any()
    o64 = off.double().requires_grad_()
    exact = R.tgn_terms(o64, xyz.double(), lab)
    eg = _term_grads(exact, o64)
    for i, n in enumerate(TGN_NAMES):
        _check_loss(n, float(terms[i]), float(exact[i]))
        _check_grad(n, grads[i], eg[i])


def test_an_empty_distance_mask_gives_a_nan_cent_loss(dev):
    off, xyz, dist, cent = tsg_inputs(2, 63, 5, seed=6)
    o, d = off.to(dev).requires_grad_(), (dist.abs() + 0.3).to(dev).requires_grad_()
    terms = _L().centroid_loss(o, xyz.to(dev), d, cent.to(dev))
    assert bool(torch.isfinite(terms[0])) and bool(torch.isnan(terms[1])) and bool(torch.isfinite(terms[2]))
    assert np.isfinite(_term_grads(terms, o)).all() and np.isfinite(_term_grads(terms, d)).all()


def test_a_label_of_16_is_reported_not_read(dev):
    off, xyz, lab = tgn_inputs(1, 300, seed=7)
    _take_error()
    good = [float(t) for t in _L().tgn_offset_losses(off.to(dev), xyz.to(dev), lab.to(dev))]
    assert _take_error() == 0
    bad = lab.clone()
    bad[0, 17] = 16
    got = [float(t) for t in _L().tgn_offset_losses(off.to(dev), xyz.to(dev), bad.to(dev))]
    from toothgroupnetwork_amd import _lib
    assert _take_error() & _lib.INDEX_ERROR_CROP
    assert np.isfinite(got).all() and np.isfinite(good).all()
    assert _take_error() == 0


# ---- 4. forms ------------------------------------------------------------------------------------------------------------------

def _forms(base):
    """(name, tensor holding the values of `base` in another form, the float32 values the kernel should see)"""
    B, _, N = base.shape
    big = torch.zeros(B * 3 * N + 5, device=base.device)
    big[5:] = base.reshape(-1)
    yield "permuted", base.permute(0, 2, 1).contiguous().permute(0, 2, 1), base
    yield "offset", big[5:].view(B, 3, N), base
    yield "fp64", base.double(), base
    yield "bf16", base.bfloat16(), base.bfloat16().float()


def test_offset_forms_give_the_bits_of_the_packed_call(dev):
    off, xyz, lab = (t.to(dev) for t in tgn_inputs(2, 333, seed=8))
    for name, form, packed in _forms(off):
        assert form.shape == off.shape and (name != "permuted" or not form.is_contiguous())
        a, b = form.requires_grad_(), packed.clone().requires_grad_()
        assert name != "offset" or a.storage_offset() == 5
        ta, tb = _L().tgn_offset_losses(a, xyz, lab), _L().tgn_offset_losses(b, xyz, lab)
        for x, y in zip(ta, tb):
            assert torch.equal(x, y), name
        (0.5 * ta[0] + ta[1] + 0.25 * ta[2]).backward()
        (0.5 * tb[0] + tb[1] + 0.25 * tb[2]).backward()
        assert a.grad.dtype == a.dtype and a.grad.shape == a.shape and a.grad.stride() == a.stride(), name
        assert torch.equal(a.grad, b.grad.to(a.dtype)), name
    ti = _L().tgn_offset_losses(off, xyz, lab.int())
    tl = _L().tgn_offset_losses(off, xyz.double(), lab.view(2, 1, -1))
    for x, y, z in zip(ti, tl, _L().tgn_offset_losses(off, xyz, lab)):
        assert torch.equal(x, z) and torch.equal(y, z)
    o = off.clone().requires_grad_()
    pair, chamf = _L().batch_center_offset_loss(o, xyz, lab), _L().batch_chamfer_distance_loss(o, xyz, lab)
    for x, y in zip((*pair, chamf), _L().tgn_offset_losses(off, xyz, lab)):
        assert torch.equal(x.detach(), y)


def test_centroid_loss_forms_give_the_bits_of_the_packed_call(dev):
    off, xyz, dist, cent = (t.to(dev) for t in tsg_inputs(2, 63, 7, seed=9))
    exists = torch.ones(2, 7, dtype=torch.bool, device=dev)
    exists[1, 3] = False
    for name, form, packed in _forms(off):
        a, b = form.requires_grad_(), packed.clone().requires_grad_()
        da, db = dist.view(2, 63).double().requires_grad_(), dist.clone().requires_grad_()
        ta = _L().centroid_loss(a, xyz, da, cent.double(), exists)
        tb = _L().centroid_loss(b, xyz, db, cent, exists)
        for x, y in zip(ta, tb):
            assert torch.equal(x, y), name
        sum(ta).backward(), sum(tb).backward()
        assert a.grad.dtype == a.dtype and a.grad.stride() == a.stride() and torch.equal(a.grad, b.grad.to(a.dtype)), name
        assert da.grad.dtype == torch.float64 and da.grad.shape == (2, 63) and torch.equal(da.grad.float().view(2, 1, 63), db.grad), name


def test_autocast_keeps_the_losses_in_float32(dev):
    off, xyz, lab = (t.to(dev) for t in tgn_inputs(1, 333, seed=10))
    o = off.bfloat16().requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        terms = _L().tgn_offset_losses(o, xyz, lab)
    want = _L().tgn_offset_losses(off.bfloat16().float(), xyz, lab)
    assert all(t.dtype == torch.float32 and torch.equal(t.detach(), w) for t, w in zip(terms, want))
    sum(terms).backward()
    assert o.grad.dtype == torch.bfloat16 and bool(torch.isfinite(o.grad).all())


# ---- 5. determinism, 6. graph ---------------------------------------------------------------------------------------------------

def _tgn_step(o, xyz, lab):
    terms = _L().tgn_offset_losses(o, xyz, lab)
    grad, = torch.autograd.grad(terms[0] + 0.5 * terms[1] + 0.25 * terms[2], o)
    return torch.stack(terms).detach(), grad


def _tsg_step(o, d, xyz, cent, exists):
    terms = _L().centroid_loss(o, xyz, d, cent, exists)
    go, gd = torch.autograd.grad(terms[0] + terms[1] + 0.1 * terms[2], (o, d))
    return torch.stack(terms).detach(), go, gd


def test_two_calls_give_the_same_bits(dev):
    off, xyz, lab = (t.to(dev) for t in tgn_inputs(3, 6000, seed=11))
    o = off.requires_grad_()
    first, again = _tgn_step(o, xyz, lab), _tgn_step(o, xyz, lab)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    off, xyz, dist, cent = (t.to(dev) for t in tsg_inputs(3, 320, 16, seed=12))
    o, d = off.requires_grad_(), dist.requires_grad_()
    first, again = _tsg_step(o, d, xyz, cent, None), _tsg_step(o, d, xyz, cent, None)
    assert all(torch.equal(a, b) for a, b in zip(first, again))


def test_forward_and_backward_replay_as_a_graph(dev):
    off, xyz, lab = (t.to(dev) for t in tgn_inputs(2, 1000, seed=13))
    off2, xyz2, dist2, cent2 = (t.to(dev) for t in tsg_inputs(2, 320, 14, seed=14))
    exists = torch.ones(2, 14, dtype=torch.bool, device=dev)
    exists[0, 5] = False
    o, o2, d2 = off.requires_grad_(), off2.requires_grad_(), dist2.requires_grad_()

    def step():
        return _tgn_step(o, xyz, lab) + _tsg_step(o2, d2, xyz2, cent2, exists)
    eager = [t.clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                       # allocator and error-word warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = step()
    for _ in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(captured, eager))


# ---- 7. the model-level check ----------------------------------------------------------------------------------------------------

CONFIG = {"model_parameter": {"input_feat": 6, "stride": [1, 4, 4, 4, 4], "nsample": [36, 24, 24, 24, 24], "blocks": [2, 3, 4, 6, 3],
                              "block_num": 5, "planes": [32, 64, 128, 256, 512], "crop_sample_size": 3072}}   # train_configs/tgnet_fps.py
WEIGHTS = (1.0, 1.0, 0.03, 0.03, 0.15)


def test_grouping_loss_terms_on_the_reference_module_case(dev, golden_r7):
    from crop_cases import digest
    from toothgroupnetwork_amd import nets, synth
    net = nets.GroupingNetworkModule(CONFIG)
    assert seeded_fill(net, 71) == golden_r7["mod_params"].tolist()
    net = net.to(dev).train()
    N = int(golden_r7["mod_points"][0])
    rows, labels = synth.labelled_arch(N, 14, seed=int(golden_r7["mod_seed"][0]))
    assert digest(rows, labels) == golden_r7["mod_digest"][0], "the scan no longer rebuilds the fixture's input"
    feats, gt = torch.from_numpy(np.ascontiguousarray(rows.T))[None].to(dev), torch.from_numpy(labels).to(dev)
    before = gt.clone()
    with torch.no_grad():
        o = net([feats, gt.view(1, 1, -1)])
    terms = _L().grouping_loss_terms(o, gt.view(1, 1, -1), feats[:, :3, :])
    assert torch.equal(gt, before), "gt_seg_label was modified"
    names = golden_r7["mod_term_names"].tolist()
    assert names[0] == "loss" and list(terms) == names[1:]
    got = [float(terms[n]) for n in terms]
    got = [sum(w * v for w, v in zip(WEIGHTS, got))] + got
    t64, t32 = golden_r7["mod_terms_64"], golden_r7["mod_terms_32"]
    print(f"\nloss terms {names}: fused {got}, reference fp64 {t64.tolist()}, reference fp32 {t32.tolist()}")
    for n, g, a, b in zip(["total"] + list(terms), got, t64, t32):
        _check_loss(n, g, float(a), float(b))
