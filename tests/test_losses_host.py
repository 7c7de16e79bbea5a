"""CPU: the float64 restatement of the loss formulas (tests/losses_ref.py) reproduces the reference's own float64 values and gradients
(tests/golden/reference_cpu_r12_losses.npz, made by tests/golden/make_golden_r12_losses.py), the fixture's inputs keep the margins that
make a float32-against-float64 comparison meaningful, and toothgroupnetwork_amd.losses refuses what it cannot take before it touches
the library."""
import os

import numpy as np
import pytest
import torch

import losses_ref as R
from conftest import GOLDEN

REL = 1e-12


@pytest.fixture(scope="module")
def golden_r12():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r12_losses.npz")))


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.max(np.abs(got - want))) / float(np.max(np.abs(want)))
    assert err <= REL, (what, err)


def _grads(terms, wrt):
    return np.stack([torch.autograd.grad(t, wrt, retain_graph=True, allow_unused=True)[0].numpy() for t in terms])


def test_restatement_reproduces_the_reference_tgn_terms(golden_r12):
    g = golden_r12
    off = torch.from_numpy(g["tgn_offset"]).double().requires_grad_()
    terms = R.tgn_terms(off, torch.from_numpy(g["tgn_xyz"]).double(), torch.from_numpy(g["tgn_labels"]).long())
    for i, name in enumerate(("offset_loss", "dir_loss", "chamf_loss")):
        _close(float(terms[i].detach()), g["tgn_loss_64"][i], name)
    _close(_grads(terms, off), g["tgn_grad_64"], "tgn gradients")


@pytest.mark.parametrize("key", ["tsg", "tsx"])
def test_restatement_reproduces_the_reference_centroid_terms(golden_r12, key):
    g = golden_r12
    off = torch.from_numpy(g[f"{key}_offset"]).double().requires_grad_()
    B, _, M = off.shape
    dist = torch.from_numpy(g[f"{key}_distance"]).double().view(B, M).requires_grad_()
    exists = torch.from_numpy(g[f"{key}_exists"]) if f"{key}_exists" in g else None
    terms = R.centroid_terms(off, torch.from_numpy(g[f"{key}_xyz"]).double(), dist, torch.from_numpy(g[f"{key}_centroid"]).double(), exists)
    for i, name in enumerate(("dist_loss", "cent_loss", "chamf_loss")):
        _close(float(terms[i].detach()), g[f"{key}_loss_64"][i], f"{key} {name}")
    _close(_grads(terms[1:], off), g[f"{key}_grad_offset_64"][1:], f"{key} offset gradients")
    assert not g[f"{key}_grad_offset_64"][0].any()
    _close(torch.autograd.grad(terms[0], dist)[0].numpy().reshape(g[f"{key}_grad_distance_64"].shape), g[f"{key}_grad_distance_64"],
           f"{key} distance gradient")


def test_fixture_inputs_keep_their_margins(golden_r12):
    g = golden_r12
    off, xyz, lab = (torch.from_numpy(g[k]) for k in ("tgn_offset", "tgn_xyz", "tgn_labels"))
    mg = R.tgn_margins(off, xyz, lab.long())
    norms = off.double().norm(dim=1)
    assert not bool(((norms > 1.9e-4) & (norms < 2.1e-4)).any())
    counts = mg["counts"].numpy()
    assert sorted(zip(*np.nonzero((counts >= 4) & (counts <= 6)))) == [(0, 3), (0, 5)] and counts[0, 3] == 4 and counts[0, 5] == 5
    assert counts[1, 7] == 0 and counts[0, 7] > 6
    assert float(norms[0][lab[0] == 9].max()) < 1.9e-4 and counts[0, 9] > 6          # in centroid_count, not in dir_count
    assert bool((norms[:, ::7] < 1.9e-4).all()) and bool((norms > 0).all())
    assert mg["ratio_gap"] >= 1e-4
    for key in ("tsg", "tsx"):
        B, _, M = g[f"{key}_offset"].shape
        exists = torch.from_numpy(g[f"{key}_exists"]) if f"{key}_exists" in g else None
        dist = torch.from_numpy(g[f"{key}_distance"]).view(B, M)
        mg = R.centroid_margins(torch.from_numpy(g[f"{key}_offset"]), torch.from_numpy(g[f"{key}_xyz"]), dist,
                                torch.from_numpy(g[f"{key}_centroid"]), exists)
        assert mg["mask"] >= 1e-3 and mg["ratio_gap"] >= 1e-4 and mg["arg_gap"] >= 1e-4, (key, mg)
        assert bool((dist <= 0.2).any()) and bool((dist > 0.2).any())
    moved = torch.from_numpy(g["tsg_xyz"] + g["tsg_offset"])[1]
    assert float(((moved - torch.from_numpy(g["tsg_centroid"])[1][:, 6:7]) ** 2).sum(0).min()) > 0.2   # masked out of the reverse term
    assert int((~g["tsx_exists"]).sum()) == 2 and g["tsx_centroid"].shape[2] == 16


def test_restatement_edge_cases():
    """what the formulas define where the reference divides 0 by 0 or raises"""
    gen = torch.Generator().manual_seed(5)
    xyz, off = torch.rand(1, 3, 40, generator=gen).double(), torch.rand(1, 3, 40, generator=gen).double()
    gingiva = torch.full((1, 40), -1)
    assert all(torch.isnan(t) for t in R.tgn_terms(off, xyz, gingiva))
    one = gingiva.clone()
    one[0, :10] = 4
    a, b, c = R.tgn_terms(off, xyz, one)
    assert torch.isfinite(a) and torch.isfinite(b) and torch.isnan(c)
    zero = torch.zeros(1, 3, 40, dtype=torch.float64, requires_grad=True)
    two = one.clone()
    two[0, 10:20] = 7
    terms = R.tgn_terms(zero, xyz, two)
    assert torch.isfinite(terms[0]) and torch.isnan(terms[1]) and torch.isfinite(terms[2])
    grad = torch.autograd.grad(terms[0] + terms[2], zero)[0]
    assert bool(torch.isfinite(grad).all())
    cent = torch.rand(1, 3, 5, generator=gen).double()
    far = torch.full((1, 40), 0.5, dtype=torch.float64)
    d, ce, ch = R.centroid_terms(off * 0, xyz, far, cent)
    assert torch.isfinite(d) and torch.isnan(ce) and torch.isfinite(ch)


def test_wrappers_refuse_before_touching_the_library(monkeypatch):
    from toothgroupnetwork_amd import _lib, losses

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    off, xyz, lab = torch.zeros(2, 3, 8), torch.zeros(2, 3, 8), torch.zeros(2, 8, dtype=torch.int64)
    for fn in (losses.tgn_offset_losses, losses.batch_center_offset_loss, losses.batch_chamfer_distance_loss):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(off, xyz, lab)
        with pytest.raises(TypeError, match="gt_seg_label"):
            fn(off, xyz, lab.float())
        with pytest.raises(ValueError, match="pred_offset"):
            fn(off.permute(0, 2, 1), xyz, lab)
        with pytest.raises(ValueError, match="sample_xyz"):
            fn(off, torch.zeros(2, 3, 9), lab)
        with pytest.raises(ValueError, match="sample_xyz"):
            fn(off, torch.zeros(1, 3, 8), lab)
        with pytest.raises(ValueError, match="gt_seg_label"):
            fn(off, xyz, torch.zeros(2, 9, dtype=torch.int64))
        with pytest.raises(TypeError, match="pred_offset"):
            fn(off.long(), xyz, lab)
    dist, cent = torch.zeros(2, 1, 8), torch.zeros(2, 3, 14)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.centroid_loss(off, xyz, dist, cent)
    with pytest.raises(ValueError, match="pred_offset"):
        losses.centroid_loss(off.permute(0, 2, 1), xyz, dist, cent)
    with pytest.raises(ValueError, match="centroid"):
        losses.centroid_loss(off, xyz, dist, torch.zeros(2, 3, 17))
    with pytest.raises(ValueError, match="centroid"):
        losses.centroid_loss(off, xyz, dist, torch.zeros(1, 3, 14))
    with pytest.raises(ValueError, match="distance"):
        losses.centroid_loss(off, xyz, torch.zeros(2, 1, 9), cent)
    with pytest.raises(ValueError, match="exists"):
        losses.centroid_loss(off, xyz, dist, cent, torch.ones(2, 13, dtype=torch.bool))
    with pytest.raises(TypeError, match="exists"):
        losses.centroid_loss(off, xyz, dist, cent, torch.ones(2, 14))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.tsegnet_centroid_loss_terms({"offset_result": off, "l3_xyz": xyz, "dist_result": dist}, cent)
    with pytest.raises(TypeError, match="gt_seg_label"):
        losses.grouping_loss_terms({"offset_1": off}, lab.float(), xyz)
