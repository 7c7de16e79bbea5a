"""GPU: losses.contrast_boundary_stage / contrast_boundary_loss on the hand-made cases of tests/golden/cbl_cases.py.

Masks, counts and stage labels equal what the reference's own ContrastHead computed (tests/golden/reference_cpu_r19_cbl.npz); losses and
latent gradients are held to the float64 restatement tests/cbl_ref.py (over the CPU oracle's neighbour lists) within cbl_cases.LOSS_BOUND
and GRAD_BOUND: twice the reference's own float32 error, rounded up to a power of two, in units of float32 epsilon times the sum of the
magnitudes of the terms added.  Points outside the mask get a zero gradient, a stage without a mixed point gives 0 at stage 0 too,
two forwards give the same bits.  The exact float64 values are computed once per case.  (The graph replay of forward and backward is
tests/test_gpu_losses_cbl_graph.py, for the reason given there.)

Measured on an MI355X (largest over the stages; loss / gradient, in units): see profiles/r19_cbl.txt."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import cbl_cases as CC  # noqa: E402
import cbl_ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r19_cbl.npz")))


@pytest.fixture(scope="module")
def exact(oracle):
    """case name -> (case, the float64 stages): computed once, shared, not modified"""
    out = {}
    for name in CC.HAND_CASES + ("flat0",):
        case = CC.build(name)
        out[name] = (case, cbl_ref.all_stages(oracle.knnquery, case))
    return out


def _device_case(case, dev):
    from toothgroupnetwork_amd import pointops
    p = [torch.from_numpy(x).to(dev) for x in case["p"]]
    o = [pointops.register_offsets(torch.from_numpy(x).to(dev), x.tolist()) for x in case["o"]]
    f = [torch.from_numpy(x).to(dev).requires_grad_() for x in case["f"]]
    return p, o, f, torch.from_numpy(case["target"]).to(dev)


def _run(case, dev):
    from toothgroupnetwork_amd import losses
    p, o, f, target = _device_case(case, dev)
    loss, counts = losses.contrast_boundary_loss([[a, b] for a, b in zip(p, o)], f, target, case["nsample"], case["stride"])
    return p, o, f, target, loss, counts


@pytest.mark.parametrize("name", CC.HAND_CASES)
def test_masks_counts_and_stage_labels_equal_the_reference(dev, fx, name):
    from toothgroupnetwork_amd import losses, pointops
    case = CC.build(name)
    p, o, f, target, loss, counts = _run(case, dev)
    assert tuple(loss.shape) == (3,) and loss.dtype == torch.float32 and tuple(counts.shape) == (3,) and counts.dtype == torch.int64
    for i in range(3):
        labels = target if i == 0 else losses.stage_vote(p[0], o[0], p[i], o[i], target, int(np.prod(case["stride"][:i])))
        assert np.array_equal(labels.cpu().numpy(), fx[f"{name}_labels_{i}"]), ("stage labels", i)
        idx = pointops.knn_indices(case["nsample"][i], p[i], p[i], o[i], o[i])[:, 1:].long()
        posmask = labels[idx] == labels[:, None]
        assert np.array_equal(posmask.cpu().numpy(), fx[f"{name}_posmask_{i}"]), ("posmask", i)
        assert int(counts[i]) == int(fx[f"{name}_point_mask_{i}"].sum()), ("count", i)
        _, count = losses.contrast_boundary_stage(p[i], f[i], o[i], labels.int(), case["nsample"][i])
        assert int(count) == int(counts[i])


@pytest.mark.parametrize("name", CC.HAND_CASES)
def test_losses_and_latent_gradients_against_float64(dev, fx, exact, name):
    case, stages = exact[name]
    p, o, f, target, loss, counts = _run(case, dev)
    got = loss.detach().double().cpu().numpy()
    for i, s in enumerate(stages):
        g, = torch.autograd.grad(loss[i], f[i], retain_graph=True)
        g = g.double().cpu().numpy()
        g64, scale = s["grad"]()
        lu = cbl_ref.loss_units(got[i], float(s["loss"].detach()), s["loss_scale"])
        gu = cbl_ref.grad_units(g, g64, scale)
        ref_lu = cbl_ref.loss_units(float(fx[f"{name}_loss_{i}"]), float(s["loss"].detach()), s["loss_scale"])
        ref_gu = cbl_ref.grad_units(fx[f"{name}_grad_{i}"], g64, scale)
        print(f"  {name} stage {i}: loss {got[i]:.9g} exact {float(s['loss'].detach()):.12g}: {lu:.3f} units (reference fp32 {ref_lu:.3f}, bound "
              f"{CC.LOSS_BOUND:g}); gradient {gu:.2f} units (reference fp32 {ref_gu:.2f}, bound {CC.GRAD_BOUND:g})")
        assert lu <= CC.LOSS_BOUND, (name, i, got[i], float(s["loss"].detach()), lu)
        assert gu <= CC.GRAD_BOUND, (name, i, gu)
        # points that no contributing list holds: exactly zero, and so is every row of a stage without a mixed point
        touched = np.zeros(g.shape[0], bool)
        touched[s["point_mask"]] = True
        touched[s["idx"][s["point_mask"]].reshape(-1)] = True
        assert not g[~touched].any(), (name, i, "gradient on a point outside every contributing list")
    assert (got[2] == 0.0) if name == "blobs4" else (got[2] > 0.0)
    # the stages are independent: the gradient of the sum is the stages' own
    total = torch.autograd.grad(loss.sum(), f)
    assert all(bool(torch.isfinite(t).all()) for t in total)


def test_an_unmasked_point_gets_no_gradient_from_its_own_row(dev, exact):
    """contrast_boundary_stage on its own: the planted point of blobs4 has no positive neighbour, so it is outside the mask; a row
    that is neither a contributing point nor in a contributing point's list gets exactly zero."""
    from toothgroupnetwork_amd import losses
    case, stages = exact["blobs4"]
    p, o, f, target = _device_case(case, dev)
    s = stages[0]
    labels = target.clone()
    loss, count = losses.contrast_boundary_stage(p[0], f[0], o[0], labels, case["nsample"][0])
    g, = torch.autograd.grad(loss, f[0])
    holders = np.zeros(g.shape[0], bool)                     # rows whose own list or a contributing neighbour's list holds them
    holders[s["point_mask"]] = True
    holders[s["idx"][s["point_mask"]].reshape(-1)] = True
    assert (~holders).any() and not g[torch.from_numpy(~holders).to(dev)].any()
    assert int(count) == s["count"] and not s["point_mask"][case["planted"]]


def test_a_stage_0_without_a_mixed_point_gives_zero(dev, exact):
    case, stages = exact["flat0"]
    assert all(s["count"] == 0 for s in stages)
    p, o, f, target, loss, counts = _run(case, dev)
    assert not loss.any() and not counts.any()
    grads = torch.autograd.grad(loss.sum(), f)
    assert all(bool(torch.isfinite(g).all()) and not g.any() for g in grads)


def test_two_forwards_give_the_same_bits(dev):
    case = CC.build("binary2")
    first, again = _run(case, dev), _run(case, dev)
    assert torch.equal(first[4], again[4]) and torch.equal(first[5], again[5])


def test_arguments_are_checked(dev):
    from toothgroupnetwork_amd import losses
    case = CC.build("binary2")
    p, o, f, target = _device_case(case, dev)
    with pytest.raises(ValueError, match="nsample"):
        losses.contrast_boundary_stage(p[0], f[0], o[0], target, 1)
    with pytest.raises(ValueError, match="same number of points"):
        losses.contrast_boundary_stage(p[0], f[1], o[0], target, 9)
    with pytest.raises(ValueError, match="one label per stage-0 point"):
        losses.contrast_boundary_loss([[p[0], o[0]]], [f[0]], target[:-1], (9,), (1,))
    with pytest.raises(ValueError, match="stages"):
        losses.contrast_boundary_loss([[p[0], o[0]]], f[:2], target, (9, 9), (1, 4))
