"""GPU: the fused contrastive-boundary stage (csrc/cbl.hip) behind losses.contrast_boundary_lists, contrast_boundary_stage_fused and
contrast_boundary_loss(fused=True).

Losses and latent gradients are held to the float64 restatement tests/cbl_ref.py within cbl_cases.LOSS_BOUND and GRAD_BOUND, the bounds
of the unfused criterion (twice the reference's own float32 error, rounded up to a power of two, in units of float32 epsilon times the
sum of the magnitudes of the terms added): on the hand-made cases over the CPU oracle's neighbour lists, and on arbitrary lists through
a stand-in `knn` that hands cbl_ref the given lists behind a dummy column 0.  Counts equal the fixture's and the unfused call's; rows
outside every contributing list get exactly zero; two calls give the same bits for loss, count AND gradient; sizes outside the kernels'
range give contrast_boundary_stage's bits; forward plus backward of one 24 000-point stage raise the peak memory by less than one
(m, K-1, C) tensor, where the unfused stage raises it by more.  The float64 values are computed once per case.

This file opens no stream (the graph replay is tests/test_gpu_losses_cbl_fused_graph.py, for the reason given there).

Measured on an MI355X: see profiles/cbl_fused_before_after.txt, section 3."""
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

P = 16      # losses.CBL_FUSED_BLOCK_POINTS, asserted below


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r19_cbl.npz")))


@pytest.fixture(scope="module")
def exact(oracle):
    """case name -> (case, the float64 stages): computed once, shared, not modified"""
    return {name: (CC.build(name), cbl_ref.all_stages(oracle.knnquery, CC.build(name))) for name in CC.HAND_CASES + ("flat0",)}


def _device_case(case, dev):
    from toothgroupnetwork_amd import pointops
    p = [torch.from_numpy(x).to(dev) for x in case["p"]]
    o = [pointops.register_offsets(torch.from_numpy(x).to(dev), x.tolist()) for x in case["o"]]
    f = [torch.from_numpy(x).to(dev).requires_grad_() for x in case["f"]]
    return p, o, f, torch.from_numpy(case["target"]).to(dev)


def _run(case, dev, fused=True):
    from toothgroupnetwork_amd import losses
    p, o, f, target = _device_case(case, dev)
    loss, counts = losses.contrast_boundary_loss([[a, b] for a, b in zip(p, o)], f, target, case["nsample"], case["stride"], fused=fused)
    return f, loss, counts


def _touched(s):
    rows = np.zeros(s["posmask"].shape[0], bool)
    rows[s["point_mask"]] = True
    rows[s["idx"][s["point_mask"]].reshape(-1)] = True
    return rows


def test_the_block_size_the_cases_below_are_built_around():
    from toothgroupnetwork_amd import losses
    assert losses.CBL_FUSED_BLOCK_POINTS == P


@pytest.mark.parametrize("name", CC.HAND_CASES)
def test_hand_made_cases_against_float64(dev, fx, exact, name):
    case, stages = exact[name]
    f, loss, counts = _run(case, dev)
    _, _, unfused_counts = _run(case, dev, fused=False)
    assert tuple(loss.shape) == (3,) and loss.dtype == torch.float32 and tuple(counts.shape) == (3,) and counts.dtype == torch.int64
    assert torch.equal(counts, unfused_counts)
    got = loss.detach().double().cpu().numpy()
    for i, s in enumerate(stages):
        assert int(counts[i]) == int(fx[f"{name}_point_mask_{i}"].sum()) == s["count"], ("count", i)
        g, = torch.autograd.grad(loss[i], f[i], retain_graph=True)
        g = g.double().cpu().numpy()
        g64, scale = s["grad"]()
        lu = cbl_ref.loss_units(got[i], float(s["loss"].detach()), s["loss_scale"])
        gu = cbl_ref.grad_units(g, g64, scale)
        print(f"  fused {name} stage {i}: loss {got[i]:.9g} exact {float(s['loss'].detach()):.12g}: {lu:.3f} units (bound {CC.LOSS_BOUND:g}); "
              f"gradient {gu:.2f} units (bound {CC.GRAD_BOUND:g})")
        assert lu <= CC.LOSS_BOUND, (name, i, got[i], float(s["loss"].detach()), lu)
        assert gu <= CC.GRAD_BOUND, (name, i, gu)
        assert not g[~_touched(s)].any(), (name, i, "gradient on a point outside every contributing list")
    assert (got[2] == 0.0) if name == "blobs4" else (got[2] > 0.0)


def test_flat0_gives_zero_everywhere(dev, exact):
    case, stages = exact["flat0"]
    assert all(s["count"] == 0 for s in stages)
    f, loss, counts = _run(case, dev)
    assert not loss.any() and not counts.any()
    grads = torch.autograd.grad(loss.sum(), f)
    assert all(bool(torch.isfinite(g).all()) and not g.any() for g in grads)


# ---- arbitrary lists ------------------------------------------------------------------------------------------------------------------

def _stand_in(idx):
    """a `knn` for cbl_ref that returns the given lists behind a dummy column 0"""
    def knn(nsample, xyz, new_xyz, offset, new_offset):
        assert nsample == idx.shape[1] + 1
        return np.concatenate([np.zeros((idx.shape[0], 1), idx.dtype), idx], 1), None
    return knn


def _lists_case(kind, m, k1, c):
    rng = np.random.default_rng(1000 * m + 10 * k1 + c)
    f = (rng.standard_normal((m, c)) * 0.5).astype(np.float32)
    idx = rng.integers(0, m, (m, k1)).astype(np.int64)
    labels = rng.integers(0, 3, m).astype(np.int64)
    if kind in ("hub", "hub_mixed"):
        idx[:, :k1 - (kind == "hub_mixed")] = 0                     # hub_mixed keeps its last, random, slot
        labels = (np.arange(m) % 2).astype(np.int64)
    elif kind == "repeats":
        idx[::2, 3] = idx[::2, 0]                                   # every other row names a neighbour twice ...
        idx[1::4, 1:4] = idx[1::4, :1]                              # ... and some four times
    elif kind == "identical":
        f[7] = f[3]                                                 # rows 3 and 7 are the same point of the latent space,
        idx[3, 0], idx[7, 2] = 7, 3                                 # and each other's neighbours
        labels[3], labels[7] = 0, 1
    return f, idx, labels


def _exact_lists(f, idx, labels):
    m = f.shape[0]
    return cbl_ref.stage(_stand_in(idx), np.zeros((m, 3), np.float32), f, np.array([m], np.int32), labels, idx.shape[1] + 1)


def _gpu_lists(f, idx, labels, dev):
    from toothgroupnetwork_amd import losses
    ft = torch.from_numpy(f).to(dev).requires_grad_()
    loss, count = losses.contrast_boundary_lists(ft, torch.from_numpy(idx).to(dev), torch.from_numpy(labels).to(dev))
    g, = torch.autograd.grad(loss, ft)
    return loss.detach(), count, g


LISTS = [("random", 40, 1, 32),                                      # k1 = 1: no point can contribute
         ("random", 200, 23, 32), ("random", 200, 35, 32), ("random", 130, 63, 32),
         ("random", P - 1, 8, 32), ("random", P, 8, 32), ("random", P + 1, 8, 32),
         ("random", 3 * P + 5, 8, 32),                               # four workgroups: the finishing kernel adds several partials
         ("random", 70 * P, 8, 32),                                  # more workgroups than the finishing wave has lanes
         ("random", 1, 5, 32),
         ("random", 90, 12, 4), ("random", 90, 12, 8), ("random", 90, 12, 16), ("random", 90, 12, 36), ("random", 90, 12, 64),
         ("random", 90, 12, 128),
         ("hub", 257, 8, 32),                                        # every list all zeros: point 0 has in-degree 2056, and no row is mixed
         ("hub_mixed", 257, 8, 32),                                  # seven slots of eight name point 0: its long list carries weights
         ("repeats", 100, 8, 32), ("identical", 60, 6, 32)]


@pytest.mark.parametrize("kind,m,k1,c", LISTS, ids=[f"{k}-{m}-{k1}-{c}" for k, m, k1, c in LISTS])
def test_arbitrary_lists_against_float64(dev, kind, m, k1, c):
    f, idx, labels = _lists_case(kind, m, k1, c)
    s = _exact_lists(f, idx, labels)
    loss, count, g = _gpu_lists(f, idx, labels, dev)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and count.dtype == torch.int64 and count.dim() == 0
    assert int(count) == s["count"]
    g = g.double().cpu().numpy()
    g64, scale = s["grad"]()
    lu = cbl_ref.loss_units(float(loss), float(s["loss"].detach()), s["loss_scale"])
    gu = cbl_ref.grad_units(g, g64, scale)
    print(f"  lists {kind} m={m} k1={k1} c={c}: count {int(count)}, loss {float(loss):.9g} exact {float(s['loss'].detach()):.12g}: {lu:.3f} units "
          f"(bound {CC.LOSS_BOUND:g}); gradient {gu:.2f} units (bound {CC.GRAD_BOUND:g})")
    assert np.isfinite(g).all()
    assert lu <= CC.LOSS_BOUND, (float(loss), float(s["loss"].detach()), lu)
    assert gu <= CC.GRAD_BOUND, gu
    assert not g[~_touched(s)].any()
    if k1 == 1 or m == 1 or kind == "hub":                           # one slot, one point, or lists of one label: nothing contributes
        assert int(count) == 0 and float(loss) == 0.0 and not g.any()
    else:
        assert int(count) > 0
    if kind == "hub_mixed":
        assert np.abs(g[0]).max() > 0 and (idx == 0).sum() >= 7 * m
    if kind == "identical":
        assert s["point_mask"][3] or s["point_mask"][7]


def test_features_scaled_by_50_underflow_without_a_nan(dev):
    """Latent features fifty times the size of the other cases'.  512 tight clusters of 8 points; a row lists 6 members of its own
    cluster (after the scaling a distance of about 0.3) and 2 points from anywhere (a distance of about 200), labels at random.  Beside
    a near neighbour every far one's e is exp(-200): exactly 0 in float32.  Rows whose near neighbours all carry another label and
    whose far ones do not have every POSITIVE e underflowed: pos = 0 and the value is -log(1e-12) in both precisions.

    Why LOSS_BOUND holds here by construction, not by luck: the float32 error of a distance of 200 is 1.5e-5, tens of units in a
    value that depended on it, and no value does -- a row's value is decided by its near neighbours alone, whose distances carry the
    error of a distance of 0.3, as in the other cases; and about one row in twenty has the value 27.6, so the mean value stays near 2
    and the one float32 rounding of the result below a third of a unit.
    The unit bound on the GRADIENT does not apply: on the rows above the float64 gradient is of the order of exp(-200) / 1e-12 and the
    float32 one exactly 0, against a scale of the same tiny order.  Every element must be finite."""
    rng = np.random.default_rng(50)
    clusters, size, c, near, far = 512, 8, 32, 6, 2
    m, k1 = clusters * size, near + far
    centre = (rng.standard_normal((clusters, c)) * 0.5).astype(np.float32)
    f = np.repeat(centre, size, 0) + (rng.standard_normal((m, c)) * 1e-3).astype(np.float32)
    f *= 50
    own = np.arange(m) // size * size
    idx = np.concatenate([own[:, None] + rng.integers(0, size, (m, near)), rng.integers(0, m, (m, far))], 1).astype(np.int64)
    labels = rng.integers(0, 3, m).astype(np.int64)
    s = _exact_lists(f, idx, labels)
    d = np.sqrt(((f[:, None, :].astype(np.float64) - f[idx]) ** 2).sum(-1) + 1e-12)
    dead = np.where(s["posmask"], d.min(1, keepdims=True) - d, -np.inf).max(1) < -104          # float32 exp gives 0 below -103.98
    assert (dead & s["point_mask"]).sum() >= 50
    loss, count, g = _gpu_lists(f, idx, labels, dev)
    assert int(count) == s["count"]
    lu = cbl_ref.loss_units(float(loss), float(s["loss"].detach()), s["loss_scale"])
    print(f"  underflow: count {int(count)}, {int((dead & s['point_mask']).sum())} rows with every positive e = 0, loss {float(loss):.9g} exact "
          f"{float(s['loss'].detach()):.12g}: {lu:.3f} units (bound {CC.LOSS_BOUND:g})")
    assert lu <= CC.LOSS_BOUND, (float(loss), float(s["loss"].detach()), lu)
    assert bool(torch.isfinite(g).all())


def test_two_calls_give_the_same_bits_gradient_included(dev):
    for kind, m, k1, c in (("hub_mixed", 257, 8, 32), ("random", 70 * P, 8, 32), ("random", 130, 63, 32)):
        f, idx, labels = _lists_case(kind, m, k1, c)
        first, again = _gpu_lists(f, idx, labels, dev), _gpu_lists(f, idx, labels, dev)
        for a, b in zip(first, again):
            assert torch.equal(a, b), (kind, m)
    case = CC.build("binary2")
    (f1, l1, c1), (f2, l2, c2) = _run(case, dev), _run(case, dev)
    assert torch.equal(l1, l2) and torch.equal(c1, c2)
    for a, b in zip(torch.autograd.grad(l1.sum(), f1), torch.autograd.grad(l2.sum(), f2)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("c,nsample", [(6, 9), (32, 65)])
def test_sizes_outside_the_kernels_go_through_the_unfused_stage(dev, c, nsample):
    from toothgroupnetwork_amd import losses, pointops
    g = torch.Generator().manual_seed(65)
    m = 200
    p = torch.rand(m, 3, generator=g).to(dev)
    o = pointops.register_offsets(torch.tensor([m], dtype=torch.int32, device=dev), [m])
    f = (torch.randn(m, c, generator=g) * 0.5).to(dev)
    labels = torch.randint(0, 3, (m,), generator=g).to(dev)
    got, want = losses.contrast_boundary_stage_fused(p, f, o, labels, nsample), losses.contrast_boundary_stage(p, f, o, labels, nsample)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and int(want[1]) > 0


def test_arguments_are_checked(dev):
    from toothgroupnetwork_amd import losses
    f, idx, labels = (torch.from_numpy(x).to(dev) for x in _lists_case("random", 40, 5, 32))
    with pytest.raises(ValueError, match="nsample"):
        losses.contrast_boundary_stage_fused(f[:, :3], f, None, labels, 1)
    with pytest.raises(ValueError, match="same number of points"):
        losses.contrast_boundary_stage_fused(f[:, :3], f[:-1], None, labels, 6)
    with pytest.raises(ValueError, match="the fused stage needs"):
        losses.contrast_boundary_lists(f, idx.repeat(1, 13), labels)                       # k1 = 65


def test_forward_and_backward_never_hold_the_difference_tensor(dev):
    """one random scan at the first stage's size: the peak over forward + backward rises by less than the bytes of ONE (m, K-1, C)
    float32 tensor with the fused stage, and by more than that with the unfused one (so the probe can see the tensor)"""
    from toothgroupnetwork_amd import losses, pointops
    m, nsample, c = 24000, 36, 32
    tensor_bytes = m * (nsample - 1) * c * 4
    assert tensor_bytes == 107520000
    g = torch.Generator().manual_seed(24)
    p = torch.rand(m, 3, generator=g).to(dev)
    o = pointops.register_offsets(torch.tensor([m], dtype=torch.int32, device=dev), [m])
    f = (torch.randn(m, c, generator=g) * 0.5).to(dev).requires_grad_()
    labels = (p[:, 0] * 4).long()
    pointops.knn_indices(nsample, p, p, o, o)                                                # the neighbour list, warmed up

    def rise(stage):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss, count = stage(p, f, o, labels, nsample)
        grad, = torch.autograd.grad(loss, f)
        torch.cuda.synchronize()
        assert int(count) > 0 and bool(torch.isfinite(grad).all())
        return torch.cuda.max_memory_allocated() - before
    fused, unfused = rise(losses.contrast_boundary_stage_fused), rise(losses.contrast_boundary_stage)
    print(f"  peak rise over forward + backward: fused {fused / 2 ** 20:.1f} MiB, unfused {unfused / 2 ** 20:.1f} MiB, one (m, K-1, C) tensor "
          f"{tensor_bytes / 2 ** 20:.1f} MiB")
    assert fused < tensor_bytes, fused
    assert unfused > tensor_bytes, unfused


def test_the_trainer_sets_the_switch_on_both_networks(dev, tmp_path):
    """tr_set.contrastive_boundary_fused reaches both PointTransformerSeg networks; the module's cbl terms with the switch on agree
    with those of the same weights with it off (equal counts; losses within cbl_cases.NET_LOSS_BOUND of each other, in units of float32
    epsilon times (0.1 + loss)), and a train step runs."""
    import copy
    from toothgroupnetwork_amd import eval_sharded, training
    torch.manual_seed(21)
    np.random.seed(21)
    eval_sharded.write_synthetic_preprocessed(str(tmp_path / "data"), 1, n_points=6144)
    loader = torch.utils.data.DataLoader(training.DentalModelGenerator(str(tmp_path / "data")), shuffle=False, batch_size=1,
                                         collate_fn=training.collate_fn)
    batch = next(iter(loader))
    cfg = {"tr_set": {"optimizer": {"lr": 1e-2, "NAME": "sgd", "momentum": 0.9, "weight_decay": 1.0e-4},
                      "scheduler": {"sched": "cosine", "warmup_epochs": 0, "full_steps": 40, "schedueler_step": 15000000, "min_lr": 1e-5},
                      "loss": {"cbl_loss_1": 1, "cbl_loss_2": 1, "tooth_class_loss_1": 1, "tooth_class_loss_2": 1, "offset_1_loss": 0.03,
                               "offset_1_dir_loss": 0.03, "chamf_1_loss": 0.15},
                      "contrastive_boundary": True},
           "model_parameter": {"input_feat": 6, "stride": [1, 4, 4, 4, 4], "nsample": [36, 24, 24, 24, 24], "blocks": [2, 3, 4, 6, 3],
                               "block_num": 5, "planes": [32, 64, 128, 256, 512], "crop_sample_size": 3072},
           "checkpoint_path": str(tmp_path / "ckpt")}
    plain = training.make_training_model("tgnet_fps", copy.deepcopy(cfg))
    nets_of = lambda model: (model.module.first_ins_cent_model, model.module.second_ins_cent_model)   # noqa: E731
    assert [n.fused_contrast for n in nets_of(plain)] == [False, False]
    cfg["tr_set"]["contrastive_boundary_fused"] = True
    model = training.make_training_model("tgnet_fps", cfg)
    assert [n.fused_contrast for n in nets_of(model)] == [True, True]
    inputs = [batch["feat"].to(dev), batch["gt_seg_label"].to(dev)]
    with torch.no_grad():
        on = model.forward(inputs)
        for n in nets_of(model):
            n.fused_contrast = False
        off = model.forward(inputs)
        for n in nets_of(model):
            n.fused_contrast = True
    for k in ("1", "2"):
        assert torch.equal(on["cbl_counts_" + k], off["cbl_counts_" + k])
        a, b = on["cbl_loss_" + k].double(), off["cbl_loss_" + k].double()
        units = ((a - b).abs() / (cbl_ref.EPS32 * (cbl_ref.WEIGHT + b.abs()))).max()
        print(f"  cbl_loss_{k}: fused {a.tolist()} unfused {b.tolist()}: {float(units):.1f} units (bound {CC.NET_LOSS_BOUND:g})")
        assert float(units) <= CC.NET_LOSS_BOUND
    lmap = model.step(0, batch, "train")
    assert {"cbl_loss_1", "cbl_loss_2"} <= set(lmap.loss_dict)
    grads = [p.grad for p in model.module.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
