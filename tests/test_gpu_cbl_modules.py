"""GPU: the contrastive-boundary criterion through the modules -- nets.PointTransformerSeg(contrast=True) against the reference's own
PointTransformerSeg.forward([feats, target]) (run on CPU by tests/golden/make_golden_r19_cbl.py, weights from tests/golden/seeded.py),
nets.GroupingNetworkModule's cbl_loss_1 / cbl_loss_2, and a tgnet_fps training step with tr_set.contrastive_boundary.

The masks depend on geometry and labels only, so the per-stage counts must EQUAL the reference's.  The losses are held to the
reference's float64 network within cbl_cases.NET_LOSS_BOUND: twice the largest error of the reference's own float32 network against it,
rounded up to a power of two, in units of float32 epsilon times (0.1 + loss) -- cbl_ref's loss scale, 0.1 * mean(1 + per-point loss).

Measured on an MI355X: see profiles/r19_cbl.txt."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import cbl_cases as CC  # noqa: E402
import cbl_ref  # noqa: E402
from seeded import seeded_fill  # noqa: E402

pytestmark = pytest.mark.gpu

MODEL_PARAMETER = {"input_feat": 6, "stride": [1, 4, 4, 4, 4], "nsample": [36, 24, 24, 24, 24], "blocks": [2, 3, 4, 6, 3], "block_num": 5,
                   "planes": [32, 64, 128, 256, 512], "crop_sample_size": 3072}          # train_configs/tgnet_fps.py
LOSS = {"cbl_loss_1": 1, "cbl_loss_2": 1, "tooth_class_loss_1": 1, "tooth_class_loss_2": 1, "offset_1_loss": 0.03, "offset_1_dir_loss": 0.03,
        "chamf_1_loss": 0.15}                                                             # train_configs/tgnet_fps.py:16-24
CBL = ("cbl_loss_1", "cbl_loss_2")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r19_cbl.npz")))


def _net(name, dev):
    from toothgroupnetwork_amd import nets
    arch, k, B, N, wseed, _ = CC.NET_CASES[name]
    net = nets.PointTransformerSeg(c=arch["c"], k=k, planes=tuple(arch["planes"]), blocks=tuple(arch["blocks"]), stride=tuple(arch["stride"]),
                                   nsample=tuple(arch["nsample"]), block_num=arch["block_num"])
    seeded_fill(net, wseed)
    return net.to(dev).eval()


@pytest.mark.parametrize("name", list(CC.NET_CASES))
def test_point_transformer_seg_against_the_reference(dev, fx, name):
    arch, k, B, N, _, _ = CC.NET_CASES[name]
    net = _net(name, dev)
    feats, labels = (torch.from_numpy(a).to(dev) for a in CC.net_inputs(name))
    assert net.cbl_counts is None
    with torch.no_grad():
        out = net([feats, labels], contrast=True)
        cbl, counts = out[0], net.cbl_counts
        flat = net([feats, labels[:, 0]], contrast=True)                  # (B, N) labels
        flat_counts = net.cbl_counts
        plain = net([feats])
    assert net.cbl_counts is None, "the counts are those of the last forward: none after one without the criterion"
    assert len(plain) == 4 and len(out) == 5 and out[3] is None
    assert tuple(cbl.shape) == (arch["block_num"],) and cbl.dtype == torch.float32
    assert tuple(counts.shape) == (arch["block_num"],) and counts.dtype == torch.int64 and torch.equal(flat_counts, counts)
    # without `contrast` the list is the old one; with it the other outputs are the same computation.  Two forwards of this network
    # do not give the same bits, with or without the criterion: the top decoder stage's TransitionUp takes its per-cloud mean with
    # Tensor.index_add_ (point_transformer.py), whose float atomics add in no fixed order -- the first module output that differs
    # between two plain forwards is that mean's linear layer, in the two-stage network too.  So the outputs are
    # compared to 1e-4 of the largest magnitude, and the second criterion run, on (B, N) labels, is held to the same bound as the
    # first below; the criterion's own forward repeats bit for bit on fixed latents (tests/test_gpu_cbl.py).
    assert (out[2] is None) == (B > 1) and (plain[1] is None) == (B > 1)
    for a, b in ((out[1], plain[0]), (out[4], plain[3])) + (((out[2], plain[1]),) if B == 1 else ()):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())
    assert np.array_equal(counts.cpu().numpy(), fx[f"net_{name}_counts"]), (counts.tolist(), fx[f"net_{name}_counts"].tolist())
    l64, l32 = fx[f"net_{name}_loss_64"], fx[f"net_{name}_loss_32"].astype(np.float64)
    scale = cbl_ref.EPS32 * (cbl_ref.WEIGHT + np.abs(l64))
    own = np.abs(l32 - l64) / scale
    for tag, value in (("(B, 1, N) labels", cbl), ("(B, N) labels", flat[0])):
        got = value.double().cpu().numpy()
        units = np.abs(got - l64) / scale
        print(f"  {name}, {tag}: cbl {np.array2string(got, precision=6)} exact {np.array2string(l64, precision=6)}: "
              f"{np.array2string(units, precision=1)} units (reference fp32 network {np.array2string(own, precision=1)}, bound {CC.NET_LOSS_BOUND:g})")
        assert (units <= CC.NET_LOSS_BOUND).all(), (name, tag, units.tolist())


def test_the_criterion_reads_the_last_head_that_ran(dev):
    """B == 1: the offset head's latent MLPs get the criterion's gradient and the class head's none; B == 2: the class head's."""
    for name, reads, idle in (("five_b1", "offset_head", "cls_head"), ("two_b2", "cls_head", "offset_head")):
        net = _net(name, dev).train()
        feats, labels = (torch.from_numpy(a).to(dev) for a in CC.net_inputs(name))
        net([feats, labels], contrast=True)[0].sum().backward()
        for i in range(net.block_num):
            g = getattr(net, reads).infer_list[i].infer[0].weight.grad
            assert g is not None and bool(torch.isfinite(g).all()) and bool(g.any()), (name, reads, i)
            assert getattr(net, idle).infer_list[i].infer[0].weight.grad is None, (name, idle, i)
            grads = [p.grad for p in getattr(net, f"dec{i + 1}").parameters()]
            assert all(x is not None and bool(torch.isfinite(x).all()) for x in grads) and any(bool(x.any()) for x in grads), (name, "decoder", i)
        assert getattr(net, reads).cls.weight.grad is None, "the criterion reads the latents, not the classifier"
    with pytest.raises(ValueError, match="inputs\\[1\\]"):
        net([feats], contrast=True)
    with pytest.raises(ValueError, match="one label per point"):
        net([feats, labels[:, :, :-1]], contrast=True)


def _config(ckpt, loss, **tr_set):
    cfg = {"tr_set": {"optimizer": {"lr": 1e-2, "NAME": "sgd", "momentum": 0.9, "weight_decay": 1.0e-4},
                      "scheduler": {"sched": "cosine", "warmup_epochs": 0, "full_steps": 40, "schedueler_step": 15000000, "min_lr": 1e-5},
                      "loss": dict(loss)},
           "model_parameter": copy.deepcopy(MODEL_PARAMETER), "checkpoint_path": ckpt}
    cfg["tr_set"].update(tr_set)
    return cfg


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    from toothgroupnetwork_amd import eval_sharded, training
    root = tmp_path_factory.mktemp("cbl_data")
    eval_sharded.write_synthetic_preprocessed(str(root), 1, n_points=6144)
    loader = torch.utils.data.DataLoader(training.DentalModelGenerator(str(root)), shuffle=False, batch_size=1, collate_fn=training.collate_fn)
    return next(iter(loader))


def test_grouping_network_module_returns_the_terms_on_request(dev, batch):
    from toothgroupnetwork_amd import nets
    torch.manual_seed(19)
    module = nets.GroupingNetworkModule({"model_parameter": copy.deepcopy(MODEL_PARAMETER)}).to(dev).train()
    points, labels = batch["feat"].to(dev), batch["gt_seg_label"].to(dev)
    with torch.no_grad():
        plain = module([points, labels])
        tested = module([points, labels], test=True, contrast=True)
        unlabelled_keys = {"sem_1", "offset_1", "mask_1", "first_features", "sem_2", "offset_2", "mask_2", "cropped_feature_ls", "nn_crop_indexes"}
    assert set(plain) == unlabelled_keys | {"cluster_gt_seg_label"} and set(tested) == set(plain)
    out = module([points, labels], contrast=True)
    assert set(out) == set(plain) | set(CBL) | {"cbl_counts_1", "cbl_counts_2"}
    for name in CBL:
        assert tuple(out[name].shape) == (5,) and out[name].dtype == torch.float32 and bool(torch.isfinite(out[name]).all())
    assert out["sem_2"].shape[0] > 1, "several crops: the second network's criterion reads its class head"
    # both networks' head MLPs and decoders receive gradient from the cbl terms ALONE
    (out["cbl_loss_1"].sum() + out["cbl_loss_2"].sum()).backward()
    for n, (net, head) in enumerate(((module.first_ins_cent_model, "offset_head"), (module.second_ins_cent_model, "cls_head")), 1):
        counts = out[f"cbl_counts_{n}"]
        assert tuple(counts.shape) == (5,) and counts.dtype == torch.int64 and bool((counts > 0).any())
        for i in range(5):
            g = getattr(net, head).infer_list[i].infer[0].weight.grad
            assert g is not None and bool(torch.isfinite(g).all()) and bool(g.any()), (head, i)
            grads = [p.grad for p in getattr(net, f"dec{i + 1}").parameters()]
            assert all(x is not None and bool(torch.isfinite(x).all()) for x in grads) and any(bool(x.any()) for x in grads), ("decoder", i)
        assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in net.parameters())


def test_a_tgnet_fps_step_with_the_criterion(dev, batch, tmp_path):
    from toothgroupnetwork_amd import training
    torch.manual_seed(20)
    np.random.seed(20)
    terms = set(training.FpsGroupingNetworkModel.TERMS)
    model = training.make_training_model("tgnet_fps", _config(str(tmp_path / "on"), LOSS, contrastive_boundary=True))
    lmap = model.step(0, batch, "train")
    assert set(lmap.loss_dict) == terms | set(CBL) and all(lmap.loss_dict[n][1] == 1 for n in CBL)
    grads = [p.grad for p in model.module.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
    printed = lmap.get_loss_dict_for_print("step")
    assert {"cbl_loss_1_step", "cbl_loss_2_step", "total_step"} <= set(printed) and all(np.isfinite(v) for v in printed.values())
    assert printed["cbl_loss_1_step"] > 0 and printed["cbl_loss_2_step"] > 0
    val = model.step(0, batch, "val")
    assert set(val.loss_dict) == terms and not model.module.training
    # the key with zero weights, and no key: the criterion is not computed at all
    for tag, loss, extra in (("zero", {**LOSS, "cbl_loss_1": 0, "cbl_loss_2": 0}, {"contrastive_boundary": True}),
                             ("absent", {k: v for k, v in LOSS.items() if k not in CBL}, {})):
        quiet = training.make_training_model("tgnet_fps", _config(str(tmp_path / tag), loss, **extra))
        assert set(quiet.step(0, batch, "train").loss_dict) == terms
        assert quiet.module.first_ins_cent_model.cbl_counts is None and quiet.module.second_ins_cent_model.cbl_counts is None
    with pytest.raises(NotImplementedError, match="cbl_loss_1.*contrastive_boundary"):
        training.make_training_model("tgnet_fps", _config(str(tmp_path / "off"), LOSS))
