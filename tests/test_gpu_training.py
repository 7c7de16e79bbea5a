"""GPU: the training entry point (toothgroupnetwork_amd/training.py, tools/train.py) and tsegnet's criterion (losses.tsegnet_loss_terms)
on an MI355X: a step of every model, tsegnet's six terms against the reference's (tests/golden/reference_cpu_r17_training.npz), an
overfit run through the trainer, the command line in a child process, and the one device read of a step's LossMap.

Point counts are the smallest each module accepts, read from the modules:
  pointnet          257    no sampling level at all: one point more than a 256-wide block, odd
  pointnetpp       1024    nets.PointNetPPSeg.sa1 samples npoint = 1024 centres
  dgcnn              20    dgcnn.DGCnnModule.k = 20 neighbours, the point itself included (feature_knn: k <= N)
  pointtransformer 6144    strides 1, 4, 4, 4, 4 leave N / 256 points at the deepest level, whose nsample is 24: 24 * 256
  tsegnet, tgnet_fps 3072  the crops hold 3072 points (nets.TSegNetModule.CROP_K, crop_sample_size; crops.check_k: k <= N)

Durations on an MI355X: under 1.5 s a test, except the first training step of a process through pointnet (7.6 s), pointnetpp (9.8 s),
tsegnet's centroid network (4.7 s) and its segmentation network (8.6 s, on two crops), and the command line's child process (6.6 s).
The same pointnetpp sequence in a fresh process right afterwards takes 0.8 s for its first step and 2.7 s in all, so the seconds are
one-off work outside the step that a later process finds done -- presumably the runtime compiling the convolution and BatchNorm
kernels of these shapes in training mode into its on-disk cache; not traced further."""
import copy
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import training_ref as R
from conftest import GOLDEN, REPO

sys.path.insert(0, GOLDEN)
import training_cases as C  # noqa: E402
import tsegnet_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu

MODEL_PARAMETER = {"input_feat": 6, "stride": [1, 4, 4, 4, 4], "nsample": [36, 24, 24, 24, 24], "blocks": [2, 3, 4, 6, 3], "block_num": 5,
                   "planes": [32, 64, 128, 256, 512], "crop_sample_size": 3072}
FPS_LOSS = {"cbl_loss_1": 0, "cbl_loss_2": 0, "tooth_class_loss_1": 1, "tooth_class_loss_2": 1, "offset_1_loss": 0.03, "offset_1_dir_loss": 0.03,
            "chamf_1_loss": 0.15}
POINTS = {"pointnet": 257, "pointnetpp": 1024, "dgcnn": 20, "pointtransformer": 6144, "tsegnet": 3072, "tgnet_fps": 3072}
INFERENCE_NAMES = ("pointnet", "pointnetpp", "dgcnn", "pointtransformer", "tsegnet")


def make_config(name, ckpt, every=15000000, opt="adam"):
    optimizer = {"lr": 1e-3, "NAME": "adam", "weight_decay": 1.0e-4} if opt == "adam" else {"lr": 1e-2, "NAME": "sgd", "momentum": 0.9, "weight_decay": 1.0e-4}
    cfg = {"tr_set": {"optimizer": optimizer, "scheduler": {"sched": "cosine", "warmup_epochs": 0, "full_steps": 40, "schedueler_step": every, "min_lr": 1e-5}},
           "checkpoint_path": ckpt}
    if name in ("pointtransformer", "tgnet_fps"):
        cfg["model_parameter"] = copy.deepcopy(MODEL_PARAMETER)
        cfg["tr_set"]["loss"] = dict(FPS_LOSS) if name == "tgnet_fps" else {"tooth_class_loss_1": 1}
    if name == "tsegnet":
        cfg["run_tooth_segmentation_module"] = False
    return cfg


def synthetic_loader(root, n, n_points, batch_size=1):
    from toothgroupnetwork_amd import eval_sharded, training
    eval_sharded.write_synthetic_preprocessed(str(root), n, n_points=n_points)
    return torch.utils.data.DataLoader(training.DentalModelGenerator(str(root)), shuffle=False, batch_size=batch_size, collate_fn=training.collate_fn)


def _snapshot(module):
    return {k: v.detach().clone() for k, v in module.state_dict().items()}


# ---- 7. a step of every model ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(POINTS))
def test_two_train_steps_and_a_validation_step(dev, tmp_path, name):
    from toothgroupnetwork_amd import inference, training
    torch.manual_seed(17)
    np.random.seed(17)
    ckpt = str(tmp_path / "ckpts" / name)
    model = training.make_training_model(name, make_config(name, ckpt, opt="sgd" if name == "tgnet_fps" else "adam"))
    batches = list(synthetic_loader(tmp_path / "data", 2, POINTS[name]))
    before = _snapshot(model.module)
    lmap = model.step(0, batches[0], "train")
    grads = {n: p.grad for n, p in model.module.named_parameters() if p.requires_grad}
    used = {n for n, g in grads.items() if g is not None}
    # (a parameter the model's objective does not reach -- a head its loss does not read, PointNet++'s unused conv1 -- has no
    #  gradient, here as in the reference; every gradient there is must be finite, and every child with parameters must have some,
    #  but for the children listed here: DGCNN's offset and distance heads, and tsegnet's seg_module, which is built and not run
    #  when run_tooth_segmentation_module is False)
    assert used and all(bool(torch.isfinite(grads[n]).all()) for n in used)
    with_parameters = [n for n, m in model.module.named_children() if any(p.requires_grad for p in m.parameters())]
    children = [c for c in with_parameters if any(n == c or n.startswith(c + ".") for n in used)]
    unreached = {"dgcnn": {"offset_conv", "dist_conv"}, "tsegnet": {"seg_module"}}.get(name, set())
    assert set(with_parameters) - set(children) == unreached
    after = _snapshot(model.module)
    for child in children:
        assert any(not torch.equal(before[k], after[k]) for k in after if k.startswith(child + ".") and before[k].is_floating_point()), child
    maps = [lmap, model.step(1, batches[1], "train")]
    frozen = _snapshot(model.module)
    maps.append(model.step(0, batches[0], "test"))
    now = _snapshot(model.module)
    assert all(torch.equal(frozen[k], now[k]) for k in now), "a validation step changed a parameter or a running statistic"
    assert not model.module.training
    for lm, post_fix in zip(maps, ("train", "step", "val")):
        printed = lm.get_loss_dict_for_print(post_fix)
        assert f"total_{post_fix}" in printed and len(printed) >= 2 and all(np.isfinite(v) for v in printed.values()), printed
    want = {"tsegnet": {"dist_loss", "cent_loss", "chamf_loss"}, "tgnet_fps": set(training.FpsGroupingNetworkModel.TERMS)}.get(name, {"tooth_class_loss_1"})
    assert set(maps[0].loss_dict) == want
    model.save("train")
    fresh = type(model.module)(model.config)
    fresh.load_state_dict(torch.load(ckpt + ".h5"), strict=True)
    if name in INFERENCE_NAMES:
        pipe = inference.make_inference_pipeline(name, [ckpt + ".h5"])
        loaded = pipe.model.state_dict()
        assert all(torch.equal(loaded[k], v) for k, v in model.module.state_dict().items())
    model.load()


def test_tgnet_fps_constructs_with_zero_cbl_weights_only(dev, tmp_path):
    from toothgroupnetwork_amd import training
    cfg = make_config("tgnet_fps", str(tmp_path / "x"))
    del cfg["tr_set"]["loss"]["cbl_loss_1"], cfg["tr_set"]["loss"]["cbl_loss_2"]
    assert isinstance(training.make_training_model("tgnet_fps", cfg), training.FpsGroupingNetworkModel)
    cfg["tr_set"]["loss"]["cbl_loss_2"] = 0.5
    with pytest.raises(NotImplementedError, match="cbl_loss_2"):
        training.make_training_model("tgnet_fps", cfg)


# ---- 8. tsegnet with the segmentation module ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fx():
    return R.fixture()


@pytest.fixture(scope="module")
def restated(fx):
    inp = R.criterion_inputs(dict(np.load(os.path.join(GOLDEN, "reference_cpu_r11_tsegnet.npz"))))
    assert TC.case_digest(inp["case"]) == fx["crit_digest"][0], "the case no longer rebuilds the fixture's input"
    terms, ids, bins, kappa = R.six_terms_64(inp)
    return dict(inp=inp, terms=terms, ids=ids, bins=bins, kappa=kappa)


def _scripted_centroids(t, batch=1):
    rep = lambda a: a.expand(batch, *a.shape[1:]).contiguous()  # noqa: E731
    return lambda x: (rep(t["l0_points"]), None, x[:, :3, :], rep(t["l3_xyz"]), rep(t["offset"]), rep(t["dist"]))


@pytest.fixture(scope="module")
def forwarded(dev, restated):
    """nets.TSegNetModule on the criterion case with both stages scripted, and its six loss terms: computed once."""
    from toothgroupnetwork_amd import losses, nets
    t = {n: torch.from_numpy(v).to(dev) for n, v in restated["inp"]["case"].items()}
    net = nets.TSegNetModule({"run_tooth_segmentation_module": True}).to(dev).train()
    net.cent_module, net.seg_module = TC.Stage(_scripted_centroids(t)), TC.Stage(C.train_seg)
    np.random.seed(TC.PERM_SEED)
    out = net([t["feats"], t["labels"]])
    terms = losses.tsegnet_loss_terms(out, t["labels"])
    torch.cuda.synchronize()
    return dict(t=t, out=out, terms=terms)


def _check_terms(fx, restated, terms, T, k):
    assert list(terms) == list(R.NAMES)
    for i, name in enumerate(R.NAMES):
        exact, got, ref32 = float(fx["crit_64"][i]), float(terms[name].detach()), float(fx["crit_32"][i])
        if i < 3:
            # the fused kernels: the rule tests/test_gpu_losses.py holds them to -- twice the reference's own float32 error, floor 2e-5
            bound = max(2.0 * abs(ref32 - exact), 2e-5 * abs(exact))
        else:
            # (log2(n) + c) * 2^-24 relative, c written out in training_ref.forward_bound
            n, kappa = (T, restated["kappa"]) if name == "id_pred_loss" else (T * k, 1.0)
            bound = R.forward_bound(name, n, kappa) * abs(exact)
        print(f"  {name}: got {got:.9g} exact {exact:.12g} |got - exact| {abs(got - exact):.3e} reference fp32's {abs(ref32 - exact):.3e} bound {bound:.3e}")
        assert abs(got - exact) <= bound, (name, got, exact, bound)


def test_the_six_terms_equal_the_reference(fx, restated, forwarded):
    _check_terms(fx, restated, forwarded["terms"], TC.MAX_CROPS, TC.CROP_K)


def test_label_centroids_and_the_assignment_equal_the_reference(fx, forwarded):
    from toothgroupnetwork_amd import losses
    t, out = forwarded["t"], forwarded["out"]
    cent, exists = losses.seg_label_to_cent(t["feats"][:, :3, :], t["labels"])
    assert tuple(cent.shape) == (1, 3, 16) and cent.dtype == torch.float32 and exists.dtype == torch.bool
    assert np.array_equal(exists[0].cpu().numpy(), fx["crit_exists16"]), "the existing slots"
    # a float32 mean of n <= 24 000 coordinates of magnitude <= max|x|: (log2(n) + 1) * 2^-24 * max|x| absolute
    bound = (np.log2(TC.N_POINTS) + 1) * R.U * float(t["feats"][:, :3, :].abs().max())
    err = np.abs(cent[0].double().cpu().numpy() - fx["crit_cent16_64"])
    print(f"  centroids: max |got - exact| {err.max():.3e} bound {bound:.3e} reference fp32's {np.abs(fx['crit_cent16'] - fx['crit_cent16_64']).max():.3e}")
    assert err.max() <= bound
    assert torch.equal(losses.seg_label_to_cent(t["feats"], t["labels"][:, 0].int())[0], cent), "more channels, (B, N) int32 labels"
    ids, bins = losses.tsegnet_crop_targets(out["center_points"], cent, exists, out["cluster_gt_seg_label"])
    assert np.array_equal(ids.cpu().numpy(), fx["crit_ids"])
    assert np.array_equal(bins.reshape(bins.shape[0], -1).sum(1).cpu().numpy(), fx["crit_bin_count"])


def test_a_batch_of_the_same_scan_twice_gives_the_terms_of_one(fx, restated, forwarded):
    """Every scan's crops are assigned against that scan's own centroids: the second scan's labels are shifted by one tooth (its
    teeth 1..14 instead of 0..13) in the labels AND in its crops' labels, so an assignment against scan 0's slots would change the terms."""
    from toothgroupnetwork_amd import losses
    t, o = forwarded["t"], forwarded["out"]
    twice = {k: torch.cat([o[k], o[k]]) for k in ("l0_xyz", "l3_xyz", "offset_result", "dist_result", "pd_1", "weight_1", "pd_2")}
    shift = lambda lab: torch.where(lab >= 0, lab + 1, lab)  # noqa: E731
    twice["cluster_gt_seg_label"] = torch.cat([o["cluster_gt_seg_label"], shift(o["cluster_gt_seg_label"])])
    twice["id_pred"] = torch.cat([o["id_pred"], torch.roll(o["id_pred"], 1, dims=1)])       # the shifted scan's logits move with its ids
    twice["center_points"] = [o["center_points"], o["center_points"]]
    labels = torch.cat([t["labels"], shift(t["labels"])])
    terms = losses.tsegnet_loss_terms(twice, labels)
    _check_terms(fx, restated, terms, 2 * TC.MAX_CROPS, TC.CROP_K)


def _tsegnet_model(tmp_path, cent_stage):
    from toothgroupnetwork_amd import training
    cfg = make_config("tsegnet", str(tmp_path / "ckpts" / "tsegnet"))
    cfg["run_tooth_segmentation_module"] = True
    torch.manual_seed(5)
    model = training.TSegNetModel(cfg)
    model.module.cent_module = cent_stage.to(model.device)
    model.optimizer = training.build_optimizer(cfg["tr_set"], model.module.parameters())
    return model


def test_a_train_step_moves_the_segmentation_module(dev, tmp_path, forwarded):
    """Two crops instead of eight, to keep the step short: only the proposals that point at teeth 3 and 9 keep their distance, the
    others get 1.0 and fail the 0.3 filter."""
    from toothgroupnetwork_amd import losses
    t = dict(forwarded["t"])
    cent, _ = losses.seg_label_to_cent(t["feats"][:, :3, :], t["labels"])
    moved = t["l3_xyz"] + t["offset"]                                                   # (1, 3, 256)
    nearest = ((moved[:, :, :, None] - cent[:, :, None, :14]) ** 2).sum(1).argmin(dim=2)  # the case has teeth 0..13
    t["dist"] = torch.where(((nearest == 3) | (nearest == 9))[:, None, :], t["dist"], torch.ones_like(t["dist"]))
    model = _tsegnet_model(tmp_path, TC.Stage(_scripted_centroids(t)))
    before = _snapshot(model.module.seg_module)
    np.random.seed(TC.PERM_SEED)
    lmap = model.step(0, {"feat": t["feats"].cpu(), "gt_seg_label": t["labels"].cpu()}, "train")
    assert list(lmap.loss_dict) == list(R.NAMES) and [w for _, w in lmap.loss_dict.values()] == [1, 1, 0.1, 1, 1, 1]
    assert all(np.isfinite(v) for v in lmap.get_loss_dict_for_print("train").values())
    after = _snapshot(model.module.seg_module)
    moved = [k for k in after if after[k].is_floating_point() and not torch.equal(before[k], after[k])]
    assert any(k.startswith("sa1_1.") for k in moved) and any(k.startswith("pd_mask_2.") for k in moved) and any(k.startswith("fc2.") for k in moved)
    assert model.skipped_segmentation == 0


def test_a_scan_without_a_centre_trains_on_the_centroid_terms(dev, tmp_path, forwarded):
    t = dict(forwarded["t"])
    t["dist"] = torch.ones_like(t["dist"])                                  # no proposal passes the 0.3 filter
    stage = C.LearnedStage(_scripted_centroids(t), scaled=(4,))             # the offsets carry a gradient, so the step has one
    model = _tsegnet_model(tmp_path, stage)
    batch = {"feat": t["feats"].cpu(), "gt_seg_label": t["labels"].cpu()}
    with pytest.raises(ValueError, match="no centroid proposal"):
        model.module([t["feats"], t["labels"]])
    lmap = model.step(0, batch, "train")
    assert list(lmap.loss_dict) == list(R.NAMES[:3]) and model.skipped_segmentation == 1
    assert float(stage.gain.detach()) != 1.0, "training went on"
    model.step(1, batch, "test")
    assert model.skipped_segmentation == 2


# ---- 9. overfit ------------------------------------------------------------------------------------------------------------------------------

def test_thirty_steps_on_two_scans_lower_the_loss(dev, tmp_path):
    from toothgroupnetwork_amd import training
    torch.manual_seed(9)
    np.random.seed(9)
    cfg = make_config("pointnet", str(tmp_path / "ckpts" / "overfit"), every=1)
    model = training.make_training_model("pointnet", cfg)
    loader = synthetic_loader(tmp_path / "data", 2, POINTS["pointnet"])
    stream = io.StringIO()
    trainer = training.Trainer(config=cfg, model=model, gen_set=[[loader, loader]], stream=stream)
    for epoch in range(15):
        trainer.train(epoch, loader)
    totals = [json.loads(x)["total_step"] for x in stream.getvalue().splitlines()]
    print("  total_step:", " ".join(f"{v:.4f}" for v in totals))
    assert len(totals) == 30 and trainer.step_count == 30
    assert np.mean(totals[-5:]) < np.mean(totals[:5])


# ---- 10. the command line ----------------------------------------------------------------------------------------------------------------------

def test_the_command_line_trains_one_epoch_in_a_child_process(dev, tmp_path):
    from toothgroupnetwork_amd import eval_sharded
    data = tmp_path / "data"
    eval_sharded.write_synthetic_preprocessed(str(data), 3, n_points=POINTS["pointnet"])
    (tmp_path / "train.txt").write_text("SYN00000\nSYN00001\n")
    (tmp_path / "val.txt").write_text("SYN00002\n")
    (tmp_path / "pointnet.py").write_text("config = " + repr({"tr_set": make_config("pointnet", "")["tr_set"]}) + "\n")
    cmd = [sys.executable, os.path.join(REPO, "tools", "train.py"), "--model_name", "pointnet", "--config_path", str(tmp_path / "pointnet.py"),
           "--experiment_name", "cli", "--input_data_dir_path", str(data), "--train_data_split_txt_path", str(tmp_path / "train.txt"),
           "--val_data_split_txt_path", str(tmp_path / "val.txt"), "--epochs", "1", "--seed", "3"]
    done = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
    assert done.returncode == 0, done.stderr[-2000:]
    lines = [json.loads(x) for x in done.stdout.splitlines()]
    assert len(lines) == 2, done.stdout
    assert set(lines[0]) == {"step", "tooth_class_loss_1_step", "total_step", "step_lr"} and lines[0]["step"] == 0 and lines[0]["step_lr"] > 0
    assert set(lines[1]) == {"epoch", "step", "tooth_class_loss_1_train", "total_train", "tooth_class_loss_1_val", "total_val"}
    assert lines[1]["epoch"] == 0 and lines[1]["step"] == 1 and all(np.isfinite(v) for v in lines[1].values())
    assert "train_set 2" in done.stderr and "validation_set 1" in done.stderr
    for suffix in (".h5", "_val.h5"):
        state = torch.load(str(tmp_path / "ckpts" / ("cli" + suffix)))
        assert any(k.startswith("first_sem_model.") for k in state)


# ---- 11. one device read per step ------------------------------------------------------------------------------------------------------------------

def test_printing_a_loss_map_reads_the_device_once(dev, monkeypatch):
    from toothgroupnetwork_amd import training
    values = [torch.tensor(v, device=dev) for v in (0.5, 1.25, 3.0)]
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            values[0].item()
            supported = False
        except RuntimeError:
            supported = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not supported:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not catch a synchronising .item() on this torch build")
    lmap = training.LossMap()
    lmap.add_loss_by_dict({"a": (values[0], 1), "b": (values[1], 0.1), "c": (values[2], 0.03)})
    reads, tolist = [], torch.Tensor.tolist

    def one_read(self):
        torch.cuda.set_sync_debug_mode("default")
        try:
            reads.append(tuple(self.shape))
            return tolist(self)
        finally:
            torch.cuda.set_sync_debug_mode("error")
    monkeypatch.setattr(torch.Tensor, "tolist", one_read)
    try:
        torch.cuda.set_sync_debug_mode("error")
        printed = [lmap.get_loss_dict_for_print(p) for p in ("train", "step", "step")]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert reads == [(3,)], "one stacked read for the step's three dictionaries"
    assert printed[0] == {"a_train": 0.5, "b_train": 0.125, "c_train": 0.09, "total_train": 0.5 + 0.125 + 0.09}
