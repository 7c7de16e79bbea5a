#!/usr/bin/env python3
"""Fixtures of the training entry point (tests/golden/reference_cpu_r17_training.npz), produced by running the REFERENCE's own classes on
CPU in the build container (open3d / trimesh / wandb stubbed, `.cuda()` served):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_r17_training.py

  aug_*    augmentator.py: for every seed of training_cases.AUG_SEEDS, every single augmentation and the default chain on the (257, 6)
           and the (257, 3) array of training_cases.aug_arrays(): np.random.seed(seed), reload, augment; then the value of the next
           np.random.rand(), which proves how many draws were consumed.
  gen_*    generator.py: the items of DentalModelGenerator over a temporary directory of three tiny files and a split file that excludes
           one patient, without and with the default augmentation (np.random.seed(ITEM_SEED + k) in front of item k, because glob's
           order is the file system's).
  lr_*     models/base_model.py: the learning rates of BaseModel's scheduler for "exp" and "cosine", after construction and after
           each of 45 `scheduler.step(k)`, and `get_last_lr()[0]` at the same points.
  loop_*   trainer.py: the events of Trainer.train / Trainer.test with a recording fake model -- scheduler steps as (epoch, batch index,
           step count), save calls -- for the (loader length, schedueler_step) pairs of training_cases.LOADERS, and for validation
           losses 3, 2, 2.5.
  map_*    loss_meter.py: LossMap.get_loss_dict_for_print and LossMeter.get_avg_results on training_cases.LOSS_TERMS.
  crit_*   models/tsegnet_model.py, models/tsg_loss.py: TSegNetModel.step(.., "test") on training_cases.criterion_case() with the
           centroid stage scripted as in the r11 fixture and training_cases.train_seg as the segmentation stage: the six terms in
           float32; the reference's functions again on float64 copies of the same inputs; ops_utils.seg_label_to_cent's 16 slots; the
           crop ids (pred_centerpoint_gt_label_ls).  Asserted: the crops are the r11 fixture's, and no crop centre is equidistant
           from two centroids."""
import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("TGN_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import training_cases as C  # noqa: E402
import tsegnet_cases as TC  # noqa: E402
from crop_cases import pack_sets  # noqa: E402
from make_golden import load_reference  # noqa: E402
from make_golden_r2_io import _stub_open3d  # noqa: E402
from make_golden_r3 import cpu_as_cuda  # noqa: E402


def _reference_modules():
    load_reference()
    sys.modules["open3d"] = _stub_open3d([])
    sys.modules.setdefault("trimesh", types.ModuleType("trimesh"))
    sys.modules["wandb"] = types.ModuleType("wandb")
    if REFERENCE not in sys.path:
        sys.path.append(REFERENCE)
    import augmentator
    import generator
    import loss_meter
    import ops_utils
    import trainer
    import models.base_model as base_model
    import models.modules.tsegnet as tsegnet_module
    import models.tsegnet_model as tsegnet_model
    import models.tsg_loss as tsg_loss
    mods = dict(aug=augmentator, gen=generator, lm=loss_meter, ou=ops_utils, trainer=trainer, base=base_model, TM=tsegnet_module,
                model=tsegnet_model, loss=tsg_loss)
    assert all(m.__file__.startswith(REFERENCE) for m in mods.values())
    return types.SimpleNamespace(**mods)


def augmentation_part(out, R):
    aug = R.aug                                                        # the configuration strings say `aug.`
    six, three = C.aug_arrays()
    for seed in C.AUG_SEEDS:
        for name, text in list(C.SINGLES.items()) + [("chain", C.DEFAULT_CHAIN)]:
            nexts = []
            for tag, base in (("6", six), ("3", three)):
                obj = eval(text)
                np.random.seed(seed)
                if name == "chain":
                    obj.reload_vals()
                    got = obj.run(base.copy())
                else:
                    obj.reload_val()
                    got = obj.augment(base.copy())
                nexts.append(np.random.rand())
                assert got.dtype == np.float32 and got.shape == base.shape
                out[f"aug_{seed}_{name}_{tag}"] = got
            assert nexts[0] == nexts[1]
            out[f"aug_{seed}_{name}_next"] = np.array(nexts[0])
    print(f"  aug: {len(C.AUG_SEEDS)} seeds x {len(C.SINGLES) + 1} augmentations x 2 widths")


def generator_part(out, R):
    with tempfile.TemporaryDirectory() as root:
        for k, name in enumerate(C.PATIENTS):
            np.save(os.path.join(root, f"{name}_sampled_points.npy"), C.patient_file(k))
        split = os.path.join(root, "split.txt")
        with open(split, "w") as f:
            f.write("".join(f" {p} \n" for p in C.SPLIT))
        for tag, text in (("plain", None), ("aug", C.DEFAULT_CHAIN)):
            ds = R.gen.DentalModelGenerator(root, split, text)
            names = sorted(os.path.basename(p)[:-len("_sampled_points.npy")] for p in ds.mesh_paths)
            assert names == [n for n in C.PATIENTS if n.split("_")[0] in C.SPLIT], names
            for i in range(len(ds)):
                name = os.path.basename(ds.mesh_paths[i])[:-len("_sampled_points.npy")]
                np.random.seed(C.ITEM_SEED + C.PATIENTS.index(name))
                item = ds[i]
                assert set(item) == {"feat", "gt_seg_label", "aug_obj", "mesh_path"}
                assert item["feat"].dtype == torch.float32 and item["gt_seg_label"].dtype == torch.int64
                assert (item["aug_obj"] is None) == (text is None) and (text is None or item["aug_obj"] is not ds.aug_obj)
                out[f"gen_{tag}_{name}_feat"] = item["feat"].numpy().copy()
                out[f"gen_{tag}_{name}_label"] = item["gt_seg_label"].numpy().astype(np.int8)
    print(f"  gen: {len(names)} of {len(C.PATIENTS)} patients in the split, feat {tuple(item['feat'].shape)}, label {tuple(item['gt_seg_label'].shape)}")


def _tr_set(sched):
    return {"tr_set": {"optimizer": {"lr": C.LR["lr"], "NAME": "adam", "weight_decay": 1.0e-4},
                       "scheduler": {"sched": sched, "warmup_epochs": 0, "full_steps": C.LR["full_steps"], "schedueler_step": 2,
                                     "min_lr": C.LR["min_lr"], "step_decay": C.LR["step_decay"]}}}


def scheduler_part(out, R):
    class Model(R.base.BaseModel):
        def get_loss(self):
            pass

        def step(self, batch_idx, batch_item):
            pass
    import warnings
    for sched in ("exp", "cosine"):
        model = Model(_tr_set(sched), lambda config: torch.nn.Linear(3, 2))
        lrs, last = [model.optimizer.param_groups[0]["lr"]], [model.scheduler.get_last_lr()[0]]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for k in range(1, C.LR["steps"] + 1):
                model.scheduler.step(k)
                lrs.append(model.optimizer.param_groups[0]["lr"])
                last.append(model.scheduler.get_last_lr()[0])
        out[f"lr_{sched}"], out[f"lr_{sched}_last"] = np.array(lrs, np.float64), np.array(last, np.float64)
        print(f"  lr {sched}: {lrs[0]:.3e} -> {lrs[1]:.3e} ... {lrs[-1]:.3e}")


class _FakeMap:
    def __init__(self, value):
        self.value = value

    def get_loss_dict_for_print(self, post_fix):
        return {f"a_{post_fix}": self.value, f"total_{post_fix}": self.value}


class _FakeModel:
    """Records what the trainer does to it."""

    def __init__(self, events, val_losses=()):
        self.events, self.val_losses, self.scheduler, self.epoch, self.batch = events, list(val_losses), self, 0, -1

    def step(self, *args):
        if len(args) == 1:                                         # the scheduler's step(step_count)
            self.events.append(f"sched {self.epoch} {self.batch} {args[0]}")
            return None
        batch_idx, _, phase = args
        self.batch = batch_idx
        return _FakeMap(self.val_losses[self.epoch] if phase == "test" else 1.0)

    def get_last_lr(self):
        return [0.0]

    def save(self, phase):
        self.events.append(f"save {self.epoch} {phase}")


def trainer_part(out, R):
    for length, every in C.LOADERS:
        events = []
        cfg = _tr_set("exp")
        cfg["tr_set"]["scheduler"]["schedueler_step"] = every
        cfg["wandb"] = {"wandb_on": False}
        model = _FakeModel(events)
        t = R.trainer.Trainer(config=cfg, model=model, gen_set=None)
        for epoch in range(2):
            model.epoch = epoch
            t.train(epoch, [{}] * length)
        out[f"loop_{length}_{every}"] = np.array(events)
        print(f"  loop ({length}, {every}): {events}")
    events = []
    cfg = _tr_set("exp")
    cfg["wandb"] = {"wandb_on": False}
    model = _FakeModel(events, C.VAL_LOSSES)
    t = R.trainer.Trainer(config=cfg, model=model, gen_set=None)
    for epoch in range(len(C.VAL_LOSSES)):
        model.epoch = epoch
        t.test(epoch, [{}], True)
    out["loop_val"] = np.array(events)
    out["loop_val_best"] = np.array(t.best_val_loss)
    print(f"  loop val: {events}, best {t.best_val_loss}")


def loss_map_part(out, R):
    meter = R.lm.LossMeter()
    for n, terms in enumerate((C.LOSS_TERMS, C.LOSS_TERMS_2)):
        lmap = R.lm.LossMap()
        lmap.add_loss_by_dict({name: (torch.tensor(value, dtype=torch.float32), weight) for name, value, weight in terms})
        printed = lmap.get_loss_dict_for_print("train")
        meter.aggr(printed)
        out[f"map_{n}"] = np.array(json.dumps(printed))
        out[f"map_{n}_sum"] = np.array(float(lmap.get_sum()), np.float64)
    out["map_avg"] = np.array(json.dumps(meter.get_avg_results()))
    print(f"  map: {printed}")


def criterion_part(out, R):
    case = C.criterion_case()
    t = {n: torch.from_numpy(v) for n, v in case.items()}
    net = R.TM.TSegNetModule({"run_tooth_segmentation_module": True})
    net.cent_module = TC.Stage(lambda x: (t["l0_points"], None, x[:, :3, :], t["l3_xyz"], t["offset"], t["dist"]))
    net.seg_module = TC.Stage(C.train_seg)
    model = R.model.TSegNetModel.__new__(R.model.TSegNetModel)
    model.config, model.module = {"run_tooth_segmentation_module": True}, net
    seen = {}
    keep = (R.ou.seg_label_to_cent, R.loss.segmentation_loss, R.ou.get_nearest_neighbor_idx)

    def cents(*a):
        seen["cent"] = keep[0](*a)
        return seen["cent"]

    def seg_loss(*a):
        seen["seg_args"] = a
        return keep[1](*a)

    def nn_idx(*a, **k):
        seen["idx"] = keep[2](*a, **k)
        return seen["idx"]
    R.ou.seg_label_to_cent, R.loss.segmentation_loss, R.ou.get_nearest_neighbor_idx = cents, seg_loss, nn_idx
    keep_forward = net.forward

    def forward(inputs):
        seen["out"] = keep_forward(inputs)
        return seen["out"]
    net.forward = forward
    import warnings
    try:
        np.random.seed(TC.PERM_SEED)
        with cpu_as_cuda(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            lmap = model.step(0, {"feat": t["feats"], "gt_seg_label": t["labels"]}, "test")
    finally:
        R.ou.seg_label_to_cent, R.loss.segmentation_loss, R.ou.get_nearest_neighbor_idx = keep
    names = ("dist_loss", "cent_loss", "chamf_loss", "seg_1_loss", "seg_2_loss", "id_pred_loss")
    assert tuple(lmap.loss_dict) == names, tuple(lmap.loss_dict)
    assert [lmap.loss_dict[n][1] for n in names] == [1, 1, 0.1, 1, 1, 1]
    o = seen["out"]
    idx = np.asarray(seen["idx"][0])
    r11 = np.load(os.path.join(HERE, "reference_cpu_r11_tsegnet.npz"))
    assert np.array_equal(pack_sets(idx), r11["mod_idxset"]), "the crops are not the r11 fixture's"
    centres = np.asarray(o["center_points"])
    assert np.array_equal(centres[0].view(np.uint32), r11["mod_cent_bits"][r11["mod_perm"].astype(np.int64)])
    cent16, exists16 = seen["cent"]
    pd_1, weight_1, pd_2, id_pred, ids, bins = seen["seg_args"]
    # uniqueness of the assignment: the two nearest existing centroids of every crop centre, in float64
    ex = exists16.reshape(-1).numpy() > 0
    gt = cent16[0].numpy().astype(np.float64).T[ex]                                     # (C, 3)
    d = ((centres[0].astype(np.float64)[:, None, :] - gt[None]) ** 2).sum(-1)
    two = np.sort(d, axis=1)[:, :2]
    assert np.all(two[:, 1] - two[:, 0] > 1e-6 * two[:, 1]), "a crop centre is equidistant from two centroids"
    assert np.array_equal(np.flatnonzero(ex)[d.argmin(1)] + 1, ids.reshape(-1).numpy().astype(np.int64))
    v32 = np.array([float(lmap.loss_dict[n][0]) for n in names], np.float64)
    # ... and the reference's own functions on float64 copies of the same inputs
    with cpu_as_cuda(torch.DoubleTensor):
        c64, e64 = keep[0](t["feats"][:, :3, :].double(), t["labels"])
        compact = c64.double()[:, :, e64.reshape(-1) > 0]
        cent_terms = R.loss.centroid_loss(o["offset_result"].double(), o["l3_xyz"].double(), o["dist_result"].double(), compact)
        seg_terms = (R.loss.first_seg_loss(pd_1.double(), weight_1.double(), bins),
                     _second_seg_loss_64(R, pd_2.double(), weight_1.double(), bins.double()),
                     R.loss.id_loss(ids, id_pred.double()))
    v64 = np.array([float(x) for x in cent_terms + seg_terms], np.float64)
    assert all(x.dtype == torch.float64 for x in cent_terms + seg_terms)
    for n, a, b in zip(names, v32, v64):
        print(f"  crit {n}: fp32 {a:.9g} fp64 {b:.12g} rel {abs(a - b) / abs(b):.2e}")
    out["crit_names"] = np.array(names)
    out["crit_32"], out["crit_64"] = v32, v64
    out["crit_cent16"] = np.where(ex[None, :], cent16[0].numpy().astype(np.float32), np.float32(0))
    out["crit_cent16_64"] = np.where(ex[None, :], c64[0].numpy().astype(np.float64), 0.0)
    out["crit_exists16"] = ex
    out["crit_ids"] = ids.reshape(-1).numpy().astype(np.int64)
    out["crit_bin_count"] = bins.reshape(bins.shape[0], -1).sum(1).numpy().astype(np.int64)
    out["crit_digest"] = np.array([TC.case_digest(case)])


def _second_seg_loss_64(R, pd_2, weight_1, gt_bin):
    """tsg_loss.second_seg_loss casts its labels to float32, which BCEWithLogitsLoss refuses next to float64 logits: the same function
    with torch.float32 standing for float64 while it runs (the labels are 0 and 1, exact in both)."""
    keep = torch.float32
    torch.float32 = torch.float64
    try:
        return R.loss.second_seg_loss(pd_2, weight_1, gt_bin)
    finally:
        torch.float32 = keep


def main():
    torch.set_num_threads(8)
    out = {}
    R = _reference_modules()
    keep = torch.nn.Module.cuda
    torch.nn.Module.cuda = lambda self, *a, **k: self
    try:
        augmentation_part(out, R)
        generator_part(out, R)
        scheduler_part(out, R)
        trainer_part(out, R)
        loss_map_part(out, R)
        criterion_part(out, R)
    finally:
        torch.nn.Module.cuda = keep
    path = os.path.join(HERE, "reference_cpu_r17_training.npz")
    np.savez_compressed(path, **out)
    print(f"wrote tests/golden/reference_cpu_r17_training.npz ({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
