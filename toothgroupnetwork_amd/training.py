"""The training entry point: what start_train.py chains in the reference -- generator.py, runner.py, loss_meter.py, trainer.py,
models/base_model.py and the seven models/*_model.py steps -- over this package's modules (nets.py), augmentations (augment.py) and
criteria (losses.py).  No new kernel: the hot path of a step is the module's forward and backward and the fused losses, which are
HIP already; this is the layer above them.

  DentalModelGenerator, collate_fn, get_generator_set   generator.py, runner.py:7-50
  load_item, LossMeter, LossMap                         generator.py:40-66 at batch size 1, loss_meter.py
  build_optimizer, build_scheduler, CosineSchedule      BaseModel.__init__ (models/base_model.py:16-28)
  TrainingModel and one step class per model name       BaseModel and models/*_model.py
  BoundarySampler                                       models/bdl_grouping_netowrk_model.py:20-35, 56-192, over tgnet.py's device functions
  make_training_model                                   start_train.py:22-49
  Trainer                                               trainer.py

Where it differs from the reference on purpose:
  * LossMap.get_loss_dict_for_print reads all terms with ONE device-to-host copy and keeps the values for the step's other post-fixes;
    the reference calls .item() per term and post-fix: nine synchronisations for a three-term step, where this has one.
  * no wandb: the trainer writes one JSON line per scheduler step and per epoch to a stream of the caller's;
    torch.cuda.empty_cache() per step is not mirrored; Trainer.run takes the number of epochs.
  * tgnet_fps trains on its five geometric and class terms and, with tr_set["contrastive_boundary"] true, on the contrastive-boundary
    terms cbl_loss_1 / cbl_loss_2 (losses.contrast_boundary_loss) with the configuration's weights.  Without that key a non-zero
    weight for either is refused, for tgnet_bdl too.  Nothing here trains silently on another objective than the configuration names.
    The criterion runs in the train phase only; the reference computes it in validation too and throws the value away.
  * tgnet_bdl (BoundarySampler, BdlGroupingNetworkModel): the frozen first module runs in eval mode, so it is a function of its
    checkpoint (the reference leaves it in train mode and its BatchNorm statistics drift); the k-means behind the boundary flags draws
    nothing from numpy's generator; the cache file is written under a temporary name and renamed; a duplicate or missing base name, a
    scan without foreground and one with too few non-boundary rows raise naming the scan.  BoundarySampler's docstring has the list.
  * tsegnet: a batch for which no tooth centre survives the join (early in a run, nets.TSegNetModule.forward(on_no_centre="skip"))
    contributes its three centroid terms only and is counted in `skipped_segmentation`; the reference would fail there.
  * the cosine schedule is what build_scheduler_from_cfg really builds from a dict: every `getattr(args, ..., default)` of
    scheduler_factory.py returns its default, so there is no warm-up, one cycle of `full_steps` steps from lr to min_lr, and min_lr after.
"""
import copy
import glob
import hashlib
import json
import math
import os
import sys

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from . import augment, config as switches, losses, nets, preprocess, tgnet

MODEL_NAMES = ("tgnet_fps", "tsegnet", "dgcnn", "pointnet", "pointnetpp", "pointtransformer", "tgnet_bdl")
SCHEDULERS = ("exp", "cosine")
OPTIMIZERS = ("sgd", "adam")
STACKED_KEYS = ("feat", "gt_seg_label", "uniform_feat", "uniform_gt_seg_label")      # runner.py:17


# ---- data -------------------------------------------------------------------------------------------------------------------------

def load_item(path):
    """One validation item the way generator.py:40-66 builds it (no augmentation), already batched by the loader's
    collate (runner.py:7-19) at batch size 1: feat (1, 6, N) fp32, gt_seg_label (1, 1, N) int64 with gingiva = -1."""
    arr = np.load(path)
    # (layout changes in numpy: torch's CPU kernels would fan a 144 000-element copy out over every hardware thread of the box --
    #  25 ms per scan on a 128-thread host under a 16-core quota, against 3 ms for the forward itself)
    feat = np.ascontiguousarray(arr[:, :6].T, dtype=np.float32)[None]
    seg = np.ascontiguousarray(arr[:, 6:].T.astype(np.int64) - 1)[None]
    return {"feat": torch.from_numpy(feat), "gt_seg_label": torch.from_numpy(seg), "mesh_path": [path]}


class DentalModelGenerator(Dataset):
    """generator.py:10-71: the `*_sampled_points.npy` files of data_dir, optionally only the patients of a split file (the patient id
    is the file name up to its first underscore, and must be a stripped line of the file).  An item is feat (6, N) float32,
    gt_seg_label (1, N) int64 with gingiva = -1, aug_obj (a deep copy of the augmentation as it was applied, None without) and
    mesh_path.  With an augmentation: reload_vals(), then run, per item.

    The un-augmented item is load_item's without its batch axis: the two build the same arrays (the columns, the float32
    cast, the `- 1`); load_item adds the loader's batch axis of 1 and wraps mesh_path in a list, which is what collate_fn does to
    one item.  The file order is glob's, as in the reference; eval_sharded.list_preprocessed sorts."""

    def __init__(self, data_dir=None, split_with_txt_path=None, aug_obj_str=None):
        self.data_dir = data_dir
        self.mesh_paths = glob.glob(os.path.join(data_dir, "*_sampled_points.npy"))
        if split_with_txt_path:
            with open(split_with_txt_path) as f:
                self.split_base_name_ls = [line.strip() for line in f]
            self.mesh_paths = [p for p in self.mesh_paths if os.path.basename(p).split("_")[0] in self.split_base_name_ls]
        self.aug_obj = augment.from_config_string(aug_obj_str)

    def __len__(self):
        return len(self.mesh_paths)

    def __getitem__(self, idx):
        path = self.mesh_paths[idx]
        item = load_item(path.strip())
        feat, seg_label = item["feat"][0], item["gt_seg_label"][0]
        if self.aug_obj:
            self.aug_obj.reload_vals()
            rows = np.ascontiguousarray(feat.numpy().T)                     # (N, 6) float32, as the reference hands it over
            feat = torch.from_numpy(self.aug_obj.run(rows)).permute(1, 0)
        return {"feat": feat, "gt_seg_label": seg_label, "aug_obj": copy.deepcopy(self.aug_obj), "mesh_path": path}


def collate_fn(batch):
    """runner.py:7-19: every key becomes the list of the items' values; the tensor keys are stacked."""
    output = {}
    for batch_item in batch:
        for key, value in batch_item.items():
            output.setdefault(key, []).append(value)
    for key in output:
        if key in STACKED_KEYS:
            output[key] = torch.stack(output[key])
    return output


def get_generator_set(config):
    """runner.py:26-50 on config["generator"]'s dict: [train loader (shuffled, augmented), validation loader (neither)]."""
    train = DataLoader(DentalModelGenerator(config["input_data_dir_path"], aug_obj_str=config["aug_obj_str"],
                                            split_with_txt_path=config["train_data_split_txt_path"]),
                       shuffle=True, batch_size=config["train_batch_size"], collate_fn=collate_fn)
    val = DataLoader(DentalModelGenerator(config["input_data_dir_path"], aug_obj_str=None,
                                          split_with_txt_path=config["val_data_split_txt_path"]),
                     shuffle=False, batch_size=config["val_batch_size"], collate_fn=collate_fn)
    return [train, val]


# ---- losses of a step ---------------------------------------------------------------------------------------------------------------

class LossMeter:
    """loss_meter.py:2-23: running sums per key and a step count; averages on request."""

    def __init__(self):
        self.init()

    def init(self):
        self.step_num = 0
        self.loss_meter_dict = {}

    def aggr(self, loss_map):
        for key, value in loss_map.items():
            self.loss_meter_dict[key] = self.loss_meter_dict.get(key, 0) + value
        self.step_num += 1

    def get_avg_results(self):
        return {key: total / self.step_num for key, total in self.loss_meter_dict.items()}


class LossMap:
    """loss_meter.py:26-61: named (value, weight) terms of one step.  get_sum() is the weighted sum the step differentiates;
    get_loss_dict_for_print(post_fix) is {"<term>_<post_fix>": value * weight, ..., "total_<post_fix>": their sum} as python floats.
    add_value(name, tensor) attaches a reported value that is no loss term (a score): read with the terms, printed as
    "<name>_<post_fix>" behind the total, part of neither get_sum() nor the total."""

    def __init__(self):
        self.loss_dict = {}
        self.value_dict = {}
        self._host = None

    def add_value(self, name, value):
        if name in self.loss_dict or name in self.value_dict:
            raise KeyError(f"LossMap already holds {name!r}")
        self.value_dict[name] = value
        self._host = None

    def add_loss(self, name, value, weight):
        self.loss_dict[name] = (value, weight)
        self._host = None

    def add_loss_by_dict(self, loss_dict):
        for key, (value, weight) in loss_dict.items():
            if key in self.loss_dict:
                raise KeyError(f"LossMap already holds a term named {key!r}")
            self.add_loss(key, value, weight)

    def del_loss(self, name):
        del self.loss_dict[name]
        self._host = None

    def get_sum(self):
        summation = 0
        for value, weight in self.loss_dict.values():
            summation = summation + value * weight
        return summation

    def _values_on_host(self):
        """Every term's and reported value's python float: the tensors are stacked on their device and read with ONE .tolist() -- one
        copy, one synchronisation, whatever their number -- and kept, because a step's map is printed under up to three
        post-fixes (trainer.py:33-35).  A float32 value becomes the same python float that .item() gives, also beside reported
        values, with which the stack is float64: every float32 is a float64, and .item() widens it the same way."""
        if self._host is None:
            values = [(n, v) for n, (v, _) in self.loss_dict.items()] + list(self.value_dict.items())
            tensors = [(n, v) for n, v in values if isinstance(v, torch.Tensor)]
            host = {n: float(v) for n, v in values if not isinstance(v, torch.Tensor)}
            if len(tensors) == 1:
                host[tensors[0][0]] = tensors[0][1].item()                                 # a single one is read where it lies
            elif tensors:
                cells = [v.detach().reshape(()) for _, v in tensors]
                if self.value_dict:
                    cells = [c.double() for c in cells]
                host.update(zip([n for n, _ in tensors], torch.stack(cells).tolist()))     # the one read
            self._host = host
        return self._host

    def get_loss_dict_for_print(self, post_fix):
        host = self._values_on_host()
        out = {f"{name}_{post_fix}": host[name] * weight for name, (_, weight) in self.loss_dict.items()}
        total = 0
        for value in out.values():
            total += value
        out[f"total_{post_fix}"] = total
        out.update((f"{name}_{post_fix}", host[name]) for name in self.value_dict)
        return out


# ---- optimiser and schedule -----------------------------------------------------------------------------------------------------------

def build_optimizer(tr_set, parameters):
    """models/base_model.py:16-19 on config["tr_set"]."""
    opt = tr_set["optimizer"]
    if opt["NAME"] == "sgd":
        return torch.optim.SGD(parameters, lr=opt["lr"], momentum=opt["momentum"], weight_decay=opt["weight_decay"])
    if opt["NAME"] == "adam":
        return torch.optim.Adam(parameters, lr=opt["lr"], weight_decay=opt["weight_decay"])
    raise ValueError(f"optimizer NAME = {opt['NAME']!r}: the supported ones are {', '.join(OPTIMIZERS)}")


class CosineSchedule:
    """The CosineLRScheduler that build_scheduler_from_cfg returns for the dict BaseModel hands it (see the module docstring): no
    warm-up, no noise, one cycle.  step(t) sets every group's rate to min_lr + (base - min_lr) / 2 * (1 + cos(pi t / full_steps)) for
    t < full_steps and to min_lr from there on; `base` is the group's rate at construction.  get_last_lr() is the reference's: the
    rates of the step AFTER the last one given to step()."""

    def __init__(self, optimizer, full_steps, min_lr):
        if min_lr < 0:
            raise ValueError(f"min_lr must not be negative, got {min_lr}")
        self.optimizer, self.t_initial, self.lr_min, self.epoch = optimizer, full_steps, min_lr, -1
        for group in optimizer.param_groups:
            group.setdefault("initial_lr", group["lr"])
        self.base_values = [group["initial_lr"] for group in optimizer.param_groups]
        self._set(self.base_values)

    def _set(self, values):
        for group, value in zip(self.optimizer.param_groups, values):
            group["lr"] = value

    def _get_lr(self, t):
        if t // self.t_initial >= 1:
            return [self.lr_min for _ in self.base_values]
        return [self.lr_min + 0.5 * (base - self.lr_min) * (1 + math.cos(math.pi * t / self.t_initial)) for base in self.base_values]

    def step(self, epoch):
        self.epoch = epoch
        self._set(self._get_lr(epoch))

    def get_last_lr(self):
        return self._get_lr(self.epoch + 1)


def check_scheduler(tr_set):
    sched = tr_set["scheduler"]["sched"]
    if sched not in SCHEDULERS:
        raise ValueError(f"sched = {sched!r}: the supported schedulers are {' and '.join(SCHEDULERS)}")


def build_scheduler(tr_set, optimizer):
    """models/base_model.py:21-28 on config["tr_set"]: "exp" is torch's ExponentialLR(step_decay), "cosine" is CosineSchedule."""
    check_scheduler(tr_set)
    sched = tr_set["scheduler"]
    if sched["sched"] == "exp":
        return torch.optim.lr_scheduler.ExponentialLR(optimizer, sched["step_decay"])
    return CosineSchedule(optimizer, sched["full_steps"], sched["min_lr"])


# ---- the same bits from the same seed -------------------------------------------------------------------------------------------------------

# model name -> the operator that stands between it and a bit-reproducible step, found by tools/reproducible_audit.py (DESIGN.md
# section 4.2 has the method and the per-model outcome).  make_training_model refuses these names when tr_set["reproducible"] is set.
NOT_REPRODUCIBLE = {}


def set_reproducible(seed=None, warn_only=False):
    """Switch the process to the forms that give the same bits on every run (same machine, same build, same seed, same data order):
    the gather family's backward along reverse lists (config.cfg.ordered_backward) and the fused BatchNorm's column sums in a fixed
    order (config.cfg.ordered_bn), both in ordered.py; torch.use_deterministic_algorithms, under which a torch operator that torch
    knows to be non-deterministic raises and names itself (warn_only: warns); torch.backends.cudnn.deterministic on and .benchmark
    off, which torch-ROCm hands to MIOpen's choice of solver.  seed: torch's generators on every device (numpy's is the caller's).
    Only ever switches ON; tr_set["reproducible"] and tools/train.py --reproducible end here."""
    switches.cfg.ordered_backward = True
    switches.cfg.ordered_bn = True
    torch.use_deterministic_algorithms(True, warn_only=warn_only)
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False
    if seed is not None:
        torch.manual_seed(seed)


def state_digest(model):
    """sha256 over the tensors of model.module.state_dict(), in key order, each as its bytes: what two runs compare instead of
    loading each other's checkpoints.  One device-to-host copy (the tensors are packed into one byte buffer on the device first)."""
    tensors = [v.detach().contiguous().view(-1).view(torch.uint8) for _, v in sorted(model.module.state_dict().items()) if v.numel()]
    packed = torch.cat(tensors) if tensors else torch.empty(0, dtype=torch.uint8)
    return hashlib.sha256(packed.cpu().numpy().tobytes()).hexdigest()


# ---- model steps ------------------------------------------------------------------------------------------------------------------------

class TrainingModel:
    """models/base_model.py: the module in train mode on the GPU, its optimiser and its scheduler; step / save / load.

    evaluate(batch_item, phase) -> (output, LossMap): the forward and its terms; phase "train" runs it in train mode with a graph,
    "val" and "test" in eval mode under torch.no_grad().  The batch moves to the device here.
    step(batch_idx, batch_item, phase) -> LossMap: evaluate and, for "train", the weighted sum's backward and an optimiser step.
    A subclass names its module class and gives `losses_of(output, seg_label, points)` -> {name: (value, weight)}.

    trainable=False is a model that is only evaluated (validation over a checkpoint): the module starts in eval mode, there is no
    optimiser and no scheduler, the configuration needs no section for either, and step(..., "train") raises.

    tr_set["ordered_backward"] true sets config.cfg.ordered_backward for the process (ordered.py; tools/train.py --ordered_backward).
    tr_set["reproducible"] true is set_reproducible() for the process: same seed, same data order, same bits."""

    module_class = None

    def __init__(self, config, module=None, trainable=True):
        self.config, self.trainable = config, trainable
        self.check_config(config, trainable)
        if config.get("tr_set", {}).get("ordered_backward"):
            # the package's switch (config.cfg.ordered_backward): every gather-family backward from here on sums along reverse
            # lists, without float atomics.  Only ever switched ON from a configuration: absent or false leaves the switch as it is
            switches.cfg.ordered_backward = True
        if config.get("tr_set", {}).get("reproducible"):
            set_reproducible()
        if not torch.cuda.is_available():
            raise RuntimeError("training needs a GPU: the modules' operators are HIP kernels and have no CPU fallback")
        self.device = torch.device("cuda")
        self.module = (module or self.module_class)(config)
        self.module.train(trainable)
        self.module.cuda()
        if trainable:
            self.optimizer = build_optimizer(config["tr_set"], self.module.parameters())
            self.scheduler = build_scheduler(config["tr_set"], self.optimizer)

    @classmethod
    def check_config(cls, config, trainable=True):
        """What can be refused before anything is built: raises for a configuration this class does not train."""
        if not trainable:
            return
        check_scheduler(config["tr_set"])
        name = config["tr_set"]["optimizer"]["NAME"]
        if name not in OPTIMIZERS:
            raise ValueError(f"optimizer NAME = {name!r}: the supported ones are {', '.join(OPTIMIZERS)}")

    def _set_model(self, phase):
        if phase not in ("train", "val", "test"):
            raise ValueError(f"phase must be 'train', 'val' or 'test', got {phase!r}")
        # only when the phase changes: Module.train() walks every submodule, 1.4 ms of a 75 ms tgnet_fps step when it runs per step
        # (tools/training_bench.py, profiles/r17_training.txt)
        if self.module.training != (phase == "train"):
            self.module.train(phase == "train")

    def load(self):
        self.module.load_state_dict(torch.load(self.config["checkpoint_path"] + ".h5"))

    def save(self, phase):
        if phase not in ("train", "val"):
            raise ValueError(f"save: phase must be 'train' or 'val', got {phase!r}")
        folder = os.path.dirname(self.config["checkpoint_path"])
        if folder:
            os.makedirs(folder, exist_ok=True)
        torch.save(self.module.state_dict(), self.config["checkpoint_path"] + (".h5" if phase == "train" else "_val.h5"))

    def forward(self, inputs):
        return self.module(inputs)

    def losses_of(self, output, seg_label, points):
        raise NotImplementedError

    def evaluate(self, batch_item, phase):
        if phase == "train" and not self.trainable:
            raise RuntimeError("this model was built with trainable=False: it has no optimiser, so it has no train phase")
        self._set_model(phase)
        points = batch_item["feat"].to(self.device)
        seg_label = batch_item["gt_seg_label"].to(self.device)
        if phase == "train":
            output = self.forward([points, seg_label])
        else:
            with torch.no_grad():
                output = self.forward([points, seg_label])
        loss_meter = LossMap()
        loss_meter.add_loss_by_dict(self.losses_of(output, seg_label, points))
        return output, loss_meter

    def step(self, batch_idx, batch_item, phase):
        _, loss_meter = self.evaluate(batch_item, phase)
        if phase == "train":
            loss_sum = loss_meter.get_sum()
            self.optimizer.zero_grad()
            loss_sum.backward()
            self.optimizer.step()
        return loss_meter


class _ClassModel(TrainingModel):
    """The four semantic models: tooth_class_loss (cross entropy on label + 1, tgn_loss.py:355-367) of one output, weight 1.
    val_terms names the terms of the test phase: the fixed schema a sharded validation (eval_sharded.ModelStep) reports under."""

    output_key, weight = "cls_pred", 1
    val_terms = ("tooth_class_loss_1",)

    def get_loss(self, gt_seg_label_1, sem_1):
        return {"tooth_class_loss_1": (losses.tooth_class_loss(sem_1, gt_seg_label_1), self.weight)}

    def losses_of(self, output, seg_label, points):
        return self.get_loss(seg_label, output[self.output_key])


class PointFirstModel(_ClassModel):
    """models/pointnet_model.py ("pointnet")."""
    module_class = nets.PointFirstModule


class PointPpFirstModel(_ClassModel):
    """models/pointnet_pp_model.py ("pointnetpp")."""
    module_class = nets.PointPpFirstModule


class DGCnnModel(_ClassModel):
    """models/dgcnn_model.py ("dgcnn")."""
    module_class = nets.DGCnnModule


class TransformerModel(_ClassModel):
    """models/transformer_model.py ("pointtransformer"): the term is read from "sem_1" and weighted by the configuration's
    tr_set.loss.tooth_class_loss_1; get_loss takes (sem_1, gt_seg_label_1), the reference's order for this model."""
    module_class, output_key = nets.PointTransformerModule, "sem_1"

    def __init__(self, config, module=None, trainable=True):
        self.weight = config["tr_set"]["loss"]["tooth_class_loss_1"]
        super().__init__(config, module, trainable)

    def get_loss(self, sem_1, gt_seg_label_1):
        return super().get_loss(gt_seg_label_1, sem_1)

    def losses_of(self, output, seg_label, points):
        return self.get_loss(output[self.output_key], seg_label)


class FpsGroupingNetworkModel(TrainingModel):
    """models/fps_grouping_network_model.py ("tgnet_fps"): the five terms of losses.grouping_loss_terms with the configuration's
    weights and, opt-in, the contrastive-boundary terms.  tr_set["contrastive_boundary"] true and a non-zero cbl_loss_1 / cbl_loss_2
    weight: the train-phase forward runs the module with contrast=True and the train-phase LossMap gains cbl_loss_1 and cbl_loss_2,
    output[...].sum() with the configuration's weights (fps_grouping_network_model.py:58-59).  Without the key a non-zero weight is
    refused; with the key and both weights zero or absent the criterion is not computed at all.  tr_set["contrastive_boundary_fused"]
    true: both networks of the module compute the criterion's stages with the fused kernels (losses.contrast_boundary_stage_fused:
    no (m, K-1, 32) difference tensor, a bit-reproducible gradient); off by default."""
    module_class = nets.GroupingNetworkModule
    model_name = "tgnet_fps"
    TERMS = ("tooth_class_loss_1", "tooth_class_loss_2", "offset_1_loss", "offset_1_dir_loss", "chamf_1_loss")
    CBL = ("cbl_loss_1", "cbl_loss_2")

    @classmethod
    def cbl_asked(cls, config):
        return [n for n in cls.CBL if config["tr_set"]["loss"].get(n, 0) != 0]

    @classmethod
    def check_config(cls, config, trainable=True):
        super().check_config(config, trainable)
        asked = cls.cbl_asked(config)
        if asked and not config["tr_set"].get("contrastive_boundary"):
            raise NotImplementedError(f"{cls.model_name}: the configuration weights {' and '.join(asked)}, and the contrastive-boundary terms are "
                                      "opt-in: set tr_set.contrastive_boundary to True to train on them, or set tr_set.loss.cbl_loss_1 and "
                                      "cbl_loss_2 to 0 (or leave them out) to train on the five class, offset, direction and chamfer "
                                      "terms alone")

    def __init__(self, config, module=None, trainable=True):
        super().__init__(config, module, trainable)
        self.contrast = bool(config["tr_set"].get("contrastive_boundary")) and bool(self.cbl_asked(config))
        for net in (self.module.first_ins_cent_model, self.module.second_ins_cent_model):
            net.fused_contrast = bool(config["tr_set"].get("contrastive_boundary_fused"))

    def forward(self, inputs):
        # self.module.training is the phase (TrainingModel._set_model): the criterion is part of the train phase only
        if self.contrast and self.module.training:
            return self.module(inputs, contrast=True)
        return self.module(inputs)

    def get_loss(self, output, gt_seg_label, input_coords):
        terms = losses.grouping_loss_terms(output, gt_seg_label, input_coords)
        out = {name: (terms[name], self.config["tr_set"]["loss"][name]) for name in self.TERMS}
        for name in self.CBL:
            if name in output:
                out[name] = (output[name].sum(), self.config["tr_set"]["loss"].get(name, 0))
        return out

    def losses_of(self, output, seg_label, points):
        return self.get_loss(output, seg_label, points[:, :3, :])


class TSegNetModel(TrainingModel):
    """models/tsegnet_model.py ("tsegnet"): losses.tsegnet_loss_terms with the reference's weights.  Honours
    run_tooth_segmentation_module (False: the centroid module alone is trained on its three terms) and
    pretrained_centroid_model_path (loaded with strict=False, as the reference does).  `skipped_segmentation` counts the steps whose
    batch had no tooth centre, so that the three segmentation terms are missing from their LossMap."""
    module_class = nets.TSegNetModule
    WEIGHTS = {"dist_loss": 1, "cent_loss": 1, "chamf_loss": 0.1, "seg_1_loss": 1, "seg_2_loss": 1, "id_pred_loss": 1}

    def __init__(self, config, module=None, trainable=True):
        super().__init__(config, module, trainable)
        self.skipped_segmentation = 0
        if config.get("pretrained_centroid_model_path") is not None:
            self.module.load_state_dict(torch.load(config["pretrained_centroid_model_path"] + ".h5"), strict=False)

    def forward(self, inputs):
        output = self.module(inputs, on_no_centre="skip")
        if self.config["run_tooth_segmentation_module"] and "pd_1" not in output:
            self.skipped_segmentation += 1
        return output

    def get_loss(self, outputs, gt):
        """gt: {"seg_label": (B, 1, N)}; the reference's centroid_coords / centroid_labels entries are computed from it on the device."""
        terms = losses.tsegnet_loss_terms(outputs, gt["seg_label"])
        return {name: (value, self.WEIGHTS[name]) for name, value in terms.items()}

    def losses_of(self, output, seg_label, points):
        return self.get_loss(output, {"seg_label": seg_label})


def _path_map(root, extension):
    """{base name: path} of the `*<extension>` files in every sub-directory of root, at any depth (bdl_grouping_netowrk_model.py:20-32).
    Files lying directly in root are not looked at (`os.walk(...)[1:]`), nor are hidden files (glob's `*`); the key is
    basename.split(".")[0].  Directories and files are visited in sorted order, and a base name found twice is a ValueError naming both
    paths: the reference keeps whichever os.walk yields last, which depends on the file system."""
    found = {}
    for dir_path, dir_names, file_names in os.walk(root):
        dir_names.sort()
        if dir_path == root:
            continue
        for name in sorted(file_names):
            if not name.endswith(extension) or name.startswith("."):
                continue
            key, path = name.split(".")[0], os.path.join(dir_path, name)
            if key in found:
                raise ValueError(f"two {extension} files are named {key!r} under {root}: {found[key]} and {path}")
            found[key] = path
    return found


class BoundarySampler:
    """The boundary-sampled inputs of tgnet's second module (bdl_grouping_netowrk_model.py:20-35, 56-192): per scan, num_of_all_points
    rows of the ORIGINAL mesh, up to num_of_bdl_points of them from where the frozen first module's instances meet, the rest by FPS.

    config: the reference's tgnet_bdl configuration; its boundary_sampling_info names the directories of the original `.obj` and
    `.json` files (keys "orginal_data_obj_path" / "orginal_data_json_path", the reference's spelling), the cache directory and the
    three numbers.  base_model: any callable with GroupingNetworkModule's call and output dict.  Constructing needs no GPU; a cache
    miss does (the base model, tgnet.second_instances, tgnet.boundary_resample: all device functions of the inference pipeline).

    Deliberate deviations from the reference:
      * k-means seeding.  The reference seeds sklearn's k-means++ from numpy's global generator BEFORE it draws the boundary
        permutation; this package's k-means draws nothing (tgnet.py).  After the same np.random.seed the two therefore permute from
        different generator states: the flags are the same, the selected boundary rows are not unless the generator is seeded again
        behind the reference's k-means.
      * float32 output.  Both paths return float32 rows; the reference's cache-miss path returns whatever its augmentation produced.
        The cache-hit path augments the float64 copy of the cached columns and rounds once, as the reference does.
      * too few non-boundary rows: tgnet.boundary_resample's ValueError, with the base name in front (the reference raises a string).
      * no foreground point: tgnet.second_instances' ValueError, with the base name in front (sklearn's escapes the reference's step).
      * a base name found twice under a root is a ValueError, one missing from a root a KeyError naming it and the root.
      * the cache file is written under a temporary name and renamed, so a killed run leaves no truncated file for the next to trust.
      * a scan is never silently replaced by other inputs: apart from the reference's own rule for a mesh below num_of_all_points
        (the batch is returned as it came), every failure raises."""

    def __init__(self, config, base_model):
        self.config, self.base_model = config, base_model
        self.info = config["boundary_sampling_info"]
        self.obj_root, self.json_root = self.info["orginal_data_obj_path"], self.info["orginal_data_json_path"]
        self.stl_path_map = _path_map(self.obj_root, ".obj")
        self.json_path_map = _path_map(self.json_root, ".json")

    def load_mesh(self, base_name):
        """-> (vertices (n, 6) float32: centred, normalised xyz and the vertex normals; labels (n, 1) int: -1 gingiva, teeth 0..15)
        of the original mesh (:116-131)."""
        for found, root, what in ((self.json_path_map, self.json_root, ".json"), (self.stl_path_map, self.obj_root, ".obj")):
            if base_name not in found:
                raise KeyError(f"no {base_name}{what} in a sub-directory of {root}")
        with open(self.json_path_map[base_name], "r") as f:
            loaded = json.load(f)
        labels = preprocess.remap_fdi_labels(loaded["labels"], loaded["jaw"]) - 1
        vertices = preprocess.normalise_vertices(preprocess.read_txt_obj_ls(self.stl_path_map[base_name])[0]).astype(np.float32)
        if labels.shape[0] != vertices.shape[0]:
            raise ValueError(f"{base_name}: {labels.shape[0]} labels for {vertices.shape[0]} vertices")
        return vertices, labels.astype(int).reshape(-1, 1)

    @staticmethod
    def base_name_of(mesh_path):
        pieces = os.path.basename(mesh_path).split("_")
        if len(pieces) < 2:
            raise ValueError(f"mesh_path {mesh_path!r}: the file name must start with <patient>_<jaw>_")
        return pieces[0] + "_" + pieces[1]

    @staticmethod
    def write_cache(cache_path, array):
        """np.save under a temporary name in cache_path's directory, then os.replace: cache_path either holds a whole array or does
        not exist."""
        folder = os.path.dirname(cache_path)
        if folder:
            os.makedirs(folder, exist_ok=True)
        tmp_path = f"{cache_path}.{os.getpid()}.tmp"
        try:
            with open(tmp_path, "wb") as f:
                np.save(f, array)
            os.replace(tmp_path, cache_path)
        except BaseException:
            if os.path.exists(tmp_path):
                os.remove(tmp_path)
            raise

    @staticmethod
    def _as_batch(rows, labels):
        return (torch.from_numpy(np.ascontiguousarray(rows.T)[None]),
                torch.from_numpy(np.ascontiguousarray(labels.astype(np.int64).reshape(-1, 1).T)[None]))

    def sample(self, batch_item):
        """batch_item: one collated scan (feat (1, 6, N), gt_seg_label (1, 1, N), aug_obj [Augmentator or None], mesh_path [path]) ->
        (feat (1, 6, num_of_all_points) float32, gt_seg_label (1, 1, num_of_all_points) int64), CPU tensors (:133-192); boundary rows
        first.  The first call for a scan runs the base model and writes <bdl_cache_path>/<base name>.npy, the un-augmented selection
        and its labels as (num_of_all_points, 7) float64 (the reference's file); later calls augment that file's rows."""
        feat, gt_seg_label = batch_item["feat"], batch_item["gt_seg_label"]
        if len(batch_item["mesh_path"]) != 1 or feat.shape[0] != 1 or gt_seg_label.shape[0] != 1:
            raise ValueError(f"the boundary sampler takes one scan per batch, got {len(batch_item['mesh_path'])} paths and feat "
                             f"{tuple(feat.shape)}: set train_batch_size and val_batch_size to 1")
        base_name = self.base_name_of(batch_item["mesh_path"][0])
        aug_obj = batch_item["aug_obj"][0]
        n_all = int(self.info["num_of_all_points"])
        cache_path = os.path.join(self.info["bdl_cache_path"], base_name + ".npy")
        if os.path.exists(cache_path):
            cached = np.load(cache_path)
            if cached.ndim != 2 or cached.shape[1] != 7:
                raise ValueError(f"{cache_path}: a cache file is (num_of_all_points, 7), got {cached.shape}")
            rows = cached[:, :6].copy()
            if aug_obj:
                rows = aug_obj.run(rows)
            return self._as_batch(rows.astype(np.float32), cached[:, 6])
        mesh, mesh_labels = self.load_mesh(base_name)
        if mesh.shape[0] < n_all:
            return feat, gt_seg_label
        device = torch.device("cuda")
        points, seg_label = feat.to(device), gt_seg_label.to(device)
        with torch.no_grad():
            output = self.base_model([points, seg_label])
        augmented = aug_obj.run(mesh.copy()) if aug_obj else mesh.copy()
        try:
            point_labels = tgnet.second_instances(points, seg_label, output)["ins"] - 1          # -1 background, clusters 0, 1, ...
            picked = tgnet.boundary_resample(augmented, points[0, :3].t().contiguous(), point_labels, info=self.info,
                                             carry=(mesh_labels, mesh))
        except ValueError as error:
            raise ValueError(f"{base_name}: {error}") from error
        rows, (labels, plain_rows) = picked[0], picked[4]
        self.write_cache(cache_path, np.concatenate([plain_rows, labels], axis=1).astype(np.float64))
        return self._as_batch(rows.astype(np.float32), labels)


class BdlGroupingNetworkModel(FpsGroupingNetworkModel):
    """models/bdl_grouping_netowrk_model.py ("tgnet_bdl"): the two-stage GroupingNetworkModule of config["model_parameter"], trained on
    BoundarySampler's inputs.  evaluate() replaces the batch's feat / gt_seg_label with self.sampler.sample(batch_item) in every phase, then
    runs tgnet_fps's evaluate: the five terms, and cbl_loss_1 / cbl_loss_2 in the train phase under the same tr_set.contrastive_boundary rule.

    The base model -- base_model, or nets.GroupingNetworkModule(config["fps_model_info"]) loaded from
    fps_model_info.load_ckpt_path + ".h5" with strict=True -- is frozen: eval mode, requires_grad False, in neither the optimiser nor
    save().  The reference never calls .eval() on it, so its BatchNorm normalises with batch statistics and its running statistics
    drift during the second training; here a frozen first module is a function of its checkpoint."""
    model_name = "tgnet_bdl"
    SECTIONS = ("boundary_sampling_info", "fps_model_info")

    @classmethod
    def check_config(cls, config, trainable=True):
        missing = [section for section in cls.SECTIONS if section not in config]
        if missing:
            raise NotImplementedError(f"tgnet_bdl trains on boundary-sampled inputs and the configuration has no {' and no '.join(missing)} "
                                      "section: boundary_sampling_info names the original meshes, their labels and the cache directory, "
                                      "fps_model_info the trained tgnet_fps module that finds the boundaries (train_configs/tgnet_bdl.py)")
        super().check_config(config, trainable)

    def __init__(self, config, module=None, base_model=None, trainable=True):
        super().__init__(config, module, trainable)
        if base_model is None:
            base_model = nets.GroupingNetworkModule(config["fps_model_info"])
            base_model.load_state_dict(torch.load(config["fps_model_info"]["load_ckpt_path"] + ".h5"), strict=True)
            base_model.cuda()
        if isinstance(base_model, torch.nn.Module):
            base_model.eval()
            base_model.requires_grad_(False)
        self.base_model = base_model
        self.sampler = BoundarySampler(config, base_model)

    def evaluate(self, batch_item, phase):
        feat, gt_seg_label = self.sampler.sample(batch_item)
        return super().evaluate(dict(batch_item, feat=feat, gt_seg_label=gt_seg_label), phase)


_MODELS = {"tgnet_fps": FpsGroupingNetworkModel, "tsegnet": TSegNetModel, "dgcnn": DGCnnModel, "pointnet": PointFirstModel,
           "pointnetpp": PointPpFirstModel, "pointtransformer": TransformerModel, "tgnet_bdl": BdlGroupingNetworkModel}


def make_training_model(model_name, config, trainable=True):
    """start_train.py:22-49: the step object of a model name.  Another name is ValueError; tgnet_bdl without its boundary_sampling_info
    and fps_model_info sections is refused (NotImplementedError) before anything else in the configuration is looked at.
    trainable=False: TrainingModel's evaluate-only form."""
    if model_name not in _MODELS:
        raise ValueError(f"undefined model {model_name!r}: the names are {', '.join(MODEL_NAMES)}")
    if config.get("tr_set", {}).get("reproducible") and model_name in NOT_REPRODUCIBLE:
        raise NotImplementedError(f"{model_name}: tr_set.reproducible is set and this model's step is not bit-reproducible: "
                                  f"{NOT_REPRODUCIBLE[model_name]}.  Nothing here trains under that flag without keeping its promise")
    return _MODELS[model_name](config, trainable=trainable)


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------

class Trainer:
    """trainer.py: train(epoch, loader), test(epoch, loader, save_best_model), run(epochs) over gen_set = [[train loader, val loader]].

    The bookkeeping is the reference's (trainer.py:26-63): the scheduler steps when (batch_idx + 1) % schedueler_step == 0, or on the
    last batch of an epoch in which it has not stepped yet, each time with the running step count; save("train") after every training
    epoch; save("val") whenever total_val improves.  Instead of wandb, `stream` (default stdout) gets one JSON line per scheduler
    step -- the step meter's averages (`*_step`), `step_lr`, `step` -- and run() one per epoch: the epoch's `*_train` and `*_val`
    averages, `epoch`, `step`, for a model that counts them `skipped_segmentation`, and with tr_set["reproducible"] `digest`
    (state_digest of the model after the epoch)."""

    def __init__(self, config=None, model=None, gen_set=None, stream=None):
        self.config, self.model, self.gen_set = config, model, gen_set
        self.stream = stream
        self.val_count = self.train_count = self.step_count = 0
        self.best_val_loss = math.inf

    def _emit(self, record):
        stream = self.stream if self.stream is not None else sys.stdout
        stream.write(json.dumps(record) + "\n")
        stream.flush()

    def train(self, epoch, data_loader):
        total_loss_meter, step_loss_meter = LossMeter(), LossMeter()
        pre_step = self.step_count
        every = self.config["tr_set"]["scheduler"]["schedueler_step"]
        last = len(data_loader) - 1
        for batch_idx, batch_item in enumerate(data_loader):
            loss = self.model.step(batch_idx, batch_item, "train")
            total_loss_meter.aggr(loss.get_loss_dict_for_print("train"))
            step_loss_meter.aggr(loss.get_loss_dict_for_print("step"))
            if (batch_idx + 1) % every == 0 or (self.step_count == pre_step and batch_idx == last):
                record = {"step": self.step_count, **step_loss_meter.get_avg_results(), "step_lr": self.model.scheduler.get_last_lr()[0]}
                self.step_count += 1
                self.model.scheduler.step(self.step_count)
                step_loss_meter.init()
                self._emit(record)
        self.train_count += 1
        self.model.save("train")
        return total_loss_meter.get_avg_results() if total_loss_meter.step_num else {}

    def test(self, epoch, data_loader, save_best_model):
        total_loss_meter = LossMeter()
        for batch_idx, batch_item in enumerate(data_loader):
            loss = self.model.step(batch_idx, batch_item, "test")
            total_loss_meter.aggr(loss.get_loss_dict_for_print("val"))
        if not total_loss_meter.step_num:
            return {}
        avg_total_loss = total_loss_meter.get_avg_results()
        self.val_count += 1
        if save_best_model and self.best_val_loss > avg_total_loss["total_val"]:
            self.best_val_loss = avg_total_loss["total_val"]
            self.model.save("val")
        return avg_total_loss

    def run(self, epochs):
        train_data_loader, val_data_loader = self.gen_set[0][0], self.gen_set[0][1]
        for epoch in range(int(epochs)):
            record = {"epoch": epoch}
            record.update(self.train(epoch, train_data_loader))
            record.update(self.test(epoch, val_data_loader, True))
            record["step"] = self.step_count
            if hasattr(self.model, "skipped_segmentation"):
                record["skipped_segmentation"] = self.model.skipped_segmentation
            if self.config.get("tr_set", {}).get("reproducible"):
                record["digest"] = state_digest(self.model)
            self._emit(record)
