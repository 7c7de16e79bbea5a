#!/usr/bin/env python3
"""What the training entry point's bookkeeping costs: one training step of `training`'s tgnet_fps and pointnetpp models on ONE
24 000-point scan, batch 1, fp32, against a bare loop in the same process.  `tgnet_fps_cbl` is tgnet_fps with the contrastive-boundary
criterion on (tr_set.contrastive_boundary, both cbl weights 1): what the criterion adds to a step is its difference to `tgnet_fps`;
`tgnet_fps_cbl_fused` is the same with tr_set.contrastive_boundary_fused (the criterion's stages as the kernels of csrc/cbl.hip);
`tgnet_fps_reproducible` is tgnet_fps with tr_set.reproducible, to be run in a process of its own.

  trainer   model.step(batch_idx, batch_item, "train") and the three get_loss_dict_for_print calls Trainer.train makes per batch: the
            host-to-device copy of the item, forward, losses, backward, optimiser, LossMap, ONE device read.
  bare      the same module, the same loss functions, the same optimiser on tensors already on the device; no LossMap, no trainer; the
            weighted sum is read once per step (.item()), which is the least a loop that logs its loss does.
  bare_with_copy   the bare loop with the item copied from pageable host memory every step, as a loop fed by a DataLoader does: what is
            left between it and `trainer` is the bookkeeping alone.
The three alternate step by step, so all see the same clocks and allocator; wall clock around a synchronised step, medians of
--steps after --warmup, with the quartiles as the run-to-run spread.  Prints one JSON line."""
import argparse
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

MODEL_PARAMETER = {"input_feat": 6, "stride": [1, 4, 4, 4, 4], "nsample": [36, 24, 24, 24, 24], "blocks": [2, 3, 4, 6, 3], "block_num": 5,
                   "planes": [32, 64, 128, 256, 512], "crop_sample_size": 3072}
CONFIGS = {
    "pointnetpp": {"tr_set": {"optimizer": {"lr": 1e-3, "NAME": "adam", "weight_decay": 1.0e-4}}},
    "tgnet_fps": {"tr_set": {"optimizer": {"lr": 1e-3, "NAME": "sgd", "momentum": 0.9, "weight_decay": 1.0e-4},
                             "loss": {"cbl_loss_1": 0, "cbl_loss_2": 0, "tooth_class_loss_1": 1, "tooth_class_loss_2": 1, "offset_1_loss": 0.03,
                                      "offset_1_dir_loss": 0.03, "chamf_1_loss": 0.15}},
                  "model_parameter": MODEL_PARAMETER},
}
# tgnet_fps with the contrastive-boundary criterion on: train_configs/tgnet_fps.py's weights for the two cbl terms
CONFIGS["tgnet_fps_cbl"] = copy.deepcopy(CONFIGS["tgnet_fps"])
CONFIGS["tgnet_fps_cbl"]["tr_set"]["loss"].update(cbl_loss_1=1, cbl_loss_2=1)
CONFIGS["tgnet_fps_cbl"]["tr_set"]["contrastive_boundary"] = True
CONFIGS["tgnet_fps_cbl_fused"] = copy.deepcopy(CONFIGS["tgnet_fps_cbl"])
CONFIGS["tgnet_fps_cbl_fused"]["tr_set"]["contrastive_boundary_fused"] = True
# tgnet_fps with tr_set.reproducible (ordered backward, ordered BatchNorm sums, torch's deterministic algorithms).  The flags are the
# process's and are never switched off again: measure it in a process of its own, `--models tgnet_fps_reproducible`
CONFIGS["tgnet_fps_reproducible"] = copy.deepcopy(CONFIGS["tgnet_fps"])
CONFIGS["tgnet_fps_reproducible"]["tr_set"]["reproducible"] = True
MODEL_NAME = {"tgnet_fps_cbl": "tgnet_fps", "tgnet_fps_cbl_fused": "tgnet_fps", "tgnet_fps_reproducible": "tgnet_fps"}


def quartiles(ms):
    q1, q2, q3 = np.percentile(ms, [25, 50, 75])
    return {"median_ms": round(float(q2), 3), "q1_ms": round(float(q1), 3), "q3_ms": round(float(q3), 3)}


def run(name, points, steps, warmup, dev):
    from toothgroupnetwork_amd import synth, training
    cfg = copy.deepcopy(CONFIGS[name])
    cfg["tr_set"]["scheduler"] = {"sched": "cosine", "full_steps": 40, "schedueler_step": 15000000, "min_lr": 1e-5}
    cfg["checkpoint_path"] = "ckpts/bench"
    rows, lab = synth.labelled_arch(points, 14, seed=3)
    item = {"feat": torch.from_numpy(np.ascontiguousarray(rows.T))[None], "gt_seg_label": torch.from_numpy(lab).view(1, 1, -1)}
    torch.manual_seed(0)
    np.random.seed(0)
    model = training.make_training_model(MODEL_NAME.get(name, name), cfg)
    bare = training.make_training_model(MODEL_NAME.get(name, name), cfg)            # its module, optimiser and loss functions, driven by hand below
    bare.module.load_state_dict(model.module.state_dict())
    feat, seg = item["feat"].to(dev), item["gt_seg_label"].to(dev)

    def trainer_step(i):
        loss = model.step(i, item, "train")
        for post_fix in ("train", "step", "step"):
            printed = loss.get_loss_dict_for_print(post_fix)
        return printed["total_step"]

    def bare_step(i, copy_item=False):
        f, g = (item["feat"].to(dev), item["gt_seg_label"].to(dev)) if copy_item else (feat, seg)
        output = bare.forward([f, g])
        total = 0
        for value, weight in bare.losses_of(output, g, f).values():
            total = total + value * weight
        bare.optimizer.zero_grad()
        total.backward()
        bare.optimizer.step()
        return total.item()

    ms = {"trainer": [], "bare": [], "bare_with_copy": []}
    first = last = None
    for i in range(warmup + steps):
        for tag, fn in (("trainer", trainer_step), ("bare", bare_step), ("bare_with_copy", lambda i: bare_step(i, True))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            value = fn(i)
            torch.cuda.synchronize()
            if i >= warmup:
                ms[tag].append((time.perf_counter() - t0) * 1e3)
            if tag == "trainer":
                first, last = (value if first is None else first), value
    out = {tag: quartiles(v) for tag, v in ms.items()}

    def each_ms(fn, reps=200):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3 / reps, 4)

    # the pieces a trainer step has and the bare loop has not, each alone on an idle device
    loss = model.step(0, item, "train")

    def three_prints():
        loss._host = None
        for post_fix in ("train", "step", "step"):
            loss.get_loss_dict_for_print(post_fix)
    one = next(iter(loss.loss_dict.values()))[0]
    out["pieces_ms"] = {"module_train_walk": each_ms(lambda: model.module.train()), "copy_item": each_ms(lambda: (item["feat"].to(dev), item["gt_seg_label"].to(dev))),
                        "three_prints_one_read": each_ms(three_prints), "one_item_read": each_ms(one.item)}
    out.update(first_total=first, last_total=last, difference_ms=round(out["trainer"]["median_ms"] - out["bare"]["median_ms"], 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=24000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--models", nargs="+", default=["pointnetpp", "tgnet_fps"], choices=sorted(CONFIGS))
    args = ap.parse_args()
    dev = torch.device("cuda")
    res = {name: run(name, args.points, args.steps, args.warmup, dev) for name in args.models}
    print(json.dumps({"workload": f"training step, 1 x {args.points} points, fp32, trainer against a bare loop", **res}))


if __name__ == "__main__":
    main()
