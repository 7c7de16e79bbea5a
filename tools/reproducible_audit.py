#!/usr/bin/env python3
"""The audit behind training.NOT_REPRODUCIBLE: does a training step of each model give the same bits twice under
tr_set["reproducible"], and if not, which operator stands in the way?  (DESIGN.md section 4.2 records the outcome.)

Per case -- pointnet 257 points, pointnetpp 1024, dgcnn 20, pointtransformer 6144, tsegnet 3072 and tgnet_fps 3072 without the
contrastive-boundary terms, with them, and with them fused: the smallest scans each module takes --

  1. one train step with training.set_reproducible(warn_only=True): the operators torch itself flags as non-deterministic, from its
     warnings;
  2. two fresh models from one seed, in this process, over the same three steps on two synthetic scans, with the flags set for
     good (an operator torch knows to be non-deterministic now raises; the message is the finding);
  3. compared byte for byte: the loss terms of every step, every gradient after step 1, state_dict and optimiser state after step 3;
  4. where they differ, the parameters whose gradients differ after step 1, in the module's registration (= forward) order.  A
     backward that does not repeat spoils its own gradient and every one UPSTREAM of it, so the LAST such parameter sits next to
     the culprit; a forward that does not repeat shows in the loss terms first.

Prints one JSON line per case.  --no_refusals audits the names in training.NOT_REPRODUCIBLE too (make_training_model refuses them
otherwise, which the line then says)."""
import argparse
import copy
import json
import os
import sys
import tempfile
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

MODEL_PARAMETER = {"input_feat": 6, "stride": [1, 4, 4, 4, 4], "nsample": [36, 24, 24, 24, 24], "blocks": [2, 3, 4, 6, 3], "block_num": 5,
                   "planes": [32, 64, 128, 256, 512], "crop_sample_size": 3072}
FPS_LOSS = {"cbl_loss_1": 0, "cbl_loss_2": 0, "tooth_class_loss_1": 1, "tooth_class_loss_2": 1, "offset_1_loss": 0.03, "offset_1_dir_loss": 0.03,
            "chamf_1_loss": 0.15}
# case -> (model name, points, tr_set extras, loss extras)
CASES = {"pointnet": ("pointnet", 257, {}, {}), "pointnetpp": ("pointnetpp", 1024, {}, {}), "dgcnn": ("dgcnn", 20, {}, {}),
         "pointtransformer": ("pointtransformer", 6144, {}, {}), "tsegnet": ("tsegnet", 3072, {}, {}),
         "tgnet_fps": ("tgnet_fps", 3072, {}, {}),
         "tgnet_fps_cbl": ("tgnet_fps", 3072, {"contrastive_boundary": True}, {"cbl_loss_1": 1, "cbl_loss_2": 1}),
         "tgnet_fps_cbl_fused": ("tgnet_fps", 3072, {"contrastive_boundary": True, "contrastive_boundary_fused": True}, {"cbl_loss_1": 1, "cbl_loss_2": 1})}


def make_config(case, ckpt):
    name, _, tr_extra, loss_extra = CASES[case]
    optimizer = {"lr": 1e-2, "NAME": "sgd", "momentum": 0.9, "weight_decay": 1.0e-4} if name == "tgnet_fps" else {"lr": 1e-3, "NAME": "adam", "weight_decay": 1.0e-4}
    cfg = {"tr_set": {"optimizer": optimizer, "scheduler": {"sched": "cosine", "warmup_epochs": 0, "full_steps": 40, "schedueler_step": 15000000, "min_lr": 1e-5},
                      "reproducible": True, **tr_extra},
           "checkpoint_path": ckpt}
    if name in ("pointtransformer", "tgnet_fps"):
        cfg["model_parameter"] = copy.deepcopy(MODEL_PARAMETER)
        cfg["tr_set"]["loss"] = {**FPS_LOSS, **loss_extra} if name == "tgnet_fps" else {"tooth_class_loss_1": 1}
    if name == "tsegnet":
        cfg["run_tooth_segmentation_module"] = False
    return cfg


def batches_of(root, n_points):
    from toothgroupnetwork_amd import eval_sharded, training
    eval_sharded.write_synthetic_preprocessed(root, 2, n_points=n_points)
    return list(torch.utils.data.DataLoader(training.DentalModelGenerator(root), shuffle=False, batch_size=1, collate_fn=training.collate_fn))


def _bytes(t):
    return t.detach().contiguous().cpu().view(-1).view(torch.uint8).numpy().tobytes()


def run_once(case, cfg, batches, seed):
    """three train steps of a fresh model -> {"loss": [per step {term: bytes}], "grad": {name: bytes} after step 1, "state": {...},
    "optim": {...}}"""
    from toothgroupnetwork_amd import ordered, pointops, training
    torch.manual_seed(seed)
    np.random.seed(seed)
    pointops.knn_cache_clear()
    ordered.lists_cache_clear()
    model = training.make_training_model(CASES[case][0], cfg)
    out = {"loss": [], "grad": {}}
    for i, b in enumerate((batches[0], batches[1], batches[0])):
        lmap = model.step(i, b, "train")
        out["loss"].append({k: _bytes(v) for k, (v, _) in lmap.loss_dict.items()})
        if i == 0:
            out["grad"] = {n: _bytes(p.grad) for n, p in model.module.named_parameters() if p.grad is not None}
    out["state"] = {k: _bytes(v) for k, v in model.module.state_dict().items()}
    out["optim"] = {f"{i}.{k}": _bytes(v) for i, st in enumerate(model.optimizer.state_dict()["state"].values()) for k, v in st.items()
                    if torch.is_tensor(v)}
    torch.cuda.synchronize()
    return out


def differing(a, b):
    assert list(a) == list(b)
    return [k for k in a if a[k] != b[k]]


def audit(case, root, seed=11):
    from toothgroupnetwork_amd import training
    name, points = CASES[case][:2]
    cfg = make_config(case, os.path.join(root, "ckpts", case))
    batches = batches_of(os.path.join(root, f"data{points}"), points)
    record = {"case": case, "model": name, "points": points}
    # 1. what torch flags
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        training.set_reproducible(warn_only=True)
        probe = copy.deepcopy(cfg)
        del probe["tr_set"]["reproducible"]           # (the flags stay warn-only for this one step)
        torch.manual_seed(seed)
        np.random.seed(seed)
        training.make_training_model(name, probe).step(0, batches[0], "train")
        torch.cuda.synchronize()
    record["torch_flags"] = sorted({str(w.message).split(".")[0] for w in caught if "deterministic" in str(w.message)})
    # 2. - 4.
    try:
        a, b = run_once(case, cfg, batches, seed), run_once(case, cfg, batches, seed)
    except (RuntimeError, NotImplementedError) as e:
        record["raised"] = f"{type(e).__name__}: {str(e)[:400]}"
        return record
    loss = [[k for k in differing(x, y)] for x, y in zip(a["loss"], b["loss"])]
    grads = differing(a["grad"], b["grad"])
    record.update(loss_terms_differ=loss, gradients=len(a["grad"]), gradients_differ=len(grads), first_gradient_that_differs=grads[0] if grads else None,
                  last_gradient_that_differs=grads[-1] if grads else None, state_differs=len(differing(a["state"], b["state"])),
                  optimizer_state_differs=len(differing(a["optim"], b["optim"])))
    record["reproducible"] = not (any(loss) or grads or record["state_differs"] or record["optimizer_state_differs"])
    return record


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--no_refusals", action="store_true", help="audit the names of training.NOT_REPRODUCIBLE as well")
    args = ap.parse_args()
    from toothgroupnetwork_amd import training
    if args.no_refusals:
        training.NOT_REPRODUCIBLE.clear()
    with tempfile.TemporaryDirectory() as root:
        for case in args.cases:
            print(json.dumps(audit(case, root)), flush=True)


if __name__ == "__main__":
    main()
