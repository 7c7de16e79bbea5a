#!/usr/bin/env python3
"""start_train.py over this package: train one of the reference's models from a directory of preprocessed scans
(`*_sampled_points.npy`, preprocess_data.py's output) on one GPU.

    python tools/train.py --model_name pointnetpp --config_path train_configs/pointnetpp.py --experiment_name run1 \\
        --input_data_dir_path data_preprocessed --train_data_split_txt_path train.txt --val_data_split_txt_path val.txt --epochs 60

The arguments are start_train.py's, plus --epochs (the reference loops 100 000 times) and --seed (numpy's and torch's generators:
shuffling, augmentation draws, initial weights, tsegnet's 8-of-T crop choice).  The configuration is the reference's:
train_configs/train_config_maker.get_default_config merged with the `config` dict of the Python file at --config_path, so the
reference's own train_configs/*.py files work as they are.  tr_set.contrastive_boundary defaults to True here, so tgnet_fps trains
on the cbl_loss_1 / cbl_loss_2 weights its file names (losses.contrast_boundary_loss); --no_contrastive_boundary leaves the key
out, and a non-zero cbl weight is then refused (training.py).  --fused_contrastive_boundary sets tr_set.contrastive_boundary_fused:
the criterion's stages run as the fused kernels of csrc/cbl.hip (no (m, K-1, 32) difference tensor, a bit-reproducible gradient;
off by default).  --ordered_backward sets tr_set.ordered_backward, which switches config.cfg.ordered_backward on: every gradient that
flows through a neighbour list is summed along reverse lists instead of with float atomics (ordered.py; off by default; the
BatchNorm kernels' float64 atomics remain: that is config.cfg.ordered_bn).  --reproducible sets tr_set.reproducible: with --seed, the
same data and the same machine, two runs end in the same bits.  It switches on both ordered forms, torch.use_deterministic_algorithms
(an operator torch knows to be non-deterministic raises and names itself) and the deterministic solver choice, adds "digest" (a
sha256 over the module's state) to the epoch line so that two runs can be compared without their checkpoints, and refuses a model
whose step is known not to repeat (training.NOT_REPRODUCIBLE; DESIGN.md section 4.2 has the audit).  tgnet_bdl (train_configs/tgnet_bdl.py with its four paths edited)
trains tgnet's boundary module from a tgnet_fps checkpoint: see training.BoundarySampler for the three directories it needs.
Prints the trainer's JSON lines: one per scheduler step, one per epoch.  Checkpoints: ckpts/<experiment_name>.h5 after every epoch,
ckpts/<experiment_name>_val.h5 at every best validation total; both load into inference.make_inference_pipeline."""
import argparse
import importlib.util
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEFAULT_AUG = "aug.Augmentator([aug.Scaling([0.85, 1.15]), aug.Rotation([-30,30], 'fixed'), aug.Translation([-0.2, 0.2])])"


def get_default_config(experiment_name, input_data_dir_path, train_data_split_txt_path, val_data_split_txt_path):
    """train_config_maker.get_default_config without its wandb block, which nothing here reads."""
    return {"generator": {"input_data_dir_path": f"{input_data_dir_path}", "train_data_split_txt_path": f"{train_data_split_txt_path}",
                          "val_data_split_txt_path": f"{val_data_split_txt_path}", "aug_obj_str": DEFAULT_AUG,
                          "train_batch_size": 1, "val_batch_size": 1},
            "checkpoint_path": f"ckpts/{experiment_name}"}


def get_train_config(config_path, experiment_name, input_data_dir_path, train_data_split_txt_path, val_data_split_txt_path):
    """train_config_maker.get_train_config: the defaults, then the top-level keys of the file's `config` over them."""
    config = get_default_config(experiment_name, input_data_dir_path, train_data_split_txt_path, val_data_split_txt_path)
    spec = importlib.util.spec_from_file_location("tgn_train_config", config_path)
    loaded = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(loaded)
    config.update(loaded.config)
    return config


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model_name", default="tsegnet", help="tsegnet | tgnet_fps | tgnet_bdl | pointnet | pointnetpp | dgcnn | pointtransformer")
    ap.add_argument("--config_path", default="train_configs/tsegnet.py", help="train config file: a Python file with a `config` dict")
    ap.add_argument("--experiment_name", default="tsegnet_0620", help="names the checkpoints: ckpts/<experiment_name>.h5")
    ap.add_argument("--input_data_dir_path", default="data_preprocessed_path", help="directory of *_sampled_points.npy")
    ap.add_argument("--train_data_split_txt_path", default="base_name_train_fold.txt", help="patient ids of the training split, one per line")
    ap.add_argument("--val_data_split_txt_path", default="base_name_val_fold.txt", help="patient ids of the validation split")
    ap.add_argument("--epochs", type=int, default=100000, help="epochs to run (the reference's loop count is the default)")
    ap.add_argument("--seed", type=int, default=None, help="seeds numpy's and torch's generators")
    ap.add_argument("--no_contrastive_boundary", action="store_true",
                    help="do not set tr_set.contrastive_boundary: tgnet_fps then refuses non-zero cbl_loss_1 / cbl_loss_2 weights")
    ap.add_argument("--fused_contrastive_boundary", action="store_true",
                    help="set tr_set.contrastive_boundary_fused: tgnet_fps / tgnet_bdl compute the criterion with the fused stage kernels")
    ap.add_argument("--ordered_backward", action="store_true",
                    help="set tr_set.ordered_backward: the gather family's backward without float atomics (config.cfg.ordered_backward)")
    ap.add_argument("--reproducible", action="store_true",
                    help="set tr_set.reproducible: ordered backward, ordered BatchNorm sums, torch's deterministic algorithms, a digest per epoch")
    args = ap.parse_args(argv)

    import numpy as np
    import torch
    from toothgroupnetwork_amd import training
    if args.seed is not None:
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
    config = get_train_config(args.config_path, args.experiment_name, args.input_data_dir_path, args.train_data_split_txt_path,
                              args.val_data_split_txt_path)
    if not args.no_contrastive_boundary and "tr_set" in config:
        config["tr_set"].setdefault("contrastive_boundary", True)
    if args.fused_contrastive_boundary and "tr_set" in config:
        config["tr_set"]["contrastive_boundary_fused"] = True
    if args.ordered_backward:
        config.setdefault("tr_set", {})["ordered_backward"] = True
    if args.reproducible:
        config.setdefault("tr_set", {})["reproducible"] = True
    model = training.make_training_model(args.model_name, config)
    gen_set = [training.get_generator_set(config["generator"])]
    print("train_set", len(gen_set[0][0]), file=sys.stderr)
    print("validation_set", len(gen_set[0][1]), file=sys.stderr)
    training.Trainer(config=config, model=model, gen_set=gen_set).run(args.epochs)


if __name__ == "__main__":
    main()
