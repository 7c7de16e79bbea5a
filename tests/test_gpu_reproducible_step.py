"""GPU: tr_set["reproducible"] (training.set_reproducible, tools/train.py --reproducible) keeps its promise -- same seed, same data
order, same bits -- for every model it does not refuse.

  one process, two models   per case of tools/reproducible_audit.py whose model is not in training.NOT_REPRODUCIBLE: two fresh models from
                            one seed, three model.step(..., "train") over the same two synthetic scans at the smallest point counts the
                            modules take (tests/test_gpu_training.py).  Byte-equal: the loss terms of every step, every gradient after
                            step 1, state_dict (BatchNorm buffers included) and optimiser state after step 3.  The runs are the audit's
                            own run_once, so the test and the table it guards cannot drift apart.
  refusals                  every name in NOT_REPRODUCIBLE is refused by make_training_model with the key set, naming the operator.
  two processes             the command line twice, pointtransformer on 3 scans of 6144 points with --reproducible --seed 3: equal
                            "digest" in the epoch lines, byte-equal checkpoint tensors, and the digest is the checkpoint's.
  without the flag          the epoch line has no "digest".

pointtransformer and tgnet_fps (with and without the contrastive-boundary terms, fused and not) must be among the cases that run: the
flag is of little use without them, so their refusal fails this file instead of shrinking it.

The flags are the process's; a fixture puts back what it found, so the tests collected after this file run as they always did."""
import hashlib
import io
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import REPO
from test_gpu_training import make_config, synthetic_loader

sys.path.insert(0, os.path.join(REPO, "tools"))
import reproducible_audit as A  # noqa: E402

pytestmark = pytest.mark.gpu


def _reproducible_cases():
    from toothgroupnetwork_amd import training
    return [case for case, spec in A.CASES.items() if spec[0] not in training.NOT_REPRODUCIBLE]


@pytest.fixture
def process_flags():
    from toothgroupnetwork_amd import config
    saved = (config.cfg.ordered_backward, config.cfg.ordered_bn, torch.are_deterministic_algorithms_enabled(),
             torch.is_deterministic_algorithms_warn_only_enabled(), torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    yield
    config.cfg.ordered_backward, config.cfg.ordered_bn = saved[0], saved[1]
    torch.use_deterministic_algorithms(saved[2], warn_only=saved[3])
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = saved[4], saved[5]


def test_the_two_networks_the_flag_is_for_are_not_refused():
    assert {"pointtransformer", "tgnet_fps", "tgnet_fps_cbl", "tgnet_fps_cbl_fused"} <= set(_reproducible_cases())


@pytest.mark.parametrize("case", _reproducible_cases())
def test_two_models_from_one_seed_stay_byte_equal_over_three_steps(dev, tmp_path, process_flags, case):
    from toothgroupnetwork_amd import config
    name, points = A.CASES[case][:2]
    cfg = A.make_config(case, str(tmp_path / "ckpts" / case))
    batches = A.batches_of(str(tmp_path / "data"), points)
    a, b = A.run_once(case, cfg, batches, 11), A.run_once(case, cfg, batches, 11)
    assert config.cfg.ordered_backward and config.cfg.ordered_bn and torch.are_deterministic_algorithms_enabled()
    assert len(a["loss"]) == 3 and a["grad"] and a["state"] and a["optim"]
    assert any(k.endswith("running_mean") for k in a["state"]) and any(k.endswith("num_batches_tracked") for k in a["state"])
    for step, (x, y) in enumerate(zip(a["loss"], b["loss"])):
        assert not A.differing(x, y), f"{case}: loss terms of step {step}"
    grads = A.differing(a["grad"], b["grad"])
    assert not grads, f"{case}: {len(grads)} of {len(a['grad'])} gradients differ after step 1, the last (nearest the cause) {grads[-1]}"
    assert not A.differing(a["state"], b["state"]) and not A.differing(a["optim"], b["optim"]), case


def test_every_name_in_the_table_is_refused_naming_the_operator(tmp_path):
    from toothgroupnetwork_amd import training
    for name, reason in training.NOT_REPRODUCIBLE.items():
        case = next(c for c, spec in A.CASES.items() if spec[0] == name)
        with pytest.raises(NotImplementedError) as e:
            training.make_training_model(name, A.make_config(case, str(tmp_path / name)))
        assert name in str(e.value) and reason in str(e.value)


def _digest_of_checkpoint(path):
    state = torch.load(path, map_location="cpu")
    h = hashlib.sha256()
    for k in sorted(state):
        if state[k].numel():
            h.update(state[k].contiguous().view(-1).view(torch.uint8).numpy().tobytes())
    return state, h.hexdigest()


def test_the_command_line_twice_gives_one_digest_and_one_checkpoint(dev, tmp_path):
    from toothgroupnetwork_amd import eval_sharded
    data = tmp_path / "data"
    eval_sharded.write_synthetic_preprocessed(str(data), 3, n_points=6144)
    (tmp_path / "train.txt").write_text("SYN00000\nSYN00001\n")
    (tmp_path / "val.txt").write_text("SYN00002\n")
    cfg = make_config("pointtransformer", "")
    (tmp_path / "pt.py").write_text("config = " + repr({"tr_set": cfg["tr_set"], "model_parameter": cfg["model_parameter"]}) + "\n")
    runs = []
    for tag in ("a", "b"):
        cmd = [sys.executable, os.path.join(REPO, "tools", "train.py"), "--model_name", "pointtransformer", "--config_path", str(tmp_path / "pt.py"),
               "--experiment_name", tag, "--input_data_dir_path", str(data), "--train_data_split_txt_path", str(tmp_path / "train.txt"),
               "--val_data_split_txt_path", str(tmp_path / "val.txt"), "--epochs", "1", "--seed", "3", "--reproducible"]
        done = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
        assert done.returncode == 0, done.stderr[-2000:]
        lines = [json.loads(x) for x in done.stdout.splitlines()]
        assert len(lines) == 2 and lines[1]["epoch"] == 0 and len(lines[1]["digest"]) == 64, done.stdout
        runs.append((lines, *_digest_of_checkpoint(str(tmp_path / "ckpts" / (tag + ".h5")))))
    (lines_a, state_a, digest_a), (lines_b, state_b, digest_b) = runs
    assert lines_a == lines_b, "every printed number, the digest included"
    assert lines_a[1]["digest"] == digest_a == digest_b, "the digest is that of the checkpoint written after the epoch"
    assert list(state_a) == list(state_b) and all(torch.equal(state_a[k], state_b[k]) for k in state_a)
    assert any(k.endswith("running_var") for k in state_a)


def test_without_the_flag_the_epoch_line_has_no_digest(dev, tmp_path):
    from toothgroupnetwork_amd import training
    cfg = make_config("pointnet", str(tmp_path / "ckpts" / "plain"), every=1)
    model = training.make_training_model("pointnet", cfg)
    loader = synthetic_loader(tmp_path / "data", 2, 257)
    stream = io.StringIO()
    training.Trainer(config=cfg, model=model, gen_set=[[loader, loader]], stream=stream).run(1)
    epoch_line = json.loads(stream.getvalue().splitlines()[-1])
    assert epoch_line["epoch"] == 0 and "digest" not in epoch_line
    assert len(training.state_digest(model)) == 64 and not torch.are_deterministic_algorithms_enabled()
