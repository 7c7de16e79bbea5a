"""Host: what the fused contrastive-boundary stage (csrc/cbl.hip, losses.contrast_boundary_lists) rests on, without a GPU.

  * the closed form the kernels compute (tests/cbl_fused_ref.py: the per-pair weights and the gradient along the reverse lists, float64
    numpy) equals the float64 restatement tests/cbl_ref.py, whose gradient is autograd's, on the hand-made cases over the CPU oracle's
    neighbour lists: within 1e-12 of cbl_ref's own scales (float64 rounding of two orders of the same sums; a scale of 0 means exact);
  * the torch statement of the reverse lists (tests/ordered_ref.reverse_lists_torch) on CPU tensors against a Python loop;
  * the entry points refuse the sizes they have no kernel for before any HIP call, naming the value;
  * the new kernels use no scratch; the points a workgroup takes are what losses.CBL_FUSED_BLOCK_POINTS says;
  * the switch is off by default at every layer, and tools/train.py --fused_contrastive_boundary sets the key."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

sys.path.insert(0, GOLDEN)
import cbl_cases as CC  # noqa: E402
import cbl_fused_ref as FR  # noqa: E402
import cbl_ref  # noqa: E402
import ordered_ref  # noqa: E402

TOL = 1e-12


@pytest.mark.parametrize("name", CC.HAND_CASES + ("flat0",))
def test_the_closed_form_equals_the_float64_restatement(oracle, name):
    case = CC.build(name)
    for i, s in enumerate(cbl_ref.all_stages(oracle.knnquery, case)):
        f = case["f"][i].astype(np.float64)
        fw = FR.forward(f, s["idx"], s["labels"])
        assert fw["count"] == s["count"] and np.array_equal(fw["on"], s["point_mask"]), (name, i)
        assert not fw["pair_w"][~fw["on"]].any()
        want = float(s["loss"].detach())
        assert abs(fw["loss"] - want) <= TOL * s["loss_scale"], (name, i, fw["loss"], want)
        g64, scale = s["grad"]()
        g = FR.backward(f, s["idx"], fw["pair_w"], fw["count"])
        assert (np.abs(g - g64) <= TOL * scale).all(), (name, i, float(np.abs(g - g64).max()))
        if name == "flat0":
            assert fw["count"] == 0 and fw["loss"] == 0.0 and not g.any()


def _loop_lists(idx):
    m = idx.shape[0]
    lists = [[] for _ in range(m)]
    for q, i in enumerate(idx.reshape(-1).tolist()):
        lists[i].append(q)
    return lists


@pytest.mark.parametrize("case", ["repeats", "hub", "one"])
def test_reverse_lists_on_cpu_tensors(case):
    g = torch.Generator().manual_seed(7)
    if case == "repeats":
        idx = torch.randint(0, 23, (23, 9), generator=g, dtype=torch.int32)
        idx[3, 2] = idx[3, 5] = idx[3, 7] = 11                 # one neighbour three times in a row's list
        assert any(len(set(r)) < len(r) for r in idx.tolist())
    elif case == "hub":
        idx = torch.zeros(257, 8, dtype=torch.int64)
    else:
        idx = torch.zeros(1, 5, dtype=torch.int32)
    m, k1 = idx.shape
    rev_start, rev_pair = ordered_ref.reverse_lists_torch(idx)
    assert rev_start.dtype == torch.int32 and tuple(rev_start.shape) == (m + 1,)
    assert rev_pair.dtype == torch.int32 and tuple(rev_pair.shape) == (m * k1,)
    assert int(rev_start[0]) == 0 and int(rev_start[-1]) == m * k1
    want = _loop_lists(idx)
    for i in range(m):
        got = rev_pair[int(rev_start[i]):int(rev_start[i + 1])].tolist()
        assert got == want[i], (case, i)
        assert got == sorted(got)
    ref_start, ref_pair = FR.reverse_lists(idx.numpy())
    assert np.array_equal(rev_start.numpy(), ref_start) and np.array_equal(rev_pair.numpy(), ref_pair)


def test_reverse_lists_checks_its_argument():
    with pytest.raises(TypeError, match="idx"):
        ordered_ref.reverse_lists_torch(torch.zeros(3, 2))
    with pytest.raises(ValueError, match="idx"):
        ordered_ref.reverse_lists_torch(torch.zeros(6, dtype=torch.int32))


@pytest.mark.parametrize("k1,c,named", [(0, 32, "k1 = 0"), (64, 32, "k1 = 64"), (8, 0, "c = 0"), (8, 6, "c = 6"), (8, 132, "c = 132")])
def test_the_entry_points_refuse_unsupported_sizes_before_any_launch(k1, c, named):
    """the checks come before the first HIP call (the buffers are never touched), so they hold without a device"""
    from toothgroupnetwork_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64 + 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    rc = L.tgn_cbl_stage_forward(1, k1, c, p, p, p, p, p, p, p, 64, None)
    assert rc == _lib.ERR_UNSUPPORTED
    msg = L.tgn_last_error().decode()
    assert msg.startswith("tgn_cbl_stage_forward: ") and named in msg and "unsupported" in msg, msg
    rc = L.tgn_cbl_stage_backward(1, k1, c, p, p, p, p, p, p, p, p, None)
    assert rc == _lib.ERR_UNSUPPORTED
    msg = L.tgn_last_error().decode()
    assert msg.startswith("tgn_cbl_stage_backward: ") and named in msg and "unsupported" in msg, msg


def test_pair_numbers_past_32_bits_are_refused_before_any_launch():
    from toothgroupnetwork_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64 + 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    m = 2 ** 31 // 63 + 1
    assert L.tgn_cbl_stage_forward(m, 63, 32, p, p, p, p, p, p, p, 64, None) == _lib.ERR_UNSUPPORTED
    assert f"m * k1 = {m * 63}" in L.tgn_last_error().decode()
    assert L.tgn_cbl_stage_backward(m, 63, 32, p, p, p, p, p, p, p, p, None) == _lib.ERR_UNSUPPORTED
    assert f"m * k1 = {m * 63}" in L.tgn_last_error().decode()


def test_the_workspace_grows_by_one_step_per_workgroup():
    from toothgroupnetwork_amd import _lib, losses
    L, P = _lib.lib(), losses.CBL_FUSED_BLOCK_POINTS
    step = L.tgn_cbl_stage_workspace_bytes(1)
    assert L.tgn_cbl_stage_workspace_bytes(0) == 0 and step > 0
    assert L.tgn_cbl_stage_workspace_bytes(P) == step and L.tgn_cbl_stage_workspace_bytes(P + 1) == 2 * step
    assert L.tgn_cbl_stage_workspace_bytes(24000) == (24000 + P - 1) // P * step


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_new_kernels_use_no_scratch():
    csrc = os.path.join(REPO, "toothgroupnetwork_amd", "csrc")
    out = subprocess.run(["python", os.path.join(csrc, "resource_usage.py"), os.path.join(csrc, "cbl.hip")],
                         capture_output=True, text=True, check=True).stdout
    rows = re.findall(r"^(?:void )?(tgn::cbl_\S+).*?scratch=\s*(\d+)", out, flags=re.M)
    names = {n for n, _ in rows}
    assert {"tgn::cbl_stage_finish_kernel", "tgn::cbl_stage_forward_kernel<0>", "tgn::cbl_stage_forward_kernel<32>",
            "tgn::cbl_stage_backward_kernel<8>"} <= names, out
    for name, scratch in rows:
        assert int(scratch) == 0, f"{name} spills ({scratch} bytes of scratch per lane)"


def test_the_switch_is_off_by_default():
    from toothgroupnetwork_amd import losses, nets
    assert inspect.signature(losses.contrast_boundary_loss).parameters["fused"].default is False
    net = nets.PointTransformerSeg(c=6, k=2, planes=(16, 32), blocks=(2, 3), stride=(1, 1), nsample=(36, 24), block_num=2)
    assert net.fused_contrast is False


def test_contrast_boundary_lists_names_the_argument_it_refuses():
    from toothgroupnetwork_amd import losses
    f, idx, lab = torch.zeros(5, 8), torch.zeros(5, 3, dtype=torch.int32), torch.zeros(5, dtype=torch.int64)
    with pytest.raises(TypeError, match="^f must be"):
        losses.contrast_boundary_lists(idx, idx, lab)
    with pytest.raises(TypeError, match="^idx must be"):
        losses.contrast_boundary_lists(f, f, lab)
    with pytest.raises(TypeError, match="^labels must be"):
        losses.contrast_boundary_lists(f, idx, f[:, 0])
    with pytest.raises(ValueError, match="^idx must be"):
        losses.contrast_boundary_lists(f, idx[:4], lab)
    with pytest.raises(ValueError, match="^labels must hold"):
        losses.contrast_boundary_lists(f, idx, lab[:4])
    with pytest.raises(ValueError, match="the fused stage needs"):
        losses.contrast_boundary_lists(torch.zeros(5, 6), idx, lab)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.contrast_boundary_lists(f, idx, lab)


def test_the_command_line_sets_the_fused_key_on_request_only(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import train as tool
    from toothgroupnetwork_amd import training
    cfg = {"tr_set": {"optimizer": {"lr": 1e-3, "NAME": "adam", "weight_decay": 1e-4},
                      "scheduler": {"sched": "cosine", "warmup_epochs": 0, "full_steps": 40, "schedueler_step": 15, "min_lr": 1e-5},
                      "loss": {"tooth_class_loss_1": 1, "tooth_class_loss_2": 1, "offset_1_loss": 0.03, "offset_1_dir_loss": 0.03,
                               "chamf_1_loss": 0.15, "cbl_loss_1": 1, "cbl_loss_2": 1}}}
    cfg_file = tmp_path / "cfg.py"
    cfg_file.write_text("config = " + repr(cfg) + "\n")
    seen = []

    def stop(name, config):
        seen.append(config)
        raise SystemExit(0)
    monkeypatch.setattr(training, "make_training_model", stop)
    base = ["--model_name", "tgnet_fps", "--config_path", str(cfg_file)]
    with pytest.raises(SystemExit):
        tool.main(base)
    assert "contrastive_boundary_fused" not in seen[-1]["tr_set"]
    with pytest.raises(SystemExit):
        tool.main(base + ["--fused_contrastive_boundary"])
    assert seen[-1]["tr_set"]["contrastive_boundary_fused"] is True and seen[-1]["tr_set"]["contrastive_boundary"] is True
