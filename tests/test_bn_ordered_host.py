"""Host: the numpy restatement of the ordered BatchNorm reductions (tests/bn_ordered_ref.py), the ordered_bn switch, the trainer's
`reproducible` key and the argument checks of tgn_bn_rows_*_ordered.  No GPU: the size function and the refusals run before any HIP call.

The restatement is held to a float64 torch.nn.BatchNorm1d within the bounds of tests/test_gpu_bn_rows_bounds.py (2 u on the
statistics, 8 u M on dbeta / dgamma), and shown to depend on the order it states: on an input whose block partials are 1e20, 1 and
-1e20 the ascending order gives 0 and another order 1.  A GPU result that equals it bit for bit therefore followed the order."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import bn_ordered_ref as R
from conftest import REPO
from test_gpu_bn_rows_bounds import C_BOUND, _ratio, backward64, forward64

SHAPES = [(2, 1), (2, 1024), (7, 3), (1000, 35), (300, 320), (8193, 4), (8197, 4)]


def _case(rows, C, seed):
    g = torch.Generator().manual_seed(seed)
    std = torch.linspace(0.5, 3.0, C)
    x = torch.randn(rows, C, generator=g) * std + torch.linspace(-1.0, 1.0, C).flip(0) * 10.0 * std
    return x, torch.randn(rows, C, generator=g), torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "plain"])
@pytest.mark.parametrize("rows,C", SHAPES)
def test_the_restatement_against_float64_batchnorm(rows, C, relu):
    x, dy, gamma, beta = _case(rows, C, rows + C)
    bn = torch.nn.BatchNorm1d(C).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(torch.randn(C, generator=torch.Generator().manual_seed(1)))       # float32 values: the kernel's buffers are
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    eps = float(np.float32(bn.eps))
    bn.eps = eps
    x64 = x.double().requires_grad_(True)
    y64 = bn(x64)
    got = R.forward(x.numpy(), bn.eps, bn.momentum, rm0.float().numpy(), rv0.float().numpy())
    f = forward64(x.double(), gamma.double(), beta.double(), eps, relu)
    assert _ratio(torch.from_numpy(got["save_mean"]), f["mean"], f["mean"].abs(), 2.0) <= 1.0
    assert _ratio(torch.from_numpy(got["save_invstd"]), f["invstd"], f["invstd"], 2.0) <= 1.0
    m = bn.momentum
    for name, new, old in (("running_mean", f["mean"], rm0.float().double()), ("running_var", f["var"] * (rows / (rows - 1.0)), rv0.float().double())):
        assert _ratio(torch.from_numpy(got[name]), getattr(bn, name), ((1.0 - m) * old).abs() + (m * new).abs(), 2.0) <= 1.0, name
    # the backward from the restatement's own float32 statistics and a float32 y, whose sign is the mask
    y32 = (y64.detach().clamp_min(0.0) if relu else y64.detach()).float()
    mask = (y32 > 0).double() if relu else torch.ones_like(y64)
    y64.backward(dy.double() * mask)
    dbeta, dgamma = R.backward_sums(x.numpy(), y32.numpy(), dy.numpy(), got["save_mean"], got["save_invstd"], relu)
    b = backward64(f, dy.double() * mask, gamma.double(), rows)
    assert torch.allclose(b["dbeta"][0], bn.bias.grad, rtol=1e-9, atol=1e-9) and torch.allclose(b["dgamma"][0], bn.weight.grad, rtol=1e-9, atol=1e-9)
    assert _ratio(torch.from_numpy(dbeta), bn.bias.grad, b["dbeta"][1], C_BOUND) <= 1.0
    assert _ratio(torch.from_numpy(dgamma), bn.weight.grad, b["dgamma"][1], C_BOUND) <= 1.0


def test_the_restatement_depends_on_the_block_order():
    """(8197, 4): five blocks of 256 threads, T = 1280.  Elements 0, 256 and 512 are the first of threads 0, 256 and 512, all in
    column 0, one per block: 1e20, 1 and -1e20.  Ascending, the 1 is lost in 1e20 before -1e20 arrives; with blocks 1 and 2 swapped
    it survives."""
    rows, C = 8197, 4
    assert R.grid(rows, C) == 5
    x = np.zeros((rows, C), np.float32)
    x.reshape(-1)[[0, 256, 512]] = [1e20, 1.0, -1e20]
    p1, _ = R.forward_partials(x)
    assert p1[0, 0] == np.float64(np.float32(1e20)) and p1[1, 0] == 1.0 and p1[2, 0] == -p1[0, 0] and not p1[3:].any()
    assert R.combine(p1)[0] == 0.0 and R.combine(p1, [0, 2, 1, 3, 4])[0] == 1.0
    a, b = R.forward(x, 1e-5, 0.1), R.forward(x, 1e-5, 0.1, block_order=[0, 2, 1, 3, 4])
    assert a["save_mean"][0] == 0.0 and b["save_mean"][0] == np.float32(1.0 / rows)
    # within a block the thread order matters in the same way: threads 0, 4, 8 share column 0
    x[:] = 0
    x.reshape(-1)[[0, 4, 8]] = [1e20, 1.0, -1e20]
    assert R.forward(x, 1e-5, 0.1)["save_mean"][0] == 0.0
    x.reshape(-1)[[0, 4, 8]] = [1e20, -1e20, 1.0]
    assert R.forward(x, 1e-5, 0.1)["save_mean"][0] == np.float32(1.0 / rows)


def test_the_grid_rule():
    assert [R.grid(*s) for s in SHAPES + [(262145, 32)]] == [1, 4, 3, 35, 15, 5, 5, 1024]
    assert R.grid(1000, 35) % 35 == 0 and R.grid(300, 320) % 5 == 0        # C / gcd(256, C) = 35 and 5


def test_the_switch_defaults_to_off_and_overrides(monkeypatch):
    from toothgroupnetwork_amd import config
    assert config.Config().ordered_bn is False
    monkeypatch.delenv("TGN_ORDERED_BN", raising=False)
    assert config.Config.from_env().ordered_bn is False
    monkeypatch.setenv("TGN_ORDERED_BN", "1")
    assert config.Config.from_env().ordered_bn is True and config.Config.from_env().ordered_backward is False
    monkeypatch.setenv("TGN_ORDERED_BN", "0")
    assert config.Config.from_env().ordered_bn is False
    before = config.cfg.ordered_bn
    with config.override(ordered_bn=True):
        assert config.cfg.ordered_bn is True
        with config.override(ordered_bn=False):
            assert config.cfg.ordered_bn is False
        assert config.cfg.ordered_bn is True
    assert config.cfg.ordered_bn is before
    assert "ordered_bn" in config.__doc__ and "TGN_ORDERED_BN" in config.__doc__


def test_the_command_line_sets_reproducible_on_request_only(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import train as tool
    from toothgroupnetwork_amd import training
    cfg_file = tmp_path / "cfg.py"
    cfg_file.write_text("config = {'tr_set': {'loss': {}}}\n")
    seen = []

    def stop(name, config):
        seen.append(config)
        raise SystemExit(0)
    monkeypatch.setattr(training, "make_training_model", stop)
    base = ["--model_name", "tgnet_fps", "--config_path", str(cfg_file)]
    with pytest.raises(SystemExit):
        tool.main(base + ["--ordered_backward", "--fused_contrastive_boundary"])
    assert "reproducible" not in seen[-1]["tr_set"]
    with pytest.raises(SystemExit):
        tool.main(base + ["--reproducible"])
    assert seen[-1]["tr_set"]["reproducible"] is True
    assert "ordered_backward" not in seen[-1]["tr_set"] and "contrastive_boundary_fused" not in seen[-1]["tr_set"]


def test_the_refusal_table_is_checked_before_anything_is_built(monkeypatch):
    from toothgroupnetwork_amd import training
    monkeypatch.setitem(training.NOT_REPRODUCIBLE, "pointnet", "some_operator_backward has no deterministic form")
    with pytest.raises(NotImplementedError, match="pointnet.*some_operator_backward"):
        training.make_training_model("pointnet", {"tr_set": {"reproducible": True}})
    assert set(training.NOT_REPRODUCIBLE) <= set(training.MODEL_NAMES)
    assert all(isinstance(v, str) and len(v) > 20 for k, v in training.NOT_REPRODUCIBLE.items() if k != "pointnet")


def test_bn_rows_calls_in_both_forms_on_a_recorder():
    """_BNRows on the recorder of tests/test_backward_call_ledger.py: with ordered_bn off, exactly the two calls there were, with the
    operands they had (the workspace arrives zeroed), whatever ordered_backward says; with it on, the two ordered calls, their
    workspace as large as the size function says and with any contents."""
    from test_backward_call_ledger import harness
    from toothgroupnetwork_amd import config, point_transformer as PT
    rows, C = 6, 5

    def run():
        bn = torch.nn.BatchNorm1d(C).train()
        x = torch.randn(rows, C, requires_grad=True)
        y = PT._BNRows.apply(x, bn.weight, bn.bias, bn, True)
        y.backward(torch.ones(rows, C))
        return bn

    for ordered_backward in (False, True):
        with harness(ordered_backward) as rec, config.override(ordered_bn=False):
            bn = run()
        assert [c[0] for c in rec.calls] == ["tgn_bn_rows_workspace_bytes", "tgn_bn_rows_forward", "tgn_bn_rows_backward"]
        fwd, bwd = rec.calls[1][2], rec.calls[2][2]
        assert fwd[:2] == [rows, C] and len(fwd) == 16 and fwd[-2] == "uint8[64]:zero" and fwd[-1] == "stream"
        assert bwd[:2] == [rows, C] and len(bwd) == 14 and bwd[-2] == "uint8[64]:zero" and bwd[-1] == "stream"
        assert "_tgn_bn_ws_ordered" not in bn.__dict__ and len(bn.__dict__["_tgn_bn_ws"]) == 1
    with harness(False) as rec, config.override(ordered_bn=True):
        bn = run()
    assert [c[0] for c in rec.calls] == ["tgn_bn_rows_ordered_workspace_bytes", "tgn_bn_rows_forward_ordered",
                                         "tgn_bn_rows_ordered_workspace_bytes", "tgn_bn_rows_backward_ordered"]
    fwd, bwd = rec.calls[1][2], rec.calls[3][2]
    assert fwd[:2] == [rows, C] and len(fwd) == 17 and fwd[-3:] == ["uint8[64]:poison", 64, "stream"]
    assert bwd[:2] == [rows, C] and len(bwd) == 15 and bwd[-3:] == ["uint8[64]:poison", 64, "stream"]
    assert bn.__dict__["_tgn_bn_ws"] == {} and len(bn.__dict__["_tgn_bn_ws_ordered"]) == 1


def test_workspace_size_grows_with_rows_and_is_zero_for_what_is_unsupported():
    from toothgroupnetwork_amd import _lib
    L = _lib.lib()
    for rows, C in SHAPES + [(262145, 32), (24000 * 36, 32), (94 * 24, 512)]:
        assert L.tgn_bn_rows_ordered_workspace_bytes(rows, C) == R.workspace_bytes(rows, C), (rows, C)
    sizes = [L.tgn_bn_rows_ordered_workspace_bytes(rows, 32) for rows in (2, 256, 257, 5000, 100000, 262144, 262145, 10 ** 7)]
    assert sizes == sorted(sizes) and sizes[0] == 2 * 32 * 8 and sizes[2] > sizes[1] and sizes[-1] == sizes[-2] == 1024 * 2 * 32 * 8
    for rows, C in ((2, 0), (2, -1), (2, 1025), (1, 4), (0, 4), (-5, 4)):
        assert L.tgn_bn_rows_ordered_workspace_bytes(rows, C) == 0, (rows, C)


def test_bad_arguments_are_refused_before_any_launch():
    from toothgroupnetwork_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    rows, C = 7, 3
    need = L.tgn_bn_rows_ordered_workspace_bytes(rows, C)

    def fwd(rows=rows, C=C, x=p, rm=p, rv=p, ws=p, nbytes=need):
        return L.tgn_bn_rows_forward_ordered(rows, C, x, p, p, 1e-5, 0.1, rm, rv, p, 1, p, p, p, ws, nbytes, None)

    def bwd(rows=rows, C=C, y=p, relu=1, ws=p, nbytes=need):
        return L.tgn_bn_rows_backward_ordered(rows, C, p, y, p, p, p, p, relu, p, p, p, ws, nbytes, None)

    for call, name in ((fwd, "tgn_bn_rows_forward_ordered"), (bwd, "tgn_bn_rows_backward_ordered")):
        for kw in (dict(rows=1), dict(C=0), dict(C=1025)):
            assert call(**kw) == _lib.ERR_UNSUPPORTED, (name, kw)
            assert L.tgn_last_error().decode().startswith(name + ": rows")
        for kw in (dict(nbytes=need - 1), dict(nbytes=0)):
            assert call(**kw) == _lib.ERR_INVALID_ARGUMENT, (name, kw)
            assert "tgn_bn_rows_ordered_workspace_bytes" in L.tgn_last_error().decode()
        assert call(ws=None) == _lib.ERR_INVALID_ARGUMENT and L.tgn_last_error().decode() == name + ": null pointer"
    assert fwd(x=None) == _lib.ERR_INVALID_ARGUMENT and fwd(rv=None) == _lib.ERR_INVALID_ARGUMENT      # one running pointer without the other
    assert bwd(y=None) == _lib.ERR_INVALID_ARGUMENT                                                    # relu needs y
