"""GPU: the ordered reductions of the fused BatchNorm over rows (tgn_bn_rows_forward_ordered / tgn_bn_rows_backward_ordered,
csrc/bnorm.hip) through the C ABI and through point_transformer.bn_rows under config.cfg.ordered_bn.

  bit for bit against tests/bn_ordered_ref.py (the header's summation order in numpy): save_mean, running_mean, running_var,
      num_batches_tracked, dbeta, dgamma -- sums, divisions and casts only.  The restatement depends on the order
      (tests/test_bn_ordered_host.py), so equality means the kernels followed it;
  within the bounds of tests/test_gpu_bn_rows_bounds.py (its run_and_check, under the switch): save_invstd, y, dx, and every quantity
      above once more against float64.

Shapes (rows, C), the smallest at which each seam of the reduction exists:
  (2, 1)                   one block, one column, 254 idle threads
  (2, 1024)                the widest C at the fewest rows: four blocks, each keeps a quarter of the columns and zero-fills the rest
  (7, 3), (1000, 35)       C does not divide 256: 3 and 35 blocks (a multiple of C / gcd(256, C)), a block's threads share columns unevenly
  (300, 320)               C > 256 and no multiple of it: 15 blocks, each keeps 256 of 320 columns
  (8193, 4), (8197, 4)     one element and an odd tail past a block's 8192: the four-in-flight loop and its tail both run
  (262 145, 32)            the 1024-block cap is reached (33 MB): 16 blocks per chain of the finishing launch
Variants: relu on / off, a misaligned x (the scalar element-wise kernels), track_running_stats=False.  Repeatability while another
stream runs grouping launches: a child process (tests/bn_ordered_stream_launcher.py, which says why).  With the switch off bn_rows makes
exactly the two calls it made before.  On the parent commit the entry points and the switch do not exist: every test here fails."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bn_ordered_ref as R
from test_gpu_bn_rows_bounds import _inputs, _module, run_and_check

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(2, 1), (2, 1024), (7, 3), (1000, 35), (300, 320), (8193, 4), (8197, 4), (262145, 32)]


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.numpy().view(np.uint32 if t.dtype == torch.float32 else np.int64)


def _equal_bits(got, want, what):
    got, want = _bits(got), np.ascontiguousarray(want).view(np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} values differ from the restatement, the first at {bad[0]}"


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "plain"])
@pytest.mark.parametrize("rows,C", SHAPES)
def test_the_c_abi_against_the_restatement_bit_for_bit(dev, rows, C, relu):
    """one forward and one backward through the library's own entry points, the workspace exactly as large as the size function says
    and full of 0xFF bytes (NaNs as doubles) on entry: the header allows any contents"""
    from toothgroupnetwork_amd import _lib
    L, st = _lib.ops(), _lib.stream()
    x, dy = _inputs(dev, rows, C, rows + C, spread=10.0)
    g = torch.Generator().manual_seed(C)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev)
    rm, rv = torch.randn(C, generator=g).to(dev), (torch.rand(C, generator=g) + 0.5).to(dev)
    rm0, rv0 = rm.cpu().numpy(), rv.cpu().numpy()
    nbt = torch.tensor([41], dtype=torch.int64, device=dev)
    nbytes = int(L.tgn_bn_rows_ordered_workspace_bytes(rows, C))
    assert nbytes == R.workspace_bytes(rows, C)
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=dev)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean, invstd, dgamma, dbeta = (torch.empty(C, device=dev) for _ in range(4))
    eps, momentum = 1e-5, 0.1
    L.tgn_bn_rows_forward_ordered(rows, C, x, gamma, beta, eps, momentum, rm, rv, nbt, int(relu), y, mean, invstd, ws, nbytes, st)
    ws.fill_(255)
    L.tgn_bn_rows_backward_ordered(rows, C, x, y, dy, gamma, mean, invstd, int(relu), dx, dgamma, dbeta, ws, nbytes, st)
    torch.cuda.synchronize()
    x_np = x.cpu().numpy()
    ref = R.forward(x_np, eps, momentum, rm0, rv0)
    _equal_bits(mean, ref["save_mean"], "save_mean")
    _equal_bits(rm, ref["running_mean"], "running_mean")
    _equal_bits(rv, ref["running_var"], "running_var")
    assert int(nbt) == 42
    # save_invstd = (float)(1 / sqrt(var + eps)) from the same double var: at most the last bit of a correctly rounded sqrt and
    # division apart, whatever the device's double sqrt does
    assert np.all(np.abs(invstd.cpu().numpy().astype(np.float64) - ref["invstd"]) <= 2.0 ** -23 * ref["invstd"])
    want_db, want_dg = R.backward_sums(x_np, y.cpu().numpy(), dy.cpu().numpy(), mean.cpu().numpy(), invstd.cpu().numpy(), relu)
    _equal_bits(dbeta, want_db, "dbeta")
    _equal_bits(dgamma, want_dg, "dgamma")
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())


@pytest.mark.parametrize("rows,C,relu", [(r, c, relu) for r, c in SHAPES[:-1] for relu in (True, False)] + [(262145, 32, True)])
def test_bn_rows_under_the_switch_within_the_bounds_and_bit_for_bit(dev, rows, C, relu):
    """point_transformer.bn_rows twice in a row on one module: every quantity within the float64 bounds (run_and_check), the sums
    bit for bit against the restatement of both steps, through the module's parked workspace"""
    from toothgroupnetwork_amd import config
    x, dy = _inputs(dev, rows, C, rows * 3 + C, spread=10.0)
    bn = _module(dev, C, C)
    rm, rv = bn.running_mean.cpu().numpy(), bn.running_var.cpu().numpy()
    with config.override(ordered_bn=True):
        res = run_and_check(dev, bn, x, dy, relu, f"ordered bn_rows ({rows},{C}) relu={relu}")
    assert bn.__dict__["_tgn_bn_ws"] == {} and len(bn.__dict__["_tgn_bn_ws_ordered"]) == 1, "the ordered calls were not the ones made"
    x_np = x.cpu().numpy()
    for _ in range(2):
        ref = R.forward(x_np, bn.eps, bn.momentum, rm, rv)
        rm, rv = ref["running_mean"], ref["running_var"]
    _equal_bits(res["mean"], ref["save_mean"], "save_mean")
    _equal_bits(bn.running_mean, rm, "running_mean after two steps")
    _equal_bits(bn.running_var, rv, "running_var after two steps")
    assert int(bn.num_batches_tracked) == 2
    want_db, want_dg = R.backward_sums(x_np, res["y"].cpu().numpy(), dy.cpu().numpy(), res["mean"].cpu().numpy(), res["invstd"].cpu().numpy(), relu)
    _equal_bits(res["dbeta"], want_db, "dbeta")
    _equal_bits(res["dgamma"], want_dg, "dgamma")


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "plain"])
def test_misaligned_rows_and_no_running_statistics_give_the_same_bits(dev, relu):
    """a contiguous (301, 8) view one float into its storage (C % 4 == 0 but no 16-byte alignment: the scalar element-wise kernels) and a
    module with track_running_stats=False: the bits of the aligned, tracking run"""
    from toothgroupnetwork_amd import config
    rows, C = 301, 8
    x, dy = _inputs(dev, rows, C, 23, spread=10.0)
    store = torch.empty(rows * C + 1, dtype=torch.float32, device=dev)
    shifted = store[1:].view(rows, C)
    shifted.copy_(x)
    assert shifted.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
    bn_a, bn_b, bn_n = _module(dev, C, 24), _module(dev, C, 24), _module(dev, C, 24, track=False)
    with config.override(ordered_bn=True):
        a = run_and_check(dev, bn_a, x, dy, relu, f"ordered bn_rows aligned relu={relu}")
        b = run_and_check(dev, bn_b, shifted, dy, relu, f"ordered bn_rows misaligned relu={relu}")
        n = run_and_check(dev, bn_n, x, dy, relu, f"ordered bn_rows track_running_stats=False relu={relu}")
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], n[k]), k
    assert torch.equal(bn_a.running_mean, bn_b.running_mean) and torch.equal(bn_a.running_var, bn_b.running_var)
    assert bn_n.running_mean is None and bn_n.num_batches_tracked is None
    assert all("_tgn_bn_ws_ordered" in m.__dict__ and m.__dict__["_tgn_bn_ws"] == {} for m in (bn_a, bn_b, bn_n))


def test_the_workspace_grows_with_the_rows_and_a_backward_follows_its_forward(dev):
    """one module, 300 rows then 9000 then 300: the parked buffer grows once and is kept; a forward made under the switch has an ordered
    backward after the switch is off again, and the other way round"""
    from toothgroupnetwork_amd import _lib, config, point_transformer as PT
    C = 4
    bn = _module(dev, C, 3)
    sizes = []
    for rows in (300, 9000, 300):
        x, dy = _inputs(dev, rows, C, rows, spread=1.0)
        with config.override(ordered_bn=True):
            y = PT.bn_rows(bn, x.requires_grad_(True), relu=True)
        y.backward(dy)                                                   # ordered: the atomic workspace is never made
        (ws,) = bn.__dict__["_tgn_bn_ws_ordered"].values()
        sizes.append(ws.numel())
        assert ws.numel() >= _lib.lib().tgn_bn_rows_ordered_workspace_bytes(rows, C) and bn.__dict__["_tgn_bn_ws"] == {}
    assert sizes[1] > sizes[0] and sizes[2] == sizes[1]
    x, dy = _inputs(dev, 300, C, 1, spread=1.0)
    y = PT.bn_rows(bn, x.requires_grad_(True), relu=True)                # atomic forward ...
    with config.override(ordered_bn=True):
        y.backward(dy)                                                   # ... atomic backward
    torch.cuda.synchronize()
    (zeroed,) = bn.__dict__["_tgn_bn_ws"].values()
    assert not bool(zeroed.any()) and sizes[2] == next(iter(bn.__dict__["_tgn_bn_ws_ordered"].values())).numel()


class _Recording:
    """the checked library view, noting the symbols called"""

    def __init__(self, real):
        self.real, self.names = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call


@pytest.mark.parametrize("ordered_backward", [False, True], ids=["atomic-gathers", "ordered-gathers"])
def test_with_the_switch_off_bn_rows_makes_the_two_calls_it_made_before(dev, monkeypatch, ordered_backward):
    from toothgroupnetwork_amd import _lib, config, point_transformer as PT
    rec = _Recording(_lib.ops())
    monkeypatch.setattr(_lib, "_ops", rec)
    x, dy = _inputs(dev, 300, 12, 2, spread=1.0)
    bn = _module(dev, 12, 5)
    with config.override(ordered_bn=False, ordered_backward=ordered_backward):
        PT.bn_rows(bn, x.requires_grad_(True), relu=True).backward(dy)
        assert rec.names == ["tgn_bn_rows_workspace_bytes", "tgn_bn_rows_forward", "tgn_bn_rows_backward"]
        del rec.names[:]
        PT.bn_rows(bn, x, relu=True).backward(dy)
        assert rec.names == ["tgn_bn_rows_forward", "tgn_bn_rows_backward"]
    del rec.names[:]
    with config.override(ordered_bn=True):
        PT.bn_rows(bn, x, relu=True).backward(dy)
    assert rec.names == ["tgn_bn_rows_ordered_workspace_bytes", "tgn_bn_rows_forward_ordered", "tgn_bn_rows_ordered_workspace_bytes",
                         "tgn_bn_rows_backward_ordered"]
    torch.cuda.synchronize()


def test_twenty_runs_under_contention_equal_the_idle_run():
    """In a child process (tests/bn_ordered_stream_launcher.py): a stream created here would stay with the test process and change
    which hardware queues the streams of later tests share."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "bn_ordered_stream_launcher.py"), "contention"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bn ordered contention ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
