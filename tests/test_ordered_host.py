"""Host: the contract of the ordered backward as tests/ordered_ref.py states it, the switch, and what the two entry points refuse
before any launch.  No GPU.

The bound of the float32 reference against float64: a row's value is a sequential sum of L terms, each term at most one rounded
product (the multiplication by sign = +-1 is exact).  L - 1 additions and one product rounding per term give, to first order,
|got - exact| <= L u sum |t_i| with u = 2^-24; the tests allow (L + 2) u sum |t_i| for the second-order part, with `exact` and
sum |t_i| evaluated in float64 from the same float32 inputs (a row without terms must be exactly 0)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import ordered_ref as R
from conftest import REPO

U32 = 2.0 ** -24


def _lists_cases():
    g = np.random.default_rng(7)
    return {
        "one": (np.zeros((1, 1), np.int64), 1),
        "square": (g.integers(0, 65, (65, 16)), 65),
        "fine_to_coarse": (g.integers(0, 40, (300, 3)), 40),
        "hub": (np.full((300, 16), 7), 300),
        "half_untargeted": (g.integers(0, 50, (100, 8)) * 2, 100),
        "out_of_range": (g.integers(-5, 70, (64, 9)), 64),
    }


@pytest.mark.parametrize("case", sorted(_lists_cases()))
def test_reference_lists_are_the_definition(case):
    """rev_pair[rev_start[r] : rev_start[r + 1]] = the ascending pair numbers whose (clamped) index is r, by brute force"""
    idx, n = _lists_cases()[case]
    rev_start, rev_pair = R.reverse_lists(idx, n)
    flat = idx.reshape(-1)
    flat = np.where((flat < 0) | (flat >= n), 0, flat)
    assert rev_start.dtype == np.int32 and rev_pair.dtype == np.int32 and rev_start.shape == (n + 1,) and rev_start[0] == 0 and rev_start[-1] == flat.size
    for r in range(n):
        assert np.array_equal(rev_pair[rev_start[r]:rev_start[r + 1]], np.nonzero(flat == r)[0]), r


@pytest.mark.parametrize("case", ["one", "square", "hub", "out_of_range"])
def test_reference_lists_equal_losses_reverse_lists(case):
    """the numpy reference against the torch statement (R.reverse_lists_torch, the lists of the fused contrastive-boundary stage), on
    square lists (m == n), the only ones it takes"""
    idx, n = _lists_cases()[case]
    assert idx.shape[0] == n
    want_start, want_pair = R.reverse_lists_torch(torch.from_numpy(idx))
    got_start, got_pair = R.reverse_lists(idx, n)
    assert np.array_equal(got_start, want_start.numpy()) and np.array_equal(got_pair, want_pair.numpy())


def test_reference_lists_of_a_dense_batch():
    g = np.random.default_rng(3)
    b, n, pairs = 3, 17, 40
    idx = g.integers(0, n, (b, pairs))
    rev_start, rev_pair = R.reverse_lists(idx, n, b)
    assert rev_start.shape == (b * n + 1,) and rev_pair.shape == (b * pairs,)
    for bi in range(b):
        own_start, own_pair = R.reverse_lists(idx[bi], n)
        assert np.array_equal(rev_start[bi * n:(bi + 1) * n + 1] - bi * pairs, own_start)
        assert np.array_equal(rev_pair[bi * pairs:(bi + 1) * pairs] - bi * pairs, own_pair)


def _check(got, exact, absum, lists, n_rows, k, what):
    rev_start = R.identity_lists(n_rows, k)[0] if lists is None else lists[0]
    length = (rev_start[1:].astype(np.int64) - rev_start[:-1])[:, None]
    err = np.abs(got.astype(np.float64) - exact)
    lim = (length + 2) * U32 * absum
    print(f"{what}: worst {float((err / np.maximum(U32 * absum, 1e-300)).max()):.2f} u sum|terms|, longest row {int(length.max())}")
    assert (err <= lim).all(), what
    assert not got[length[:, 0] == 0].any() and not np.signbit(got[length[:, 0] == 0]).any(), f"{what}: a row without pairs is +0.0"


@pytest.mark.parametrize("c", [1, 3, 35])
def test_reference_scatter_against_float64_autograd(c):
    """the three backward forms against torch autograd in float64 on the CPU: grouping (pair rows), subtraction (identity segments
    and pair rows with sign -1), interpolation (query rows, g = 1)"""
    g = torch.Generator().manual_seed(c)
    n, m, k = 40, 90, 5
    idx = torch.randint(0, n, (m, k), generator=g)
    idx[:, 0] = 3                                                           # a hub of m pairs
    go = torch.randn(m, k, c, generator=g)
    lists = R.reverse_lists(idx.numpy(), n)
    # grouping
    x = torch.zeros(n, c, dtype=torch.float64, requires_grad=True)
    x[idx].backward(go.double())
    got = R.scatter(n, lists, go.numpy().reshape(-1, c))
    exact, absum = R.scatter_f64(n, lists, go.numpy().reshape(-1, c))
    assert np.allclose(exact, x.grad.numpy(), rtol=1e-13, atol=1e-13)
    _check(got, x.grad.numpy(), absum, lists, n, 1, "grouping")
    # subtraction: out[i, j] = a[i] - b[idx[i, j]]
    a = torch.zeros(m, c, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(n, c, dtype=torch.float64, requires_grad=True)
    (a[:, None, :] - b[idx]).backward(go.double())
    _, absum1 = R.scatter_f64(m, None, go.numpy().reshape(-1, c), k=k)
    _check(R.scatter(m, None, go.numpy().reshape(-1, c), k=k), a.grad.numpy(), absum1, None, m, k, "subtraction g1")
    _check(R.scatter(n, lists, go.numpy().reshape(-1, c), sign=-1.0), b.grad.numpy(), absum, lists, n, 1, "subtraction g2")
    # interpolation: out[i] = sum_j f[idx[i, j]] * w[i, j]
    w = torch.rand(m, k, generator=g)
    gq = torch.randn(m, c, generator=g)
    f = torch.zeros(n, c, dtype=torch.float64, requires_grad=True)
    (f[idx] * w.double()[:, :, None]).sum(1).backward(gq.double())
    _, absum_q = R.scatter_f64(n, lists, gq.numpy(), coef=w.numpy().reshape(-1, 1), k=k)
    _check(R.scatter(n, lists, gq.numpy(), coef=w.numpy().reshape(-1, 1), k=k), f.grad.numpy(), absum_q, lists, n, 1, "interpolation")


def test_reference_scatter_is_sequential_and_rounds_every_term():
    """an order-sensitive sum: 2^24 + 1 + 1 (each 1 is lost) against 1 + 1 + 2^24, and a product that is rounded before the add"""
    big = np.float32(2.0 ** 24)
    src = np.array([[big], [1.0], [1.0]], np.float32)
    first = (np.array([0, 3], np.int32), np.array([0, 1, 2], np.int32))
    last = (np.array([0, 3], np.int32), np.array([1, 2, 0], np.int32))
    assert R.scatter(1, first, src)[0, 0] == big and R.scatter(1, last, src)[0, 0] == big + np.float32(2.0)
    x, w = np.float32(1.0 + 2.0 ** -12), np.float32(1.0 + 2.0 ** -12)      # x * w = 1 + 2^-11 + 2^-24: rounds to 1 + 2^-11
    got = R.scatter(1, (np.array([0, 2], np.int32), np.array([0, 1], np.int32)), np.array([[-1.0], [x]], np.float32),
                    coef=np.array([[1.0], [w]], np.float32), k=1)
    assert got[0, 0] == np.float32(2.0 ** -11)          # -1 + round(x * w); a fused multiply-add would keep the 2^-24


def test_the_switch_defaults_to_off_and_overrides(monkeypatch):
    from toothgroupnetwork_amd import config
    assert config.Config().ordered_backward is False
    monkeypatch.delenv("TGN_ORDERED_BACKWARD", raising=False)
    assert config.Config.from_env().ordered_backward is False
    monkeypatch.setenv("TGN_ORDERED_BACKWARD", "1")
    assert config.Config.from_env().ordered_backward is True
    monkeypatch.setenv("TGN_ORDERED_BACKWARD", "0")
    assert config.Config.from_env().ordered_backward is False
    before = config.cfg.ordered_backward
    with config.override(ordered_backward=True):
        assert config.cfg.ordered_backward is True
        with config.override(ordered_backward=False):
            assert config.cfg.ordered_backward is False
    assert config.cfg.ordered_backward is before
    assert "ordered_backward" in config.__doc__ and "TGN_ORDERED_BACKWARD" in config.__doc__


def test_the_command_line_sets_the_key_on_request_only(tmp_path, monkeypatch):
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
        tool.main(base)
    assert "ordered_backward" not in seen[-1]["tr_set"]
    with pytest.raises(SystemExit):
        tool.main(base + ["--ordered_backward"])
    assert seen[-1]["tr_set"]["ordered_backward"] is True


def test_the_python_front_end_refuses_what_it_would_misread():
    from toothgroupnetwork_amd import ordered
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ordered.reverse_lists(torch.zeros(4, 2, dtype=torch.int32), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ordered.scatter(torch.zeros(8, 3), 4)


def _ptr():
    buf = ctypes.create_string_buffer(64)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_workspace_size_and_the_2_31_limits_before_any_launch():
    """the size function is arithmetic (counts + one sum per 1024-row scan tile + slots, int32 each); past 2^31 rows or pairs it
    returns 0 and the call is TGN_ERR_INVALID_ARGUMENT with a message, before the first HIP call"""
    from toothgroupnetwork_amd import _lib
    L = _lib.lib()
    assert L.tgn_reverse_lists_workspace_bytes(1, 24000, 24000 * 16) == 4 * (24000 + 24 + 24000 * 16)
    assert L.tgn_reverse_lists_workspace_bytes(3, 1025, 7) == 4 * (3075 + 4 + 21)
    assert L.tgn_reverse_lists_workspace_bytes(1, 2 ** 31 - 1, 1) > 0
    assert L.tgn_reverse_lists_workspace_bytes(2, 2 ** 30, 1) == 0 and L.tgn_reverse_lists_workspace_bytes(2, 5, 2 ** 30) == 0
    buf, p = _ptr()
    for b, n, pairs in ((2, 2 ** 30, 1), (2, 5, 2 ** 30), (1, 5, 2 ** 31)):
        assert L.tgn_reverse_lists(b, n, pairs, p, 0, p, p, p, 64, None) == _lib.ERR_INVALID_ARGUMENT
        assert "below 2^31" in L.tgn_last_error().decode()
    assert L.tgn_reverse_lists(1, 4, 4, p, 0, p, p, p, 8, None) == _lib.ERR_INVALID_ARGUMENT      # a workspace that is too small
    assert "tgn_reverse_lists_workspace_bytes" in L.tgn_last_error().decode()


def test_scatter_refuses_bad_arguments_before_any_launch():
    from toothgroupnetwork_amd import _lib
    L = _lib.lib()
    buf, p = _ptr()
    assert L.tgn_scatter_ordered(0, 4, 1, 1, p, p, p, None, 1.0, p, None) == 0                       # nothing to do
    for args in ((4, 4, 1, 1, p, None, p, None, 1.0, p),        # one list without the other
                 (4, 4, 1, 1, p, p, p, None, 0.5, p),           # sign
                 (4, 4, 0, 1, None, None, p, None, 1.0, p),     # k
                 (4, 6, 1, 4, p, p, p, p, 1.0, p)):             # g does not divide c
        assert L.tgn_scatter_ordered(*args, None) == _lib.ERR_INVALID_ARGUMENT, args
        assert L.tgn_last_error().decode().startswith("tgn_scatter_ordered:")
