"""GPU: tgn_linear_act_max (csrc/linear_max.hip) through the C ABI, against its contract:

    out[b, c] = max_{n < N} act( (sum_{k < K} x[b, k, n] * Wt[k, c]) + shift[c] )

Accuracy is held to a float64 evaluation of the same float32 operands with the derived bound of a K-term fma chain, one add and one
activation multiply, g = (K + 2) u / (1 - (K + 2) u), u = 2^-24, times max_n (sum_k |x Wt| + |shift|): the max moves by no more than
its worst candidate's error.  No extra factor.  The shapes are the smallest that reach every edge of the tiling (128 points x 128
channels x 16 k): one point, one row into a second point tile, partial tiles in every dimension, several chunks and scans."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

ACTS = {"identity": 0, "relu": 1, "leaky": 2}
U = 2.0 ** -24


def run(x, Wt, shift, act, slope=0.0, ws_bytes=None, out=None):
    """The kernel on the current stream; x (B, K, N), Wt (K, C), shift (C) float32 contiguous -> (rc, out (B, C))."""
    from toothgroupnetwork_amd import _lib
    L = _lib.lib()
    B, K, N = x.shape
    C = Wt.shape[1]
    assert x.is_contiguous() and Wt.is_contiguous() and Wt.shape[0] == K and shift.shape == (C,)
    need = L.tgn_linear_act_max_workspace_bytes(B, N, K, C)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    if out is None:
        out = torch.full((B, C), 12345.0, dtype=torch.float32, device=x.device)
    rc = L.tgn_linear_act_max(B, N, K, C, _lib.ptr(x), _lib.ptr(Wt), _lib.ptr(shift), ACTS[act], ctypes.c_float(slope), _lib.ptr(out),
                              _lib.ptr(ws), need if ws_bytes is None else ws_bytes, _lib.stream())
    return rc, out


def ok(x, Wt, shift, act, slope=0.0):
    rc, out = run(x, Wt, shift, act, slope)
    assert rc == 0
    return out


def exact(x, Wt, shift, act, slope=0.0):
    """float64 evaluation of the float32 operands -> (result (B, C), magnitude max_n (sum_k |x Wt| + |shift|) (B, C))."""
    x64, W64, s64 = x.double(), Wt.double(), shift.double()
    pre = torch.einsum("bkn,kc->bcn", x64, W64) + s64[None, :, None]
    if act == "relu":
        pre = pre.clamp_min(0.0)
    elif act == "leaky":
        pre = torch.where(pre > 0, pre, pre * float(torch.tensor(slope, dtype=torch.float32)))
    mag = torch.einsum("bkn,kc->bcn", x64.abs(), W64.abs()) + s64.abs()[None, :, None]
    return pre.max(dim=2)[0], mag.max(dim=2)[0]


def operands(dev, B, K, C, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, K, N, generator=g)
    Wt = torch.randn(K, C, generator=g) * (1.4 / K ** 0.5)
    shift = torch.randn(C, generator=g) * 0.3
    return x.to(dev), Wt.to(dev), shift.to(dev)


CASES = [
    (1, 128, 1024, 1, "relu"),          # a single point
    (1, 128, 1024, 129, "relu"),        # one row into a second point tile
    (2, 256, 2048, 1000, "identity"),   # PointNet's wide layer, partial last tile
    (3, 192, 1024, 257, "leaky"),       # DGCNN's conv6 shape
    (1, 6, 17, 63, "identity"), (1, 6, 17, 63, "relu"), (1, 6, 17, 63, "leaky"),            # K and C below one tile
    (2, 70, 100, 300, "identity"), (2, 70, 100, 300, "relu"), (2, 70, 100, 300, "leaky"),   # K no multiple of 16, C none of 4
]


@pytest.mark.parametrize("B,K,C,N,act", CASES)
def test_accuracy_against_float64_with_the_derived_bound(dev, B, K, C, N, act):
    x, Wt, shift = operands(dev, B, K, C, N, seed=1000 + K + N)
    slope = 0.2 if act == "leaky" else 0.0
    got = ok(x, Wt, shift, act, slope)
    want, mag = exact(x, Wt, shift, act, slope)
    g = (K + 2) * U / (1.0 - (K + 2) * U)
    ratio = float(((got.double() - want).abs() / (g * mag)).max())
    print(f"\nlinear_act_max (B, K, C, N) = ({B}, {K}, {C}, {N}) {act}: worst |got - exact| / bound = {ratio:.3g}")
    assert torch.isfinite(got).all()
    assert ratio <= 1.0


def test_rows_beyond_n_do_not_take_part(dev):
    """Every product is negative and shift is large and positive on some channels: a zero-padded row of the last tile would
    evaluate to shift[c] and win."""
    B, K, C, N = 1, 128, 1024, 129
    g = torch.Generator().manual_seed(7)
    x = (torch.rand(B, K, N, generator=g) + 0.5).to(dev)
    Wt = (-(torch.rand(K, C, generator=g) + 0.5) / K).to(dev)
    shift = torch.zeros(C)
    shift[::3] = 50.0
    shift = shift.to(dev)
    got = ok(x, Wt, shift, "identity")
    want, mag = exact(x, Wt, shift, "identity")
    assert (got < shift[None]).all()
    bound = (K + 2) * U / (1.0 - (K + 2) * U) * mag
    assert ((got.double() - want).abs() <= bound).all()


def test_running_max_starts_at_minus_infinity(dev):
    B, K, C, N = 2, 32, 200, 300
    g = torch.Generator().manual_seed(8)
    x = (torch.rand(B, K, N, generator=g) + 0.5).to(dev)
    Wt = (-(torch.rand(K, C, generator=g) + 0.5)).to(dev)
    shift = torch.full((C,), -1.0, device=dev)
    got = ok(x, Wt, shift, "identity")
    assert (got < 0).all()
    want, mag = exact(x, Wt, shift, "identity")
    assert ((got.double() - want).abs() <= (K + 2) * U / (1.0 - (K + 2) * U) * mag).all()
    assert (ok(x, Wt, shift, "relu") == 0).all()


def test_a_scan_does_not_depend_on_its_batch(dev):
    x, Wt, shift = operands(dev, 3, 128, 1024, 700, seed=9)
    both = ok(x, Wt, shift, "relu")
    alone = ok(x[1:2].contiguous(), Wt, shift, "relu")
    assert torch.equal(both[1:2], alone)


def test_the_split_of_n_does_not_change_a_bit(dev):
    x, Wt, shift = operands(dev, 2, 256, 300, 1000, seed=10)
    for act, slope in (("identity", 0.0), ("leaky", 0.2)):
        whole = ok(x, Wt, shift, act, slope)
        a = ok(x[:, :, :600].contiguous(), Wt, shift, act, slope)
        b = ok(x[:, :, 600:].contiguous(), Wt, shift, act, slope)
        assert torch.equal(whole, torch.maximum(a, b)), act
    # many chunks against few: one scan (the launch cuts N finely) and the same scan repeated 40 times (it does not)
    one = ok(x[:1].contiguous(), Wt, shift, "identity")
    many = ok(x[:1].repeat(40, 1, 1), Wt, shift, "identity")
    assert torch.equal(many, one.expand(40, -1))


def test_nan_and_inf_propagate_like_torch_max(dev):
    x, Wt, shift = operands(dev, 3, 70, 100, 300, seed=11)
    clean = ok(x, Wt, shift, "relu")
    bad = x.clone()
    bad[1, 3, 277] = float("nan")
    got = ok(bad, Wt, shift, "relu")
    assert torch.isnan(got[1]).all()
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])
    # the NaN in the first row of the first tile, and under the other activations
    bad = x.clone()
    bad[0, 69, 0] = float("nan")
    for act in ("identity", "leaky"):
        got = ok(bad, Wt, shift, act, 0.2)
        assert torch.isnan(got[0]).all() and not torch.isnan(got[1:]).any()
    big = x.clone()
    big[2, 5, 130] = float("inf")
    got = ok(big, Wt.abs() + 0.01, shift, "identity")        # positive weights: the candidate is +inf in every channel
    assert (got[2] == float("inf")).all() and torch.isfinite(got[:2]).all()


def test_bad_arguments_are_refused_before_any_launch(dev):
    from toothgroupnetwork_amd import _lib
    L = _lib.lib()
    x, Wt, shift = operands(dev, 1, 16, 8, 4, seed=12)
    out = torch.full((1, 8), 12345.0, device=dev)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)

    def call(B, N, K, C, ws_bytes):
        return L.tgn_linear_act_max(B, N, K, C, _lib.ptr(x), _lib.ptr(Wt), _lib.ptr(shift), 1, ctypes.c_float(0.0), _lib.ptr(out),
                                    _lib.ptr(ws), ws_bytes, _lib.stream())
    assert call(1, 0, 16, 8, 1 << 16) == _lib.ERR_UNSUPPORTED
    assert L.tgn_last_error().decode() == "tgn_linear_act_max: N must be at least 1 (got 0)"
    assert call(1, 4, 513, 8, 1 << 16) == _lib.ERR_UNSUPPORTED
    assert L.tgn_last_error().decode() == "tgn_linear_act_max: K must be 1 .. 512 (got 513)"
    assert call(0, 4, 16, 8, 1 << 16) == _lib.ERR_UNSUPPORTED and "B must be" in L.tgn_last_error().decode()
    assert call(1, 4, 16, 0, 1 << 16) == _lib.ERR_UNSUPPORTED and "C must be" in L.tgn_last_error().decode()
    need = L.tgn_linear_act_max_workspace_bytes(1, 4, 16, 8)
    assert need == 8 * 4
    assert call(1, 4, 16, 8, need - 1) == _lib.ERR_INVALID_ARGUMENT
    assert L.tgn_last_error().decode() == "tgn_linear_act_max: ws_bytes 31 is short of tgn_linear_act_max_workspace_bytes = 32"
    assert L.tgn_linear_act_max_workspace_bytes(1, 4, 513, 8) == 0
    torch.cuda.synchronize()
    assert (out == 12345.0).all()                               # nothing ran
    assert call(1, 4, 16, 8, need) == 0
    torch.cuda.synchronize()
    assert (out != 12345.0).all()


def test_runs_on_a_side_stream_and_in_a_captured_graph(dev):
    from toothgroupnetwork_amd import _lib
    x, Wt, shift = operands(dev, 2, 128, 1024, 500, seed=13)
    want = ok(x, Wt, shift, "relu")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        got = ok(x, Wt, shift, "relu")
    side.synchronize()
    assert torch.equal(got, want)
    # no allocation and no synchronisation inside: the two launches record into a graph and replay on new data
    L = _lib.lib()
    B, K, N = x.shape
    C = Wt.shape[1]
    need = L.tgn_linear_act_max_workspace_bytes(B, N, K, C)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    xs, out = x.clone(), torch.zeros(B, C, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = L.tgn_linear_act_max(B, N, K, C, _lib.ptr(xs), _lib.ptr(Wt), _lib.ptr(shift), 1, ctypes.c_float(0.0), _lib.ptr(out),
                                  _lib.ptr(ws), need, _lib.stream())
    assert rc == 0
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    xs.copy_(-x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ok((-x).contiguous(), Wt, shift, "relu"))
