"""Host: the library calls behind every neighbour-list operator, forward and backward, in both backward forms, as a ledger.  No GPU
and no built library: `_lib._ops` is a recorder, `_lib.lib` a stub, and `require_cuda`, `stream`, `torch.cuda.current_stream` and
`torch.cuda.is_current_stream_capturing` are harmless stand-ins in the modules that imported them, so the operators run on small
CPU tensors and every launch is written down instead of made.

Per call the recorder notes the symbol, every scalar (a float with its type), "stream" for the stream, None for a null pointer
and, per tensor, dtype, shape and whether it arrives all-zero, all-poison or with data.  For the duration of a case `torch.empty` and
`torch.empty_like` fill what they return with NaN (floats) or -1 (integers; 255 in uint8): an accumulator that an atomic kernel adds
into must arrive "zero", an output that a kernel fully writes may arrive "poison".  The recorder writes nothing itself, so what a
kernel would have produced stays poison downstream (a saved softmax, the k-NN lists of `interpolation`).  Beside the calls a case
notes dtype and shape of the operator's output and of every gradient that comes back.

The expected ledger is tests/golden/backward_call_ledger.json.  It was written by this module's own recorder,

    python tests/test_backward_call_ledger.py record

at the commit BEFORE the gradients of the gather family were gathered in ordered.py, when every `backward` carried both bodies, and
is committed unchanged: the test fails on any difference, with the switch off and on.  `Aggregation` is in it because it is unswitched
and must stay so.  The fused contrastive-boundary stage is asserted directly below: its lists are ordered.reverse_lists',
not the ledger's."""
import contextlib
import json
import os
import sys

import pytest
import torch

from conftest import GOLDEN

LEDGER = os.path.join(GOLDEN, "backward_call_ledger.json")
STREAM = object()


class _Stream:
    cuda_stream = 0


def _fill(t):
    if t.numel() == 0:
        return "empty"
    if t.is_floating_point():
        if bool(torch.isnan(t).all()):
            return "poison"
    elif bool((t == (255 if t.dtype == torch.uint8 else -1)).all()):
        return "poison"
    return "zero" if bool((t == 0).all()) else "data"


def _sig(t):
    return None if t is None else f"{str(t.dtype)[6:]}{list(t.shape)}"


def _note(a):
    if isinstance(a, torch.Tensor):
        return f"{_sig(a)}:{_fill(a)}"
    if a is STREAM:
        return "stream"
    if a is None or type(a) is int:
        return a
    return f"{type(a).__name__} {a!r}"


class Recorder:
    """Stands where the ctypes handle stands: any symbol is a function that notes its arguments as they are NOW and returns 0, or 64
    for a *_workspace_bytes."""

    def __init__(self):
        self.calls = []     # (symbol, the arguments themselves, their notes)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args, [_note(a) for a in args]))
            return 64 if name.endswith("_workspace_bytes") else 0
        return call

    def ledger(self):
        return [[name] + notes for name, _, notes in self.calls]

    def of(self, name):
        return [c for c in self.calls if c[0] == name]


def _poisoned(make):
    def made(*args, **kwargs):
        t = make(*args, **kwargs)
        if t.dtype != torch.bool and t.numel():
            t.fill_(float("nan") if t.is_floating_point() else (255 if t.dtype == torch.uint8 else -1))
        return t
    return made


@contextlib.contextmanager
def harness(ordered_backward):
    from toothgroupnetwork_amd import _lib, config, losses, ordered, point_transformer, pointnet2_utils, pointops
    rec = Recorder()
    with pytest.MonkeyPatch.context() as mp, config.override(ordered_backward=ordered_backward):
        mp.setattr(_lib, "_ops", rec)
        mp.setattr(_lib, "lib", lambda: rec)
        for mod in (_lib, losses, ordered, point_transformer, pointnet2_utils, pointops):
            for name, stand_in in (("require_cuda", lambda *tensors: None), ("stream", lambda: STREAM)):
                if name in vars(mod):
                    mp.setattr(mod, name, stand_in)
        mp.setattr(torch.cuda, "current_stream", lambda *a, **k: _Stream())
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
        mp.setattr(torch, "empty", _poisoned(torch.empty))
        mp.setattr(torch, "empty_like", _poisoned(torch.empty_like))
        pointops.knn_cache_clear()
        ordered.lists_cache_clear()
        try:
            yield rec
        finally:
            pointops.knn_cache_clear()
            ordered.lists_cache_clear()


# ---- the cases: each returns (output, the inputs a gradient is asked for) -------------------------------------------------------------
N, M, NS, C = 7, 5, 3, 4        # packed: n support rows, m queries, nsample, channels
B, DN, S, K, D = 2, 6, 3, 2, 5  # dense: B clouds of DN points, S centres of K neighbours, D feature channels


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _f(g, *shape, grad=True):
    return torch.randn(*shape, generator=g).requires_grad_(grad)


def _idx(g, high, *shape, dtype=torch.int32):
    return torch.randint(0, high, shape, generator=g).to(dtype)


def _P():
    from toothgroupnetwork_amd import pointops
    return pointops


def _U():
    from toothgroupnetwork_amd import pointnet2_utils
    return pointnet2_utils


def _grouping(idx_dtype):
    def case():
        g = _gen(1)
        x = _f(g, N, C)
        return _P().grouping(x, _idx(g, N, M, NS, dtype=idx_dtype)), [x]
    return case


def _query_group(use_xyz, xyz_grad, new_grad):
    def case():
        g = _gen(2)
        xyz, new_xyz, feat = _f(g, N, 3, grad=xyz_grad), _f(g, M, 3, grad=new_grad), _f(g, N, C)
        return _P()._QueryGroup.apply(xyz, new_xyz, feat, _idx(g, N, M, NS), use_xyz), [xyz, new_xyz, feat]
    return case


def _queryandgroup(own_idx, use_xyz):
    def case():
        g = _gen(3)
        xyz, feat = _f(g, N, 3), _f(g, N, C)
        o = torch.tensor([N], dtype=torch.int32)
        idx = None if own_idx else _idx(g, N, N, NS, dtype=torch.int64)
        return _P().queryandgroup(NS, xyz, None, feat, idx, o, o, use_xyz=use_xyz), [xyz, feat]
    return case


def _subtraction():
    g = _gen(4)
    a, b = _f(g, N, C), _f(g, N, C)
    return _P().subtraction(a, b, _idx(g, N, N, NS)), [a, b]


def _aggregation():
    g = _gen(5)
    x, p, w = _f(g, N, C), _f(g, N, NS, C), _f(g, N, NS, 2)
    return _P().aggregation(x, p, w, _idx(g, N, N, NS)), [x, p, w]


def _weighted_gather():
    g = _gen(6)
    feat = _f(g, N, C)
    return _P()._WeightedGather.apply(feat, _idx(g, N, M, NS), torch.rand(M, NS, generator=g)), [feat]


def _interpolation(which):
    def case():
        g = _gen(7)
        xyz, new_xyz, feat = _f(g, N, 3, grad=False), _f(g, M, 3, grad=False), _f(g, N, C)
        o, no = torch.tensor([N], dtype=torch.int32), torch.tensor([M], dtype=torch.int32)
        return getattr(_P(), which)(xyz, new_xyz, feat, o, no, 3), [feat]
    return case


def _dense_idx(g, high, *shape, dtype):
    idx = _idx(g, high, *shape, dtype=dtype)
    idx.view(-1)[1] = -2        # wraps to high - 2, as torch's advanced indexing does
    return idx


def _index_points(dtype, with_k):
    def case():
        g = _gen(8)
        pts = _f(g, B, DN, D)
        return _U().index_points(pts, _dense_idx(g, DN, *((B, S, K) if with_k else (B, S)), dtype=dtype)), [pts]
    return case


def _empty_batch(which):
    """B = 0: the dense operators take an empty batch, forward and backward, and return (0, N, C) gradients"""
    def case():
        g = _gen(13)
        idx = torch.zeros(0, S, K, dtype=torch.int64)
        if which == "index_points":
            pts = _f(g, 0, DN, D)
            return _U().index_points(pts, idx), [pts]
        if which == "group_points":
            xyz, new_xyz, pts = _f(g, 0, DN, 3), _f(g, 0, S, 3), _f(g, 0, DN, D)
            return _U().group_points(xyz, new_xyz, pts, idx), [xyz, new_xyz, pts]
        pts = _f(g, 0, S, D)
        return _U().three_interpolate(pts, torch.rand(0, DN, 3, generator=g), torch.zeros(0, DN, 3, dtype=torch.int64)), [pts]
    return case


def _group_points(dtype, xyz_first, with_points, xyz_grad=True, new_grad=True):
    def case():
        g = _gen(9)
        xyz, new_xyz = _f(g, B, DN, 3, grad=xyz_grad), _f(g, B, S, 3, grad=new_grad)
        pts = _f(g, B, DN, D) if with_points else None
        out = _U().group_points(xyz, new_xyz, pts, _dense_idx(g, DN, B, S, K, dtype=dtype), xyz_first=xyz_first)
        return out, [xyz, new_xyz] + ([pts] if with_points else [])
    return case


def _three_interpolate(batch, dtype):
    def case():
        g = _gen(10)
        pts = _f(g, batch, S, D)
        dist = torch.rand(batch, DN, 3, generator=g)
        return _U().three_interpolate(pts, dist, _idx(g, S, batch, DN, 3, dtype=dtype)), [pts]
    return case


def _softmax_aggregate():
    from toothgroupnetwork_amd import point_transformer
    g = _gen(11)
    x_v, p_r, logit = _f(g, N, C), _f(g, M, NS, C), _f(g, M, NS, 2)
    return point_transformer.pt_softmax_aggregate(x_v, p_r, logit, _idx(g, N, M, NS)), [x_v, p_r, logit]


CASES = {
    "grouping[int32]": _grouping(torch.int32),
    "grouping[int64]": _grouping(torch.int64),
    "_QueryGroup[use_xyz,xyz+new]": _query_group(True, True, True),
    "_QueryGroup[use_xyz,xyz]": _query_group(True, True, False),
    "_QueryGroup[use_xyz,new]": _query_group(True, False, True),
    "_QueryGroup[use_xyz,feat only]": _query_group(True, False, False),
    "_QueryGroup[no xyz]": _query_group(False, True, True),
    "queryandgroup[own idx]": _queryandgroup(True, True),
    "queryandgroup[idx given]": _queryandgroup(False, True),
    "queryandgroup[idx given,no xyz]": _queryandgroup(False, False),
    "subtraction": _subtraction,
    "aggregation": _aggregation,
    "_WeightedGather": _weighted_gather,
    "interpolation": _interpolation("interpolation"),
    "interpolation2": _interpolation("interpolation2"),
    "index_points[int64,(B,S)]": _index_points(torch.int64, False),
    "index_points[int32,(B,S,K)]": _index_points(torch.int32, True),
    "group_points[int64,xyz_first]": _group_points(torch.int64, True, True),
    "group_points[int32,points first]": _group_points(torch.int32, False, True),
    "group_points[int64,points=None]": _group_points(torch.int64, True, False),
    "group_points[int32,points=None,points first]": _group_points(torch.int32, False, False),
    "group_points[int64,points grad only]": _group_points(torch.int64, True, True, xyz_grad=False, new_grad=False),
    "group_points[int32,new_xyz grad only]": _group_points(torch.int32, False, False, xyz_grad=False, new_grad=True),
    "three_interpolate[B=2,int64]": _three_interpolate(2, torch.int64),
    "three_interpolate[B=1,int32]": _three_interpolate(1, torch.int32),
    "pt_softmax_aggregate": _softmax_aggregate,
    "index_points[B=0]": _empty_batch("index_points"),
    "group_points[B=0]": _empty_batch("group_points"),
    "three_interpolate[B=0]": _empty_batch("three_interpolate"),
}
MODES = {"atomic": False, "ordered": True}


def run_case(name, mode):
    with harness(MODES[mode]) as rec:
        out, inputs = CASES[name]()
        asked = [t for t in inputs if t.requires_grad]
        grad_out = torch.randn(out.shape, generator=_gen(99))
        grads = torch.autograd.grad(out, asked, grad_out, allow_unused=True)
        return {"calls": rec.ledger(), "output": _sig(out), "grads": [_sig(g) for g in grads]}


def record():
    ledger = {name: {mode: run_case(name, mode) for mode in MODES} for name in CASES}
    with open(LEDGER, "w") as fh:
        json.dump(ledger, fh, indent=1)
        fh.write("\n")
    print(f"wrote {LEDGER}: {len(ledger)} cases x {len(MODES)} modes, {sum(len(m['calls']) for c in ledger.values() for m in c.values())} calls")


@pytest.fixture(scope="module")
def expected():
    with open(LEDGER) as fh:
        return json.load(fh)


def test_the_ledger_names_exactly_these_cases(expected):
    assert sorted(expected) == sorted(CASES) and all(sorted(v) == sorted(MODES) for v in expected.values())


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_operator_makes_the_recorded_calls(expected, name, mode):
    got = json.loads(json.dumps(run_case(name, mode)))
    want = expected[name][mode]
    assert got["output"] == want["output"] and got["grads"] == want["grads"], (name, mode)
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"{name}, {mode}: call {i} differs\n  now      {g}\n  recorded {w}"
    assert len(got["calls"]) == len(want["calls"]), (name, mode, [c[0] for c in got["calls"]], [c[0] for c in want["calls"]])


def test_an_atomic_accumulator_arrives_zeroed_and_the_switch_changes_the_calls(expected):
    """A check of the FIXTURE alone (it reads the committed ledger and runs no operator): what makes the ledger worth comparing against.
    The poison is recognisable, the atomic kernels' accumulators are noted "zero" ("empty" for an empty batch), and every switched
    operator makes other calls with the switch on; Aggregation makes the same."""
    acc = {"tgn_grouping_backward": [6], "tgn_scatter_add_points": [8], "tgn_interpolation_backward": [7],
           "tgn_subtraction_backward": [6, 7], "tgn_aggregation_backward": [10, 11, 12]}
    seen = set()
    for name, modes in expected.items():
        for call in modes["atomic"]["calls"]:
            for pos in acc.get(call[0], ()):
                assert call[pos].endswith(":empty" if "B=0" in name else ":zero"), (name, call)
                seen.add(call[0])
            assert call[0] not in ("tgn_reverse_lists", "tgn_scatter_ordered"), (name, call)
        if name == "aggregation":
            assert modes["atomic"] == modes["ordered"]
        else:
            ordered_calls = [c[0] for c in modes["ordered"]["calls"]]
            assert "tgn_reverse_lists" in ordered_calls and not set(ordered_calls) & set(acc), (name, ordered_calls)
            out = [c[10] for c in modes["ordered"]["calls"] if c[0] == "tgn_scatter_ordered"]
            assert all(o.endswith(":empty" if "B=0" in name else ":poison") for o in out), (name, out)
    assert seen == set(acc)
    xv = [c for c in expected["pt_softmax_aggregate"]["atomic"]["calls"] if c[0] == "tgn_pt_softmax_aggregate_backward"]
    assert len(xv) == 1 and xv[0][10].endswith(":zero") and xv[0][11].endswith(":poison")


@pytest.mark.parametrize("mode", sorted(MODES))
def test_the_fused_contrastive_boundary_stage_builds_its_lists_with_the_kernel(mode):
    """forward: tgn_reverse_lists_workspace_bytes(1, m, m k1) and tgn_reverse_lists(1, m, m k1, idx int32, 0, ...) come before
    tgn_cbl_stage_forward, on the index tensor the stage reads; backward: tgn_cbl_stage_backward receives those two list tensors
    themselves.  Without a gradient to f no list is built.  The switch does not bear on it."""
    from toothgroupnetwork_amd import losses
    m, k1, c = 9, 4, 8
    g = _gen(12)
    idx, lab = _idx(g, m, m, k1, dtype=torch.int64), _idx(g, 3, m, dtype=torch.int64)
    with harness(MODES[mode]) as rec:
        f = _f(g, m, c)
        loss, count = losses.contrast_boundary_lists(f, idx, lab)
        names = [call[0] for call in rec.calls]
        assert [n for n in names if n != "tgn_cbl_stage_workspace_bytes"] == ["tgn_reverse_lists_workspace_bytes", "tgn_reverse_lists",
                                                                              "tgn_cbl_stage_forward"], names
        (_, size_args, _), (_, build_args, build_notes), (_, fwd_args, _) = (rec.of(n)[0] for n in ("tgn_reverse_lists_workspace_bytes",
                                                                                                    "tgn_reverse_lists", "tgn_cbl_stage_forward"))
        assert size_args == (1, m, m * k1)
        assert build_args[:3] == (1, m, m * k1) and build_args[4] == 0 and build_args[8] == 64 and build_args[9] is STREAM
        assert build_notes[3] == f"int32[{m}, {k1}]:data" and build_args[3] is fwd_args[4]
        assert build_notes[5] == f"int32[{m + 1}]:poison" and build_notes[6] == f"int32[{m * k1}]:poison" and build_notes[7] == "uint8[64]:poison"
        loss.backward()
        (_, bwd_args, bwd_notes), = rec.of("tgn_cbl_stage_backward")
        assert bwd_args[:3] == (m, k1, c) and bwd_args[4] is build_args[3]
        assert bwd_args[7] is build_args[5] and bwd_args[8] is build_args[6]
        assert bwd_notes[10] == f"float32[{m}, {c}]:poison" and bwd_args[11] is STREAM
        assert len(rec.of("tgn_reverse_lists")) == 1 and not rec.of("tgn_scatter_ordered")
    with harness(MODES[mode]) as rec:
        losses.contrast_boundary_lists(_f(g, m, c, grad=False), idx, lab)
        assert [call[0] for call in rec.calls if call[0] != "tgn_cbl_stage_workspace_bytes"] == ["tgn_cbl_stage_forward"]


if __name__ == "__main__":
    if sys.argv[1:] != ["record"]:
        raise SystemExit("usage: python tests/test_backward_call_ledger.py record")
    record()
