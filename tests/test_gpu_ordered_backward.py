"""GPU: the atomic-free backward of the gather family (csrc/scatter_ordered.hip, toothgroupnetwork_amd/ordered.py).

1. tgn_reverse_lists equals tests/ordered_ref.reverse_lists element for element (tests/test_ordered_host.py ties that reference to
   the torch statement, ordered_ref.reverse_lists_torch), and that torch statement itself on the device wherever it can state the case: square lists, and
   lists whose rows index a SHORTER cloud with valid indices (its first n + 1 starts are then the same).
2. tgn_scatter_ordered equals tests/ordered_ref.scatter bit for bit: every lane width, both forms, both signs, identity segments,
   a hub, empty rows into an output pre-filled with NaN.
3. Every switched operator under config.cfg.ordered_backward: bits of the reference, the same bytes twice, within the float64 bound
   of tests/test_gpu_training_backward.py (|got - exact| <= 8 u sum |terms|, u = 2^-24) and so within twice that of the atomic path;
   with the switch off the atomic kernels run as before, checked on inputs whose sums are exact in any order.

The graph composition is tests/test_gpu_ordered_backward_graph.py (a file that opens a stream sorts behind test_gpu_hotpath_configs.py).
"""
import numpy as np
import pytest
import torch

import ordered_ref as R
from operator_forms import gen_for, q16

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
TINY = 1e-30
# csrc/scatter_ordered.hip: threads of a pass over pairs or rows, rows per workgroup of the scan, segment lengths the wave sort takes,
# pairs the workgroup sort stages per round
REV_BLOCK, REV_SCAN_TILE, REV_WAVE_SEGMENT, REV_LONG_TILE = 256, 1024, 64, 1024


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.int32)


def _same_bits(got, want, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == np.float32 and want.dtype == np.float32, (what, got.shape, want.shape)
    ne = got.view(np.int32) != want.view(np.int32)
    assert not ne.any(), f"{what}: {int(ne.sum())} of {ne.size} elements differ in bits, the first at {np.argwhere(ne)[0].tolist()}: " \
                         f"got {got[ne][0]!r}, want {want[ne][0]!r}"


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the lists
# ---------------------------------------------------------------------------------------------------------------------------
def _list_case(name):
    g = gen_for("ordered_lists_" + name)
    ri = lambda hi, *shape: torch.randint(0, hi, shape, generator=g)
    if name == "one":
        return torch.zeros(1, 1, dtype=torch.int64), 1, 1
    if name == "square_65x16":
        return ri(65, 65, 16), 65, 1
    if name == "fine_300x3_onto_40":
        return ri(40, 300, 3), 40, 1
    if name == "all_equal_hub_4800":                # one segment of m * k = 4800 pairs: longer than a workgroup and than its LDS tile
        return torch.full((300, 16), 123, dtype=torch.int64), 300, 1
    if name == "half_untargeted":
        return ri(50, 100, 8) * 2, 100, 1
    if name == "out_of_range":
        return torch.randint(-5, 70, (64, 9), generator=g), 64, 1
    if name == "dense_b3_int64":
        return ri(50, 3, 37 * 8), 50, 3
    if name == "seams_one_past":                     # rows: one past a scan tile; pairs: one past a workgroup; b: one past one run
        return ri(REV_SCAN_TILE + 1, 2, REV_BLOCK + 1), REV_SCAN_TILE + 1, 2
    if name == "seams_one_short":
        return ri(REV_SCAN_TILE - 1, 1, REV_BLOCK - 1), REV_SCAN_TILE - 1, 1
    if name == "segment_seams":                      # segments of 63, 64, 65 pairs (wave sort / workgroup sort) and of 1024, 1025
        lens = [63, 64, 65, 0, REV_LONG_TILE, REV_LONG_TILE + 1, 1]
        idx = torch.cat([torch.full((n,), r, dtype=torch.int64) for r, n in enumerate(lens)])
        return idx[torch.randperm(idx.numel(), generator=g)].view(1, -1), len(lens), 1
    raise KeyError(name)


LIST_CASES = ["one", "square_65x16", "fine_300x3_onto_40", "all_equal_hub_4800", "half_untargeted", "out_of_range", "dense_b3_int64",
              "seams_one_past", "seams_one_short", "segment_seams"]


# both index widths where the width can matter (the count and the claim pass read the indices), one elsewhere
LIST_PARAMS = [(name, torch.int64 if name == "dense_b3_int64" else torch.int32) for name in LIST_CASES] + \
              [(name, torch.int64) for name in ("square_65x16", "out_of_range", "seams_one_past")]


@pytest.mark.parametrize("name,itype", LIST_PARAMS, ids=[f"{n}-{'i64' if t == torch.int64 else 'i32'}" for n, t in LIST_PARAMS])
def test_lists_equal_the_reference_and_losses_reverse_lists(dev, name, itype):
    from toothgroupnetwork_amd import ordered
    idx, n, batch = _list_case(name)
    want_start, want_pair = R.reverse_lists(idx.numpy(), n, batch)
    d_idx = idx.to(itype).to(dev)
    ordered.lists_cache_clear()
    rev_start, rev_pair = ordered.reverse_lists(d_idx, n, batch)
    assert rev_start.dtype == torch.int32 and rev_pair.dtype == torch.int32
    assert np.array_equal(rev_start.cpu().numpy(), want_start), name
    assert np.array_equal(rev_pair.cpu().numpy(), want_pair), name
    if batch == 1 and idx.dim() == 2 and idx.shape[0] >= n and (idx.shape[0] == n or bool(((idx >= 0) & (idx < n)).all())):
        l_start, l_pair = R.reverse_lists_torch(d_idx)
        assert torch.equal(l_start[:n + 1], rev_start) and torch.equal(l_pair, rev_pair), f"{name}: against the torch statement on the device"


def test_lists_are_memoised_per_tensor_version_and_not_across_writes(dev):
    from toothgroupnetwork_amd import ordered
    idx = torch.randint(0, 40, (90, 5), generator=gen_for("memo")).int().to(dev)
    ordered.lists_cache_clear()
    before = ordered.lists_cache_stats()
    a = ordered.reverse_lists(idx, 40)
    b = ordered.reverse_lists(idx, 40)
    assert a[0] is b[0] and a[1] is b[1]
    c = ordered.reverse_lists(idx.clone(), 40)             # another tensor: another entry
    assert c[0] is not a[0] and torch.equal(c[1], a[1])
    idx[0, 0] = (int(idx[0, 0]) + 1) % 40                   # an in-place write bumps the version
    d = ordered.reverse_lists(idx, 40)
    assert d[0] is not a[0] and np.array_equal(d[1].cpu().numpy(), R.reverse_lists(idx.cpu().numpy(), 40)[1])
    after = ordered.lists_cache_stats()
    assert after["builds"] - before["builds"] == 3 and after["hits"] - before["hits"] == 1


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the scatter
# ---------------------------------------------------------------------------------------------------------------------------
def _values(g, exact, *shape):
    return q16(g, *shape) if exact else torch.randn(*shape, generator=g)


def _scatter_case(dev, c, form, exact, g_=1, hub=False):
    """-> (got, want): ordered.scatter on the device against ordered_ref.scatter"""
    from toothgroupnetwork_amd import ordered
    g = gen_for(f"ordered_scatter{c}{form}{exact}{g_}{hub}")
    n, m, k = 40, 90, 5
    idx = torch.randint(0, n, (m, k), generator=g)
    if hub:
        idx[:, :4] = 11                                      # 360 of the 450 pairs target one row
    idx[idx == 17] = 18                                      # and nothing targets row 17
    lists = R.reverse_lists(idx.numpy(), n)
    d_lists = tuple(torch.from_numpy(x).to(dev) for x in lists)
    if form in ("pairs", "minus"):
        src, sign = _values(g, exact, m * k, c), (-1.0 if form == "minus" else 1.0)
        return ordered.scatter(src.to(dev), n, d_lists, sign=sign), R.scatter(n, lists, src.numpy(), sign=sign)
    if form == "query":
        src, coef = _values(g, exact, m, c), _values(g, exact, m * k, g_)
        return ordered.scatter(src.to(dev), n, d_lists, coef=coef.to(dev), k=k), R.scatter(n, lists, src.numpy(), coef=coef.numpy(), k=k)
    assert form == "identity"
    src = _values(g, exact, m * k, c)
    return ordered.scatter(src.to(dev), m, None, k=k, sign=-1.0), R.scatter(m, None, src.numpy(), k=k, sign=-1.0)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("c", [1, 3, 4, 35, 64, 130])
def test_scatter_equals_the_reference_bit_for_bit(dev, c, exact):
    for form, g_ in [("pairs", 1), ("minus", 1), ("query", 1), ("identity", 1)] + ([("query", 4)] if c % 4 == 0 else []):
        got, want = _scatter_case(dev, c, form, exact, g_)
        _same_bits(got, want, f"c = {c}, {form}, g = {g_}")
        assert not want[17].any() or form == "identity"


@pytest.mark.parametrize("form,c,g_", [("pairs", 35, 1), ("query", 64, 4), ("minus", 3, 1)])
def test_scatter_of_a_hub_equals_the_reference(dev, form, c, g_):
    got, want = _scatter_case(dev, c, form, False, g_, hub=True)
    _same_bits(got, want, f"hub, c = {c}, {form}")


def test_scatter_writes_every_element_and_empty_rows_are_plus_zero(dev):
    """the raw call into an output pre-filled with NaN: half the rows have no pairs"""
    from toothgroupnetwork_amd import _lib
    g = gen_for("ordered_empty")
    n, m, k, c = 64, 50, 3, 35
    idx = torch.randint(0, n // 2, (m, k), generator=g) * 2
    lists = R.reverse_lists(idx.numpy(), n)
    src = -torch.rand(m * k, c, generator=g)
    out = torch.full((n, c), float("nan"), device=dev)
    d = [torch.from_numpy(x).to(dev) for x in lists]
    _lib.ops().tgn_scatter_ordered(n, c, 1, 1, d[0], d[1], src.to(dev), None, 1.0, out, _lib.stream())
    _same_bits(out, R.scatter(n, lists, src.numpy()), "NaN pre-fill")
    assert not bool(torch.isnan(out).any()) and np.all(_bits(out[1::2]) == 0), "a row without pairs is +0.0f, bit pattern 0"


def test_scatter_rounds_every_term_and_adds_in_list_order(dev):
    """the two order- and contraction-sensitive sums of tests/test_ordered_host.py, on the device"""
    from toothgroupnetwork_amd import ordered
    big = 2.0 ** 24
    src = torch.tensor([[big], [1.0], [1.0]], device=dev)
    start = torch.tensor([0, 3], dtype=torch.int32, device=dev)
    first, last = torch.tensor([0, 1, 2], dtype=torch.int32, device=dev), torch.tensor([1, 2, 0], dtype=torch.int32, device=dev)
    assert float(ordered.scatter(src, 1, (start, first))) == big and float(ordered.scatter(src, 1, (start, last))) == big + 2.0
    x = 1.0 + 2.0 ** -12
    got = ordered.scatter(torch.tensor([[-1.0], [x]], device=dev), 1, (torch.tensor([0, 2], dtype=torch.int32, device=dev), first[:2].clone()),
                          coef=torch.tensor([[1.0], [x]], device=dev), k=1)
    assert float(got) == 2.0 ** -11, "the product is rounded to float32 before it is added: no fused multiply-add"


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the switched operators
# ---------------------------------------------------------------------------------------------------------------------------
class Op:
    """run() -> the gradients (device tensors); specs() -> per gradient the arguments of ordered_ref.scatter that state it (or None
    for a gradient this feature does not touch).  `exact`: values whose sums are exact in float32 in any order."""

    def __init__(self, run, specs, names):
        self.run, self.specs, self.names = run, specs, names


def _grads(out, inputs, go):
    return [g.detach() for g in torch.autograd.grad(out, inputs, go)]


def _op_grouping(dev, exact, c=35):
    from toothgroupnetwork_amd import pointops as P
    g = gen_for(f"op_grouping{exact}")
    n, m, k = 70, 65, 16
    idx = torch.randint(0, n, (m, k), generator=g).int()
    x, go = _values(g, exact, n, c).to(dev).requires_grad_(), _values(g, exact, m, k, c)
    d_idx, d_go = idx.to(dev), go.to(dev)
    return Op(lambda: _grads(P.grouping(x, d_idx), [x], d_go),
              lambda: [dict(n_rows=n, lists=R.reverse_lists(idx.numpy(), n), src=go.numpy().reshape(-1, c))], ["grad_input"])


def _op_queryandgroup(dev, exact, c=32):
    from toothgroupnetwork_amd import pointops as P
    g = gen_for(f"op_qg{exact}")
    n, m, k = 70, 65, 16
    idx = torch.randint(0, n, (m, k), generator=g).int()
    xyz, new_xyz, feat = (_values(g, exact, *s).to(dev).requires_grad_() for s in ((n, 3), (m, 3), (n, c)))
    go = _values(g, exact, m, k, 3 + c)
    d_idx, d_go = idx.to(dev), go.to(dev)
    o, no = torch.tensor([n], dtype=torch.int32, device=dev), torch.tensor([m], dtype=torch.int32, device=dev)
    lists = R.reverse_lists(idx.numpy(), n)
    rel, gf = np.ascontiguousarray(go.numpy()[:, :, :3]).reshape(-1, 3), np.ascontiguousarray(go.numpy()[:, :, 3:]).reshape(-1, c)
    return Op(lambda: _grads(P.queryandgroup(k, xyz, new_xyz, feat, d_idx, o, no, use_xyz=True), [xyz, new_xyz, feat], d_go),
              lambda: [dict(n_rows=n, lists=lists, src=rel), dict(n_rows=m, lists=None, src=rel, k=k, sign=-1.0), dict(n_rows=n, lists=lists, src=gf)],
              ["g_xyz", "g_new_xyz", "g_feat"])


def _op_subtraction(dev, exact, c=35):
    from toothgroupnetwork_amd import pointops as P
    g = gen_for(f"op_sub{exact}")
    n, k = 70, 16
    idx = torch.randint(0, n, (n, k), generator=g).int()
    a, b = (_values(g, exact, n, c).to(dev).requires_grad_() for _ in range(2))
    go = _values(g, exact, n, k, c)
    d_idx, d_go = idx.to(dev), go.to(dev)
    flat = go.numpy().reshape(-1, c)
    return Op(lambda: _grads(P.subtraction(a, b, d_idx), [a, b], d_go),
              lambda: [dict(n_rows=n, lists=None, src=flat, k=k), dict(n_rows=n, lists=R.reverse_lists(idx.numpy(), n), src=flat, sign=-1.0)],
              ["grad_input1", "grad_input2"])


def _op_weighted_gather(dev, exact, c=64, k=3):
    from toothgroupnetwork_amd import pointops as P
    g = gen_for(f"op_wg{exact}{k}")
    m, n = 40, 300                                           # 300 fine rows onto 40 coarse rows
    idx = torch.randint(0, m, (n, k), generator=g).int()
    w = q16(g, n, k) if exact else torch.rand(n, k, generator=g)
    feat, go = _values(g, exact, m, c).to(dev).requires_grad_(), _values(g, exact, n, c)
    d_idx, d_w, d_go = idx.to(dev), w.to(dev), go.to(dev)
    return Op(lambda: _grads(P._WeightedGather.apply(feat, d_idx, d_w), [feat], d_go),
              lambda: [dict(n_rows=m, lists=R.reverse_lists(idx.numpy(), m), src=go.numpy(), coef=w.numpy().reshape(-1, 1), k=k)], ["grad_feat"])


def _op_interpolation(dev, exact, k, c=64):
    """Interpolation.apply finds its own neighbours and weights; the same search states the reference (k = 1: every weight is 1)"""
    from toothgroupnetwork_amd import pointops as P
    g = gen_for(f"op_interp{exact}{k}")
    m, n = 40, 300
    xyz, new_xyz = torch.rand(m, 3, generator=g).to(dev), torch.rand(n, 3, generator=g).to(dev)
    o, no = torch.tensor([m], dtype=torch.int32, device=dev), torch.tensor([n], dtype=torch.int32, device=dev)
    feat, go = _values(g, exact, m, c).to(dev).requires_grad_(), _values(g, exact, n, c)
    d_go = go.to(dev)

    def specs():
        idx, dist2 = P._knn_raw(k, xyz, new_xyz, o, no)
        w = P._inverse_distance_weights(torch.sqrt(dist2)).contiguous()
        return [dict(n_rows=m, lists=R.reverse_lists(idx.cpu().numpy(), m), src=go.numpy(), coef=w.cpu().numpy().reshape(-1, 1), k=k)]
    return Op(lambda: _grads(P.interpolation2(xyz, new_xyz, feat, o, no, k), [feat], d_go), specs, ["grad_input"])


def _op_softmax_aggregate(dev, exact, c=32, g_=4):
    """g_xv is the ordered sum of the g_pr rows the kernel writes: the reference is stated over the device's own g_pr"""
    from toothgroupnetwork_amd import point_transformer as PT
    g = gen_for(f"op_sma{exact}")
    n, k = 70, 16
    idx = torch.randint(0, n, (n, k), generator=g).int()
    xv, pr, lg = (_values(g, exact, *s).to(dev).requires_grad_() for s in ((n, c), (n, k, c), (n, k, g_)))
    go = _values(g, exact, n, c)
    d_idx, d_go = idx.to(dev), go.to(dev)
    kept = {}

    def run():
        kept["g"] = _grads(PT.pt_softmax_aggregate(xv, pr, lg, d_idx), [xv, pr, lg], d_go)
        return kept["g"]
    return Op(run, lambda: [dict(n_rows=n, lists=R.reverse_lists(idx.numpy(), n), src=kept["g"][1].cpu().numpy().reshape(-1, c)), None, None],
              ["g_xv", "g_pr", "g_logit"])


def _op_index_points(dev, exact, c=35):
    from toothgroupnetwork_amd import pointnet2_utils as U
    g = gen_for(f"op_index{exact}")
    B, N, S, K = 3, 50, 37, 8
    idx = torch.randint(-N, N, (B, S, K), generator=g)      # negative indices wrap, as in torch's advanced indexing
    pts, go = _values(g, exact, B, N, c).to(dev).requires_grad_(), _values(g, exact, B, S, K, c)
    d_idx, d_go = idx.to(dev), go.to(dev)
    wrapped = torch.where(idx < 0, idx + N, idx).numpy()
    return Op(lambda: [x.view(B * N, c) for x in _grads(U.index_points(pts, d_idx), [pts], d_go)],
              lambda: [dict(n_rows=B * N, lists=R.reverse_lists(wrapped, N, B), src=go.numpy().reshape(-1, c))], ["grad_points"])


def _op_group_points(dev, exact, D=35):
    from toothgroupnetwork_amd import pointnet2_utils as U
    g = gen_for(f"op_group{exact}")
    B, N, S, K = 3, 50, 37, 8
    idx = torch.randint(0, N, (B, S, K), generator=g).int()
    xyz, pts = (_values(g, exact, B, N, w).to(dev).requires_grad_() for w in (3, D))
    new_xyz = _values(g, exact, B, S, 3).to(dev)
    go = _values(g, exact, B, S, K, 3 + D)
    d_idx, d_go = idx.to(dev), go.to(dev)
    lists = R.reverse_lists(idx.numpy(), N, B)
    rel, gf = np.ascontiguousarray(go.numpy()[..., :3]).reshape(-1, 3), np.ascontiguousarray(go.numpy()[..., 3:]).reshape(-1, D)
    return Op(lambda: [x.view(B * N, -1) for x in _grads(U.group_points(xyz, new_xyz, pts, d_idx), [xyz, pts], d_go)],
              lambda: [dict(n_rows=B * N, lists=lists, src=rel), dict(n_rows=B * N, lists=lists, src=gf)], ["g_xyz", "g_points"])


def _op_three_interpolate(dev, exact, C=64):
    """the weights are the forward kernel's own (saved for the backward): read from the graph node"""
    from toothgroupnetwork_amd import pointnet2_utils as U
    g = gen_for(f"op_three{exact}")
    B, N, S = 2, 150, 40
    xyz1, xyz2 = torch.rand(B, N, 3, generator=g).to(dev), torch.rand(B, S, 3, generator=g).to(dev)
    dist, idx = U.three_nn(xyz1, xyz2)
    pts2, go = _values(g, exact, B, S, C).to(dev).requires_grad_(), _values(g, exact, B, N, C)
    d_go = go.to(dev)
    kept = {}

    def run():
        out = U.three_interpolate(pts2, dist, idx)
        kept["w"] = [t for t in out.grad_fn.saved_tensors if t.dtype == torch.float32][0]
        return [x.view(B * S, C) for x in _grads(out, [pts2], d_go)]
    return Op(run, lambda: [dict(n_rows=B * S, lists=R.reverse_lists(idx.cpu().numpy(), S, B), src=go.numpy().reshape(-1, C),
                                 coef=kept["w"].cpu().numpy().reshape(-1, 1), k=3)], ["grad_points2"])


OPS = {"grouping": _op_grouping, "queryandgroup": _op_queryandgroup, "subtraction": _op_subtraction, "weighted_gather_k3": _op_weighted_gather,
       "interpolation_k1": lambda dev, exact: _op_interpolation(dev, exact, 1), "interpolation_k3": lambda dev, exact: _op_interpolation(dev, exact, 3),
       "softmax_aggregate": _op_softmax_aggregate, "index_points": _op_index_points, "group_points": _op_group_points,
       "three_interpolate": _op_three_interpolate}
# the cases whose every term is exact with values on the 1/16 grid (the others carry weights of a search or a softmax)
EXACT_OPS = ["grouping", "queryandgroup", "subtraction", "weighted_gather_k3", "interpolation_k1", "index_points", "group_points"]


@pytest.mark.parametrize("name", sorted(OPS))
def test_operator_under_the_switch_reference_bits_twice_and_the_float64_bound(dev, name):
    from toothgroupnetwork_amd import config, ordered
    op = OPS[name](dev, False)
    ordered.lists_cache_clear()
    with config.override(ordered_backward=False):
        atomic = op.run()
    builds = ordered.lists_cache_stats()["builds"]
    with config.override(ordered_backward=True):
        first = [t.clone() for t in op.run()]
        specs = op.specs()
        second = op.run()
    assert ordered.lists_cache_stats()["builds"] > builds, "the ordered path did not run"
    for got, again, old, spec, what in zip(first, second, atomic, specs, op.names):
        what = f"{name}.{what}"
        assert np.array_equal(_bits(got), _bits(again)), f"{what}: two calls, different bytes"
        if spec is None:        # not a scatter: the switch must not change it at all
            assert np.array_equal(_bits(got), _bits(old)), f"{what}: changed by the switch"
            continue
        _same_bits(got, R.scatter(**spec), what)
        exact, absum = R.scatter_f64(**spec)
        err = np.abs(got.cpu().numpy().astype(np.float64) - exact)
        print(f"{what}: ordered worst {float((err / (U32 * absum + TINY)).max()):.2f} u sum|terms|")
        assert (err <= 8 * U32 * absum + TINY).all(), f"{what}: over 8 u sum|terms| of the float64 result"
        gap = np.abs(got.cpu().numpy().astype(np.float64) - old.cpu().numpy().astype(np.float64))
        assert (gap <= 16 * U32 * absum + TINY).all(), f"{what}: further than twice the float64 bound from the atomic path"


@pytest.mark.parametrize("name", EXACT_OPS)
def test_switch_off_is_the_atomic_path_and_both_paths_agree_on_exact_sums(dev, name):
    """values on the 1/16 grid: every sum is exact in any order, so the atomic kernels (switch off: the code as it was, no list is
    built) and the ordered path both give the reference.  Values are compared, not bits: -(sum) of the torch path is -0.0 where the
    ordered sum is +0.0."""
    from toothgroupnetwork_amd import config, ordered
    op = OPS[name](dev, True)
    ordered.lists_cache_clear()
    builds = ordered.lists_cache_stats()["builds"]
    with config.override(ordered_backward=False):
        off = op.run()
    assert ordered.lists_cache_stats()["builds"] == builds, "switch off, and a list was built"
    with config.override(ordered_backward=True):
        on = op.run()
        specs = op.specs()
    for a, b, spec, what in zip(off, on, specs, op.names):
        want = R.scatter(**spec)
        assert np.array_equal(a.cpu().numpy(), want), f"{name}.{what}: the atomic path"
        _same_bits(b, want, f"{name}.{what}: the ordered path")


def test_softmax_aggregate_backward_without_its_scatter_keeps_the_other_outputs_bits(dev):
    """the raw call with grad_xv == NULL against the call with it, both kernel forms (merged: nsample <= 64 and g | 64; the fallback):
    grad_pr and grad_logit byte-equal, grad_xv untouched; and the scatter of the first call = the ordered sum of grad_pr on exact sums"""
    from toothgroupnetwork_amd import _lib, ordered
    O, st = _lib.ops(), _lib.stream()
    for n, ns, c, g_ in ((70, 16, 32, 4), (50, 8, 48, 6), (30, 65, 32, 4)):
        g = gen_for(f"sma_raw{c}{ns}")
        xv, pr = q16(g, n, c).to(dev), q16(g, n, ns, c).to(dev)
        sm, go = (q16(g, n, ns, g_).abs() / 4).to(dev), q16(g, n, c).to(dev)
        idx = torch.randint(0, n, (n, ns), generator=g).int().to(dev)
        with_xv = [torch.zeros(n, c, device=dev), torch.empty(n, ns, c, device=dev), torch.empty(n, ns, g_, device=dev)]
        O.tgn_pt_softmax_aggregate_backward(n, ns, c, g_, xv, pr, sm, idx, go, *with_xv, st)
        without = [torch.full((n, ns, c), float("nan"), device=dev), torch.full((n, ns, g_), float("nan"), device=dev)]
        O.tgn_pt_softmax_aggregate_backward(n, ns, c, g_, xv, pr, sm, idx, go, None, *without, st)
        assert np.array_equal(_bits(with_xv[1]), _bits(without[0])) and np.array_equal(_bits(with_xv[2]), _bits(without[1])), (n, ns, c, g_)
        summed = ordered.scatter(without[0].view(n * ns, c), n, ordered.reverse_lists(idx, n))
        assert torch.equal(summed, with_xv[0]), (n, ns, c, g_)
