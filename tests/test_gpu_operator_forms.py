"""GPU: every public operator called with tensors that are not fresh, packed, 16-byte-aligned float32 / expected-width indices.

tests/operator_forms.py holds the table (rows, shapes, values, forms, expected outcomes).  For every row: one baseline call, then
one call per form and argument with that one argument changed.  A call either returns outputs torch.equal to the baseline's with
the same dtypes and shapes, or raises TypeError / ValueError / AssertionError / RuntimeError naming the argument, after which a
fresh baseline call on the same stream is exact again.  Which of the two happened must be what the table says.  Different values
never pass.

Gradients of the differentiable rows: leaves in every form (layouts, float64, float16, bfloat16, stride-0 expansion where the row
allows it), non-contiguous and expanded grad_output; every gradient has its leaf's dtype and shape.  Rows whose accumulation is exact
on these values must reproduce the packed fp32 call's gradients, cast once to the leaf's dtype, bit for bit; rows with weighted
sums are held, form by form, to a float64 autograd restatement with the bound of tests/test_gpu_training_backward.py
(|got - exact| <= 8 u sum|terms|; a half-precision gradient must be the rounding of a value within it), never to another run of
the code under test.  An error that comes from the device, not from a wrapper, ends the session: nothing more is launched.
"""
import re

import numpy as np
import pytest
import torch

import operator_forms as T
from test_gpu_training_backward import TINY, U32, _sa_exact, _within
from test_gpu_bn_rows_bounds import C_BOUND, U_RND, _module as _bn_module, _ratio, backward64, forward64, run_and_check as _bn_run_and_check

pytestmark = pytest.mark.gpu

ROWS = {r["name"]: r for r in T.ROWS}
_BASE = {}


_DEVICE_ERROR = re.compile(r"HIP|hip[A-Z]|illegal memory access|failed \(status 2\)")      # (status 2: the library's launch error)


def _device_error(e):
    return type(e).__name__ == "AcceleratorError" or bool(_DEVICE_ERROR.search(str(e)))


def _stop(e):
    """a fault of the device is no outcome of a probe: nothing more is started on this GPU"""
    pytest.exit(f"GPU error, the session ends here: {type(e).__name__}: {e}", returncode=3)


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        _stop(e)


def _call(row, a):
    out = T._tensors(row["call"](a))
    _sync()
    return out


def _names(msg, names):
    return any(re.search(rf"(?<![A-Za-z0-9_]){re.escape(n)}(?![A-Za-z0-9_])", msg) for n in names)


def _baseline(row, dev):
    if row["name"] not in _BASE:
        _BASE[row["name"]] = _call(row, row["build"](dev))
    return _BASE[row["name"]]


def _same(got, want, follow=None):
    """None when got equals want (count, shapes, dtypes, bits), else what differs"""
    if len(got) != len(want):
        return f"{len(got)} outputs for {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        if tuple(g.shape) != tuple(w.shape):
            return f"output {i}: shape {tuple(g.shape)} for {tuple(w.shape)}"
        if follow is not None and w.is_floating_point():
            if g.dtype != follow:
                return f"output {i}: dtype {g.dtype}, the input's is {follow}"
            g, w = g.float(), w.float()
        if g.dtype != w.dtype:
            return f"output {i}: dtype {g.dtype} for {w.dtype}"
        if not torch.equal(g, w):
            bad = g != w
            return f"output {i}: {int(bad.sum())} of {g.numel()} entries differ"
    return None


def _probe(row, dev, arg, form, v, want_outputs):
    """-> (outcome, problem or None)"""
    a = row["build"](dev)
    a[arg] = v
    follow = v.dtype if row.get("dtype_follows_input") and v.is_floating_point() else None
    try:
        got = T._tensors(row["call"](a))
    except T.RAISES as e:
        if _device_error(e):
            _stop(e)
        names = {arg, row.get("arg_names", {}).get(arg, arg)}
        problem = None if _names(str(e), names) else f"raised {type(e).__name__} without naming {sorted(names)}: {e}"
        again = _same(_call(row, row["build"](dev)), _baseline(row, dev))
        if again is not None:
            problem = f"the baseline call after the raise is off: {again}"
        return "raises", problem
    _sync()
    return "equal", _same(got, want_outputs, follow)


@pytest.mark.parametrize("name", list(ROWS))
def test_forward_forms(dev, name):
    row = ROWS[name]
    base = _baseline(row, dev)
    assert base and all(torch.isfinite(t).all() for t in base if t.is_floating_point())
    assert _same(_call(row, row["build"](dev)), base) is None, "two baseline calls differ: the row is not deterministic"
    problems, record = [], []
    fresh = row["build"](dev)
    probes = [(arg, f, v) for arg in row["floats"] if fresh.get(arg) is not None for f, v in T.float_forms_of(row, arg, fresh[arg])]
    probes += [(arg, f, v) for arg in row["ints"] for f, v in T.index_forms_of(fresh[arg])]
    assert probes
    for arg, form, v in probes:
        want = base
        if form == "expanded":                     # other values than the baseline's: the packed copy of them is the baseline here
            a = row["build"](dev)
            a[arg] = v.contiguous()
            want = _call(row, a)
        outcome, problem = _probe(row, dev, arg, form, v, want)
        record.append(f"{arg}:{form}={outcome}")
        if outcome != T.expected(row, arg, form):
            problems.append(f"{arg}:{form}: {outcome}, the table says {T.expected(row, arg, form)}" + (f" ({problem})" if problem else ""))
        elif problem:
            problems.append(f"{arg}:{form}: {problem}")
    print(f"\nFORMS {name}: " + " ".join(record))
    assert not problems, f"{name}:\n  " + "\n  ".join(problems)


@pytest.mark.parametrize("name", [n for n, r in ROWS.items() if r.get("torch_ref") is not None])
def test_gather_baselines_equal_torch_indexing(dev, name):
    row = ROWS[name]
    a = row["build"](dev)
    want = row["torch_ref"]({k: (v.long() if k in row["ints"] else v) for k, v in a.items()})
    got, = _baseline(row, dev)
    assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------------
# gradients
# ---------------------------------------------------------------------------------------------------------------------------
def _go_for(out, name):
    return T.q16(T.gen_for("go " + name), *out.shape).to(out.device)


def _run_backward(row, a, go):
    """leaves for the row's differentiable arguments (in whatever form they are in `a`), forward, backward -> (out, grads)"""
    a = dict(a)
    for d in row["diff"]:
        a[d] = a[d].detach().requires_grad_(True)
    out, = T._tensors(row["call"](a))
    if go is None:
        out.sum().backward()
    else:
        out.backward(go)
    _sync()
    for d in row["diff"]:
        g = a[d].grad
        assert g is not None and g.dtype == a[d].dtype and g.shape == a[d].shape, (d, None if g is None else (g.dtype, g.shape))
    return out.detach(), {d: a[d].grad for d in row["diff"]}, a


def _held(got, exact, absterms, what):
    """_within for fp32 / float64 results.  A float16 / bfloat16 gradient is an fp32 gradient rounded once by autograd: it must be
    the rounding of SOME value within the same bound, i.e. lie between the roundings of the bound's two ends (rounding is monotone;
    torch rounds float64 -> fp32 -> half, which is the path an fp32 value at either end would take)."""
    if got.dtype not in (torch.float16, torch.bfloat16):
        return _within(got.float() if got.dtype == torch.float32 else got, exact, absterms, what)
    assert got.shape == exact.shape and torch.isfinite(got).all(), what
    lim = 8.0 * U32 * absterms + TINY
    lo, hi = (exact - lim).to(got.dtype), (exact + lim).to(got.dtype)
    bad = (got < lo) | (got > hi)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {got.numel()} {got.dtype} entries are no rounding of a value within 8 u sum|terms|"


def _restate64(name, a, idx_extra):
    """float64 restatement of a weighted-sum row on the leaves x (a dict of float64 tensors)"""
    if name.startswith("aggregation"):
        il = a["idx_n"].long()
        n, ns, c = a["position"].shape
        wc = a["weight"].shape[2]
        v = a["feat"][il] + a["position"]
        return (v * a["weight"].repeat(1, 1, c // wc)).sum(1)              # weight channel of output channel ch: ch % wc
    if name.startswith("interpolation"):
        idx, w = idx_extra
        return (a["feat"][idx.long()] * w.unsqueeze(-1)).sum(1)
    if name == "three_interpolate":
        r = 1.0 / (a["dist"] + 1e-8)
        w = (r / r.sum(-1, keepdim=True)).detach()
        bi = torch.arange(a["idx"].shape[0], device=w.device).view(-1, 1, 1)
        return (a["points2"][bi, a["idx"].long()] * w.unsqueeze(-1)).sum(2)
    raise KeyError(name)


def _check_bound(row, dev, a_used, out, grads, go, what):
    """out and every gradient of one call against float64 autograd of the restatement; sum|terms| is the same function and its
    gradients on the absolute values of inputs and grad_output (every term of these rows is a product of the inputs)."""
    name = row["name"]
    go64 = (torch.ones_like(out) if go is None else go).double()
    if name == "pt_softmax_aggregate":
        want = _sa_exact(a_used["x_v"].float(), a_used["p_r"].float(), a_used["logit"].float(), a_used["idx"], go64.float())
        _within(out, want["out"], want["out_abs"], f"{what} out")
        for d, k in (("x_v", "xv"), ("p_r", "pr"), ("logit", "lg")):
            _held(grads[d], want[f"d_{k}"], want[f"d{k}_abs"], f"{what} d_{d}")
        return
    extra = None
    if name.startswith("interpolation"):
        from toothgroupnetwork_amd import pointops as P
        base = row["build"](dev)                                    # neighbours and distances of the packed fp32 coordinates
        idx, dist = P.knnquery(3, base["xyz"], base["new_xyz"], base["offset"], base["new_offset"])
        r = 1.0 / (dist.double() + 1e-8)
        extra = (idx, r / r.sum(1, keepdim=True))

    def run(absolute):
        x = {}
        for k, v in a_used.items():
            if isinstance(v, torch.Tensor) and v.is_floating_point():
                v = v.detach().double()
                x[k] = (v.abs() if absolute else v).contiguous().requires_grad_(k in row["diff"])
            else:
                x[k] = v
        ex = (extra[0], extra[1].abs()) if extra is not None else None
        o = _restate64(name, x, ex)
        o.backward(go64.abs() if absolute else go64)
        return o.detach(), {d: x[d].grad for d in row["diff"]}
    exact, g_exact = run(False)
    terms, g_terms = run(True)
    _within(out, exact, terms, f"{what} out")
    for d in row["diff"]:
        _held(grads[d], g_exact[d], g_terms[d], f"{what} d_{d}")


@pytest.mark.parametrize("name", [n for n, r in ROWS.items() if r.get("diff")])
def test_gradient_forms(dev, name):
    row = ROWS[name]
    if name == "bn_rows":
        return _bn_rows_gradient_forms(dev, row)
    exact = row["grad"] == "exact"
    cases = [("baseline", None, None, "packed")] + [(f"{d}:{f}", d, f, "packed") for d in row["diff"] for f in T.GRAD_LEAF_FORMS
                                                    if f != "expanded" or d in row.get("expand", ())]
    cases += [("grad_output:strided_t", None, None, "strided_t"), ("grad_output:expanded", None, None, "expanded")]
    base, record = {}, []
    for what, arg, form, go_form in cases:
        a = row["build"](dev)
        if arg is not None:
            v = T.float_form(a[arg], form)
            if v is None:
                continue
            a[arg] = v
        out0 = _baseline(row, dev)[0]
        go = _go_for(out0, name)
        if go_form == "strided_t":
            go = T.float_form(go, "strided_t")
            assert go is not None and not go.is_contiguous()
        elif go_form == "expanded":
            go = None                                                    # out.sum().backward(): a stride-0 gradient of ones
        out, grads, used = _run_backward(row, a, go)
        if form == "expanded":                                           # other values: the packed copy of the expanded leaf is the baseline
            packed = dict(row["build"](dev), **{arg: a[arg].contiguous()})
            want_out, want_grads, _ = _run_backward(row, packed, go)
            assert torch.equal(out, want_out), f"{what}: the forward differs from the packed copy's"
            for d in row["diff"]:
                assert torch.equal(grads[d], want_grads[d]), f"{what}: d_{d} differs from the packed copy's"
            record.append(what)
            continue
        assert torch.equal(out, out0), f"{what}: the forward under autograd differs from the baseline"
        if exact:
            key = go_form == "expanded"
            if key not in base:                                          # the packed fp32 leaves with the same grad_output values
                go_b = torch.ones_like(out0) if key else _go_for(out0, name)
                base[key] = _run_backward(row, row["build"](dev), go_b)[1]
            for d in row["diff"]:                                        # (exact fp32 sums; autograd casts once to the leaf's dtype)
                assert torch.equal(grads[d], base[key][d].to(grads[d].dtype)), f"{what}: d_{d} differs from the packed fp32 call's"
        else:
            _check_bound(row, dev, used, out, grads, go, f"{name} {what}")
        record.append(what)
    print(f"\nGRADS {name} ({row['grad']}): " + " ".join(record))
    assert len(record) >= 4


def _bn_rows_half_leaf(dev, x, dy, xh):
    """a float16 / bfloat16 leaf: y (fp32) within the bound of tests/test_gpu_bn_rows_bounds.py, dx in the leaf's dtype and the
    rounding of a value within that bound"""
    from toothgroupnetwork_amd import point_transformer as PT
    bn = _bn_module(dev, x.shape[1], 3)
    rows = x.shape[0]
    xg = xh.detach().requires_grad_(True)
    y = PT.bn_rows(bn, xg, relu=True)
    assert type(y.grad_fn).__name__ == "_BNRowsBackward" and y.dtype == torch.float32
    y.backward(dy)
    _sync()
    assert xg.grad.dtype == xh.dtype and xg.grad.shape == xh.shape
    gamma, beta = bn.weight.detach().cpu().double(), bn.bias.detach().cpu().double()
    f = forward64(x.cpu().double(), gamma, beta, float(np.float32(bn.eps)), True)
    assert _ratio(y, f["y"], f["M_y"], C_BOUND) <= 1.0
    dx, M = backward64(f, dy.cpu().double() * (y.detach().cpu() > 0), gamma, rows)["dx"]
    lim = C_BOUND * U_RND * M + 1e-30
    got = xg.grad.cpu()
    bad = (got < (dx - lim).to(got.dtype)) | (got > (dx + lim).to(got.dtype))
    assert torch.isfinite(got).all() and not bool(bad.any()), f"bn_rows {xh.dtype} leaf: {int(bad.sum())} entries of dx outside the bound"


def _bn_rows_gradient_forms(dev, row):
    """bn_rows: x and dy in every form through the float64 restatement of tests/test_gpu_bn_rows_bounds.py (fresh module each)"""
    x = row["build"](dev)["x"]
    dy = _go_for(x, "bn_rows")
    seen = []
    for form in ("f16", "bf16"):
        _bn_rows_half_leaf(dev, x, dy, T.float_form(x, form))
        seen.append(f"x:{form}")
    for form in (None, "offset", "strided_t", "strided_col", "f64"):
        xv = x if form is None else T.float_form(x, form)
        _bn_run_and_check(dev, _bn_module(dev, x.shape[1], 3), xv, dy, True, f"bn_rows x:{form}")
        seen.append(f"x:{form}")
    for form in ("strided_t", "strided_col"):
        _bn_run_and_check(dev, _bn_module(dev, x.shape[1], 3), x, T.float_form(dy, form), True, f"bn_rows dy:{form}")
        seen.append(f"grad_output:{form}")
    print("\nGRADS bn_rows (bound): " + " ".join(seen))


def test_edgeconv_out_on_the_wrong_device_raises(dev):
    row = ROWS["edgeconv_max[C64,two_layers,out=slice]"]
    a = row["build"](dev)
    a["out"] = a["out"].cpu()
    with pytest.raises(TypeError, match="out"):
        row["call"](a)
    assert _same(_call(row, row["build"](dev)), _baseline(row, dev)) is None


def test_argument_errors_of_the_set_abstraction_and_interpolation_entries(dev):
    """the checks these entries make on out=, Wt and add: an error naming the argument, and the next baseline call is exact"""
    from toothgroupnetwork_amd import pointnet2_utils as U
    row = ROWS["sa_level_mlp2_max[D5,out=view]"]
    a = row["build"](dev)
    convs, bns = T._sa_modules(dev, "sa2", 8, [32, 48])
    args = (a["xyz"], a["new_xyz"], a["points"], a["idx"], convs, bns, True)
    wide = torch.zeros(T.DB, T.DS, 96, device=dev)
    with torch.no_grad():
        with pytest.raises(TypeError, match=r"\bout\b"):
            U.sa_level_mlp2_max(*args, out=wide.double()[:, :, :48])
        with pytest.raises(TypeError, match=r"\bout\b"):
            U.sa_level_mlp2_max(*args, out=torch.zeros(T.DB, T.DS, 48))
        with pytest.raises(ValueError, match=r"\bout\b"):
            U.sa_level_mlp2_max(*args, out=wide[:, :, :47])
        with pytest.raises(ValueError, match=r"\bout\b"):
            U.sa_level_mlp2_max(*args, out=wide[:, :, ::2])
    assert _same(_call(row, row["build"](dev)), _baseline(row, dev)) is None
    row = ROWS["sa_point_transform[D5]"]
    a = row["build"](dev)
    with pytest.raises(ValueError, match=r"\bWt\b"):
        U.sa_point_transform(a["xyz"], a["points"], a["Wt"][:-1])
    assert _same(_call(row, row["build"](dev)), _baseline(row, dev)) is None
    row = ROWS["three_interpolate_add_relu"]
    a = row["build"](dev)
    with pytest.raises(ValueError, match=r"\badd\b"):
        U.three_interpolate_add_relu(a["points2"], a["dist"], a["idx"], add=a["add"][:, :-1], relu=True)
    assert _same(_call(row, row["build"](dev)), _baseline(row, dev)) is None
