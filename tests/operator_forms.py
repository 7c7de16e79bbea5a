"""The table of operators behind tests/test_gpu_operator_forms.py and tests/test_operator_forms_host.py: one row per public
operator that hands a tensor's raw pointer to a kernel, and the tensor FORMS every row is called with.

A row holds a builder of baseline arguments (fresh tensors on every call: some operators write into an argument), the names of
its float and index tensor arguments, how to call it, whether it is differentiable and in which arguments, and -- per form -- the
expected outcome: "equal" (outputs torch.equal to the baseline's, same dtypes and shapes) or "raises" (TypeError, ValueError,
AssertionError or RuntimeError naming the argument, nothing launched, the next baseline call exact).  Everything is "equal" unless
the row's `expect` says otherwise, so a change from one outcome to the other is a visible diff of this file.

Values.  Every float input is randint(-64, 65) / 16 from a seeded generator: exact in float16, bfloat16, float32 and float64, so
every dtype copy holds the same numbers and unweighted gather / scatter sums are exact in any order.

Forms of a float argument: "offset" (contiguous view one element into a larger buffer, data_ptr() % 16 == 4), "strided_t"
(transposed storage), "strided_col" (column slice of a buffer twice as wide), "expanded" (stride 0, rows that allow it: the
baseline is then the packed copy of the same expanded values), and the dtype copies "f64", "f32", "f16", "bf16" other than the
baseline's.  Forms of an index argument: the other width ("i32" / "i64") and "strided" (every second element of a buffer twice as
long, or a column slice).  A probe narrower than the baseline's dtype (float16 / bfloat16 for float32, any of them and float32 for
a float64 baseline, int32 for int64) is the leading slice of a zero-filled buffer of twice the bytes a kernel would touch if a
wrapper forgot to cast it.

Gradients (rows with `diff`): a leaf that requires grad in every form -- "offset", "strided_t", "strided_col", "f64", "f16",
"bf16", and "expanded" where the row allows it -- and the grad_output forms "strided_t" and "expanded" (out.sum().backward()).
Every gradient comes back in the leaf's dtype and shape.  grad == "exact": equal to the packed fp32 call's gradient, cast once
to the leaf's dtype (an expanded leaf: to that of its packed copy); grad == "bound": held to the float64 restatement and bound of
tests/test_gpu_training_backward.py (tests/test_gpu_bn_rows_bounds.py for bn_rows), for a float16 / bfloat16 leaf as the
rounding to that dtype of some value within the bound -- no tolerance of its own.

Not covered.  Offsets tensors whose VALUES are wrong (not cumulative, last != n): validating them costs a host synchronisation
that knnquery deliberately avoids.  Tensors on different devices: the test machines have one GPU.

INTERNAL lists the functions and classes that pass raw pointers to the library without a row of their own, with the row that covers them;
tests/test_operator_forms_host.py fails for a wrapper that is neither a row nor listed there.
"""
import torch

FLOAT_DTYPES = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
FLOAT_LAYOUTS = ("offset", "strided_t", "strided_col")
INDEX_DTYPES = {"i32": torch.int32, "i64": torch.int64}
GRAD_LEAF_FORMS = ("offset", "strided_t", "strided_col", "f64", "f16", "bf16", "expanded")
RAISES = (TypeError, ValueError, AssertionError, RuntimeError)


# ---------------------------------------------------------------------------------------------------------------------------
# values and forms
# ---------------------------------------------------------------------------------------------------------------------------
def q16(gen, *shape):
    """randint(-64, 65) / 16 on the CPU generator `gen`"""
    return torch.randint(-64, 65, shape, generator=gen).float() / 16


def gen_for(name):
    return torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003)


def _slice_of_buffer(t, dtype, lead, factor):
    """the values of t as `dtype`, a contiguous view `lead` elements into a zero-filled buffer of factor * numel + lead elements"""
    n = t.numel()
    buf = torch.zeros(factor * n + lead, dtype=dtype, device=t.device)
    v = buf[lead:lead + n].view(t.shape)
    v.copy_(t)
    return v


def float_form(t, form):
    """t in `form`, or None where the shape does not allow that form (the view would be contiguous)"""
    if form == "offset":
        v = _slice_of_buffer(t, t.dtype, 1, 1)
        assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size(), form      # fp32: data_ptr() % 16 == 4
        return v
    if form == "strided_t":
        if t.dim() < 2:
            return None
        v = t.transpose(-1, -2).contiguous().transpose(-1, -2)
    elif form == "strided_col":
        buf = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
        v = buf[..., :t.shape[-1]]
        v.copy_(t)
    elif form == "expanded":
        v = t[:1].expand_as(t)
    elif form in FLOAT_DTYPES:
        dt = FLOAT_DTYPES[form]
        if dt == t.dtype:
            return None
        # narrower than the baseline: a leading slice of a buffer at least twice the bytes a read in the baseline's dtype takes
        v = _slice_of_buffer(t, dt, 0, 2 * t.element_size() // dt.itemsize) if dt.itemsize < t.element_size() else t.to(dt)
        assert torch.equal(v.to(t.dtype), t), "the values are not exact in " + form
        return v
    else:
        raise KeyError(form)
    return None if v.is_contiguous() else v


def index_form(t, form):
    if form in INDEX_DTYPES:
        dt = INDEX_DTYPES[form]
        if dt == t.dtype:
            return None
        return _slice_of_buffer(t, dt, 0, 2 * t.element_size() // dt.itemsize) if dt.itemsize < t.element_size() else t.to(dt)
    if form == "strided":
        if t.dim() >= 2 and t.shape[-1] > 1:
            buf = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
            v = buf[..., :t.shape[-1]]
        else:
            buf = torch.zeros((2 * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
            v = buf[::2]
        v.copy_(t)
        return None if v.is_contiguous() else v
    raise KeyError(form)


def float_forms_of(row, arg, t):
    """the (form, tensor) probes of float argument `arg`"""
    forms = list(FLOAT_LAYOUTS) + list(FLOAT_DTYPES) + (["expanded"] if arg in row.get("expand", ()) else [])
    return [(f, v) for f in forms for v in [float_form(t, f)] if v is not None]


def index_forms_of(t):
    return [(f, v) for f in list(INDEX_DTYPES) + ["strided"] for v in [index_form(t, f)] if v is not None]


def expected(row, arg, form):
    e = row.get("expect", {})
    return e.get(f"{arg}:{form}", e.get(form, "equal"))


# ---------------------------------------------------------------------------------------------------------------------------
# shapes (the smallest that reach the vector path and the scalar tail of the kernels)
# ---------------------------------------------------------------------------------------------------------------------------
PN, PM = 257, 61                       # packed: n points in two segments, m queries
P_OFF, P_NOFF = (130, 257), (30, 61)
DB, DN, DS, DK = 2, 200, 37, 8         # dense: B, N, S, K
EN, EK = 300, 20                       # EdgeConv: N, K
CN, CK = 600, 64                       # crops and tsegnet: N, k


def _packed(dev, name, ns=8, c=20):
    g = gen_for(name)
    a = dict(xyz=q16(g, PN, 3).to(dev), new_xyz=q16(g, PM, 3).to(dev), feat=q16(g, PN, c).to(dev),
             offset=torch.tensor(P_OFF, dtype=torch.int32, device=dev), new_offset=torch.tensor(P_NOFF, dtype=torch.int32, device=dev),
             idx=torch.randint(0, PN, (PM, ns), generator=g, dtype=torch.int32).to(dev),
             idx_n=torch.randint(0, PN, (PN, ns), generator=g, dtype=torch.int32).to(dev))
    return a, g


def _dense(dev, name, D=5):
    g = gen_for(name)
    xyz = q16(g, DB, DN, 3)
    a = dict(xyz=xyz.to(dev), new_xyz=xyz[:, :DS].clone().to(dev), points=q16(g, DB, DN, D).to(dev) if D else None,
             idx=torch.randint(0, DN, (DB, DS, DK), generator=g).to(dev))
    return a, g


def _sa_modules(dev, name, c_in, widths):
    torch.manual_seed(len(name))
    convs, bns, last = [], [], c_in
    for w in widths:
        convs.append(torch.nn.Conv2d(last, w, 1).to(dev))
        bn = torch.nn.BatchNorm2d(w).to(dev).eval()
        with torch.no_grad():
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
        bns.append(bn)
        last = w
    return convs, bns


_MODULES = {}


def _memo(key, make):
    """modules (fixed parameters, not probed arguments) are built once per row and device: the fold memos key on them"""
    if key not in _MODULES:
        _MODULES[key] = make()
    return _MODULES[key]


def _tensors(x):
    """an operator's result as a flat tuple of tensors"""
    if isinstance(x, torch.Tensor):
        return (x,)
    if x is None:
        return ()
    if isinstance(x, (int, float)):
        return (torch.tensor(x),)
    out = ()
    for y in x:
        out += _tensors(y)
    return out


ROWS = []


def row(name, module, covers, build, call, floats, ints, **kw):
    ROWS.append(dict(name=name, module=module, covers=covers, build=build, call=call, floats=floats, ints=ints, **kw))


# ---------------------------------------------------------------------------------------------------------------------------
# pointops (packed layout)
# ---------------------------------------------------------------------------------------------------------------------------
def _P():
    from toothgroupnetwork_amd import pointops
    return pointops


row("furthestsampling", "pointops", ["furthestsampling", "FurthestSampling", "fps_with_coords"],
    lambda dev: _packed(dev, "fps")[0],
    lambda a: _P().furthestsampling(a["xyz"], a["offset"], a["new_offset"]),
    floats=["xyz"], ints=["offset", "new_offset"], outputs=["idx"])

row("knnquery", "pointops", ["knnquery", "KNNQuery", "_knn_raw"],
    lambda dev: _packed(dev, "knn")[0],
    lambda a: _P().knnquery(8, a["xyz"], a["new_xyz"], a["offset"], a["new_offset"]),
    floats=["xyz", "new_xyz"], ints=["offset", "new_offset"], outputs=["idx", "dist"], expand=["new_xyz"])

for _c in (20, 32):
    row(f"grouping[c{_c}]", "pointops", ["grouping", "Grouping"],
        lambda dev, c=_c: _packed(dev, "grouping", 16, c)[0],
        lambda a: _P().grouping(a["feat"], a["idx"]),
        floats=["feat"], ints=["idx"], outputs=["out"], diff=["feat"], grad="exact", arg_names={"feat": "input"},
        torch_ref=lambda a: a["feat"][a["idx"].long()])

for _own in (False, True):
    for _use in (True, False):
        row(f"queryandgroup[{'knn' if _own else 'idx'},{'xyz' if _use else 'feat_only'}]", "pointops", ["queryandgroup", "_QueryGroup"],
            lambda dev: _packed(dev, "queryandgroup", 8, 20)[0],
            lambda a, own=_own, use=_use: _P().queryandgroup(8, a["xyz"], a["new_xyz"], a["feat"], None if own else a["idx"],
                                                             a["offset"], a["new_offset"], use_xyz=use),
            floats=["xyz", "new_xyz", "feat"], ints=(["offset", "new_offset"] if _own else ["idx"]), outputs=["out"],
            diff=(["xyz", "new_xyz", "feat"] if _use else ["feat"]), grad="exact", expand=["new_xyz"],
            torch_ref=None if _own else (lambda a, use=_use: torch.cat(
                ([a["xyz"][a["idx"].long()] - a["new_xyz"].unsqueeze(1)] if use else []) + [a["feat"][a["idx"].long()]], -1)))


def _sub_build(dev):
    a, g = _packed(dev, "subtraction", 16, 32)
    a["input2"] = q16(g, PN, 32).to(dev)
    return a


row("subtraction", "pointops", ["subtraction", "Subtraction"], _sub_build,
    lambda a: _P().subtraction(a["feat"], a["input2"], a["idx_n"]),
    floats=["feat", "input2"], ints=["idx_n"], outputs=["out"], diff=["feat", "input2"], grad="exact",
    arg_names={"feat": "input1", "idx_n": "idx"},
    torch_ref=lambda a: a["feat"].unsqueeze(1) - a["input2"][a["idx_n"].long()])


def _agg_build(dev, c):
    a, g = _packed(dev, "aggregation", 8, c)
    a["position"], a["weight"] = q16(g, PN, 8, c).to(dev), q16(g, PN, 8, 4).to(dev)
    return a


for _c in (20, 32):
    row(f"aggregation[c{_c}]", "pointops", ["aggregation", "Aggregation"], lambda dev, c=_c: _agg_build(dev, c),
        lambda a: _P().aggregation(a["feat"], a["position"], a["weight"], a["idx_n"]),
        floats=["feat", "position", "weight"], ints=["idx_n"], outputs=["out"], diff=["feat", "position", "weight"], grad="bound",
        arg_names={"feat": "input", "idx_n": "idx"})


def _interp_build(dev, name):
    """the coarse cloud (m points) carries the features, the fine one (n points) receives them"""
    g = gen_for(name)
    return dict(xyz=q16(g, PM, 3).to(dev), new_xyz=q16(g, PN, 3).to(dev), feat=q16(g, PM, 20).to(dev),
                offset=torch.tensor(P_NOFF, dtype=torch.int32, device=dev), new_offset=torch.tensor(P_OFF, dtype=torch.int32, device=dev))


row("interpolation", "pointops", ["interpolation", "_WeightedGather"], lambda dev: _interp_build(dev, "interpolation"),
    lambda a: _P().interpolation(a["xyz"], a["new_xyz"], a["feat"], a["offset"], a["new_offset"]),
    floats=["xyz", "new_xyz", "feat"], ints=["offset", "new_offset"], outputs=["out"], diff=["feat"], grad="bound")

row("interpolation2", "pointops", ["interpolation2", "Interpolation"], lambda dev: _interp_build(dev, "interpolation2"),
    lambda a: _P().interpolation2(a["xyz"], a["new_xyz"], a["feat"], a["offset"], a["new_offset"], 3),
    floats=["xyz", "new_xyz", "feat"], ints=["offset", "new_offset"], outputs=["out"], diff=["feat"], grad="bound",
    arg_names={"feat": "input"})


# ---------------------------------------------------------------------------------------------------------------------------
# pointnet2_utils (dense layout)
# ---------------------------------------------------------------------------------------------------------------------------
def _U():
    from toothgroupnetwork_amd import pointnet2_utils
    return pointnet2_utils


row("square_distance", "pointnet2_utils", ["square_distance", "_SquareDistance3"],
    lambda dev: {k: v for k, v in _dense(dev, "sqd")[0].items() if k in ("xyz", "new_xyz")},
    lambda a: _U().square_distance(a["xyz"], a["new_xyz"]),
    floats=["xyz", "new_xyz"], ints=[], outputs=["dist"], diff=["xyz", "new_xyz"], grad="exact", expand=["new_xyz"],
    arg_names={"xyz": "src", "new_xyz": "dst"})

for _nd in (2, 3):
    row(f"index_points[idx{_nd}d]", "pointnet2_utils", ["index_points", "_IndexPoints"],
        lambda dev, nd=_nd: (lambda a: dict(points=a["points"], idx=a["idx"] if nd == 3 else a["idx"][:, :, 0].contiguous()))(_dense(dev, "index_points", 5)[0]),
        lambda a: _U().index_points(a["points"], a["idx"]),
        floats=["points"], ints=["idx"], outputs=["out"], diff=["points"], grad="exact",
        torch_ref=lambda a: a["points"][torch.arange(DB, device=a["idx"].device).view(DB, *([1] * (a["idx"].dim() - 1))), a["idx"]])

row("farthest_point_sample", "pointnet2_utils", ["farthest_point_sample", "_fps_dense"],
    lambda dev: dict(xyz=_dense(dev, "fps_dense")[0]["xyz"]),
    lambda a: _U().farthest_point_sample(a["xyz"], DS), floats=["xyz"], ints=[], outputs=["idx"])

row("query_ball_point", "pointnet2_utils", ["query_ball_point"],
    lambda dev: {k: v for k, v in _dense(dev, "ball")[0].items() if k in ("xyz", "new_xyz")},
    lambda a: _U().query_ball_point(2.0, DK, a["xyz"], a["new_xyz"]), floats=["xyz", "new_xyz"], ints=[], outputs=["idx"])


def _group_ref(a, xyz_first):
    bi = torch.arange(DB, device=a["idx"].device).view(DB, 1, 1)
    rel = a["xyz"][bi, a["idx"]] - a["new_xyz"].unsqueeze(2)
    if a.get("points") is None:
        return rel
    return torch.cat([rel, a["points"][bi, a["idx"]]] if xyz_first else [a["points"][bi, a["idx"]], rel], -1)


for _D, _first in ((5, True), (5, False), (64, True), (0, True)):
    row(f"group_points[D{_D},{'xyz_first' if _first else 'points_first'}]", "pointnet2_utils", ["group_points", "_GroupPoints"],
        lambda dev, D=_D: _dense(dev, "group_points", D)[0],
        lambda a, first=_first: _U().group_points(a["xyz"], a["new_xyz"], a["points"], a["idx"], xyz_first=first),
        floats=["xyz", "new_xyz"] + (["points"] if _D else []), ints=["idx"], outputs=["out"],
        diff=["xyz", "new_xyz"] + (["points"] if _D else []), grad="exact", expand=["new_xyz"],
        torch_ref=lambda a, first=_first: _group_ref(a, first))

row("sample_and_group", "pointnet2_utils", ["sample_and_group"],
    lambda dev: {k: v for k, v in _dense(dev, "sample_and_group", 5)[0].items() if k in ("xyz", "points")},
    lambda a: _U().sample_and_group(DS, 2.0, DK, a["xyz"], a["points"], returnfps=True),
    floats=["xyz", "points"], ints=[], outputs=["new_xyz", "new_points", "grouped_xyz", "fps_idx"])

row("three_nn", "pointnet2_utils", ["three_nn"],
    lambda dev: {k: v for k, v in _dense(dev, "three_nn")[0].items() if k in ("xyz", "new_xyz")},
    lambda a: _U().three_nn(a["xyz"], a["new_xyz"]), floats=["xyz", "new_xyz"], ints=[], outputs=["dist", "idx"],
    arg_names={"xyz": "xyz1", "new_xyz": "xyz2"})


def _three_build(dev, name, add=False):
    g = gen_for(name)
    a = dict(points2=q16(g, DB, DS, 20).to(dev), dist=q16(g, DB, DN, 3).abs().to(dev), idx=torch.randint(0, DS, (DB, DN, 3), generator=g).to(dev))
    if add:
        a["add"] = q16(g, DB, DN, 20).to(dev)
    return a


row("three_interpolate", "pointnet2_utils", ["three_interpolate", "_ThreeInterpolate"], lambda dev: _three_build(dev, "three_interpolate"),
    lambda a: _U().three_interpolate(a["points2"], a["dist"], a["idx"]),
    floats=["points2", "dist"], ints=["idx"], outputs=["out"], diff=["points2"], grad="bound")

row("three_interpolate_add_relu", "pointnet2_utils", ["three_interpolate_add_relu"], lambda dev: _three_build(dev, "three_add", add=True),
    lambda a: _U().three_interpolate_add_relu(a["points2"], a["dist"], a["idx"], add=a["add"], relu=True),
    floats=["points2", "dist", "add"], ints=["idx"], outputs=["out"])


def _sa_build(dev, name, D):
    a, g = _dense(dev, name, D)
    ball = _U().query_ball_point(2.0, DK, a["xyz"], a["new_xyz"])
    a["idx"] = ball
    return a, g


def _wt_build(dev, D):
    a, g = _dense(dev, "sa_point_transform", D)
    return dict(xyz=a["xyz"], points=a["points"], Wt=q16(g, D + 3, 32).to(dev))


for _D in (5, 64):
    row(f"sa_point_transform[D{_D}]", "sa_fused", ["sa_point_transform"], lambda dev, D=_D: _wt_build(dev, D),
        lambda a: _U().sa_point_transform(a["xyz"], a["points"], a["Wt"]), floats=["xyz", "points", "Wt"], ints=[], outputs=["A"])

    def _call_level(a, D=_D, reduce_max=True):
        convs, bns = _memo(("sa1", D, a["xyz"].device), lambda: _sa_modules(a["xyz"].device, "sa1", 3 + D, [32]))
        with torch.no_grad():
            if reduce_max:
                return _U().sa_level_max(a["xyz"], a["new_xyz"], a["points"], a["idx"], convs[0], bns[0], True)
            return _U().sa_first_layer(a["xyz"], a["new_xyz"], a["points"], a["idx"], convs[0], bns[0], True)

    row(f"sa_level_max[D{_D}]", "sa_fused", ["sa_level_max"], lambda dev, D=_D: _sa_build(dev, "sa_level_max", D)[0], _call_level,
        floats=["xyz", "new_xyz", "points"], ints=["idx"], outputs=["out"])
    row(f"sa_first_layer[D{_D}]", "sa_fused", ["sa_first_layer"], lambda dev, D=_D: _sa_build(dev, "sa_first_layer", D)[0],
        lambda a, f=_call_level: f(a, reduce_max=False), floats=["xyz", "new_xyz", "points"], ints=["idx"], outputs=["out"])

    def _call_mlp2(a, D=_D, all_points=False):
        dev = a["xyz"].device
        convs, bns = _memo(("sa2", D, dev), lambda: _sa_modules(dev, "sa2", 3 + D, [32, 48]))
        with torch.no_grad():
            if all_points:
                return _U().sa_all_mlp2_max(a["xyz"], a["points"], convs, bns)
            cat = torch.zeros(DB, DS, 80, dtype=torch.float32, device=dev)
            _U().sa_level_mlp2_max(a["xyz"], a["new_xyz"], a["points"], a["idx"], convs, bns, True, out=cat[:, :, 16:64])
            return cat

    row(f"sa_level_mlp2_max[D{_D},out=view]", "sa_fused", ["sa_level_mlp2_max", "split_second_layer"],
        lambda dev, D=_D: _sa_build(dev, "sa_level_mlp2_max", D)[0], _call_mlp2,
        floats=["xyz", "new_xyz", "points"], ints=["idx"], outputs=["cat"])
    row(f"sa_all_mlp2_max[D{_D}]", "sa_fused", ["sa_all_mlp2_max"],
        lambda dev, D=_D: {k: v for k, v in _dense(dev, "sa_all_mlp2_max", D)[0].items() if k in ("xyz", "points")},
        lambda a, f=_call_mlp2: f(a, all_points=True), floats=["xyz", "points"], ints=[], outputs=["out"])


# ---------------------------------------------------------------------------------------------------------------------------
# point_transformer
# ---------------------------------------------------------------------------------------------------------------------------
def _PT():
    from toothgroupnetwork_amd import point_transformer
    return point_transformer


def _sa_tail_build(dev):
    g = gen_for("pt_softmax_aggregate")
    return dict(x_v=q16(g, PN, 32).to(dev), p_r=q16(g, PN, 8, 32).to(dev), logit=q16(g, PN, 8, 4).to(dev),
                idx=torch.randint(0, PN, (PN, 8), generator=g, dtype=torch.int32).to(dev))


row("pt_softmax_aggregate", "point_transformer", ["pt_softmax_aggregate", "_SoftmaxAggregate"], _sa_tail_build,
    lambda a: _PT().pt_softmax_aggregate(a["x_v"], a["p_r"], a["logit"], a["idx"]),
    floats=["x_v", "p_r", "logit"], ints=["idx"], outputs=["out"], diff=["x_v", "p_r", "logit"], grad="bound")


def _attn_build(dev):
    g = gen_for("pt_attention")
    return dict(p=q16(g, PN, 3).to(dev), x_q=q16(g, PN, 32).to(dev), x_k=q16(g, PN, 32).to(dev), x_v=q16(g, PN, 32).to(dev),
                idx=torch.randint(0, PN, (PN, 16), generator=g, dtype=torch.int32).to(dev))


def _attn_call(a):
    dev = a["p"].device

    def make():
        torch.manual_seed(7)
        return _PT().PointTransformerLayer(32, 32, 8, 16).to(dev).eval()
    layer = _memo(("pt_layer", dev), make)
    with torch.no_grad():
        return _PT().pt_attention(a["p"], a["x_q"], a["x_k"], a["x_v"], a["idx"], _PT().fold_pt_layer(layer))


row("pt_attention", "point_transformer", ["pt_attention"], _attn_build, _attn_call,
    floats=["p", "x_q", "x_k", "x_v"], ints=["idx"], outputs=["out"])


def _bn_call(a):
    dev = a["x"].device

    def make():
        torch.manual_seed(9)
        bn = torch.nn.BatchNorm1d(20).to(dev).train()
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
        return bn
    return _PT().bn_rows(_memo(("bn_rows", dev), make), a["x"], relu=True)


row("bn_rows", "point_transformer", ["bn_rows", "_BNRows"], lambda dev: dict(x=q16(gen_for("bn_rows"), PN, 20).to(dev)), _bn_call,
    floats=["x"], ints=[], outputs=["y"], diff=["x"], grad="bound")


# ---------------------------------------------------------------------------------------------------------------------------
# dgcnn
# ---------------------------------------------------------------------------------------------------------------------------
def _G():
    from toothgroupnetwork_amd import dgcnn
    return dgcnn


def _edge_build(dev, C):
    g = gen_for("edgeconv")
    return dict(x=q16(g, DB, C, EN).to(dev), idx=torch.randint(0, EN, (DB, EN, EK), generator=g).to(dev))


def _edge_call(a, two, into_slice):
    dev, C = a["x"].device, a["x"].shape[1]

    def make():
        torch.manual_seed(C)
        c1, b1 = torch.nn.Conv2d(2 * C, 64, 1, bias=False).to(dev), torch.nn.BatchNorm2d(64).to(dev).eval()
        c2, b2 = torch.nn.Conv2d(64, 64, 1, bias=False).to(dev), torch.nn.BatchNorm2d(64).to(dev).eval()
        with torch.no_grad():
            return _G()._edge_first_layer(c1, b1), _G()._second_layer(c2, b2)
    first, second = _memo(("edge", C, dev), make)
    with torch.no_grad():
        if into_slice:
            out = a["out"] if "out" in a else torch.zeros(DB, 192, EN, dtype=torch.float32, device=dev)
            return _G().edgeconv_max(a["x"], a["idx"], first, second if two else None, out=out, coff=64)
        return _G().edgeconv_max(a["x"], a["idx"], first, second if two else None)


row("feature_knn", "dgcnn", ["feature_knn"], lambda dev: dict(x=_edge_build(dev, 6)["x"]),
    lambda a: _G().feature_knn(a["x"], EK), floats=["x"], ints=[], outputs=["idx", "dist2"])
row("edgeconv_max[C6,one_layer]", "dgcnn", ["edgeconv_max"], lambda dev: _edge_build(dev, 6),
    lambda a: _edge_call(a, False, False), floats=["x"], ints=["idx"], outputs=["out"])
row("edgeconv_max[C64,two_layers,out=slice]", "dgcnn", ["edgeconv_max"],
    lambda dev: dict(_edge_build(dev, 64), out=torch.zeros(DB, 192, EN, dtype=torch.float32, device=dev)),
    lambda a: _edge_call(a, True, True), floats=["x", "out"], ints=["idx"], outputs=["out"],
    expect={"out:f64": "raises", "out:f16": "raises", "out:bf16": "raises", "out:strided_t": "raises", "out:strided_col": "raises"})
row("get_graph_feature", "dgcnn", ["get_graph_feature"], lambda dev: dict(x=_edge_build(dev, 6)["x"]),
    lambda a: _G().get_graph_feature(a["x"], k=EK), floats=["x"], ints=[], outputs=["feature"], dtype_follows_input=True)


# ---------------------------------------------------------------------------------------------------------------------------
# crops, cluster, tsegnet
# ---------------------------------------------------------------------------------------------------------------------------
def _crop_build(dev, name):
    g = gen_for(name)
    return dict(feats=q16(g, DB, 6, CN).to(dev), labels=torch.randint(-1, 4, (DB, CN), generator=g).to(dev))


def _crop_call(a):
    from toothgroupnetwork_amd import crops
    return crops.tooth_crops(a["feats"], a["labels"], k=CK)


_FP32_ONLY = {f: "raises" for f in ("f64", "f16", "bf16")}

row("tooth_crops", "crops", ["tooth_crops"], lambda dev: _crop_build(dev, "tooth_crops"), _crop_call,
    floats=["feats"], ints=["labels"], outputs=["cropped", "nn_crop_indexes", "cluster_gt_seg_label", "centroids"],
    expect={"feats:" + f: "raises" for f in _FP32_ONLY})


def _blobs(name, n=400, spread=2):
    """n points in three blobs on the 1/16 grid"""
    g = gen_for(name)
    centres = torch.tensor([[-2.0, -2.0, 0.0], [0.0, 2.0, 1.0], [2.0, -1.0, -1.0]])
    which = torch.arange(n) % 3
    return centres[which] + torch.randint(-spread, spread + 1, (n, 3), generator=g).float() / 16, g


def _C():
    from toothgroupnetwork_amd import cluster
    return cluster


row("dbscan", "cluster", ["dbscan"], lambda dev: dict(points=_blobs("dbscan")[0].to(dev)),
    lambda a: _C().dbscan(a["points"], 0.2, 5), floats=["points"], ints=[], outputs=["labels", "core"],
    expect={"points:" + f: "raises" for f in _FP32_ONLY})
row("mean_shift", "cluster", ["mean_shift", "_mean_shift_seeds"], lambda dev: dict(points=_blobs("mean_shift")[0].double().to(dev)),
    lambda a: _C().mean_shift(a["points"], 0.5), floats=["points"], ints=[], outputs=["labels", "centers"],
    expect={"points:" + f: "raises" for f in ("f32", "f16", "bf16")})


def _gcl_build(dev):
    """DBSCAN(0.03, 30) is fixed inside: on the 1/16 grid only equal points are neighbours, so every blob is two grid points held by
    ~60 points each, plus 12 single points (noise, which the 10-nearest vote relabels); a fifth of all points is gingiva (label 0)"""
    pts, g = _blobs("get_clustering_labels", 388, 0)
    pts[:, 0] += (torch.arange(388) // 3 % 2).float() / 16
    stray = pts[:12] + torch.tensor([0.0, 0.25, 0.0]) + torch.arange(12).float().view(12, 1) / 16
    moved = torch.cat([pts, stray])
    labels = (torch.arange(400) % 5 != 0).long() * 3
    labels[388:] = 3
    return dict(moved_points=moved.to(dev), labels=labels.to(dev))


row("get_clustering_labels", "cluster", ["get_clustering_labels"], _gcl_build,
    lambda a: _C().get_clustering_labels(a["moved_points"], a["labels"]), floats=["moved_points"], ints=["labels"], outputs=["labels"])


def _T():
    from toothgroupnetwork_amd import tsegnet
    return tsegnet


def _prop_build(dev):
    g = gen_for("centroid_proposals")
    return dict(l3_xyz=q16(g, DB, 3, 64).to(dev), offset=q16(g, DB, 3, 64).to(dev), dist=(q16(g, DB, 1, 64) / 8 + 0.25).to(dev))


row("centroid_proposals", "tsegnet", ["centroid_proposals"], _prop_build,
    lambda a: _T().centroid_proposals(a["l3_xyz"], a["offset"], a["dist"]), floats=["l3_xyz", "offset", "dist"], ints=[],
    outputs=["moved", "counts"], expect=dict(_FP32_ONLY))


def _cropf_build(dev):
    g = gen_for("crop_features")
    return dict(feats=q16(g, DB, 6, CN).to(dev), l0_points=q16(g, DB, 20, CN).to(dev), c0=q16(g, 3, 3).to(dev), c1=q16(g, 2, 3).to(dev),
                labels=torch.randint(-1, 4, (DB, CN), generator=g).to(dev))


row("crop_features", "tsegnet", ["crop_features"], _cropf_build,
    lambda a: _T().crop_features(a["feats"], a["l0_points"], [a["c0"], a["c1"]], k=CK, labels=a["labels"]),
    floats=["feats", "l0_points", "c0", "c1"], ints=["labels"], outputs=["cropped", "nn_crop_indexes", "crop_labels"],
    arg_names={"c0": "centres", "c1": "centres"},
    expect=dict({f"{a}:{f}": "raises" for a in ("feats", "l0_points") for f in _FP32_ONLY}, **{"labels:i32": "raises"}))


def _paint_build(dev):
    g = gen_for("paint_labels")
    return dict(i0=torch.randint(0, CN, (3, CK), generator=g).to(dev), i1=torch.randint(0, CN, (2, CK), generator=g).to(dev),
                pd_2=q16(g, 5, 1, CK).to(dev), id_pred=q16(g, 5, 9).to(dev))


row("paint_labels", "tsegnet", ["paint_labels"], _paint_build,
    lambda a: _T().paint_labels([a["i0"], a["i1"]], a["pd_2"], a["id_pred"], CN),
    floats=["pd_2", "id_pred"], ints=["i0", "i1"], outputs=["labels"], arg_names={"i0": "nn_crop_indexes", "i1": "nn_crop_indexes"},
    expect=dict({"pd_2:" + f: "raises" for f in _FP32_ONLY}, **{"i0:i32": "raises", "i1:i32": "raises"}))


# ---------------------------------------------------------------------------------------------------------------------------
# wrappers that pass raw pointers to the library without a row of their own: name -> (module, the row that covers them, why)
# ---------------------------------------------------------------------------------------------------------------------------
INTERNAL = {
    "crop_knn": ("crops", "tooth_crops", "the host layer's launch for crops, cluster and tsegnet, whose wrappers validate and pack first; it "
                 "takes float32 / int32 contiguous operands only and raises for anything else (tests/test_operator_forms_host.py)"),
    "label_centroids": ("crops", "tooth_crops", "as crop_knn: float32 feats and int64 labels, contiguous, or it raises"),
    "dbscan_counts": ("cluster", "dbscan", "dbscan is dbscan_counts(...)[:2]: the same validation and launch, one more output"),
    "_LinearSplitK": ("point_transformer", "bn_rows", "reached through mlp_train next to bn_rows; takes the kernel only for fp32 rows "
                      "and packs them itself, every other dtype goes to torch.bmm"),
    "_launch_point_transform": ("sa_fused", "sa_point_transform[D5]", "the launch under sa_point_transform, which normalises the operands first"),
    "launch_branch": ("sa_fused", "sa_level_max[D5]", "the launch under sa_level_max / sa_level_mlp2_max, which normalise the operands "
                      "first; HotPath calls it with buffers it allocated packed itself"),
    "TransitionDown": ("point_transformer", "sa_point_transform[D5]", "a module: its fused eval path launches the kernels of "
                       "sa_point_transform / sa_level_max on operands it normalises the same way"),
}

REFERENCE_POINTOPS_NAMES = ["FurthestSampling", "furthestsampling", "KNNQuery", "knnquery", "Grouping", "grouping", "queryandgroup",
                            "Subtraction", "subtraction", "Aggregation", "aggregation", "interpolation", "Interpolation", "interpolation2"]
SWEPT_MODULES = ["pointops", "pointnet2_utils", "sa_fused", "dgcnn", "crops", "cluster", "tsegnet", "point_transformer"]


def covered_names(module):
    names = {n for r in ROWS if r["module"] == module for n in r["covers"]}
    return names | {n for n, (m, _, _) in INTERNAL.items() if m == module}
