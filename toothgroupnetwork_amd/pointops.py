"""MI355X implementation of the reference's ``external_libs/pointops/functions/pointops.py``.

Same public names, positional arguments, return layouts and dtypes as the reference operators
(limhoyeon/ToothGroupNetwork, pointops.py:10-216), so ``models/modules/cbl_point_transformer/*``
and ``gen_utils.fps`` import it unchanged through ``external_libs/pointops/functions/pointops.py``.

Layout conventions of the reference ("packed batch"): xyz (n,3) fp32, features (n,c) fp32,
``offset`` (b) int32 cumulative end of every cloud.  Everything runs through the C ABI of
libtgn_pointops.so on the current HIP stream; there is no CPU path.
"""
import os
from collections import OrderedDict

import torch
from torch.autograd import Function
from torch.utils.weak import WeakTensorKeyDictionary

from . import _lib, config, fps, ordered
from ._lib import as_int, f32c, idx32c, ops, require_cuda, stream

_fwd = torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
_bwd = torch.amp.custom_bwd(device_type="cuda")


def _packed(t, what):
    """Guard inside the autograd Functions, which callers in this package reach directly (.apply): the kernels behind them read
    `t` through its raw pointer as packed fp32."""
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{what} must be float32 and contiguous here, got {t.dtype} with strides {tuple(t.stride())}; "
                         "the public functions of this module normalise their arguments")
    return t


def _packed_idx(t, what):
    if t.dtype != torch.int32 or not t.is_contiguous():
        raise ValueError(f"{what} must be int32 and contiguous here, got {t.dtype} with strides {tuple(t.stride())}")
    return t


def _offsets_host(offset):
    """Offsets are device tensors in the reference API; the output size depends on their values, so one
    device->host copy per call is inherent (the reference syncs b+1 times, pointops.py:18-21)."""
    return [int(v) for v in offset.detach().cpu().tolist()]


# Host copies of offset tensors whose values the caller already knows (a dense batch: b * n; a transition-down level:
# counts // stride).  With them the sampling call needs no device->host copy at all, which is what makes a whole
# Point-Transformer forward capturable in a HIP graph (tools/pt_forward_bench.py).  Keyed by tensor identity (weakly) and
# version counter: an in-place write invalidates the entry.
_known_offsets = WeakTensorKeyDictionary()


def _version(t):
    try:
        return t._version
    except RuntimeError:      # inference tensors carry no version counter; they cannot be written in place either
        return -1


def register_offsets(offset, values):
    """Tell this module the host values of a device offset tensor (a list of ints of the same length)."""
    values = [int(v) for v in values]
    assert len(values) == offset.numel()
    _known_offsets[offset] = (_version(offset), values)
    return offset


def offsets_host(*offsets):
    """Host values of offset tensors: from register_offsets where known, else ONE device->host copy for the rest."""
    out, missing = [None] * len(offsets), []
    for i, t in enumerate(offsets):
        hit = _known_offsets.get(t)
        if hit is not None and hit[0] == _version(t):
            out[i] = hit[1]
        else:
            missing.append(i)
    if missing:
        flat = _offsets_host(torch.cat([offsets[i].reshape(-1) for i in missing]))
        for i in missing:
            n = offsets[i].numel()
            out[i], flat = flat[:n], flat[n:]
    return out


# Farthest-point sampling lives in fps.py (one front end and one book for the packed and the dense layout); the names of this
# module stay.  cfg.fps_prefix is aliased as FPS_PREFIX below.
fps_workspace = fps.workspace
fps_prefix_stats = fps.stats
fps_prefix_clear = fps.clear
fps_prefix_adopt = fps.adopt


def fps_with_coords(xyz, offset, new_offset, cuda_compat=False, prefix=False):
    """fps.sample_packed with the host offsets from this module: one device->host copy, or none (register_offsets)."""
    return fps.sample_packed(xyz, offset, new_offset, cuda_compat, prefix, host=offsets_host(offset, new_offset))


class FurthestSampling(Function):
    @staticmethod
    def forward(ctx, xyz, offset, new_offset):
        """
        input: xyz: (n, 3), offset: (b), new_offset: (b)
        output: idx: (m)            [reference: pointops.py:10-24]
        """
        idx, _ = fps_with_coords(xyz, offset, new_offset)
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, grad):
        return None, None, None


furthestsampling = FurthestSampling.apply


def _knn_raw(nsample, xyz, new_xyz, offset, new_offset):
    nsample = as_int(nsample)
    if new_xyz is None:
        new_xyz = xyz
    require_cuda(xyz, new_xyz, offset, new_offset)
    xyz, new_xyz = f32c(xyz.detach(), "xyz"), f32c(new_xyz.detach(), "new_xyz")
    offset, new_offset = idx32c(offset, "offset"), idx32c(new_offset, "new_offset")
    m = new_xyz.shape[0]
    idx = torch.empty(m, nsample, dtype=torch.int32, device=xyz.device)
    dist2 = torch.empty(m, nsample, dtype=torch.float32, device=xyz.device)
    b, n = offset.shape[0], xyz.shape[0]
    if config.cfg.knn_grid and nsample <= 63 and b > 0 and n >= config.cfg.knn_grid_min_points * b:
        # big segments: per-segment grids, a query looks at the cells around it (same result)
        nbytes = int(ops().tgn_knnquery_grid_workspace_bytes(b, n, m))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=xyz.device) if nbytes else None
        ops().tgn_knnquery_grid(b, n, m, nsample, xyz, new_xyz, offset, new_offset, idx, dist2, ws, nbytes, stream())
        return idx, dist2
    nbytes = int(ops().tgn_knnquery_workspace_bytes(m))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=xyz.device) if nbytes else None
    ops().tgn_knnquery_ws(b, m, nsample, xyz, new_xyz, offset, new_offset, idx, dist2, ws, nbytes, stream())
    return idx, dist2


# cfg.knn_grid / cfg.knn_grid_min_points (average points per segment) / cfg.knn_cache_size: toothgroupnetwork_amd.config; the
# module-level names of rounds 1-4 stay as live aliases
config.legacy_attributes(__name__, {"KNN_GRID": "knn_grid", "KNN_GRID_MIN_POINTS": "knn_grid_min_points", "_KNN_CACHE_SIZE": "knn_cache_size",
                                    "FPS_PREFIX": "fps_prefix"})


# kNN memo.  The reference recomputes identical neighbour lists again and again: PointTransformerLayer calls
# queryandgroup(idx=None) twice with the same arguments (blocks.py:34-35) and every block of a stage repeats it.
# Results are keyed on the identity (pointer, shape, strides, dtype) AND version counter of the argument tensors (kept alive by the cache, so an
# address can not be recycled under a live key) and on the current stream (a result is only handed to launches that
# are stream-ordered after the one that produced it); an in-place write bumps the version and misses.  Tensors
# without a version counter (torch.inference_mode) bypass the memo.  Writes that torch cannot see -- through
# `.data`, raw pointers, the pointops_cuda shim -- do not bump the version: call knn_cache_clear() after them.
_KNN_CACHE = OrderedDict()


def _knn_cached(nsample, xyz, new_xyz, offset, new_offset):
    if config.cfg.knn_cache_size <= 0:
        return _knn_raw(nsample, xyz, new_xyz, offset, new_offset)
    tensors = (xyz, xyz if new_xyz is None else new_xyz, offset, new_offset)
    try:
        # inference tensors (torch.inference_mode) carry no version counter: _version raises -> no memo for them
        key = (as_int(nsample), torch.cuda.current_stream().cuda_stream) + tuple(
            (t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride()), t.dtype) for t in tensors)
    except RuntimeError:
        return _knn_raw(nsample, xyz, new_xyz, offset, new_offset)
    hit = _KNN_CACHE.get(key)
    if hit is not None:
        _KNN_CACHE.move_to_end(key)
        return hit[1], hit[2]
    idx, dist2 = _knn_raw(nsample, xyz, new_xyz, offset, new_offset)
    _KNN_CACHE[key] = (tensors, idx, dist2)
    while len(_KNN_CACHE) > config.cfg.knn_cache_size:
        _KNN_CACHE.popitem(last=False)
    return idx, dist2


def knn_cache_clear():
    _KNN_CACHE.clear()


def knn_indices(nsample, xyz, new_xyz, offset, new_offset):
    """The neighbour rows of knnquery -- (m, nsample) int32 -- for callers inside this package that only READ them: the memo's own
    tensor (no clone) and no distance output (no sqrt pass); 84 of each per Point-Transformer forward otherwise."""
    require_cuda(xyz, offset, new_offset)
    return _knn_cached(nsample, xyz, new_xyz, offset, new_offset)[0]


class KNNQuery(Function):
    @staticmethod
    def forward(ctx, nsample, xyz, new_xyz, offset, new_offset):
        """
        input: xyz: (n, 3), new_xyz: (m, 3), offset: (b), new_offset: (b)
        output: idx: (m, nsample), dist: (m, nsample)  (sqrt of the squared distances) [pointops.py:30-43]
        """
        idx, dist2 = _knn_cached(nsample, xyz, new_xyz, offset, new_offset)
        idx = idx.clone()  # callers may write into the result; the memo must stay intact
        dist = torch.sqrt(dist2)
        ctx.mark_non_differentiable(idx, dist)
        return idx, dist

    @staticmethod
    def backward(ctx, *grads):
        return None, None, None, None, None


knnquery = KNNQuery.apply


class Grouping(Function):
    # .apply takes packed operands only -- float32 features, int32 indices, contiguous -- and raises ValueError otherwise (the
    # reference's kernels read int32 too); the function of the same name in lower case casts and packs any dtype and layout
    @staticmethod
    def gather_rows(input, idx):
        """The launch, shared with _QueryGroup without use_xyz: input (n, c), idx (m, nsample), packed -> input[idx] (m, nsample, c)"""
        m, nsample, c = idx.shape[0], idx.shape[1], input.shape[1]
        output = torch.empty(m, nsample, c, dtype=torch.float32, device=input.device)
        ops().tgn_grouping_forward(m, nsample, c, input, idx, output, stream())
        return output

    @staticmethod
    @_fwd
    def forward(ctx, input, idx):
        """
        input: input: (n, c), idx : (m, nsample)
        output: (m, nsample, c)     [pointops.py:48-61]
        """
        require_cuda(input, idx)
        _packed(input, "input"), _packed_idx(idx, "idx")
        ctx.n = input.shape[0]
        ctx.save_for_backward(idx)
        return Grouping.gather_rows(input, idx)

    @staticmethod
    @_bwd
    def backward(ctx, grad_output):
        """
        input: grad_out: (m, nsample, c)
        output: (n, c), None        [pointops.py:63-74]
        """
        idx, = ctx.saved_tensors
        return ordered.gather_backward(grad_output.contiguous().float(), idx, ctx.n), None


def grouping(input, idx):
    """input (n, c) of any floating dtype and layout, idx (m, nsample) of any integer dtype -> (m, nsample, c) float32"""
    require_cuda(input, idx)
    return Grouping.apply(f32c(input, "input"), idx32c(idx, "idx"))


class _QueryGroup(Function):
    """gather + centre + concat of queryandgroup as ONE kernel per tensor (pointops.py:89-100).

    The reference materialises xyz[idx], subtracts, gathers feat[idx] and concatenates (4 tensors);
    here the (m, nsample, 3+c) result is written once.  Gradients flow to xyz, new_xyz and feat exactly
    as torch autograd would give for the reference's fancy indexing."""

    @staticmethod
    @_fwd
    def forward(ctx, xyz, new_xyz, feat, idx, use_xyz):
        _packed(feat, "feat"), _packed_idx(idx, "idx")
        if use_xyz:
            _packed(xyz, "xyz"), _packed(new_xyz, "new_xyz")
        m, nsample = idx.shape
        n, c = feat.shape
        if use_xyz and (tuple(xyz.shape) != (n, 3) or tuple(new_xyz.shape) != (m, 3)):
            raise ValueError(f"xyz must be ({n}, 3) and new_xyz ({m}, 3), got {tuple(xyz.shape)} and {tuple(new_xyz.shape)}")
        ctx.n, ctx.use_xyz = n, use_xyz
        ctx.save_for_backward(idx)
        if not use_xyz:
            return Grouping.gather_rows(feat, idx)
        out = torch.empty(m, nsample, 3 + c, dtype=torch.float32, device=feat.device)
        # packed layout == dense layout with B=1: rows of new_xyz are the S "centres", K = nsample
        ops().tgn_group_points(1, n, m, nsample, c, xyz, new_xyz, feat, idx, 0, 1, out, stream())
        return out

    @staticmethod
    @_bwd
    def backward(ctx, grad_out):
        idx, = ctx.saved_tensors
        g_feat = grad_out.contiguous().float()
        lists = ordered.gather_lists(idx, ctx.n)        # xyz and features share them
        g_xyz = g_new = None
        if ctx.use_xyz:
            g_rel, g_feat = g_feat[:, :, :3].contiguous(), g_feat[:, :, 3:].contiguous()
            if ctx.needs_input_grad[0]:
                g_xyz = ordered.gather_backward(g_rel, idx, ctx.n, lists=lists)
            if ctx.needs_input_grad[1]:
                # (the ordered form is a kernel's sum; pointnet2_utils._GroupPoints keeps torch's sum for its centres in both forms)
                g_new = ordered.centres_backward(g_rel)
        return g_xyz, g_new, ordered.gather_backward(g_feat, idx, ctx.n, lists=lists), None, None


def queryandgroup(nsample, xyz, new_xyz, feat, idx, offset, new_offset, use_xyz=True):
    """
    input: xyz: (n, 3), new_xyz: (m, 3), feat: (n, c), idx: (m, nsample), offset: (b), new_offset: (b)
    output: new_feat: (m, nsample, 3+c) if use_xyz else (m, nsample, c)     [pointops.py:79-100]
    """
    nsample = as_int(nsample)
    if new_xyz is None:
        new_xyz = xyz
    require_cuda(xyz, new_xyz, feat)
    same = new_xyz is xyz
    xyz, feat = f32c(xyz, "xyz"), f32c(feat, "feat")
    new_xyz = xyz if same else f32c(new_xyz, "new_xyz")
    own_idx = idx is None
    if own_idx:
        idx, _ = knnquery(nsample, xyz, new_xyz, offset, new_offset)  # (m, nsample)
    idx = idx32c(idx, "idx")
    if not own_idx and use_xyz:
        _lib.begin_index_check()
    out = _QueryGroup.apply(xyz, new_xyz, feat, idx, bool(use_xyz))
    if not own_idx and use_xyz:
        # a caller's index tensor may hold anything; the reference's fancy indexing (pointops.py:89-95) raises
        _lib.raise_on_index_error("queryandgroup")
    return out


class Subtraction(Function):
    # .apply takes packed operands only -- float32 features, int32 indices, contiguous -- and raises ValueError otherwise (the
    # reference's kernels read int32 too); the function of the same name in lower case casts and packs any dtype and layout
    @staticmethod
    @_fwd
    def forward(ctx, input1, input2, idx):
        """
        input: input1: (n, c), input2: (n, c), idx: (n, nsample)
        output:  (n, nsample, c)    [pointops.py:103-116]
        """
        require_cuda(input1, input2, idx)
        _packed(input1, "input1"), _packed(input2, "input2"), _packed_idx(idx, "idx")
        n, c = input1.shape
        nsample = idx.shape[-1]
        output = torch.empty(n, nsample, c, dtype=torch.float32, device=input1.device)
        ops().tgn_subtraction_forward(n, nsample, c, input1, input2, idx, output, stream())
        ctx.n2 = input2.shape[0]
        ctx.save_for_backward(idx)
        return output

    @staticmethod
    @_bwd
    def backward(ctx, grad_output):
        """
        input: grad_out: (n, nsample, c)
        output: grad_input1: (n, c), grad_input2: (n, c)    [pointops.py:118-128]
        """
        idx, = ctx.saved_tensors
        return ordered.subtraction_backward(grad_output.contiguous().float(), idx, ctx.n2) + (None,)


def subtraction(input1, input2, idx):
    """input1, input2 (n, c) of any floating dtype and layout, idx (n, nsample) of any integer dtype -> (n, nsample, c) float32"""
    require_cuda(input1, input2, idx)
    return Subtraction.apply(f32c(input1, "input1"), f32c(input2, "input2"), idx32c(idx, "idx"))


class Aggregation(Function):
    # .apply takes packed operands only -- float32 features, int32 indices, contiguous -- and raises ValueError otherwise (the
    # reference's kernels read int32 too); the function of the same name in lower case casts and packs any dtype and layout
    @staticmethod
    @_fwd
    def forward(ctx, input, position, weight, idx):
        """
        input: input: (n, c), position: (n, nsample, c), weight : (n, nsample, c'), idx: (n, nsample)
        output: (n, c)              [pointops.py:133-146]
        """
        require_cuda(input, position, weight, idx)
        _packed(input, "input"), _packed(position, "position"), _packed(weight, "weight"), _packed_idx(idx, "idx")
        n, nsample, c = position.shape
        w_c = weight.shape[-1]
        output = torch.zeros(n, c, dtype=torch.float32, device=input.device)
        ops().tgn_aggregation_forward(n, nsample, c, w_c, input, position, weight, idx, output, stream())
        ctx.save_for_backward(input, position, weight, idx)
        return output

    @staticmethod
    @_bwd
    def backward(ctx, grad_output):
        """
        input: grad_out: (n, c)
        output: grad_input: (n, c), grad_position: (n, nsample, c), grad_weight : (n, nsample, c')  [pointops.py:148-159]
        """
        input, position, weight, idx = ctx.saved_tensors
        grad_output = grad_output.contiguous().float()
        n, nsample, c = position.shape
        w_c = weight.shape[-1]
        grad_input = torch.zeros(input.shape[0], c, dtype=torch.float32, device=grad_output.device)
        grad_position = torch.zeros(n, nsample, c, dtype=torch.float32, device=grad_output.device)
        grad_weight = torch.zeros(n, nsample, w_c, dtype=torch.float32, device=grad_output.device)
        ops().tgn_aggregation_backward(n, nsample, c, w_c, input, position, weight, idx, grad_output, grad_input, grad_position, grad_weight,
                                       stream())
        return grad_input, grad_position, grad_weight, None


def aggregation(input, position, weight, idx):
    """input (n, c), position (n, nsample, c), weight (n, nsample, c') of any floating dtype and layout, idx (n, nsample) of any
    integer dtype -> (n, c) float32"""
    require_cuda(input, position, weight, idx)
    return Aggregation.apply(f32c(input, "input"), f32c(position, "position"), f32c(weight, "weight"), idx32c(idx, "idx"))


def _inverse_distance_weights(dist):
    dist_recip = 1.0 / (dist + 1e-8)
    norm = torch.sum(dist_recip, dim=1, keepdim=True)
    return dist_recip / norm


class _WeightedGather(Function):
    """out[n,:] = sum_i feat[idx[n,i],:] * weight[n,i]  -- the loop of pointops.py:177-179 / the native
    interpolation kernel (interpolation_cuda_kernel.cu:5-18) with its atomic backward (:20-33)."""

    @staticmethod
    def launch(ctx, feat, idx, weight):
        """The forward launch, shared with Interpolation, and what the backward needs on ctx."""
        n, k = idx.shape
        m, c = feat.shape
        output = torch.zeros(n, c, dtype=torch.float32, device=feat.device)
        ops().tgn_interpolation_forward(n, c, k, feat, idx, weight, output, stream())
        ctx.m = m
        ctx.save_for_backward(idx, weight)
        return output

    @staticmethod
    @_fwd
    def forward(ctx, feat, idx, weight):
        _packed(feat, "feat"), _packed_idx(idx, "idx"), _packed(weight, "weight")
        return _WeightedGather.launch(ctx, feat, idx, weight)

    @staticmethod
    @_bwd
    def backward(ctx, grad_output):
        return ordered.weighted_gather_backward(grad_output.contiguous().float(), *ctx.saved_tensors, ctx.m), None, None


def interpolation(xyz, new_xyz, feat, offset, new_offset, k=3):
    """
    input: xyz: (m, 3), new_xyz: (n, 3), feat: (m, c), offset: (b), new_offset: (b)
    output: (n, c)                  [pointops.py:164-180; weights detached as there]
    """
    require_cuda(xyz, new_xyz, feat)
    xyz, new_xyz, feat = f32c(xyz, "xyz"), f32c(new_xyz, "new_xyz"), f32c(feat, "feat")
    k = as_int(k)
    idx, dist = knnquery(k, xyz, new_xyz, offset, new_offset)  # (n, k), (n, k)
    weight = _inverse_distance_weights(dist).detach().contiguous()
    return _WeightedGather.apply(feat, idx, weight)


class Interpolation(Function):
    # _WeightedGather behind an uncached k-NN and its inverse-distance weights (and, unlike it, without the autocast decorators)
    @staticmethod
    def forward(ctx, xyz, new_xyz, input, offset, new_offset, k=3):
        """
        input: xyz: (m, 3), new_xyz: (n, 3), input: (m, c), offset: (b), new_offset: (b)
        output: (n, c)              [pointops.py:183-201]
        """
        require_cuda(xyz, new_xyz, input)
        _packed(input, "input")
        k = as_int(k)
        idx, dist2 = _knn_raw(k, xyz, new_xyz, offset, new_offset)      # (normalises xyz, new_xyz and the offsets itself)
        weight = _inverse_distance_weights(torch.sqrt(dist2)).contiguous()
        return _WeightedGather.launch(ctx, input, idx, weight)

    @staticmethod
    def backward(ctx, grad_output):
        """
        output: None, None, grad_input (m, c), None, None, None     [pointops.py:203-214]
        """
        return None, None, ordered.weighted_gather_backward(grad_output.contiguous().float(), *ctx.saved_tensors, ctx.m), None, None, None


def interpolation2(xyz, new_xyz, input, offset, new_offset, k=3):
    """Interpolation.apply on arguments of any floating dtype and layout (the gradient reaches `input` only, as in the reference)"""
    require_cuda(xyz, new_xyz, input)
    return Interpolation.apply(f32c(xyz, "xyz"), f32c(new_xyz, "new_xyz"), f32c(input, "input"), offset, new_offset, k)
