"""MI355X implementation of the reference's ``external_libs/pointnet2_utils/pointnet2_utils.py``.

Every public name of the reference module (pointnet2_utils.py:8-352) is provided with the same
signature, layouts (dense ``(B, N, C)`` / channel-first modules) and dtypes (int64 indices), so
``models/modules/pointnet_pp.py``, ``tsg_centroid_module.py``, ``tsg_seg_module.py``, ``tsegnet.py``,
``tgn_loss.py`` and ``tsg_loss.py`` import it unchanged.

What differs is how the work is done: FPS, ball query, the gather+centre+concat of grouping, three_nn
and three_interpolate are single HIP kernels (include/tgn_pointops.h section 3) instead of chains of
torch kernels that materialise (B,S,N) matrices and sort them.  The shared MLPs stay nn.Conv/BatchNorm
layers with the reference's parameter names, so state_dicts are interchangeable.

Retained reference fallbacks.  About 25 lines of the reference's own torch logic live on here, on paths the fast kernels do
not cover, because they ARE the semantics to preserve there: the three ``nn.Module`` constructors (sub-module names and order
decide the state_dict keys), the train-mode tails ``F.relu(bn(conv(x)))`` of the set-abstraction / feature-propagation
stacks (pointnet2_utils.py:229-236, :289-294, :345-351 -- BatchNorm needs batch statistics there), the general-C form of
``square_distance`` (:36-40; the kernel covers C = 3) and the sort-based three-nearest-neighbour weights for DIFFERENTIABLE
coordinates (:333-340; no reference model has them).  Everything on the eval and C = 3 paths is this package's own.
"""
import os
from time import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function

from . import _derived, _lib, config, fold, fps, ordered
from ._lib import as_int, f32c, ops, require_cuda, stream
from .sa_fused import (fold_first_layer, fold_second_layer, pad16, sa_all_mlp2_max,  # noqa: F401
                       sa_first_layer, sa_level_max, sa_level_mlp2_max, sa_point_transform, split_point_transform, split_second_layer)

_fwd = torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
_bwd = torch.amp.custom_bwd(device_type="cuda")


def timeit(tag, t):
    print("{}: {}s".format(tag, time() - t))
    return time()


def pc_normalize(pc):
    centroid = np.mean(pc, axis=0)
    pc = pc - centroid
    m = np.max(np.sqrt(np.sum(pc ** 2, axis=1)))
    pc = pc / m
    return pc


# ---------------------------------------------------------------------------------------------
# square_distance
# ---------------------------------------------------------------------------------------------
class _SquareDistance3(Function):
    """square_distance for 3-D points with the reference's exact (torch-CPU) arithmetic:
    dot = fma(z1,z2,fma(y1,y2,x1*x2)); d = ((-2*dot) + |src|^2) + |dst|^2   (pointnet2_utils.py:20-41)."""

    @staticmethod
    @_fwd
    def forward(ctx, src, dst):
        src, dst = f32c(src), f32c(dst)
        B, N, _ = src.shape
        if dst.shape[0] != B:
            raise RuntimeError(f"square_distance: batch sizes differ ({B} vs {dst.shape[0]})")
        M = dst.shape[1]
        out = torch.empty(B, N, M, dtype=torch.float32, device=src.device)
        ops().tgn_square_distance(B, N, M, src, dst, out, stream())
        ctx.save_for_backward(src, dst)
        return out

    @staticmethod
    @_bwd
    def backward(ctx, g):
        src, dst = ctx.saved_tensors
        g = g.float()
        g_src = g_dst = None
        if ctx.needs_input_grad[0]:
            g_src = 2.0 * (src * g.sum(-1, keepdim=True) - torch.matmul(g, dst))
        if ctx.needs_input_grad[1]:
            g_dst = 2.0 * (dst * g.sum(-2).unsqueeze(-1) - torch.matmul(g.transpose(1, 2), src))
        return g_src, g_dst


def square_distance(src, dst):
    """All-pairs squared distances, src (B,N,C) x dst (B,M,C) -> (B,N,M), in the expanded form
    -2*src.dst + |src|^2 + |dst|^2 of the reference (so values can be slightly negative, as there)."""
    require_cuda(src, dst)
    if src.shape[-1] == 3 and dst.shape[-1] == 3:
        return _SquareDistance3.apply(src, dst)
    # C != 3 never occurs in the reference models; same formula, generic C (pointnet2_utils.py:38-41)
    B, N, _ = src.shape
    _, M, _ = dst.shape
    dist = -2 * torch.matmul(src, dst.permute(0, 2, 1))
    dist += torch.sum(src ** 2, -1).view(B, N, 1)
    dist += torch.sum(dst ** 2, -1).view(B, 1, M)
    return dist


# ---------------------------------------------------------------------------------------------
# index_points
# ---------------------------------------------------------------------------------------------
class _IndexPoints(Function):
    @staticmethod
    @_fwd
    def forward(ctx, points, idx):
        B, N, C = points.shape
        M = idx.numel() // B if B else 0
        out = torch.empty(tuple(idx.shape) + (C,), dtype=torch.float32, device=points.device)
        _lib.begin_index_check()
        ops().tgn_gather_points(B, N, M, C, points, idx, int(idx.dtype == torch.int64), out, stream())
        _lib.raise_on_index_error("index_points")
        ctx.shape = (B, N, M)
        ctx.save_for_backward(idx)
        return out

    @staticmethod
    @_bwd
    def backward(ctx, g):
        idx, = ctx.saved_tensors
        B, N, M = ctx.shape
        return ordered.gather_backward(g.contiguous().float(), idx, N, (B, M)), None


def index_points(points, idx):
    """points (B,N,C) gathered with idx (B,S) or (B,S,K) (int64/int32, per-cloud indices) -> (B,S[,K],C);
    differentiable w.r.t. points (scatter-add backward).  Negative indices wrap and an index outside [-N, N) raises
    IndexError, as torch's advanced indexing does in the reference (pointnet2_utils.py:56-60); the check costs one
    stream synchronisation per call (TGN_INDEX_CHECK=off drops it: such rows are then zero-filled and
    _lib.take_index_error() reports them)."""
    require_cuda(points, idx)
    if idx.dtype not in (torch.int64, torch.int32):
        idx = idx.long()
    points = f32c(points)
    out = _IndexPoints.apply(points, idx.contiguous())
    return out


# ---------------------------------------------------------------------------------------------
# farthest point sampling: fps.py, shared with pointops; the names of this module stay and FPS_PREFIX is cfg.fps_prefix (below).
# The set-abstraction modules in eval mode ask for the FPS-of-an-FPS-result shortcut (prefix=True), the plain operators do not.
# ---------------------------------------------------------------------------------------------
_fps_dense = fps.sample_dense
fps_prefix_stats = fps.stats
fps_prefix_clear = fps.clear


def farthest_point_sample(xyz, npoint):
    """(B,N,3) -> (B,npoint) int64 indices local to each cloud; the first sample is point 0, as in the kernel the
    reference calls (pointnet2_utils.py:87-98 / sampling_cuda_kernel.cu:39).  Tie order / contraction follow
    _lib.set_fps_mode() (TGN_FPS_TIES, TGN_FPS_FMA): 'first' = torch-CPU semantics (default), 'tree' = the
    reference CUDA kernel's reduction order."""
    return _fps_dense(xyz, npoint)[0]


def farthest_point_sample_np(xyz, npoint):
    """numpy in / numpy out variant with a RANDOM first sample (pointnet2_utils.py:103-118), indices bit-identical
    to the reference's torch-CPU loop for the same torch RNG state -- ties included -- for float32 input.  (float64 input:
    the reference keeps the numpy dtype, computes the squared distances in float64 and rounds them to float32 only when
    it stores them (:113-116); here the coordinates are rounded to float32 first, so the arg-max may differ where two
    candidates are closer than float32 resolution.)

    The start is drawn with the reference's own call, torch.randint(0, N, (B,), dtype=torch.long) (:109).  The GPU
    kernel always starts at a cloud's first point, so each cloud is sampled as [p_start, p_0, ..., p_{N-1}]: the copy
    in front makes p_start the first sample, every later arg-max sees the original points in their original order
    (first-index ties as in torch.max, :117), and the copy itself sits at distance 0 like p_start.  Index 0 of the
    padded cloud maps back to `start` for the first sample and to point 0 afterwards (an exhausted or all-NaN cloud,
    where torch.max returns index 0)."""
    xyz_t = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32))
    B, N, _ = xyz_t.shape
    farthest = torch.randint(0, N, (B,), dtype=torch.long)
    first = torch.gather(xyz_t, 1, farthest.view(B, 1, 1).expand(B, 1, 3))
    padded = torch.cat([first, xyz_t], dim=1).to(torch.device("cuda"))
    # this function IS the torch-CPU semantics (first-index ties, unfused distance), whatever mode the kernels are in:
    # the flags go with the call, the process-wide mode is not touched (other threads may be sampling)
    idx = _fps_dense(padded, npoint, mode=0)[0].cpu() - 1
    if idx.shape[1] > 0:
        idx[:, 0] = farthest
    idx.clamp_(min=0)
    return idx.numpy()


# ---------------------------------------------------------------------------------------------
# ball query and grouping
# ---------------------------------------------------------------------------------------------
_ws_cache = {}


def _workspace(nbytes, device):
    if nbytes == 0:
        return None
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def query_ball_point(radius, nsample, xyz, new_xyz):
    """xyz (B,N,3) cloud, new_xyz (B,S,3) centres -> (B,S,nsample) int64: per centre the first `nsample` point
    indices, in ascending index order, whose expanded-form squared distance is <= radius**2; short rows repeat
    their first hit (reference pointnet2_utils.py:120-144, without its (B,S,N) matrix and sort)."""
    require_cuda(xyz, new_xyz)
    nsample = as_int(nsample)
    xyz, new_xyz = f32c(xyz.detach()), f32c(new_xyz.detach())
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    # `sqrdists > radius ** 2`: python evaluates radius**2 in double, torch compares in fp32
    r2 = float(torch.tensor(float(radius) ** 2, dtype=torch.float32).item())
    group_idx = torch.empty(B, S, nsample, dtype=torch.int64, device=xyz.device)
    nbytes = int(ops().tgn_ball_query_workspace_bytes(B, N, S))
    ws = _workspace(nbytes, xyz.device)
    ops().tgn_ball_query(B, N, S, nsample, r2, xyz, new_xyz, group_idx, 1, ws, nbytes, stream())
    return group_idx


class _GroupPoints(Function):
    """out[b,s,k,:] = concat(xyz[b,idx]-new_xyz[b,s], points[b,idx]) (xyz_first) or the Msg order
    (points first) -- pointnet2_utils.py:162-169 / 281-285 -- in one kernel."""

    @staticmethod
    @_fwd
    def forward(ctx, xyz, new_xyz, points, idx, xyz_first):
        B, N, _ = xyz.shape
        _, S, K = idx.shape
        D = 0 if points is None else points.shape[2]
        out = torch.empty(B, S, K, 3 + D, dtype=torch.float32, device=xyz.device)
        _lib.begin_index_check()
        ops().tgn_group_points(B, N, S, K, D, xyz, new_xyz, points, idx, int(idx.dtype == torch.int64), int(xyz_first), out, stream())
        _lib.raise_on_index_error("group_points")
        ctx.dims = (B, N, S * K, D, bool(xyz_first))
        ctx.save_for_backward(idx)
        return out

    @staticmethod
    @_bwd
    def backward(ctx, g):
        idx, = ctx.saved_tensors
        B, N, M, D, xyz_first = ctx.dims
        g = g.contiguous().float()
        g_rel = (g[..., :3] if xyz_first else g[..., D:]).contiguous()
        lists = ordered.gather_lists(idx, N, (B, M))    # xyz and features share them
        g_xyz = g_new = g_pts = None
        if ctx.needs_input_grad[0]:
            g_xyz = ordered.gather_backward(g_rel, idx, N, (B, M), lists)
        if ctx.needs_input_grad[1]:
            g_new = -g_rel.sum(2)       # torch's sum in both forms (pointops._QueryGroup takes ordered.centres_backward for its centres)
        if D and ctx.needs_input_grad[2]:
            g_pts = ordered.gather_backward((g[..., 3:] if xyz_first else g[..., :D]).contiguous(), idx, N, (B, M), lists)
        return g_xyz, g_new, g_pts, None, None


def group_points(xyz, new_xyz, points, idx, xyz_first=True):
    """Fused gather + centre + concat: (B,S,K,3+D) = [xyz[idx]-new_xyz, points[idx]] (xyz_first, reference :162-169)
    or [points[idx], xyz[idx]-new_xyz] (:281-285).  Raises IndexError where the reference's indexing would -- an
    empty ball yields index N (pointnet2_utils.py:136-141) -- after one stream synchronisation per call;
    TGN_INDEX_CHECK=off drops check and sync (rows with a bad index are then filled from point 0)."""
    require_cuda(xyz, new_xyz, idx)
    out = _GroupPoints.apply(f32c(xyz), f32c(new_xyz), None if points is None else f32c(points),
                             idx.contiguous(), bool(xyz_first))
    return out


def sample_and_group(npoint, radius, nsample, xyz, points, returnfps=False):
    """FPS -> ball query -> fused grouping.  xyz (B,N,3), points (B,N,D) or None ->
    new_xyz (B,npoint,3), new_points (B,npoint,nsample,3+D) in [centred xyz, features] order (reference :168);
    with returnfps also the gathered absolute coordinates and the FPS indices."""
    fps_idx = farthest_point_sample(xyz, npoint)  # [B, npoint]
    new_xyz = index_points(xyz, fps_idx)
    idx = query_ball_point(radius, nsample, xyz, new_xyz)
    new_points = group_points(xyz, new_xyz, points, idx, xyz_first=True)
    if returnfps:
        grouped_xyz = index_points(xyz, idx)
        return new_xyz, new_points, grouped_xyz, fps_idx
    return new_xyz, new_points


def sample_and_group_all(xyz, points):
    """One group holding the whole cloud: new_xyz (B,1,3) zeros, new_points (B,1,N,3+D) = [xyz, points]."""
    device = xyz.device
    B, N, C = xyz.shape
    new_xyz = torch.zeros(B, 1, C).to(device)
    grouped_xyz = xyz.view(B, 1, N, C)
    if points is not None:
        new_points = torch.cat([grouped_xyz, points.view(B, 1, N, -1)], dim=-1)
    else:
        new_points = grouped_xyz
    return new_xyz, new_points


# ---------------------------------------------------------------------------------------------
# three_nn / three_interpolate
# ---------------------------------------------------------------------------------------------
def three_nn(xyz1, xyz2):
    """3 nearest points of xyz2 (B,S,3) for every point of xyz1 (B,N,3): (dist (B,N,3) squared,
    expanded form, ascending by (dist, index); idx (B,N,3) int64) -- pointnet2_utils.py:333-335."""
    require_cuda(xyz1, xyz2)
    xyz1, xyz2 = f32c(xyz1.detach()), f32c(xyz2.detach())
    B, N, _ = xyz1.shape
    S = xyz2.shape[1]
    dist = torch.empty(B, N, 3, dtype=torch.float32, device=xyz1.device)
    idx = torch.empty(B, N, 3, dtype=torch.int64, device=xyz1.device)
    ops().tgn_three_nn(B, N, S, xyz1, xyz2, dist, idx, 1, stream())
    return dist, idx


class _ThreeInterpolate(Function):
    @staticmethod
    @_fwd
    def forward(ctx, points2, dist, idx):
        B, S, C = points2.shape
        N = dist.shape[1]
        out = torch.empty(B, N, C, dtype=torch.float32, device=points2.device)
        weight = torch.empty(B, N, 3, dtype=torch.float32, device=points2.device)
        ops().tgn_three_interpolate(B, N, S, C, points2, dist, idx, int(idx.dtype == torch.int64), out, weight, stream())
        ctx.dims = (B, S)
        ctx.save_for_backward(idx, weight)
        return out

    @staticmethod
    @_bwd
    def backward(ctx, g):
        idx, weight = ctx.saved_tensors
        B, S = ctx.dims
        return ordered.weighted_gather_backward(g.contiguous().float(), idx, weight, S, B), None, None


def linear_relu(x, W, b):
    """relu(x @ W.T + b) over the last axis of contiguous fp32 rows, the ReLU in the GEMM's epilogue (hipBLASLt through
    torch._addmm_activation: bit-identical to F.linear followed by relu_, one pass over the output less); any other input takes
    those two calls."""
    if (hasattr(torch, "_addmm_activation") and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and W.dtype == torch.float32
            and b is not None and not (torch.is_grad_enabled() and (x.requires_grad or W.requires_grad or b.requires_grad))):
        y = torch._addmm_activation(b, x.reshape(-1, x.shape[-1]), W.t(), use_gelu=False)
        return y.view(*x.shape[:-1], W.shape[0])
    return torch.relu_(F.linear(x, W, b))


def three_interpolate_add_relu(points2, dist, idx, add=None, relu=False):
    """[relu](three_interpolate(points2, dist, idx) (+ add)) in ONE kernel, no autograd: the epilogue of the eval-mode feature
    propagation (first convolution commuted onto the coarse points; `add` = the skip features' share of that convolution plus the
    folded bias).  `add` (B,N,C) is overwritten with the result when given (it is a temporary there)."""
    require_cuda(points2, dist, idx)
    if idx.dtype not in (torch.int64, torch.int32):
        idx = idx.long()
    points2, dist, idx = f32c(points2), f32c(dist), idx.contiguous()
    B, S, C = points2.shape
    N = dist.shape[1]
    if add is not None:
        add = f32c(add)
        if tuple(add.shape) != (B, N, C):
            raise ValueError(f"three_interpolate_add_relu: add must be ({B}, {N}, {C}), got {tuple(add.shape)}")
    out = add if add is not None else torch.empty(B, N, C, dtype=torch.float32, device=points2.device)
    ops().tgn_three_interpolate_ex(B, N, S, C, points2, dist, idx, int(idx.dtype == torch.int64), add, int(bool(relu)), out, None, stream())
    return out


def three_interpolate(points2, dist, idx):
    """inverse-(squared)-distance weighted sum of the 3 neighbours (pointnet2_utils.py:337-340) -> (B,N,C)."""
    require_cuda(points2, dist, idx)
    if idx.dtype not in (torch.int64, torch.int32):
        idx = idx.long()
    return _ThreeInterpolate.apply(f32c(points2), f32c(dist), idx.contiguous())


# ---------------------------------------------------------------------------------------------
# fused set abstraction (eval mode): WHEN the modules below take the fused kernels.  Operand layout, kernel choice and the
# operators (sa_level_max, sa_level_mlp2_max, sa_first_layer, sa_all_mlp2_max) are sa_fused.py's; the modules call them through
# this module's names.
# ---------------------------------------------------------------------------------------------
# The switches of this module live in toothgroupnetwork_amd.config (cfg.fused_sa, cfg.commute_fp -- feature propagation: first
# convolution on the coarse points, below --, cfg.sa_bf16x3 -- sa_fused.plan_branch).  FUSED_SA / COMMUTE_FP / SA_BF16X3 remain as
# live aliases of those fields (reads and writes).
config.legacy_attributes(__name__, {"FUSED_SA": "fused_sa", "COMMUTE_FP": "commute_fp", "SA_BF16X3": "sa_bf16x3", "FPS_PREFIX": "fps_prefix"})


def _can_fuse(module, *tensors):
    """Eval-mode, no autograd through the inputs: BatchNorm is a fixed affine map and can be folded."""
    if not config.cfg.fused_sa or module.training:
        return False
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        return False
    if torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters()):
        return False
    return True


def _fuse_pays(N, S, K, c_in, c1):
    """A MULTI-layer MLP still needs its (B,S,K,C1) first-layer output; the commuted first layer trades the grouped
    tensor (S*K rows of c_in) for a per-point one (N rows of c1): worth it once the former is the larger (sa1 of the
    reference net, c_in = 9 -> 128 channels: it is not; measured 0.89x)."""
    return S * K * c_in > N * c1


def _mlp2_shape_ok(K, C1):
    """tgn_sa_mlp2_max keeps the per-query constants of its 4 (K <= 32) or 2 queries in LDS next to the tile buffers."""
    return 1 <= K <= 64 and (4 if K <= 32 else 2) * pad16(C1) <= 8192


def _fused_level(xyz_c, new_xyz, points_c, idx, convs, bns, xyz_first, N, S, K):
    """The fused eval-mode forms of one (radius, nsample) branch, or None when the shared MLP / shape has none:
    one layer -> sa_level_max; two layers (every level of the reference networks) -> sa_level_mlp2_max; more -> fused first
    layer (where it is cheaper than grouping) + the remaining layers in torch.  Returns (B, C', S)."""
    n = len(convs)
    if n == 0 or not _fused_shape_ok(K, convs[0].out_channels):
        return None
    if n == 1:
        return sa_level_max(xyz_c, new_xyz, points_c, idx, convs[0], bns[0], xyz_first).permute(0, 2, 1)
    if n == 2 and _mlp2_shape_ok(K, convs[0].out_channels):
        return sa_level_mlp2_max(xyz_c, new_xyz, points_c, idx, convs, bns, xyz_first).permute(0, 2, 1)
    if _fuse_pays(N, S, K, 3 + (0 if points_c is None else points_c.shape[2]), convs[0].out_channels):
        y = sa_first_layer(xyz_c, new_xyz, points_c, idx, convs[0], bns[0], xyz_first=xyz_first)
        return _mlp_tail_and_max(y, convs, bns, 1)
    return None


def _fused_shape_ok(K, C1):
    return K <= 64 and C1 % 4 == 0


def _mlp_tail_and_max(x_bskc, convs, bns, first):
    """Layers `first`.. of the shared MLP on a (B,S,K,C) tensor, then max over K -> (B,C',S)."""
    x = x_bskc.permute(0, 3, 2, 1)  # [B, C, K, S] view, exactly what the reference feeds its Conv2d stack
    for j in range(first, len(convs)):
        x = F.relu(bns[j](convs[j](x)))
    return torch.max(x, 2)[0]


# ---------------------------------------------------------------------------------------------
# modules (constructor signatures and parameter names of pointnet2_utils.py:198-352)
# ---------------------------------------------------------------------------------------------
class PointNetSetAbstraction(nn.Module):
    def __init__(self, npoint, radius, nsample, in_channel, mlp, group_all):
        super(PointNetSetAbstraction, self).__init__()
        self.npoint = npoint
        self.radius = radius
        self.nsample = nsample
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last_channel = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(nn.Conv2d(last_channel, out_channel, 1))
            self.mlp_bns.append(nn.BatchNorm2d(out_channel))
            last_channel = out_channel
        self.group_all = group_all

    def forward(self, xyz, points):
        """channel-first in, channel-first out: xyz (B,3,N), points (B,D,N) or None ->
        new_xyz (B,3,S) sampled centres, features (B,D',S)."""
        xyz = xyz.permute(0, 2, 1)
        if points is not None:
            points = points.permute(0, 2, 1)
        if not self.group_all and len(self.mlp_convs) > 0 and _can_fuse(self, xyz, points):
            # eval fast path: FPS (+coordinates) -> ball query -> fused shared MLP + max; `grouped` is never built
            xyz_c = f32c(xyz)
            points_c = None if points is None else f32c(points)
            _, new_xyz = _fps_dense(xyz_c, self.npoint, want_coords=True, prefix=True)
            idx = query_ball_point(self.radius, self.nsample, xyz_c, new_xyz)
            new_points = _fused_level(xyz_c, new_xyz, points_c, idx, self.mlp_convs, self.mlp_bns, True, xyz_c.shape[1],
                                      self.npoint, self.nsample)
            if new_points is None:      # no fused form for this MLP / shape: group, then the reference's stack
                new_points = _mlp_tail_and_max(group_points(xyz_c, new_xyz, points_c, idx, xyz_first=True), self.mlp_convs,
                                               self.mlp_bns, 0)
            return new_xyz.permute(0, 2, 1), new_points
        if (self.group_all and len(self.mlp_convs) == 2 and xyz.shape[1] >= 1 and _can_fuse(self, xyz, points)
                and _mlp2_shape_ok(min(xyz.shape[1], 64), self.mlp_convs[0].out_channels)):
            # eval fast path of the form the reference builds (tsg_seg_module.py:28): the whole cloud is one group
            y = sa_all_mlp2_max(f32c(xyz), None if points is None else f32c(points), self.mlp_convs, self.mlp_bns)
            return xyz.new_zeros(xyz.shape[0], xyz.shape[2], 1), y.unsqueeze(2)
        if self.group_all:
            new_xyz, new_points = sample_and_group_all(xyz, points)
        else:
            new_xyz, new_points = sample_and_group(self.npoint, self.radius, self.nsample, xyz, points)
        new_points = new_points.permute(0, 3, 2, 1)  # [B, C+D, nsample, npoint]
        for i, conv in enumerate(self.mlp_convs):
            bn = self.mlp_bns[i]
            new_points = F.relu(bn(conv(new_points)))
        new_points = torch.max(new_points, 2)[0]
        new_xyz = new_xyz.permute(0, 2, 1)
        return new_xyz, new_points


class PointNetSetAbstractionMsg(nn.Module):
    def __init__(self, npoint, radius_list, nsample_list, in_channel, mlp_list):
        super(PointNetSetAbstractionMsg, self).__init__()
        self.npoint = npoint
        self.radius_list = radius_list
        self.nsample_list = nsample_list
        self.conv_blocks = nn.ModuleList()
        self.bn_blocks = nn.ModuleList()
        for i in range(len(mlp_list)):
            convs = nn.ModuleList()
            bns = nn.ModuleList()
            last_channel = in_channel + 3
            for out_channel in mlp_list[i]:
                convs.append(nn.Conv2d(last_channel, out_channel, 1))
                bns.append(nn.BatchNorm2d(out_channel))
                last_channel = out_channel
            self.conv_blocks.append(convs)
            self.bn_blocks.append(bns)

    def forward(self, xyz, points):
        """channel-first in, channel-first out: xyz (B,3,N), points (B,D,N) or None ->
        new_xyz (B,3,S) sampled centres, features (B,D',S)."""
        xyz = xyz.permute(0, 2, 1)
        if points is not None:
            points = points.permute(0, 2, 1)
        S = self.npoint
        # one FPS launch yields both the indices and the sampled coordinates (:276)
        if xyz.requires_grad:
            new_xyz = index_points(xyz, farthest_point_sample(xyz, S))
        else:
            _, new_xyz = _fps_dense(xyz, S, want_coords=True, prefix=not self.training)
        xyz_c = f32c(xyz)
        points_c = None if points is None else f32c(points)
        fuse = _can_fuse(self, xyz, points)
        new_points_list = []
        chained = fuse and all(len(c) == 2 and _fused_shape_ok(k, c[0].out_channels) and _mlp2_shape_ok(k, c[0].out_channels)
                               for c, k in zip(self.conv_blocks, self.nsample_list))
        with _lib.deferred_index_check("set abstraction (grouping)"):      # one flag read for all branches
            if chained:
                # every branch is one chained kernel: they write their columns of the concatenated output side by side (:296-298)
                widths = [c[1].out_channels for c in self.conv_blocks]
                cat = torch.empty(xyz_c.shape[0], S, sum(widths), dtype=torch.float32, device=xyz_c.device)
                col = 0
                for i, radius in enumerate(self.radius_list):
                    group_idx = query_ball_point(radius, self.nsample_list[i], xyz_c, new_xyz)
                    sa_level_mlp2_max(xyz_c, new_xyz, points_c, group_idx, self.conv_blocks[i], self.bn_blocks[i], False,
                                      out=cat[:, :, col:col + widths[i]])
                    col += widths[i]
                return new_xyz.permute(0, 2, 1), cat.permute(0, 2, 1)
            for i, radius in enumerate(self.radius_list):
                K = self.nsample_list[i]
                group_idx = query_ball_point(radius, K, xyz_c, new_xyz)
                convs, bns = self.conv_blocks[i], self.bn_blocks[i]
                new_points = _fused_level(xyz_c, new_xyz, points_c, group_idx, convs, bns, False, xyz_c.shape[1], S, K) if fuse else None
                if new_points is None:
                    grouped_points = group_points(xyz_c, new_xyz, points_c, group_idx, xyz_first=False)  # [feat, rel_xyz] (:285)
                    new_points = _mlp_tail_and_max(grouped_points, convs, bns, 0)                        # (:286-294)
                new_points_list.append(new_points)
        new_xyz = new_xyz.permute(0, 2, 1)
        new_points_concat = torch.cat(new_points_list, dim=1)
        return new_xyz, new_points_concat


def fold_fp_stack(convs, bns):
    """[(W', b')] of a feature-propagation stack of Conv1d(1x1) + eval-mode BatchNorm1d pairs, memoised on its first BatchNorm."""
    return _derived.cached(bns[0], "fp_eval", _derived.sources(*convs, *bns), None,
                           lambda: [fold.affine(c, b) for c, b in zip(convs, bns)])


class PointNetFeaturePropagation(nn.Module):
    def __init__(self, in_channel, mlp):
        super(PointNetFeaturePropagation, self).__init__()
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last_channel = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(nn.Conv1d(last_channel, out_channel, 1))
            self.mlp_bns.append(nn.BatchNorm1d(out_channel))
            last_channel = out_channel

    def forward(self, xyz1, xyz2, points1, points2):
        """xyz1 (B,3,N) dense level, xyz2 (B,3,S) coarse level, points1 (B,D1,N) skip features or None,
        points2 (B,D2,S) coarse features -> (B,D',N): inverse-distance interpolation of points2 onto xyz1,
        concatenated after points1, then the Conv1d/BN/ReLU stack."""
        xyz1 = xyz1.permute(0, 2, 1)
        xyz2 = xyz2.permute(0, 2, 1)
        points2 = points2.permute(0, 2, 1)
        B, N, C = xyz1.shape
        _, S, _ = xyz2.shape

        if (config.cfg.commute_fp and S > 1 and S < N and len(self.mlp_convs) > 0 and not (xyz1.requires_grad or xyz2.requires_grad)
                and points2.dtype == torch.float32):
            # The first 1x1 convolution commutes with the interpolation (a weighted sum whose weights do not depend on the
            # features): W * [p1, sum_i w_i f2[idx_i]] + b = W1 * p1 + sum_i w_i (W2 * f2)[idx_i] + b.  The coarse features are
            # transformed ONCE per coarse point (S rows instead of N: fp1 of the reference net 1024 instead of 24 000 rows of a
            # 512-wide contraction), and neither the interpolated (B,N,D2) tensor nor the concatenated (B,D1+D2,N) one exists.
            # Exact algebra; fp32 rounding differs in summation order only.  Differentiable like the plain form.
            conv0 = self.mlp_convs[0]
            W = conv0.weight.squeeze(-1)                                        # (C1, D1 + D2), columns [points1, points2] (:345)
            D2 = points2.shape[2]
            D1 = W.shape[1] - D2
            dist, idx = three_nn(xyz1, xyz2)
            if _can_fuse(self, xyz1, xyz2, points1, points2):
                # eval: every BatchNorm folded into its 1x1 convolution (memoised), the whole stack on channel-last rows -- one GEMM
                # with bias + an in-place ReLU per layer, no normalisation kernels and no (B,N,C) <-> (B,C,N) copies in between; the
                # result goes out as the channel-first VIEW of the channel-last tensor
                layers = fold_fp_stack(self.mlp_convs, self.mlp_bns)
                W0, b0 = layers[0]
                # relu(interpolation of the transformed coarse rows + the skip features' share + bias): the bias rides in the COARSE
                # GEMM (S contiguous rows; the interpolation weights sum to one, so it comes through unchanged up to one rounding --
                # the skip features arrive as a channel-first view, where torch would add a bias in a pass of its own), sum and ReLU
                # in the interpolation kernel -- no elementwise pass over the (B, N, C1) tensor
                coarse = F.linear(points2, W0[:, D1:], b0)
                skip = F.linear(points1.permute(0, 2, 1), W0[:, :D1]) if points1 is not None else None
                y = three_interpolate_add_relu(coarse, dist, idx, add=skip, relu=True)      # (B, N, C1)
                for Wi, bi in layers[1:]:
                    y = linear_relu(y, Wi, bi)
                return y.permute(0, 2, 1)
            y = three_interpolate(F.linear(points2, W[:, D1:]), dist, idx)      # (B, N, C1)
            if points1 is not None:
                y = y + F.linear(points1.permute(0, 2, 1), W[:, :D1])
            if conv0.bias is not None:
                y = y + conv0.bias
            new_points = F.relu(self.mlp_bns[0](y.permute(0, 2, 1)))
            for i in range(1, len(self.mlp_convs)):
                new_points = F.relu(self.mlp_bns[i](self.mlp_convs[i](new_points)))
            return new_points
        if S == 1:
            interpolated_points = points2.repeat(1, N, 1)
        elif xyz1.requires_grad or xyz2.requires_grad:
            # differentiable coordinates (never the case in the reference models): same maths in torch so
            # that the interpolation weights carry gradient as they would in the reference (:333-340)
            dists = square_distance(xyz1, xyz2)
            dists, idx = dists.sort(dim=-1)
            dists, idx = dists[:, :, :3], idx[:, :, :3]
            dist_recip = 1.0 / (dists + 1e-8)
            norm = torch.sum(dist_recip, dim=2, keepdim=True)
            weight = dist_recip / norm
            interpolated_points = torch.sum(index_points(points2, idx) * weight.view(B, N, 3, 1), dim=2)
        else:
            dist, idx = three_nn(xyz1, xyz2)
            interpolated_points = three_interpolate(points2, dist, idx)

        if points1 is not None:
            points1 = points1.permute(0, 2, 1)
            new_points = torch.cat([points1, interpolated_points], dim=-1)
        else:
            new_points = interpolated_points

        new_points = new_points.permute(0, 2, 1)
        for i, conv in enumerate(self.mlp_convs):
            bn = self.mlp_bns[i]
            new_points = F.relu(bn(conv(new_points)))
        return new_points
