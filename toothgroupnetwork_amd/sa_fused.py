"""Fused set abstraction (eval mode): the operand layout of the tgn_sa_* kernels and the choice between them, in ONE place.

The kernels (include/tgn_pointops.h) evaluate the shared MLP of a set-abstraction level without the grouped (B,S,K,3+D) tensor.
They read their weights in a layout of their own, and which of them runs depends on the shape.  Three layers, used by the
modules of pointnet2_utils, by HotPath (what bench.py --fused measures), by TransitionDown and by the tools alike:

  packers   pure tensor functions, on whatever device their inputs live: plain (C_out, C_in) matrices -> kernel operands
              Wt  (D+3, C1)       rows [features..., x, y, z], BatchNorm scale folded into the columns -- tgn_sa_point_transform
              Wxs (3, C1)         the x, y, z rows of Wt        -- centre term of tgn_sa_gather_max / tgn_sa_gather_act
              Wd  (16, C1)        rows [x, y, z, features..., 0] -- the direct forms (3+D <= 16)
              b   (C,)            shift + scale * bias
              W2f (C1p/8, C2, 8)  W2f[kb, c, i] = scale[c] * W[c, 8*kb + i], zero for the padded input channels
            C1p = C1 rounded up to 16 (pad16), zero columns added: what the two-layer kernels want of the first layer.
            scale and shift of a module's BatchNorm come from fold.scale_shift (fold.py: the one place that knows the fold); the
            packers take them as plain arguments and scale inside the layout they own;
  plan      plan_branch: everything that depends on shape and configuration only -- direct or commuted first layer, padding, the
            bf16 x 3 weight images, one or two layers -- decided once per (weights, shape);
  launch    launch_branch: the per-point transform where the plan is commuted, then exactly one level kernel.  It only enqueues.
"""
import torch

from . import _derived, _lib, config, fold
from ._lib import f32c, idx_packed, ops, require_cuda, stream


def _sa_operands(xyz, new_xyz, points, idx):
    """The tensor arguments of the fused set-abstraction entries as the kernels read them: packed fp32 rows, packed indices.  The
    modules pass them in that form already (then nothing is copied); a direct caller may pass any floating dtype or layout."""
    require_cuda(xyz, new_xyz, points, idx)
    return (f32c(xyz.detach()), None if new_xyz is None else f32c(new_xyz.detach()), None if points is None else f32c(points.detach()),
            None if idx is None else idx_packed(idx))


# ---------------------------------------------------------------------------------------------
# packers
# ---------------------------------------------------------------------------------------------
def pad16(C1):
    return (C1 + 15) // 16 * 16


def _pad_cols(t, C1p):
    if t.shape[-1] == C1p:
        return t.contiguous()
    out = t.new_zeros(t.shape[:-1] + (C1p,))
    out[..., :t.shape[-1]] = t
    return out


def _scaled(W, scale):
    return W if scale is None else W * scale[:, None]


def _folded_bias(W, bias, scale, shift):
    # an absent term is skipped, not replaced by 1 or 0: the present ones arrive bit for bit (the sign of a zero included)
    b = bias if (bias is None or scale is None) else scale * bias
    if shift is not None:
        b = shift if b is None else shift + b
    return W.new_zeros(W.shape[0]) if b is None else b.contiguous()


def pack_first_layer(W, bias, scale, shift, D, xyz_first):
    """W (C1, 3+D) fp32 with the columns [x, y, z, features...] (xyz_first: sample_and_group) or [features..., x, y, z] (Msg);
    bias, scale, shift (C1,) or None -> dict(Wt, Wxs, Wd, b, C1).  Wd is all zero where 3+D > 16 (no direct form there)."""
    C1 = W.shape[0]
    Wx, Wp = (W[:, :3], W[:, 3:]) if xyz_first else (W[:, D:], W[:, :D])
    Ws = W.new_empty(C1, 3 + D)
    Ws[:, :D], Ws[:, D:] = _scaled(Wp, scale), _scaled(Wx, scale)
    Wt = Ws.t().contiguous()
    Wd = W.new_zeros(16, C1)
    if 3 + D <= 16:
        Wd[:3], Wd[3:3 + D] = Wt[D:], Wt[:D]
    return dict(Wt=Wt, Wxs=Wt[D:].contiguous(), Wd=Wd, b=_folded_bias(W, bias, scale, shift), C1=C1)


def pack_second_layer(W, bias, scale, shift, C1p):
    """W (C2, C1) fp32; bias, scale, shift (C2,) or None -> W2f (C1p/8, C2, 8), b2 (C2,)."""
    C2, C1 = W.shape
    Wp = W.new_zeros(C2, C1p)
    Wp[:, :C1] = _scaled(W, scale)
    return Wp.view(C2, C1p // 8, 8).permute(1, 0, 2).contiguous(), _folded_bias(W, bias, scale, shift)


def _conv_operands(conv, bn):
    W = conv.weight.detach().reshape(conv.out_channels, -1).float()
    return (W, None if conv.bias is None else conv.bias.detach().float()) + fold.scale_shift(bn)


def fold_first_layer(conv, bn, D, xyz_first):
    """pack_first_layer of the first Conv2d(1x1) + eval-mode BatchNorm2d of a shared MLP, memoised on `bn` until a parameter /
    running statistic of the two modules changes (_derived.cached)."""
    return _derived.cached(bn, "first_layer", _derived.sources(conv, bn), (D, bool(xyz_first)),
                           lambda: pack_first_layer(*_conv_operands(conv, bn), D, xyz_first))


def fold_second_layer(conv, bn, C1p):
    """pack_second_layer of the second Conv2d(1x1) + eval-mode BatchNorm2d of a shared MLP, memoised like the first."""
    return _derived.cached(bn, "second_layer", _derived.sources(conv, bn), C1p, lambda: pack_second_layer(*_conv_operands(conv, bn), C1p))


def split_second_layer(W2f):
    """The bf16 x 3 image of a folded second-layer weight matrix W2f (C1p/8, C2, 8) for tgn_sa_mlp2_max_bf16x3."""
    C1p, C2 = W2f.shape[0] * 8, W2f.shape[1]
    img = torch.empty(int(ops().tgn_sa_mlp2_split_bytes(C1p, C2)), dtype=torch.uint8, device=W2f.device)
    ops().tgn_sa_mlp2_split_weights(C1p, C2, W2f, img, stream())
    return img


def split_point_transform(Wt):
    """The bf16 x 3 image of a per-point first-layer matrix Wt (D+3, C1) for tgn_sa_point_transform_bf16x3: rows padded with zeros
    to a multiple of 16, arranged (Kp/8, C1, 8) and split like a second layer (tgn_sa_mlp2_split_weights)."""
    Kc, C1 = Wt.shape
    Kp = pad16(Kc)
    Wp = Wt.new_zeros(Kp, C1)
    Wp[:Kc] = Wt
    return split_second_layer(Wp.view(Kp // 8, 8, C1).permute(0, 2, 1).contiguous()), Kp


# ---------------------------------------------------------------------------------------------
# plan and launch
# ---------------------------------------------------------------------------------------------
def plan_branch(first, second, K, D, *, bf16x3):
    """Everything about one (radius, nsample) branch that shape and configuration decide.  first = pack_first_layer(...), second =
    pack_second_layer(..., pad16(first["C1"])) or None, both on the GPU; K = nsample, D = feature channels of the level's input.
      direct   the first layer is computed from the gathered rows (narrow inputs) instead of commuted onto the points
      C1p      width of the first layer as the kernels see it (two layers: padded to 16), C_out that of the branch's output
      W1, b1   Wd (direct) or Wxs (commuted) and the folded bias, padded to C1p;  Wt likewise, None when direct
      bf16x3   two-layer branches only: W2s / Wts = the bf16 x 3 images of W2f / Wt (the matrix cores' bf16 rate at fp32 accuracy:
               three-way split of both operands, six products; an infinite activation or weight turns into NaN there)."""
    C1 = first["C1"]
    if second is None:
        direct = bool(ops().tgn_sa_direct_supported(K, D, C1))
        return dict(nlayers=1, K=K, D=D, direct=direct, C1p=C1, C_out=C1, W1=first["Wd"] if direct else first["Wxs"], b1=first["b"],
                    Wt=None if direct else first["Wt"], Wts=None)
    W2f, b2 = second
    C1p = pad16(C1)
    if W2f.shape[0] * 8 != C1p:
        raise ValueError(f"plan_branch: second layer packed for {W2f.shape[0] * 8} input channels, the first layer has {C1p}")
    direct = bool(ops().tgn_sa_mlp2_direct_supported(K, D))
    Wt = None if direct else _pad_cols(first["Wt"], C1p)
    return dict(nlayers=2, K=K, D=D, direct=direct, C1p=C1p, C_out=b2.shape[0], W1=_pad_cols(first["Wd"] if direct else first["Wxs"], C1p),
                b1=_pad_cols(first["b"], C1p), Wt=Wt, Wts=split_point_transform(Wt) if (bf16x3 and not direct) else None,
                W2f=W2f, b2=b2, W2s=split_second_layer(W2f) if bf16x3 else None)


def _module_plan(convs, bns, K, D, xyz_first, bf16x3):
    """plan_branch of a one- or two-layer Conv2d/BatchNorm2d stack, memoised on its last BatchNorm (some 40 small launches per
    branch otherwise, every forward)."""
    def build():
        first = fold_first_layer(convs[0], bns[0], D, xyz_first)
        second = fold_second_layer(convs[1], bns[1], pad16(first["C1"])) if len(convs) == 2 else None
        return plan_branch(first, second, K, D, bf16x3=bf16x3)
    return _derived.cached(bns[-1], "sa_plan", _derived.sources(*convs, *bns), (K, D, bool(xyz_first), bool(bf16x3)), build)


def _launch_point_transform(M, D, C1, xyz, points, Wt, Wts, A, st):
    if Wts is not None and M <= 65535 * 128:        # (the bf16 x 3 kernel's grid: one block per 128 rows)
        img, Kp = Wts
        ops().tgn_sa_point_transform_bf16x3(M, D, Kp, C1, xyz, points, img, A, st)
    else:
        ops().tgn_sa_point_transform(M, D, C1, xyz, points, Wt, A, st)


def launch_branch(plan, B, N, S, xyz, new_xyz, points, idx, idx64, out, A, st):
    """One branch of a fused level on stream st: xyz (B,N,3), new_xyz (B,S,3), points (B,N,D) or None, idx (B,S,K) -> out (B,S,C_out)
    (two layers: any row stride).  A: the caller's (B,N,C1p) buffer for the per-point transform, None for a direct plan.  Packed
    fp32 / int32 or int64 (idx64) operands; nothing is allocated, synchronised or checked here."""
    L, K, D, C1p, W1, b1 = ops(), plan["K"], plan["D"], plan["C1p"], plan["W1"], plan["b1"]
    if not plan["direct"]:
        _launch_point_transform(B * N, D, C1p, xyz, points, plan["Wt"], plan["Wts"], A, st)
    if plan["nlayers"] == 2 and plan["W2s"] is not None:
        L.tgn_sa_mlp2_max_bf16x3(B, N, S, K, D, C1p, plan["C_out"], A, xyz, points, new_xyz, W1, b1, idx, int(idx64), plan["W2s"], plan["b2"],
                                 out, out.stride(1), st)
    elif plan["nlayers"] == 2:
        L.tgn_sa_mlp2_max(B, N, S, K, D, C1p, plan["C_out"], A, xyz, points, new_xyz, W1, b1, idx, int(idx64), plan["W2f"], plan["b2"], out,
                          out.stride(1), st)
    elif plan["direct"]:
        L.tgn_sa_direct_max(B, N, S, K, D, C1p, xyz, new_xyz, points, W1, b1, idx, int(idx64), 1, out, st)
    else:
        L.tgn_sa_gather_max(B, N, S, K, C1p, A, new_xyz, W1, b1, idx, int(idx64), 1, out, st)


# ---------------------------------------------------------------------------------------------
# the operators the modules call
# ---------------------------------------------------------------------------------------------
def sa_point_transform(xyz, points, Wt, Wts=None):
    """A[b,n,:] = [points[b,n,:], xyz[b,n,:]] @ Wt -- the per-POINT half of a fused first layer, on the matrix cores.
    xyz (B,N,3), points (B,N,D) or None, Wt (D+3, C1) -> (B,N,C1).  Wts = split_point_transform(Wt): the bf16 x 3 form
    (tgn_sa_point_transform_bf16x3, fp32-class rounding at up to 2.7x the rate); None: exact fp32 MFMA (tgn_sa_point_transform)."""
    xyz, _, points, _ = _sa_operands(xyz, None, points, None)
    Wt = f32c(Wt, "Wt")
    B, N, _ = xyz.shape
    D = 0 if points is None else points.shape[2]
    if Wt.dim() != 2 or Wt.shape[0] != D + 3:
        raise ValueError(f"sa_point_transform: Wt must be ({D + 3}, C1) for points with {D} channels, got {tuple(Wt.shape)}")
    A = torch.empty(B, N, Wt.shape[1], dtype=torch.float32, device=xyz.device)
    _launch_point_transform(B * N, D, Wt.shape[1], xyz, points, Wt, Wts, A, stream())
    return A


def _level(who, xyz, new_xyz, points, idx, convs, bns, xyz_first, out):
    xyz, new_xyz, points, idx = _sa_operands(xyz, new_xyz, points, idx)
    B, N, _ = xyz.shape
    _, S, K = idx.shape
    plan = _module_plan(convs, bns, K, 0 if points is None else points.shape[2], xyz_first, config.cfg.sa_bf16x3)
    C = plan["C_out"]
    if out is None:
        out = torch.empty(B, S, C, dtype=torch.float32, device=xyz.device)
    if out.dtype != torch.float32 or out.device != xyz.device:
        raise TypeError(f"{who}: out must be float32 on {xyz.device}, got {out.dtype} on {out.device}")
    if tuple(out.shape) != (B, S, C) or out.stride(2) != 1 or out.stride(0) != S * out.stride(1):
        raise ValueError(f"{who}: out must be ({B}, {S}, {C}) with unit last stride and evenly spaced rows, got "
                         f"{tuple(out.shape)} with strides {tuple(out.stride())}")
    A = None if plan["direct"] else torch.empty(B, N, plan["C1p"], dtype=torch.float32, device=xyz.device)
    _lib.begin_index_check()
    launch_branch(plan, B, N, S, xyz, new_xyz, points, idx, idx.dtype == torch.int64, out, A, stream())
    _lib.raise_on_index_error("set abstraction (grouping)")
    return out


def sa_level_max(xyz, new_xyz, points, idx, conv, bn, xyz_first):
    """A whole single-layer set-abstraction level after sampling and ball query:
        max_k relu(bn(conv([xyz[idx]-new_xyz, points[idx]])))  ->  (B,S,C1)
    (pointnet2_utils.py:162-169 + 229-236, or 281-294 for Msg) with nothing of size S*K ever written: narrow inputs go
    through the direct kernel (gather -> matrix cores -> max), wide ones through the per-point transform + gather-max."""
    return _level("sa_level_max", xyz, new_xyz, points, idx, [conv], [bn], xyz_first, None)


def sa_level_mlp2_max(xyz, new_xyz, points, idx, convs, bns, xyz_first, out=None):
    """A whole set-abstraction level with a TWO-layer shared MLP after sampling and ball query:
        max_k relu(bn2(conv2(relu(bn1(conv1([xyz[idx]-new_xyz, points[idx]]))))))  ->  (B,S,C2)
    (pointnet2_utils.py:162-169 + 229-236, or 281-294 for Msg) in ONE kernel after the per-point transform of the first
    layer (wide inputs) or with the first layer computed from the gathered rows (3+D <= 16): nothing of size S*K is
    written, no torch convolution runs (tgn_sa_mlp2_max[_bf16x3]).  out: optional (B,S,C2) view into a wider row-major tensor
    (last stride 1) -- a multi-scale level writes its branches side by side."""
    return _level("sa_level_mlp2_max", xyz, new_xyz, points, idx, list(convs[:2]), list(bns[:2]), xyz_first, out)


def sa_first_layer(xyz, new_xyz, points, idx, conv, bn, xyz_first, reduce_max=False):
    """relu(bn(conv(grouped))) of the FIRST shared-MLP layer without ever building `grouped`
    (pointnet2_utils.py:162-169 + 229-233, or 281-292 for Msg).  The 1x1 convolution commutes with the gather:
        W*[points[idx], xyz[idx]-c] + b = (W_p*points + W_x*xyz)[idx] + (b - W_x*c)
    so the contraction runs over the N points (tgn_sa_point_transform, fp32 MFMA) instead of the S*K grouped rows and
    the per-query kernel only gathers, adds the centre term and applies ReLU.  Returns (B,S,K,C1), or (B,S,C1) with
    reduce_max (= sa_level_max).  Eval-mode BatchNorm statistics are folded in."""
    if reduce_max:
        return sa_level_max(xyz, new_xyz, points, idx, conv, bn, xyz_first)
    xyz, new_xyz, points, idx = _sa_operands(xyz, new_xyz, points, idx)
    B, N, _ = xyz.shape
    _, S, K = idx.shape
    f = fold_first_layer(conv, bn, 0 if points is None else points.shape[2], xyz_first)
    A = sa_point_transform(xyz, points, f["Wt"])
    out = torch.empty(B, S, K, f["C1"], dtype=torch.float32, device=xyz.device)
    _lib.begin_index_check()
    ops().tgn_sa_gather_act(B, N, S, K, f["C1"], A, new_xyz, f["Wxs"], f["b"], idx, int(idx.dtype == torch.int64), 1, out, stream())
    _lib.raise_on_index_error("set abstraction (grouping)")
    return out


def sa_all_mlp2_max(xyz, points, convs, bns):
    """PointNetSetAbstraction(group_all=True) with a two-layer shared MLP, eval mode (pointnet2_utils.py:178-195 + 229-236; the one
    instantiation is tsg_seg_module.py:28, 515 -> [256, 512] over 256 points):
        max_n relu(bn2(conv2(relu(bn1(conv1([xyz_n, points_n]))))))  ->  (B, C2)
    The first layer runs once per point on the fp32 matrix cores (tgn_sa_point_transform; 3+D <= 16: inside the kernel), the second
    layer and the maximum over the cloud in tgn_sa_all_mlp2_max: no (B,1,N,.) tensor, no torch convolution."""
    xyz, _, points, _ = _sa_operands(xyz, None, points, None)
    B, N, _ = xyz.shape
    D = 0 if points is None else points.shape[2]
    L = ops()
    plan = _module_plan(list(convs[:2]), list(bns[:2]), 64, D, True, False)     # (its "groups" are chunks of at most 64 points)
    C1p, C2 = plan["C1p"], plan["C_out"]
    out = torch.empty(B, C2, dtype=torch.float32, device=xyz.device)
    chunks = int(L.tgn_sa_all_chunks(N))
    part = torch.empty(B, chunks, C2, dtype=torch.float32, device=xyz.device) if chunks > 1 else None
    A1 = None if plan["direct"] else sa_point_transform(xyz, points, plan["Wt"])
    L.tgn_sa_all_mlp2_max(B, N, D, C1p, C2, A1, xyz, points, plan["W1"] if plan["direct"] else None, plan["b1"], plan["W2f"], plan["b2"], part,
                          out, C2, stream())
    return out
