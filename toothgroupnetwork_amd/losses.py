"""The geometric training losses of tgnet_fps and tsegnet as fused HIP kernels (csrc/loss.hip, include/tgn_pointops.h):

  batch_center_offset_loss, batch_chamfer_distance_loss   models/tgn_loss.py:6-61, 263-302 (names and argument order kept)
  tgn_offset_losses                                       all three terms of the two above from ONE forward and ONE backward pass
  centroid_loss                                           models/tsg_loss.py:57-61, plus an optional `exists` mask of the centroids
  grouping_loss_terms                                     FpsGroupingNetworkModel.get_loss (models/fps_grouping_network_model.py:8-24)
  tsegnet_centroid_loss_terms                             the three centroid terms of TSegNetModel.get_loss (models/tsegnet_model.py:15-24)

The reference loops over B x 16 teeth with boolean masks (one host round trip per tooth and scan) and sorts a (B, M, C) distance
matrix to read two columns; here a forward is the per-tooth counts and centroids (crops.label_centroids), a point pass and a finishing
kernel, a backward is one element-wise launch.  Nothing allocates inside the library, nothing synchronises, no float atomic: the same
inputs give the same bits, and forward plus backward can be captured in a graph.  Squared distances are the direct form (a-b).(a-b) in
float32 (the reference's |a|^2 + |b|^2 - 2ab cancels), sums across points are float64 rounded once.

Where the results differ from the reference on purpose:
  * a point the direction term does not keep (|offset| <= 0.0002), an exactly zero offset included, gets a ZERO direction gradient.
    The reference's autograd gives NaN for an exact zero: the excluded rows still pass through 0 / 0 in the backward of the division.
  * a scan with fewer than two valid teeth gives NaN for the chamfer term, where the reference raises (finding out needs a host read).
  * centroid_loss takes `exists` (B, C): absent centroids are skipped in both directions, so batches whose scans hold different teeth
    keep static shapes.  The reference compacts absent teeth away on the host, which pins it to batch 1.
  * an empty denominator gives NaN, as 0 / 0 does in the reference; the gradient of such a term is zero, not NaN.
A label outside [-1, 16) latches _lib.INDEX_ERROR_CROP on the stream, as crops.label_centroids does; it is neither cleared nor read here.

Arguments: floating tensors of any dtype and strides are cast and packed to contiguous float32 by differentiable torch operations in
front of the kernels, so the gradient comes back in the caller's dtype and layout; labels go through crops.labels_2d; anything else
raises TypeError / ValueError naming the argument before the library is touched; CPU tensors raise (no CPU fallback)."""
import torch
import torch.nn.functional as F
from torch.autograd import Function

from . import _lib, crops

_fwd = torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
_bwd = torch.amp.custom_bwd(device_type="cuda")

MAX_CENTROIDS = crops.NUM_LABELS     # tgn_centroid_loss_*'s limit
_SCALES = 2 * crops.NUM_LABELS + 1   # csrc/loss.hip: kLossScales


def _grads(*g):
    """The incoming gradients of the three loss values as one (3,) float32 device tensor (no host read)."""
    return torch.stack([x.reshape(()).to(torch.float32) for x in g]).contiguous()


class _TgnOffsetLosses(Function):
    """(offset_loss, dir_loss, chamf_loss) of packed float32 pred_offset, sample_xyz (B, 3, N) and int64 labels (B, N)."""

    @staticmethod
    @_fwd
    def forward(ctx, pred_offset, sample_xyz, labels):
        B, _, N = pred_offset.shape
        L, dev = _lib.ops(), pred_offset.device
        counts, cent = crops.label_centroids(sample_xyz, labels, crops.NUM_LABELS)
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        scales = torch.empty(B, _SCALES, dtype=torch.float32, device=dev)
        ws_bytes = L.tgn_offset_loss_workspace_bytes(B, N)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        L.tgn_offset_loss_forward(B, N, pred_offset, sample_xyz, labels, counts, cent, losses, scales, ws, ws_bytes, _lib.stream())
        ctx.save_for_backward(pred_offset, sample_xyz, labels, counts, cent, scales)
        return losses[0], losses[1], losses[2]

    @staticmethod
    @_bwd
    def backward(ctx, g_off, g_dir, g_chamf):
        pred_offset, sample_xyz, labels, counts, cent, scales = ctx.saved_tensors
        B, _, N = pred_offset.shape
        g = _grads(g_off, g_dir, g_chamf)
        grad = torch.empty_like(pred_offset)
        _lib.ops().tgn_offset_loss_backward(B, N, pred_offset, sample_xyz, labels, counts, cent, scales, g, grad, _lib.stream())
        return grad, None, None


class _CentroidLoss(Function):
    """(dist_loss, cent_loss, chamf_loss) of packed float32 pred_offset, sample_xyz (B, 3, M), distance (B, M), centroid (B, 3, C) and
    exists (B, C) uint8 or None."""

    @staticmethod
    @_fwd
    def forward(ctx, pred_offset, sample_xyz, distance, centroid, exists):
        B, _, M = pred_offset.shape
        C = centroid.shape[2]
        L, dev = _lib.ops(), pred_offset.device
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        scales = torch.empty(4, dtype=torch.float32, device=dev)
        rev_arg = torch.empty(B, MAX_CENTROIDS, dtype=torch.int32, device=dev)
        ws_bytes = L.tgn_centroid_loss_workspace_bytes(B)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        L.tgn_centroid_loss_forward(B, M, C, pred_offset, sample_xyz, distance, centroid, exists, losses, scales, rev_arg, ws, ws_bytes,
                                    _lib.stream())
        ctx.save_for_backward(pred_offset, sample_xyz, distance, centroid, exists, scales, rev_arg)
        return losses[0], losses[1], losses[2]

    @staticmethod
    @_bwd
    def backward(ctx, g_dist, g_cent, g_chamf):
        pred_offset, sample_xyz, distance, centroid, exists, scales, rev_arg = ctx.saved_tensors
        B, _, M = pred_offset.shape
        g = _grads(g_dist, g_cent, g_chamf)
        grad_offset, grad_distance = torch.empty_like(pred_offset), torch.empty_like(distance)
        _lib.ops().tgn_centroid_loss_backward(B, M, centroid.shape[2], pred_offset, sample_xyz, distance, centroid, exists, scales, rev_arg, g,
                                              grad_offset, grad_distance, _lib.stream())
        return grad_offset, None, grad_distance, None, None


def _channel_first(t, what, B=None, N=None):
    """A floating (B, 3, N) tensor of any dtype and strides, or an error that names it.  Returns its shape."""
    if not isinstance(t, torch.Tensor) or not t.is_floating_point():
        raise TypeError(f"{what} must be a floating-point tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if t.dim() != 3 or t.shape[1] != 3:
        raise ValueError(f"{what} must be channel-first (B, 3, N), got {tuple(t.shape)}")
    if B is not None and (t.shape[0] != B or t.shape[2] != N):
        raise ValueError(f"{what} must be ({B}, 3, {N}) like pred_offset, got {tuple(t.shape)}")
    return t.shape[0], t.shape[2]


def _tgn_operands(pred_offset, sample_xyz, gt_seg_label):
    B, N = _channel_first(pred_offset, "pred_offset")
    _channel_first(sample_xyz, "sample_xyz", B, N)
    try:
        labels = crops.labels_2d(gt_seg_label, B, N, (torch.int32, torch.int64))
    except (TypeError, ValueError) as e:
        raise type(e)(f"gt_seg_label: {e}") from None
    _lib.require_cuda(pred_offset, sample_xyz, labels)
    return _lib.f32c(pred_offset), _lib.f32c(sample_xyz.detach()), labels


def tgn_offset_losses(pred_offset, sample_xyz, gt_seg_label):
    """pred_offset, sample_xyz (B, 3, N) floating; gt_seg_label (B, N) or (B, 1, N), int32 or int64, -1 = gingiva, teeth 0..15 ->
    (offset_loss, dir_loss, chamf_loss), float32 scalars: batch_center_offset_loss's two values and batch_chamfer_distance_loss's,
    from one forward and one backward pass.  sample_xyz and the labels get no gradient.  No synchronisation."""
    return _TgnOffsetLosses.apply(*_tgn_operands(pred_offset, sample_xyz, gt_seg_label))


def batch_center_offset_loss(pred_offset, sample_xyz, gt_seg_label):
    """models/tgn_loss.py:6-61 -> (offset_loss, dir_loss).  A caller that wants the chamfer term too saves a pass with tgn_offset_losses."""
    return tgn_offset_losses(pred_offset, sample_xyz, gt_seg_label)[:2]


def batch_chamfer_distance_loss(pred_offset, sample_xyz, gt_seg_label):
    """models/tgn_loss.py:263-302 -> chamf_loss."""
    return tgn_offset_losses(pred_offset, sample_xyz, gt_seg_label)[2]


def centroid_loss(pred_offset, sample_xyz, distance, centroid, exists=None):
    """models/tsg_loss.py:57-61: pred_offset, sample_xyz (B, 3, M), distance of B * M elements in any shape (the network gives (B, 1, M)),
    centroid (B, 3, C) with C <= 16, exists (B, C) bool or None (every centroid exists) -> (dist_loss, cent_loss, chamf_loss), float32
    scalars.  Gradients reach pred_offset and distance.  No synchronisation."""
    B, M = _channel_first(pred_offset, "pred_offset")
    _channel_first(sample_xyz, "sample_xyz", B, M)
    if not isinstance(distance, torch.Tensor) or not distance.is_floating_point():
        raise TypeError(f"distance must be a floating-point tensor, got {getattr(distance, 'dtype', type(distance).__name__)}")
    if distance.numel() != B * M:
        raise ValueError(f"distance must hold B * M = {B * M} elements, got {tuple(distance.shape)}")
    if not isinstance(centroid, torch.Tensor) or not centroid.is_floating_point():
        raise TypeError(f"centroid must be a floating-point tensor, got {getattr(centroid, 'dtype', type(centroid).__name__)}")
    if centroid.dim() != 3 or centroid.shape[0] != B or centroid.shape[1] != 3 or not 1 <= centroid.shape[2] <= MAX_CENTROIDS:
        raise ValueError(f"centroid must be ({B}, 3, C) with 1 <= C <= {MAX_CENTROIDS}, got {tuple(centroid.shape)}")
    if exists is not None:
        if not isinstance(exists, torch.Tensor) or exists.dtype != torch.bool:
            raise TypeError(f"exists must be a bool tensor or None, got {getattr(exists, 'dtype', type(exists).__name__)}")
        if tuple(exists.shape) != (B, centroid.shape[2]):
            raise ValueError(f"exists must be (B, C) = ({B}, {centroid.shape[2]}), got {tuple(exists.shape)}")
    _lib.require_cuda(pred_offset, sample_xyz, distance, centroid, exists)
    mask = None if exists is None else exists.to(torch.uint8).contiguous()
    return _CentroidLoss.apply(_lib.f32c(pred_offset), _lib.f32c(sample_xyz.detach()), _lib.f32c(distance.reshape(B, M)), _lib.f32c(centroid.detach()), mask)


def grouping_loss_terms(output, gt_seg_label, input_coords):
    """FpsGroupingNetworkModel.get_loss (models/fps_grouping_network_model.py:8-24) on the output dict of nets.GroupingNetworkModule:
    {"tooth_class_loss_1", "tooth_class_loss_2", "offset_1_loss", "offset_1_dir_loss", "chamf_1_loss"}, unweighted.  The two class
    terms are tooth_class_loss = cross entropy on label + 1 (tgn_loss.py:355-372) with the half-jaw labels for the first stage and the
    binary crop labels for the second; the three geometric terms come from tgn_offset_losses.  gt_seg_label is not modified."""
    B, N = _channel_first(output["offset_1"], "output['offset_1']")
    try:
        labels = crops.labels_2d(gt_seg_label, B, N, (torch.int32, torch.int64))
    except (TypeError, ValueError) as e:
        raise type(e)(f"gt_seg_label: {e}") from None
    half = torch.where(labels >= 9, labels - 8, labels)
    crop_labels = output["cluster_gt_seg_label"].reshape(output["sem_2"].shape[0], -1).long()
    crop_labels = torch.where(crop_labels >= 0, torch.zeros_like(crop_labels), crop_labels)
    offset_loss, dir_loss, chamf_loss = tgn_offset_losses(output["offset_1"], input_coords, labels)
    return {"tooth_class_loss_1": F.cross_entropy(output["sem_1"].float(), half + 1),
            "tooth_class_loss_2": F.cross_entropy(output["sem_2"].float(), crop_labels + 1),
            "offset_1_loss": offset_loss, "offset_1_dir_loss": dir_loss, "chamf_1_loss": chamf_loss}


def tsegnet_centroid_loss_terms(outputs, centroid_coords, exists=None):
    """The centroid terms of TSegNetModel.get_loss (models/tsegnet_model.py:15-24) on the output dict of the centroid network:
    {"dist_loss", "cent_loss", "chamf_loss"}, unweighted.  centroid_coords (B, 3, C); with `exists` (B, C) the 16 slots of
    ops_utils.seg_label_to_cent can be passed as they are instead of compacted on the host."""
    dist_loss, cent_loss, chamf_loss = centroid_loss(outputs["offset_result"], outputs["l3_xyz"], outputs["dist_result"], centroid_coords, exists)
    return {"dist_loss": dist_loss, "cent_loss": cent_loss, "chamf_loss": chamf_loss}
