"""The geometric training losses of tgnet_fps and tsegnet as fused HIP kernels (csrc/loss.hip, include/tgn_pointops.h):

  batch_center_offset_loss, batch_chamfer_distance_loss   models/tgn_loss.py:6-61, 263-302 (names and argument order kept)
  tgn_offset_losses                                       all three terms of the two above from ONE forward and ONE backward pass
  centroid_loss                                           models/tsg_loss.py:57-61, plus an optional `exists` mask of the centroids
  grouping_loss_terms                                     FpsGroupingNetworkModel.get_loss (models/fps_grouping_network_model.py:8-24)
  tsegnet_centroid_loss_terms                             the three centroid terms of TSegNetModel.get_loss (models/tsegnet_model.py:15-24)
  first_seg_loss, second_seg_loss, id_loss,               models/tsg_loss.py:63-135 (names and argument order kept): torch compositions with
  segmentation_loss                                       autograd over crops x 3072 elements, no kernel of their own
  seg_label_to_cent                                       ops_utils.seg_label_to_cent through crops.label_centroids: 16 slots and an `exists` mask
  tsegnet_loss_terms                                      all six terms of TSegNetModel.get_loss from the module's output dict and the labels
  contrast_boundary_stage, contrast_boundary_loss         the contrastive-boundary criterion (models/modules/cbl_point_transformer/heads.py:63-253
                                                          with default.yaml's configuration): the neighbour lists are tgn_knnquery*, the
                                                          (m, K-1, 32) latent differences and their gradient tgn_subtraction_forward / _backward
  contrast_boundary_lists,                                the same stage as two fused kernels (csrc/cbl.hip: tgn_cbl_stage_forward / _backward) that
  contrast_boundary_stage_fused                           never form the difference tensor and whose gradient is bit-reproducible (summed along
                                                          ordered.reverse_lists): behind contrast_boundary_loss(fused=True), off by default

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
import numpy as np
import torch
import torch.nn.functional as F
from torch.autograd import Function

from . import _lib, crops, ordered, pointops

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
        # the float64-summed mean: numpy's float32 sum is off by about sqrt(points of the tooth) roundings, which the gradients
        # 2 (m - c) see magnified by |c| / |m - c| (the reference takes torch's mean, a tree sum)
        counts, cent = crops.label_centroids(sample_xyz, labels, crops.NUM_LABELS, f64_sum=True)
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


def _class_cross_entropy(logits, target):
    """Cross entropy of (B, C, N) logits against (B, N) classes.  torch's CUDA kernel for this layout (nll_loss2d) adds its terms with
    float atomics and has no deterministic form: under torch.use_deterministic_algorithms (training.set_reproducible) it raises.  There
    the same mean is taken over the (B N, C) rows, whose kernel reduces in a fixed order: the same value up to the order of its sum."""
    if torch.are_deterministic_algorithms_enabled():
        return F.cross_entropy(logits.permute(0, 2, 1).reshape(-1, logits.shape[1]), target.reshape(-1))
    return F.cross_entropy(logits, target)


def tooth_class_loss(cls_pred, gt_cls):
    """tgn_loss.py:355-367 without weights / smoothing: cross entropy of (B, 17, N) logits against labels shifted by one
    (gingiva -1 -> class 0)"""
    b = gt_cls.shape[0]
    return _class_cross_entropy(cls_pred.float(), gt_cls.view(b, -1).long() + 1)


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
    return {"tooth_class_loss_1": _class_cross_entropy(output["sem_1"].float(), half + 1),
            "tooth_class_loss_2": _class_cross_entropy(output["sem_2"].float(), crop_labels + 1),
            "offset_1_loss": offset_loss, "offset_1_dir_loss": dir_loss, "chamf_1_loss": chamf_loss}


def first_seg_loss(pred_mask_1, pred_weight_1, gt_bin_label):
    """models/tsg_loss.py:63-75: pred_mask_1 (T, 2, k), the first mask head's softmax; pred_weight_1 (T, 1, k) confidence logits;
    gt_bin_label (T, 1, k), 1 inside the tooth -> mean((nll * w)^2 + (1 - w)^2) with w = sigmoid(pred_weight_1) and nll the reference's
    NLLLoss of the PROBABILITIES (minus the probability of the true class, not its logarithm: the reference's own choice, kept)."""
    T = gt_bin_label.shape[0]
    target = gt_bin_label.reshape(T, 1, -1).long()
    nll = -pred_mask_1.gather(1, target)[:, 0]
    w = torch.sigmoid(pred_weight_1).reshape(T, -1)
    return torch.mean((nll * w) ** 2 + (1 - w) ** 2)


def second_seg_loss(pred_mask_2, pred_weight_1, gt_bin_label):
    """models/tsg_loss.py:92-104: pred_mask_2 (T, 1, k) mask logits -> mean((2 - w) * binary cross entropy with logits)."""
    T = gt_bin_label.shape[0]
    bce = F.binary_cross_entropy_with_logits(pred_mask_2.reshape(T, -1), gt_bin_label.reshape(T, -1).to(torch.float32), reduction="none")
    w = torch.sigmoid(pred_weight_1).reshape(T, -1)
    return torch.mean((2.0 - w) * bce)


def id_loss(gt_label, pred_id):
    """models/tsg_loss.py:122-128: gt_label, T tooth ids 1..16 in any shape and integer or float dtype; pred_id (T, 17) logits -> cross entropy."""
    return F.cross_entropy(pred_id, gt_label.reshape(-1).long())


def segmentation_loss(pd_1, weight_1, pd_2, id_pred, pred_cluster_gt_ids, pred_cluster_gt_points_bin_labels):
    """models/tsg_loss.py:130-135 -> (seg_1_loss, seg_2_loss, id_pred_loss).  Torch compositions with autograd, on whatever device the
    tensors live: crops x 3072 elements, nothing a kernel would win."""
    return (first_seg_loss(pd_1, weight_1, pred_cluster_gt_points_bin_labels),
            second_seg_loss(pd_2, weight_1, pred_cluster_gt_points_bin_labels),
            id_loss(pred_cluster_gt_ids, id_pred))


def seg_label_to_cent(feats_xyz, gt_seg_label):
    """ops_utils.seg_label_to_cent on the GPU: feats_xyz (B, 3, N) floating (more channels are ignored), gt_seg_label (B, N) or
    (B, 1, N) int32 or int64, -1 = gingiva -> (centroid (B, 3, 16) float32, exists (B, 16) bool): the mean of every tooth's points
    (crops.label_centroids: one launch, no loop over the teeth, no host synchronisation) and whether the tooth has a point.  An absent
    tooth's column is zero where the reference writes (-10, -10, -10): `exists` carries the information, as centroid_loss takes it.
    The reference flattens the batch and is meaningful for B = 1; here every scan has its own 16 slots."""
    if not isinstance(feats_xyz, torch.Tensor) or not feats_xyz.is_floating_point():
        raise TypeError(f"feats_xyz must be a floating-point tensor, got {getattr(feats_xyz, 'dtype', type(feats_xyz).__name__)}")
    if feats_xyz.dim() != 3 or feats_xyz.shape[1] < 3:
        raise ValueError(f"feats_xyz must be channel-first (B, C >= 3, N), got {tuple(feats_xyz.shape)}")
    B, _, N = feats_xyz.shape
    try:
        labels = crops.labels_2d(gt_seg_label, B, N, (torch.int32, torch.int64))
    except (TypeError, ValueError) as e:
        raise type(e)(f"gt_seg_label: {e}") from None
    _lib.require_cuda(feats_xyz, labels)
    counts, cent = crops.label_centroids(_lib.f32c(feats_xyz.detach()), labels, crops.NUM_LABELS)
    exists = counts > 0
    return torch.where(exists[:, :, None], cent, torch.zeros_like(cent)).permute(0, 2, 1), exists


def _stacked_centres(center_points, B, dev):
    """TSegNetModule's `center_points` -- a (1, T, 3) array for B = 1, a list over scans of (1, T_b, 3) arrays otherwise -> ((T, 3) float32
    on dev, (T,) int64 scan of every centre)."""
    per_scan = [center_points] if B == 1 and not isinstance(center_points, (list, tuple)) else list(center_points)
    if len(per_scan) != B:
        raise ValueError(f"center_points must hold the centres of {B} scans, got {len(per_scan)}")
    flat = [c.reshape(-1, 3) if isinstance(c, torch.Tensor) else np.asarray(c, np.float32).reshape(-1, 3) for c in per_scan]
    cent, scan, _ = crops.stack_centres(flat, B, dev, "center_points")
    return cent, scan.to(torch.int64)


def tsegnet_crop_targets(center_points, centroid, exists, cluster_gt_seg_label):
    """The targets of tsegnet's segmentation terms (models/tsegnet_model.py:26-32): every crop centre (T, 3) is assigned to the nearest
    EXISTING ground-truth centroid of its own scan (float32 direct-form squared distance, argmin: the first slot on a tie); the crop's
    tooth id is that slot + 1, its binary labels are cluster_gt_seg_label + 1 == id.  centroid (B, 3, 16), exists (B, 16) as
    seg_label_to_cent gives them -> (ids (T,) int64, bin_labels (T, 1, k) int64).  Plain torch on the tensors' device; the reference
    indexes scan 0 for every crop, which is the same for B = 1."""
    B = centroid.shape[0]
    cent, scan = _stacked_centres(center_points, B, centroid.device)
    diff = cent[:, :, None] - centroid.detach().to(torch.float32)[scan]                      # (T, 3, 16)
    d = (diff * diff).sum(1)
    d = torch.where(exists[scan], d, torch.full_like(d, float("inf")))
    ids = d.argmin(dim=1) + 1
    return ids, (cluster_gt_seg_label + 1 == ids[:, None, None]).to(torch.int64)


def tsegnet_segmentation_loss_terms(outputs, centroid, exists):
    """The three segmentation terms of TSegNetModel.get_loss (models/tsegnet_model.py:25-40) on nets.TSegNetModule's output dict and
    the 16 centroid slots of seg_label_to_cent: {"seg_1_loss", "seg_2_loss", "id_pred_loss"}, unweighted."""
    ids, bin_labels = tsegnet_crop_targets(outputs["center_points"], centroid, exists, outputs["cluster_gt_seg_label"])
    seg_1, seg_2, id_pred = segmentation_loss(outputs["pd_1"], outputs["weight_1"], outputs["pd_2"], outputs["id_pred"], ids, bin_labels)
    return {"seg_1_loss": seg_1, "seg_2_loss": seg_2, "id_pred_loss": id_pred}


def tsegnet_loss_terms(outputs, gt_seg_label):
    """TSegNetModel.get_loss and the label work of TSegNetModel.step (models/tsegnet_model.py:14-60) on nets.TSegNetModule's output dict
    and the (B, 1, N) labels: always {"dist_loss", "cent_loss", "chamf_loss"} (fused kernels, the 16 slots passed with `exists`
    instead of compacted on the host) and, when the dict has the segmentation outputs, {"seg_1_loss", "seg_2_loss", "id_pred_loss"}.
    Unweighted: the reference's weights (1, 1, 0.1, 1, 1, 1) are the step class's.  For B > 1, where the reference indexes scan 0 and
    means nothing, every scan's crops are assigned against that scan's own centroids."""
    centroid, exists = seg_label_to_cent(outputs["l0_xyz"], gt_seg_label)
    terms = tsegnet_centroid_loss_terms(outputs, centroid, exists)
    if "pd_1" in outputs:
        terms.update(tsegnet_segmentation_loss_terms(outputs, centroid, exists))
    return terms


def tsegnet_centroid_loss_terms(outputs, centroid_coords, exists=None):
    """The centroid terms of TSegNetModel.get_loss (models/tsegnet_model.py:15-24) on the output dict of the centroid network:
    {"dist_loss", "cent_loss", "chamf_loss"}, unweighted.  centroid_coords (B, 3, C); with `exists` (B, C) the 16 slots of
    ops_utils.seg_label_to_cent can be passed as they are instead of compacted on the host."""
    dist_loss, cent_loss, chamf_loss = centroid_loss(outputs["offset_result"], outputs["l3_xyz"], outputs["dist_result"], centroid_coords, exists)
    return {"dist_loss": dist_loss, "cent_loss": cent_loss, "chamf_loss": chamf_loss}


# ---- the contrastive-boundary criterion -----------------------------------------------------------------------------------------------

CBL_WEIGHT = 0.1      # default.yaml `weight: w.1`
CBL_EPS = 1e-12       # basic_operators._eps
_VOTE_BASE = 1 << 20  # stage_vote packs (count, label) into one int64: labels stay below it


def stage_vote(p0, o0, p, o, target, kr):
    """The labels of a coarser decoder stage (basic_operators.get_subscene_label and the arg-max of heads.posmask_cnt): every point of
    (p, o) takes the `kr` nearest stage-0 points of its own scan (knnquery(kr, p0, p, o0, o)); the reference averages their one-hot
    targets and takes the arg-max.  The averaged counts are small integers over the same kr, so that is a majority vote, computed here
    on integers; equal counts go to the LOWEST label (the first maximum, what the reference's CPU arg-max returns), stated here instead
    of left to the device's arg-max.  target (n,) int64 in [0, 2^20) -> (m,) int64.  No synchronisation."""
    idx = pointops.knn_indices(kr, p0, p, o0, o).long()
    votes = target[idx]                                                     # (m, kr)
    if kr == 1:
        return votes[:, 0]
    count = (votes[:, :, None] == votes[:, None, :]).sum(2)                 # (m, kr): how often slot j's label occurs in the row
    key = count * _VOTE_BASE + (_VOTE_BASE - 1 - votes)                     # the largest count first, then the lowest label
    return _VOTE_BASE - 1 - key.max(1).values % _VOTE_BASE


def contrast_boundary_stage(p, f, o, stage_labels, nsample):
    """heads.ContrastHead.point_contrast for one decoder stage: p (m, 3), latent features f (m, C), offsets o (b), integer labels
    stage_labels (m,), nsample = K -> (loss, count): the soft nearest-neighbour contrast -log(sum_j e_ij [label_j == label_i] /
    sum_j e_ij + 1e-12) with e_ij = exp(-d_ij + min_j d_ij), d_ij = sqrt(|f_i - f_j|^2 + 1e-12) over the K - 1 columns 1.. of
    knnquery(K, p, p, o, o) -- column 0 is dropped whatever it holds, and the slots a scan shorter than K leaves are its first
    point, as in the reference -- averaged over the points that have both a neighbour of their own label and one of another, times
    0.1; `count` is the number of such points, an int64 device scalar.

    Static shapes: points outside the mask are skipped with torch.where and get a zero gradient, the mean is sum / max(count, 1), so
    a stage without such a point gives 0 (the reference returns 0.0 for stages >= 1 and raises at stage 0).  The differences
    f_i - f_idx[i, j] are pointops.subtraction (tgn_subtraction_forward; the gradient is tgn_subtraction_backward's float atomics), so
    no gathered copy of the neighbour features is kept beside the (m, K-1, C) difference tensor.  The rest is float32 torch on (m, K-1).
    No synchronisation; forward and backward can be captured in a graph."""
    K1 = int(nsample) - 1
    if K1 < 1:
        raise ValueError(f"nsample must be at least 2 (one neighbour beside the dropped column 0), got {nsample}")
    lab = stage_labels.reshape(-1).long()
    if lab.shape[0] != p.shape[0] or f.shape[0] != p.shape[0]:
        raise ValueError(f"p, f and stage_labels must hold the same number of points, got {p.shape[0]}, {f.shape[0]} and {lab.shape[0]}")
    idx = pointops.knn_indices(int(nsample), p, p, o, o)[:, 1:].contiguous()            # (m, K-1) int32
    posmask = lab[idx.long()] == lab[:, None]
    npos = posmask.sum(1)
    point_mask = (npos > 0) & (npos < K1)
    diff = pointops.subtraction(f, f, idx)                                               # (m, K-1, C) float32
    z = -torch.sqrt((diff * diff).sum(2) + CBL_EPS)
    e = torch.exp(z - z.max(1, keepdim=True).values)
    neg = e.sum(1)
    pos = torch.where(point_mask, (e * posmask).sum(1), neg)                             # unmasked rows: log(1 + eps), a finite backward
    per_point = -torch.log(pos / neg + CBL_EPS)
    count = point_mask.sum()
    total = torch.where(point_mask, per_point, torch.zeros_like(per_point)).sum()
    return total / count.clamp(min=1).to(total.dtype) * CBL_WEIGHT, count


CBL_FUSED_MAX_K1 = 63        # csrc/cbl.hip: kCblMaxK1, one lane of a wave per neighbour slot
CBL_FUSED_MAX_C = 128        # kCblMaxC; and C a multiple of 4
CBL_FUSED_BLOCK_POINTS = 16  # kCblPointsPerBlock: the points one workgroup of the forward takes (a partial sum each)


class _CblStage(Function):
    """(loss, count) of packed float32 f (m, C), int32 idx (m, k1) and int64 labels (m,)."""

    @staticmethod
    @_fwd
    def forward(ctx, f, idx, labels):
        m, c = f.shape
        k1 = idx.shape[1]
        L, dev = _lib.ops(), f.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        pair_w = torch.empty(m, k1, dtype=torch.float32, device=dev)
        ws_bytes = L.tgn_cbl_stage_workspace_bytes(m)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        # the lists the backward gathers along: row i's are the pair numbers q = i' * k1 + j with idx[i', j] == i, ascending
        lists = ordered.reverse_lists(idx, m) if ctx.needs_input_grad[0] else ()
        L.tgn_cbl_stage_forward(m, k1, c, f, idx, labels, loss, count, pair_w, ws, ws_bytes, _lib.stream())
        if lists:
            ctx.save_for_backward(f, idx, pair_w, count, *lists)
        n = count[0]
        ctx.mark_non_differentiable(n)
        return loss[0], n

    @staticmethod
    @_bwd
    def backward(ctx, g_loss, _g_count):
        f, idx, pair_w, count, rev_start, rev_pair = ctx.saved_tensors
        m, c = f.shape
        g = g_loss.reshape(1).to(torch.float32).contiguous()
        grad = torch.empty_like(f)
        _lib.ops().tgn_cbl_stage_backward(m, idx.shape[1], c, f, idx, pair_w, count, rev_start, rev_pair, g, grad, _lib.stream())
        return grad, None, None


def _cbl_fused_supported(c, k1):
    return 1 <= k1 <= CBL_FUSED_MAX_K1 and 4 <= c <= CBL_FUSED_MAX_C and c % 4 == 0


def contrast_boundary_lists(f, idx, labels):
    """One stage of the criterion on neighbour lists the caller supplies, as fused kernels: latent features f (m, C) floating, idx
    (m, k1) integer -- the lists WITHOUT their column 0 -- and integer labels (m,) -> (loss, count) as contrast_boundary_stage defines
    them.  The (m, k1, C) differences are never formed: the forward keeps one (m, k1) float32 weight per pair, the backward gathers
    every row's gradient along ordered.reverse_lists(idx, m) without float atomics, so loss, count AND gradient are the same bits for the same
    inputs.  1 <= k1 <= 63, C a multiple of 4 in 4..128 and m * k1 < 2^31, otherwise ValueError; an index outside [0, m) reads point 0
    and latches _lib.INDEX_ERROR_GATHER on the stream.  No synchronisation; forward and backward can be captured in a graph."""
    f = _lib.f32c(f, "f")
    idx = _lib.idx32c(idx, "idx")
    if not isinstance(labels, torch.Tensor) or labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
        raise TypeError(f"labels must be an integer tensor, got {getattr(labels, 'dtype', type(labels).__name__)}")
    if f.dim() != 2:
        raise ValueError(f"f must be (m, C), got {tuple(f.shape)}")
    m, c = f.shape
    if idx.dim() != 2 or idx.shape[0] != m:
        raise ValueError(f"idx must be (m, k1) with m = {m} like f, got {tuple(idx.shape)}")
    if labels.numel() != m:
        raise ValueError(f"labels must hold one label per point ({m}), got {tuple(labels.shape)}")
    k1 = idx.shape[1]
    if not _cbl_fused_supported(c, k1) or m * k1 >= 2 ** 31:
        raise ValueError(f"f (m, C) = {tuple(f.shape)} and idx (m, k1) = {tuple(idx.shape)}: the fused stage needs 1 <= k1 <= {CBL_FUSED_MAX_K1}, "
                         f"C a multiple of 4 with 4 <= C <= {CBL_FUSED_MAX_C} and m * k1 < 2^31")
    _lib.require_cuda(f, idx, labels)
    return _CblStage.apply(f, idx, labels.reshape(-1).long().contiguous())


def contrast_boundary_stage_fused(p, f, o, stage_labels, nsample):
    """contrast_boundary_stage with the part behind the neighbour search as fused kernels (contrast_boundary_lists): the same arguments,
    the same (loss, count), the same lists pointops.knn_indices(K, p, p, o, o)[:, 1:].  Against contrast_boundary_stage the peak memory
    loses the (m, K-1, C) tensor it holds up to 2.5 times, and the gradient is bit-reproducible; the values agree to float32 rounding
    (another, fixed, order of the same sums).  A latent width or an nsample outside the kernels' range (C a multiple of 4 in 4..128,
    2 <= nsample <= 64) goes through contrast_boundary_stage."""
    K1 = int(nsample) - 1
    if K1 < 1:
        raise ValueError(f"nsample must be at least 2 (one neighbour beside the dropped column 0), got {nsample}")
    if not _cbl_fused_supported(f.shape[-1], K1):
        return contrast_boundary_stage(p, f, o, stage_labels, nsample)
    lab = stage_labels.reshape(-1)
    if lab.shape[0] != p.shape[0] or f.shape[0] != p.shape[0]:
        raise ValueError(f"p, f and stage_labels must hold the same number of points, got {p.shape[0]}, {f.shape[0]} and {lab.shape[0]}")
    idx = pointops.knn_indices(int(nsample), p, p, o, o)[:, 1:].contiguous()            # (m, K-1) int32
    return contrast_boundary_lists(f, idx, lab)


def contrast_boundary_loss(up_points, latents, target, nsample, stride, fused=False):
    """heads.ContrastHead.forward over the decoder stages (`stage: Ua`): up_points = [[p_i, o_i], ...], latents = [f_i (m_i, 32), ...],
    target (n_0,) integer, already + 1 (cbl_point_transformer_module.py:200-202) -> (losses (stages,), counts (stages,) int64).  Stage 0
    is labelled by the target itself, stage i >= 1 by stage_vote with kr = prod(stride[:i]) (get_model sets nstride = stride).
    fused=True: every stage through contrast_boundary_stage_fused instead of contrast_boundary_stage."""
    if len(up_points) != len(latents):
        raise ValueError(f"{len(up_points)} stages of points and {len(latents)} of latent features")
    target = target.reshape(-1).long()
    p0, o0 = up_points[0]
    if target.shape[0] != p0.shape[0]:
        raise ValueError(f"target must hold one label per stage-0 point ({p0.shape[0]}), got {target.shape[0]}")
    stage = contrast_boundary_stage_fused if fused else contrast_boundary_stage
    stage_losses, counts = [], []
    for i, ((p, o), f) in enumerate(zip(up_points, latents)):
        labels = target if i == 0 else stage_vote(p0, o0, p, o, target, int(np.prod(stride[:i])))
        loss, count = stage(p, f, o, labels, nsample[i])
        stage_losses.append(loss)
        counts.append(count)
    return torch.stack(stage_losses), torch.stack(counts)
