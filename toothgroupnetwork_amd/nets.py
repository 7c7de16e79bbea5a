"""Whole-network compositions of the drop-in modules, state_dict-compatible with the reference's networks.

The reference's own model files import this package's operators unchanged; these mirrors exist for the
places where the reference checkout is not available -- the GPU box's parity tests and benches -- and as the entry points
of the fused eval paths.  Parameter names and shapes equal the reference classes', so trained weights load into them
(tests/test_host_logic.py compares the key lists with the reference's own classes in the build container):

  PointNetPPSeg        models/modules/pointnet_pp.py:6-70 (`get_model`): three multi-scale set-abstraction levels, three
                       feature-propagation levels, offset / distance / class heads; BASELINE.json config 2's network.
  TsgCentroidNet       models/modules/tsg_centroid_module.py:5-46 and
  TsgSegNet            models/modules/tsg_seg_module.py:4-80 -- the two modules of tsegnet (models/modules/tsegnet.py:15-16, the network behind
                       models/tsegnet_model.py): PointNet++-MSG trunks; the second one ends in the ONLY PointNetSetAbstraction(group_all=True)
                       of the reference (`flatten_sa`, :28).
  PointTransformerSeg  models/modules/cbl_point_transformer/cbl_point_transformer_module.py:28-216 with the configuration
                       the reference ships (default.yaml: five stages, `multi` heads over the decoder stages, latent
                       features concatenated); BASELINE.json configs 3 / 4's network.  forward(contrast=True) adds the
                       contrastive-boundary criterion of training (heads.py:62-253) as losses.contrast_boundary_loss.
  DGCnnModule          models/modules/dgcnn.py:43-143 (the "dgcnn" model): three EdgeConv levels over feature-space kNN graphs,
                       fused in eval mode (dgcnn.py of this package, re-exported here).
  PointFirstModule     models/modules/pointnet.py:49-68 (the "pointnet" model): PointNet at scale 2 with both transform regressors;
                       its three linear + max-over-points layers are one fp32-MFMA kernel in eval mode (pointnet.py of this
                       package, re-exported here).
  GroupingNetworkModule  models/modules/grouping_network_module.py:7-101, tgnet_fps's network (train_configs/tgnet_fps.py): a
                       PointTransformerSeg over the scan, on-device tooth crops (crops.tooth_crops), a second PointTransformerSeg over
                       all crops as one batch.  Without labels the centroids come from on-device clustering (cluster.py, which
                       reaches crop.hip's kNN and label means through crops.py).  The offset, direction and chamfer terms of its loss are
                       losses.grouping_loss_terms (fused kernels, csrc/loss.hip); forward(contrast=True) adds cbl_loss_1 / cbl_loss_2.
                       `block_num` 5 (tgnet_fps, tgnet's first module) or 2 (tgnet's boundary module,
                       inference_pipeline_maker.py:43-54); up to crops.MAX_CLUSTERS labels.
  PointPpFirstModule, PointTransformerModule  models/modules/pointnet_pp.py:73-92 and models/modules/point_transformer.py:4-28: the wrappers
                       whose state_dict the "pointnetpp" and "pointtransformer" checkpoints hold (inference.make_inference_pipeline).
  TSegNetModule        models/modules/tsegnet.py:10-88 (the "tsegnet" model): TsgCentroidNet, the join on the GPU (tsegnet.py of this
                       package: proposal filter, DBSCAN, cluster means, crops with the distance feature; the means and the crops'
                       kNN through crops.py's wrappers of crop.hip), TsgSegNet over the crops.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

import functools

import numpy as np

from . import _lib, cluster as _cluster, crops as _crops, fold, losses as _losses, point_transformer as PT, pointops, tsegnet as _tsg
from .dgcnn import DGCnnModule  # noqa: F401
from .pointnet import PointFirstModule  # noqa: F401
from .pointnet2_utils import PointNetFeaturePropagation, PointNetSetAbstraction, PointNetSetAbstractionMsg, linear_relu, square_distance


def _one_index_check(forward):
    """The gather kernels latch out-of-range indices in a device word that the checked operators read back after their launch -- a
    stream synchronisation each (the price of raising IndexError like torch's advanced indexing, pointnet2_utils.py:56-60).  A whole
    network forward issues six to twelve of them, and at the small levels the GPU then idles behind the host (~0.4 ms of a 4.9 ms
    PointNet++ forward, profiles/r05_pnpp_forward_sequence.txt): the network mirrors read the word ONCE, when the forward is
    through.  The IndexError is the same; it is raised at the end of the forward instead of inside the offending level."""
    @functools.wraps(forward)
    def wrapped(self, *args, **kwargs):
        with _lib.deferred_index_check(type(self).__name__ + " forward"):
            return forward(self, *args, **kwargs)
    return wrapped


def fold_head(conv1, bn1, conv2):
    """(W1', b1', W2, b2) of a prediction head Conv1d(1x1) + eval-mode BatchNorm1d + ReLU + Conv1d(1x1)."""
    return fold.affine(conv1, bn1) + fold.affine(conv2)


class PointNetPPSeg(nn.Module):
    def __init__(self, input_feature_num=6, scale=4, cls_pred=True):
        super().__init__()
        s, self.cls_pred = scale, cls_pred
        self.sa1 = PointNetSetAbstractionMsg(1024, [0.025, 0.05], [32, 64], input_feature_num, [[32 * s, 32 * s]] * 2)
        self.sa2 = PointNetSetAbstractionMsg(512, [0.05, 0.1], [32, 64], 64 * s, [[64 * s, 128 * s]] * 2)
        self.sa3 = PointNetSetAbstractionMsg(256, [0.1, 0.2], [32, 64], 256 * s, [[196 * s, 256 * s]] * 2)
        self.fp3 = PointNetFeaturePropagation(768 * s, [256 * s, 256 * s])
        self.fp2 = PointNetFeaturePropagation(320 * s, [128 * s, 128 * s])
        self.fp1 = PointNetFeaturePropagation(128 * s + input_feature_num, [64 * s, 32 * s])
        for head, width in (("offset", 3), ("dist", 1)):
            setattr(self, f"{head}_conv_1", nn.Conv1d(32 * s, 16, 1))
            setattr(self, f"{head}_bn_1", nn.BatchNorm1d(16))
        self.offset_conv_2, self.dist_conv_2 = nn.Conv1d(16, 3, 1), nn.Conv1d(16, 1, 1)
        if cls_pred:
            self.cls_conv_1, self.cls_bn_1, self.cls_conv_2 = nn.Conv1d(32 * s, 17, 1), nn.BatchNorm1d(17), nn.Conv1d(17, 17, 1)
        nn.init.zeros_(self.offset_conv_2.weight)
        nn.init.zeros_(self.dist_conv_2.weight)
        self.conv1, self.bn1 = nn.Conv1d(32, 16, 1), nn.BatchNorm1d(16)     # declared and unused in the reference too (:38-40)

    def _head(self, name, x):
        conv1, bn1, conv2 = getattr(self, f"{name}_conv_1"), getattr(self, f"{name}_bn_1"), getattr(self, f"{name}_conv_2")
        if fold.frozen(self, x) and x.dtype == torch.float32:
            # eval: on channel-last rows (x arrives as the channel-first view of a channel-last tensor, so the permute is free), the
            # BatchNorm folded into the first 1x1 convolution (memoised): two GEMMs with bias, no layout copies of the (B, C, N) features
            W1, b1, W2, b2 = fold_head(conv1, bn1, conv2)
            y = linear_relu(x.permute(0, 2, 1), W1, b1)       # (ReLU in the GEMM's epilogue where the rows are contiguous)
            return F.linear(y, W2, b2).permute(0, 2, 1)
        return conv2(F.relu(bn1(conv1(x))))

    @_one_index_check
    def forward(self, xyz_in):
        """xyz_in: [features (B, C, N)] with xyz in the first three channels -> the reference's output list
        [l0_points, l3_points, l0_xyz, l3_xyz, offset, dist(, cls)] (pointnet_pp.py:60-68)."""
        feats = xyz_in[0]
        xyz = [feats[:, :3, :]]
        pts = [feats]
        for sa in (self.sa1, self.sa2, self.sa3):
            x, p = sa(xyz[-1], pts[-1])
            xyz.append(x)
            pts.append(p)
        up = pts[3]
        for lvl, fp in ((2, self.fp3), (1, self.fp2), (0, self.fp1)):
            up = fp(xyz[lvl], xyz[lvl + 1], pts[lvl], up)
        out = [up, pts[3], xyz[0], xyz[3], self._head("offset", up), self._head("dist", up)]
        if self.cls_pred:
            out.append(self._head("cls", up))
        return out


def _msg_sa(mod, suffix, c_in):
    """The three multi-scale set-abstraction levels both tsegnet modules share (tsg_centroid_module.py:10-12, tsg_seg_module.py:11-13 /
    :24-26), registered on `mod` as sa{1,2,3}{suffix}."""
    levels = ((1024, [0.025, 0.05], c_in, [32, 32]), (512, [0.05, 0.1], 64, [64, 128]), (256, [0.1, 0.2], 256, [196, 256]))
    for i, (S, radii, c, widths) in enumerate(levels, 1):
        setattr(mod, f"sa{i}{suffix}", PointNetSetAbstractionMsg(S, radii, [32, 64], c, [widths, widths]))


def _msg_fp(mod, suffix, c_in):
    """... and their three feature-propagation levels fp{3,2,1}{suffix} (:15-17 / :16-18 / :30-32)."""
    for i, (c, widths) in ((3, (768, [256, 256])), (2, (320, [128, 128])), (1, (128 + c_in, [64, 32]))):
        setattr(mod, f"fp{i}{suffix}", PointNetFeaturePropagation(c, widths))


def _run_trunk(mod, suffix, feats):
    """-> (per-point features (B, 32, N), xyz / features of the three coarse levels)"""
    xyz, pts = [feats[:, :3, :]], [feats]
    for i in (1, 2, 3):
        x, p = getattr(mod, f"sa{i}{suffix}")(xyz[-1], pts[-1])
        xyz.append(x)
        pts.append(p)
    up = pts[3]
    for lvl in (3, 2, 1):
        up = getattr(mod, f"fp{lvl}{suffix}")(xyz[lvl - 1], xyz[lvl], pts[lvl - 1], up)
    return up, xyz, pts


class TsgCentroidNet(nn.Module):
    """tsg_centroid_module.get_model: per coarse point (256 of them) an offset to the nearest tooth centroid and its distance."""

    def __init__(self):
        super().__init__()
        _msg_sa(self, "", 6)
        _msg_fp(self, "", 6)
        for head, width in (("offset", 3), ("dist", 1)):
            setattr(self, f"{head}_conv_1", nn.Conv1d(515, 256, 1))
            setattr(self, f"{head}_bn_1", nn.BatchNorm1d(256))
        self.offset_conv_2, self.dist_conv_2 = nn.Conv1d(256, 3, 1), nn.Conv1d(256, 1, 1)
        nn.init.zeros_(self.offset_conv_2.weight)
        nn.init.zeros_(self.dist_conv_2.weight)

    @_one_index_check
    def forward(self, feats):
        """feats (B, 6, N), xyz first -> [l0_points, l3_points, l0_xyz, l3_xyz, offset (B,3,256), dist (B,1,256)] (:29-46)"""
        up, xyz, pts = _run_trunk(self, "", feats)
        coarse = torch.cat([pts[3], xyz[3]], 1)
        heads = [getattr(self, f"{h}_conv_2")(F.relu(getattr(self, f"{h}_bn_1")(getattr(self, f"{h}_conv_1")(coarse)))) for h in ("offset", "dist")]
        return [up, pts[3], xyz[0], xyz[3]] + heads


class TsgSegNet(nn.Module):
    """tsg_seg_module.get_model: two trunks on a cropped tooth neighbourhood (36 input channels; the second sees the first's
    foreground probabilities), a per-point mask each, and a tooth-id head on the max over ALL 256 coarse points -- the reference's
    one PointNetSetAbstraction(group_all=True), which runs on tgn_sa_all_mlp2_max in eval mode."""

    def __init__(self, input_feature_num=36):
        super().__init__()
        _msg_sa(self, "_1", input_feature_num)
        _msg_fp(self, "_1", input_feature_num)
        self.pd_mask_1, self.pd_mask_1_softmax, self.wt_mask_1 = nn.Conv1d(32, 2, 1), nn.Softmax(dim=1), nn.Conv1d(32, 1, 1)
        _msg_sa(self, "_2", input_feature_num + 2)                       # (module order = the reference's: state_dict keys line up)
        self.flatten_sa = PointNetSetAbstraction(None, None, None, 512 + 3, [256, 512], True)
        _msg_fp(self, "_2", input_feature_num + 2)
        self.pd_mask_2 = nn.Conv1d(32, 1, 1)
        self.fc1, self.bn1, self.fc2 = nn.Linear(512, 256), nn.LayerNorm(256), nn.Linear(256, 17)
        nn.init.zeros_(self.fc2.weight)
        nn.init.zeros_(self.fc2.bias)

    @_one_index_check
    def forward(self, feats):
        """feats (B, 36, N), xyz first -> (pd_1 (B,2,N), weight_1 (B,1,N), pd_2 (B,1,N), id_pred (B,17)) (:45-79)"""
        up1, _, _ = _run_trunk(self, "_1", feats)
        pd_1 = self.pd_mask_1_softmax(self.pd_mask_1(up1))
        weight_1 = self.wt_mask_1(up1)
        up2, xyz, pts = _run_trunk(self, "_2", torch.cat([feats, pd_1], 1))
        _, pooled = self.flatten_sa(xyz[3], pts[3])
        id_pred = self.fc2(F.relu(self.bn1(self.fc1(pooled.view(feats.shape[0], 512)))))
        return pd_1, weight_1, self.pd_mask_2(up2), id_pred


class _LatentMLP(nn.Module):
    """blocks.py:159-194 with ftype 'latent': Linear + BatchNorm + ReLU to base_fdim, held as `.infer`."""

    def __init__(self, fdim, d_out):
        super().__init__()
        self.infer = nn.Sequential(nn.Linear(fdim, d_out), nn.BatchNorm1d(d_out), nn.ReLU(inplace=True))

    def forward(self, x):
        if fold.frozen(self, x) and x.dtype == torch.float32:
            return PT.mlp_eval(self.infer, x)
        return PT.mlp_train(self.infer, x)


class MultiHead(nn.Module):
    """heads.py:13-61 for `multi: {stage: Ua, ftype: latent, combine: concat}`: every decoder stage's features go through
    their own latent MLP, are carried to the finest stage by nearest-neighbour interpolation (pointops.interpolation, k = 1)
    and concatenated in front of one linear classifier."""

    def __init__(self, fdims, k, base_fdim=32):
        super().__init__()
        self.infer_list = nn.ModuleList([_LatentMLP(f, base_fdim) for f in fdims])
        self.cls = nn.Linear(base_fdim * len(fdims), k)

    def forward(self, up_list, latents=None):
        """latents: a list that receives every stage's MLP output BEFORE interpolation -- what the reference stores back as
        stage['latent'] (heads.py:56-57) and its contrastive-boundary criterion reads."""
        p0, _, o0 = up_list[0]
        cols = []
        for i, ((p, x, o), mlp) in enumerate(zip(up_list, self.infer_list)):
            y = mlp(x)
            if latents is not None:
                latents.append(y)
            cols.append(y if i == 0 else pointops.interpolation(p, p0, y.contiguous(), o, o0, k=1))
        return self.cls(torch.cat(cols, 1))


class PointTransformerSeg(nn.Module):
    """`block_num` stages (cbl_point_transformer_module.py:46-57): 5, the network the reference ships for every scan-level model, or 2,
    tgnet's boundary network (inference_pipeline_maker.py:43-54: planes [16, 32], stride [1, 1]).  The top decoder stage is the head
    (`TransitionUp(in, None)`), and the heads' latent width is the reference's fixed base_fdim = 32 (:227), not planes[0]."""

    BASE_FDIM = 32

    def __init__(self, c=6, k=17, planes=(32, 64, 128, 256, 512), blocks=(2, 3, 4, 6, 3), stride=(1, 4, 4, 4, 4),
                 nsample=(36, 24, 24, 24, 24), share_planes=8, block_num=5):
        super().__init__()
        if block_num not in (2, 5):
            raise ValueError(f"block_num = {block_num}: the reference's forward exists for 2, 3 and 5 stages; 2 and 5 are mirrored")
        self.c, self.k, self.block_num = c, k, block_num
        self.stride, self.nsample = tuple(stride)[:block_num], tuple(nsample)[:block_num]     # the criterion's nstride and nsample
        self.cbl_counts = None                                                                # see forward(contrast=True)
        self.fused_contrast = False     # forward(contrast=True): the criterion's stages as fused kernels (contrast_boundary_loss(fused=True))
        planes = tuple(planes)[:block_num]
        in_planes = c
        for i in range(block_num):
            layers = [PT.TransitionDown(in_planes, planes[i], stride[i], nsample[i])]
            in_planes = planes[i]
            layers += [PT.PointTransformerBlock(in_planes, in_planes, share_planes, nsample[i]) for _ in range(1, blocks[i])]
            setattr(self, f"enc{i + 1}", nn.Sequential(*layers))
        for i in range(block_num - 1, -1, -1):
            layers = [PT.TransitionUp(in_planes, None if i == block_num - 1 else planes[i])]
            in_planes = planes[i]
            layers.append(PT.PointTransformerBlock(in_planes, in_planes, share_planes, nsample[i]))
            setattr(self, f"dec{i + 1}", nn.Sequential(*layers))
        self.mask_head = MultiHead(planes, 2, self.BASE_FDIM)
        self.cls_head = MultiHead(planes, k, self.BASE_FDIM)
        self.offset_head = MultiHead(planes, 3, self.BASE_FDIM)

    @_one_index_check
    def forward(self, inputs, all_offsets=False, contrast=False):
        """inputs: [features (B, C, N)] -> [cls (B, k, N), offset (1, 3, N) or None, None, x1 (B*N, planes[0])]
        (cbl_point_transformer_module.py:196-216 without the training criterion).  The offset head runs for B == 1 only, as in the
        reference; all_offsets=True runs it for any B (GroupingNetworkModule's unlabelled path, one scan at a time).

        contrast=True: inputs = [features, labels (B, 1, N) or (B, N)] -> [cbl_loss (block_num,), cls, offset, None, x1], the reference's
        list for two inputs (:198-204): losses.contrast_boundary_loss on target = labels + 1 with this network's nsample and stride
        (and fused=self.fused_contrast, an attribute the trainer sets: off unless asked for),
        over the latent features the LAST head that ran left behind -- every head overwrites stage['latent'] (heads.py:57), so the
        criterion reads the offset head's when it ran (B == 1, or all_offsets) and the class head's otherwise.  Checkpoints trained
        with the reference carry that quirk, so it is kept.  `self.cbl_counts` is the number of contributing points per stage of THIS
        forward, an int64 device tensor (a stage without one gives 0, where the reference raises at stage 0), and None after a forward
        without the criterion; GroupingNetworkModule hands it on in its output dict."""
        feats = inputs[0]
        if contrast:
            if len(inputs) < 2 or inputs[1] is None:
                raise ValueError("contrast=True needs the labels as inputs[1], (B, 1, N) or (B, N)")
            if inputs[1].numel() != feats.shape[0] * feats.shape[2]:
                raise ValueError(f"inputs[1] must hold one label per point, (B, 1, N) or (B, N) = ({feats.shape[0]}, {feats.shape[2]}), "
                                 f"got {tuple(inputs[1].shape)}")
        B, C, N = feats.shape
        pxo = feats.permute(0, 2, 1)
        x = pxo.reshape(-1, C).contiguous()
        p = pxo[:, :, :3].reshape(-1, 3).contiguous()
        o = pointops.register_offsets(torch.arange(1, B + 1, dtype=torch.int32, device=feats.device) * N,
                                      [N * (i + 1) for i in range(B)])
        stages = self.block_num
        down, cur = [], [p, x, o]
        for i in range(1, stages + 1):
            cur = getattr(self, f"enc{i}")(cur)
            down.append(cur)
        up, above = [None] * stages, None
        for i in range(stages - 1, -1, -1):
            pi, xi, oi = down[i]
            dec = getattr(self, f"dec{i + 1}")
            head = dec[0]([pi, xi, oi]) if above is None else dec[0]([pi, xi, oi], above)
            xi = dec[1:]([pi, head, oi])[1]
            above = up[i] = [pi, xi, oi]
        if not contrast:
            self.cbl_counts = None
            cls = self.cls_head(up).view(B, N, self.k).permute(0, 2, 1)
            offset = self.offset_head(up).view(B, N, 3).permute(0, 2, 1) if B == 1 or all_offsets else None
            return [cls, offset, None, up[0][1]]
        latents = []
        cls = self.cls_head(up, latents).view(B, N, self.k).permute(0, 2, 1)
        offset = None
        if B == 1 or all_offsets:
            latents = []
            offset = self.offset_head(up, latents).view(B, N, 3).permute(0, 2, 1)
        cbl_loss, self.cbl_counts = _losses.contrast_boundary_loss([[pi, oi] for pi, _, oi in up], latents, inputs[1].reshape(-1).long() + 1,
                                                                     self.nsample, self.stride, fused=self.fused_contrast)
        return [cbl_loss, cls, offset, None, up[0][1]]


class PointPpFirstModule(nn.Module):
    """models/modules/pointnet_pp.py:73-92 (the "pointnetpp" model): PointNetPPSeg as `first_sem_model`, its class logits as "cls_pred"."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.first_sem_model = PointNetPPSeg()

    def forward(self, inputs, test=False):
        return {"cls_pred": self.first_sem_model(inputs)[6]}


class PointTransformerModule(nn.Module):
    """models/modules/point_transformer.py:4-28 (the "pointtransformer" model): a 17-class PointTransformerSeg as `first_ins_cent_model`."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        mp = config["model_parameter"]
        self.first_ins_cent_model = PointTransformerSeg(c=mp["input_feat"], k=16 + 1, planes=tuple(mp["planes"]), blocks=tuple(mp["blocks"]),
                                                        stride=tuple(mp["stride"]), nsample=tuple(mp["nsample"]), block_num=mp.get("block_num", 5))

    def forward(self, inputs, test=False):
        sem_1, offset_1, mask_1, first_features = self.first_ins_cent_model([inputs[0]])
        return {"sem_1": sem_1, "offset_1": offset_1, "mask_1": mask_1, "first_features": first_features, "cls_pred": sem_1}


class GroupingNetworkModule(nn.Module):
    """models/modules/grouping_network_module.py:7-101 (tgnet_fps): `first_ins_cent_model` (PointTransformerSeg, 10 classes) over the
    whole scan; around every tooth the `crop_sample_size` nearest points, centred (crops.tooth_crops: three HIP kernels where the
    reference runs numpy, an sklearn KDTree and python gathers on the host); `second_ins_cent_model` (PointTransformerSeg, 2 classes)
    over all crops as one batch.  Same constructor argument and state_dict as the reference's class, so its checkpoints load with
    strict=True.

    Centroids: the labels' (inputs[1], the reference's path whenever len(inputs) >= 2), `centroids` given by the caller, or, with
    neither, the unlabelled path of grouping_network_module.py:57-69: per scan, the first stage's class argmax, the moved points xyz +
    offset_1, cluster.get_clustering_labels on them (DBSCAN, the PCA split test, MeanShift, the noise vote -- HIP kernels where the
    reference runs sklearn) and the float32 mean of the moved foreground points of every cluster, ascending
    (cluster.cluster_centroids, over crops.label_centroids).  The reference's
    unlabelled path works for B == 1 only (it indexes inputs[b_idx] and its offset head runs for B == 1); here every scan of a batch
    is clustered on its own, and offset_1 is then returned for every B.  The contrastive-boundary terms cbl_loss_1 / cbl_loss_2 of
    training (the reference's criterion, heads.py:62-253) are computed on request only: forward(contrast=True) with labels and
    `not test` adds them (PointTransformerSeg.forward(contrast=True) of both stages); the reference computes them whenever it has
    labels and `not test`.  Without `contrast`, `test` changes nothing here.  One host synchronisation per forward with labels (the tooth count, see
    crops.tooth_crops); the unlabelled path adds the clustering's (cluster.get_clustering_labels) and one per scan for its cluster
    count."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        mp = config["model_parameter"]
        block_num = mp.get("block_num", 5)
        if block_num not in (2, 5):
            raise ValueError(f"block_num = {block_num}: the five-stage network (train_configs/tgnet_fps.py) and tgnet's two-stage boundary "
                             "network (inference_pipeline_maker.py:43-54) are mirrored")
        arch = dict(planes=tuple(mp["planes"]), blocks=tuple(mp["blocks"]), stride=tuple(mp["stride"]), nsample=tuple(mp["nsample"]),
                    block_num=block_num)
        class_num = 9
        self.first_ins_cent_model = PointTransformerSeg(c=mp["input_feat"], k=class_num + 1, **arch)
        self.second_ins_cent_model = PointTransformerSeg(c=mp["input_feat"], k=2, **arch)
        self.crop_sample_size = int(mp["crop_sample_size"])

    def forward(self, inputs, test=False, centroids=None, contrast=False):
        """inputs: [features (B, C, N)] or [features, labels (B, 1, N)] -> the reference's output dict (sem_1, offset_1, mask_1,
        first_features, sem_2, offset_2, mask_2, cropped_feature_ls, nn_crop_indexes and, with labels, cluster_gt_seg_label);
        offset_2 is None unless there is exactly one crop (the reference's head runs for B == 1 only).
        contrast=True, with labels and `not test`: also cbl_loss_1 and cbl_loss_2, (block_num,) each, and cbl_counts_1 / cbl_counts_2, the
        number of contributing points per stage (int64, on the device) -- the first network's criterion
        on the half-jaw labels (labels >= 9 minus 8: 10 classes with gingiva), the second's on the crops' labels with every tooth set
        to 0 (grouping_network_module.py:26-28, 79-82)."""
        feats = inputs[0]
        labels = inputs[1] if len(inputs) >= 2 else None
        B = feats.shape[0]
        unlabelled = labels is None and centroids is None
        contrast = bool(contrast) and labels is not None and not test
        if contrast:
            half_seg_label = torch.where(labels >= 9, labels - 8, labels)
            cbl_loss_1, sem_1, offset_1, mask_1, first_features = self.first_ins_cent_model([feats, half_seg_label], contrast=True)
        elif unlabelled and B > 1:
            sem_1, offset_1, mask_1, first_features = self.first_ins_cent_model([feats], all_offsets=True)
        else:
            sem_1, offset_1, mask_1, first_features = self.first_ins_cent_model([feats])
        out = {"sem_1": sem_1, "offset_1": offset_1, "mask_1": mask_1, "first_features": first_features}
        if contrast:
            out["cbl_loss_1"], out["cbl_counts_1"] = cbl_loss_1, self.first_ins_cent_model.cbl_counts
        if unlabelled:
            centroids = [self._cluster_centroids(feats[b], sem_1[b], offset_1[b]) for b in range(B)]
        # labels: up to crops.MAX_CLUSTERS of them, not the 16 of a ground-truth jaw -- tgnet's boundary pass hands in cluster numbers
        cr = _crops.tooth_crops(feats, labels, centroids, self.crop_sample_size, num_labels=_crops.MAX_CLUSTERS)
        if labels is not None:
            out["cluster_gt_seg_label"] = cr.cluster_gt_seg_label
        if contrast:
            crop_labels = cr.cluster_gt_seg_label
            crop_labels = torch.where(crop_labels >= 0, torch.zeros_like(crop_labels), crop_labels)
            out["cbl_loss_2"], sem_2, offset_2, mask_2, _ = self.second_ins_cent_model([cr.cropped, crop_labels], contrast=True)
            out["cbl_counts_2"] = self.second_ins_cent_model.cbl_counts
        else:
            sem_2, offset_2, mask_2, _ = self.second_ins_cent_model([cr.cropped])
        out.update({"sem_2": sem_2, "offset_2": offset_2, "mask_2": mask_2, "cropped_feature_ls": cr.cropped,
                    "nn_crop_indexes": cr.nn_crop_indexes})
        return out

    @staticmethod
    def _cluster_centroids(feats, sem, offset):
        """grouping_network_module.py:59-68 for one scan: feats (C, N), sem (k, N), offset (3, N) -> (T, 3) float32 centroids."""
        with torch.no_grad():
            cls = torch.argmax(sem, dim=0)                                  # np.argmax: the first index on ties
            moved = (feats[:3].t() + offset.t()).contiguous()               # float32, as the reference adds its numpy copies
            fg_labels = _cluster.get_clustering_labels(moved, cls)
            return _cluster.cluster_centroids(moved[cls != 0], fg_labels)


class TSegNetModule(nn.Module):
    """models/modules/tsegnet.py:10-88 (the "tsegnet" model): `cent_module` (TsgCentroidNet) proposes tooth centroids from 256 coarse
    points, `seg_module` (TsgSegNet) segments a 3072-point crop around each centre.  Same constructor argument, attribute names and
    state_dict as the reference's class, so its checkpoints load with strict=True.  The join between the stages -- the proposal
    filter, DBSCAN(0.05, 3), the cluster means, the KDTree crops, the gathers and the distance feature -- is host work with a device
    round trip at every step in the reference; here it is tsegnet.py's HIP kernels (tsegnet.hip, and cluster.py's DBSCAN and crops.py's
    label means and kNN for the steps it shares with tgnet_fps).

    Like the reference, at most 8 centres are kept, chosen by `np.random.permutation(T)[:8]` on numpy's GLOBAL generator: the same
    `np.random.seed` gives the same crops as the reference (one call per scan, in scan order).  The reference is only meaningful for
    B = 1 (its `.T.reshape(-1, 3)` mixes scans); here every scan of a batch is clustered on its own in one ragged DBSCAN launch.
    `center_points` is what the reference returns for B = 1, a (1, T, 3) float32 numpy array, and for B > 1 a list over scans of
    (1, T_b, 3) arrays.  Host synchronisations per forward: tsegnet.py's two (kept counts, cluster counts) and the copy of
    `center_points` to the host that the reference's return type asks for.  In eval mode the segmentation module runs scan by scan
    (`segment`), so a scan's outputs do not depend on the rest of the batch.  All six terms of its loss are losses.tsegnet_loss_terms: the
    centroid terms as fused kernels (csrc/loss.hip), segmentation_loss and id_loss as torch compositions; training.TSegNetModel is its step."""

    MAX_CROPS = 8            # tsegnet.py:70
    CROP_K = 3072            # tsegnet.py:73

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.cent_module = TsgCentroidNet()
        self.seg_module = TsgSegNet()
        self.run_seg_module = bool(self.config["run_tooth_segmentation_module"])

    def get_ddf(self, cropped_coord, center_points):
        """cropped_coord (T, k, 3) float32 on the GPU, center_points (1, T, 3) numpy array or tensor -> (T, 1, k):
        exp(-4 sqrt(square_distance(crop point, its centre))) (tsegnet.py:24-33).  forward does not call it: the fused crop kernel
        writes the same feature (tgn_tsg_crop_features)."""
        if not isinstance(center_points, torch.Tensor):
            center_points = torch.from_numpy(center_points)
        center_points = center_points.to(cropped_coord.device, cropped_coord.dtype)
        ddf = square_distance(cropped_coord.contiguous(), center_points.permute(1, 0, 2).contiguous())
        ddf = torch.exp(torch.sqrt(ddf) * (-4))
        return ddf.permute(0, 2, 1)

    def segment(self, cropped, per_scan):
        """The segmentation module on the crops (T, 36, k) of a batch, per_scan = the number of crops of every scan.  Train mode: all
        crops as ONE batch, as the reference runs them (its BatchNorm statistics are taken over all of them).  Eval mode: one scan's
        crops at a time, so that what a scan gets does not depend on what else is in the batch -- the same crop in a batch of 8 and in
        a batch of 16 differs in the last bits (measured on an MI355X: up to 2.6e-6 relative in pd_2, on bit-equal input; the
        presumed cause, not traced to a layer, is that the library GEMMs behind the network pick their kernels by the row count).
        The price is B passes of the segmentation network's launches instead of one in eval mode.  Scan 0 of a B = 2 forward is then bit-equal to the B = 1 forward."""
        if self.training or len(per_scan) == 1:
            return self.seg_module(cropped)
        outs = [self.seg_module(c) for c in cropped.split(per_scan)]
        return tuple(torch.cat(parts) for parts in zip(*outs))

    def forward(self, inputs, on_no_centre="raise"):
        """inputs: [features (B, 6, N), labels (B, 1, N)] (labels may be left out: cluster_gt_seg_label is then None) -> the
        reference's output dict: l0_points, l3_points, l0_xyz, l3_xyz, offset_result, dist_result and, when the segmentation module
        runs, pd_1, weight_1, pd_2, id_pred, center_points, cluster_gt_seg_label, cropped_feature_ls.
        A scan for which no centre survives the join (no proposal below the threshold, or no DBSCAN cluster) raises ValueError naming
        the scan -- the reference dies there with an IndexError.  on_no_centre="skip" returns the centroid outputs alone for such a
        batch instead, which is what a training step early in a run needs (training.TSegNetModel)."""
        if on_no_centre not in ("raise", "skip"):
            raise ValueError(f"on_no_centre must be 'raise' or 'skip', got {on_no_centre!r}")
        feats = inputs[0]
        labels = inputs[1] if len(inputs) >= 2 else None
        l0_points, l3_points, l0_xyz, l3_xyz, offset_result, dist_result = self.cent_module(feats)
        outputs = {"l0_points": l0_points, "l3_points": l3_points, "l0_xyz": l0_xyz, "l3_xyz": l3_xyz,
                   "offset_result": offset_result, "dist_result": dist_result}
        if not self.run_seg_module:
            return outputs
        with torch.no_grad():
            moved, counts = _tsg.centroid_proposals(l3_xyz, offset_result, dist_result)
            try:
                centres = _tsg.cluster_centers(moved, counts)
            except _tsg.NoCentre:
                if on_no_centre == "skip":
                    return outputs
                raise
            chosen = []
            for c in centres:
                rand_indexes = np.random.permutation(c.shape[0])[:self.MAX_CROPS]
                chosen.append(c.index_select(0, torch.from_numpy(rand_indexes).to(c.device, non_blocking=True)))
        cropped, _, crop_labels = _tsg.crop_features(feats, l0_points, chosen, self.CROP_K, labels)
        pd_1, weight_1, pd_2, id_pred = self.segment(cropped, [int(c.shape[0]) for c in chosen])
        center_points = [c.cpu().numpy()[None] for c in chosen]
        outputs.update({"pd_1": pd_1, "weight_1": weight_1, "pd_2": pd_2, "id_pred": id_pred,
                        "center_points": center_points[0] if len(center_points) == 1 else center_points,
                        "cluster_gt_seg_label": crop_labels, "cropped_feature_ls": cropped})
        return outputs
