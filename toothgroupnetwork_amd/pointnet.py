"""PointNet (models/modules/pointnet.py, external_libs/pointnet2_utils/pointnet_utils.py; the "pointnet" branch of
inference_pipeline_maker.py): state_dict-compatible mirrors and the fused layer they stand on.

  linear_act_max(x, conv, bn, act, slope)   max over the points of act(bn(conv(x))) for a 1x1 convolution in eval mode, on
                            tgn_linear_act_max (csrc/linear_max.hip, fp32 MFMA): the (B, C, N) tensor the reference writes in front
                            of every torch.max (98 MB per 24 000-point scan at C = 1024, 197 MB at 2048) never exists.
  STN3d, STNkd, PointNetEncoder, feature_transform_reguliarzer    pointnet_utils.py:10-143, the reference's names and shapes.
  get_model, get_loss, PointFirstModule(config)                   pointnet.py:9-68.

Eval mode (frozen: no gradient wanted, float32 input) sends stn.conv3, fstn.conv3 and feat.conv3 through linear_act_max, runs the
narrow layers as torch GEMMs with the BatchNorm folded, and takes the head's conv1 (2176 -> 1024) by the commuted split
DGCnnModule._head uses for conv7: its first 2048 input channels see the global feature repeated over the points, so
W[:, :2048] g is computed once per scan and added to W[:, 2048:] pointfeat -- neither the (B, 2048, N) nor the (B, 2176, N) tensor
exists.  Train mode, or any forward that wants a gradient, is the reference's formulation in torch ops (autograd), on any device.

Two rules of the eval path.  (1) Every torch GEMM sees ONE scan, whatever the batch: a BLAS picks its blocking by the shape, and at
this network's activations (up to ~100) two blockings differ by 3e-5 in the log-probabilities, so a scan's result would depend on
its neighbours in the batch; the fused kernel is batch-invariant by contract and takes the whole batch in one launch.  (2) What is
small and feeds everything runs in float64: the regressors' fc layers (a 3 x 3 and a 128 x 128 matrix per scan), the head's
per-scan term W[:, :2048] g (a 2048-term sum) and the 17-row conv4 with its log_softmax.  The GPU BLAS sums each dot product as
one long chain, where the reference's CPU BLAS sums in blocks; measured on the fixture of tests/test_gpu_pointnet_module.py, fp32 in
those places puts the forward at 2.7e-5 of the float64 result (the reference's formulation on the same GPU: 2.7e-5; on its CPU:
0.8e-5).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _derived, fold
from ._lib import f32c, ops, require_cuda, stream

_ACTS = {"identity": 0, "relu": 1, "leaky_relu": 2}


def _folded_t(conv, bn):
    """fold.affine(conv, bn) with the weight as tgn_linear_act_max reads it: (K, C) row-major.  Memoised on the convolution."""
    def build():
        W, t = fold.affine(conv, bn)
        return W.t().contiguous(), t
    src = _derived.sources(conv) + (_derived.sources(bn) if bn is not None else [])
    return _derived.cached(conv, "pointnet_folded_t", src, None, build)


def linear_act_max(x, conv, bn, act, slope=0.0):
    """x (B, K, N) on the GPU -> (B, C) float32: max over the N points of act(bn(conv(x))), conv a 1x1 Conv1d (K -> C), bn its
    eval-mode BatchNorm1d (running statistics) or None, act "identity" | "relu" | "leaky_relu" (with `slope`).  The activation
    comes before the max and a NaN candidate gives NaN, as the torch composition does; the result for one scan depends neither
    on the batch nor on N's split (bit equality).  1 <= K <= 512."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"linear_act_max: x must be a tensor, got {type(x).__name__}")
    require_cuda(x)
    if not x.is_floating_point():
        raise TypeError(f"linear_act_max: x must be a floating-point tensor, got {x.dtype}")
    if x.dim() != 3:
        raise ValueError(f"linear_act_max: x must be (B, K, N), got {tuple(x.shape)}")
    if not isinstance(conv, nn.Conv1d) or conv.kernel_size != (1,) or conv.stride != (1,) or conv.groups != 1:
        raise TypeError("linear_act_max: conv must be a 1x1 nn.Conv1d (stride 1, one group)")
    if bn is not None and not isinstance(bn, nn.BatchNorm1d):
        raise TypeError(f"linear_act_max: bn must be an nn.BatchNorm1d or None, got {type(bn).__name__}")
    if bn is not None and bn.running_var is None:
        raise ValueError("linear_act_max: bn must track running statistics (the eval-mode fold needs them)")
    if act not in _ACTS:
        raise ValueError(f"linear_act_max: act must be one of {sorted(_ACTS)}, got {act!r}")
    B, K, N = x.shape
    C = conv.out_channels
    if conv.in_channels != K:
        raise ValueError(f"linear_act_max: x has {K} channels, conv takes {conv.in_channels}")
    if B < 1 or N < 1:
        raise ValueError(f"linear_act_max: x must hold at least one scan and one point, got {tuple(x.shape)}")
    if not 1 <= K <= 512:
        raise ValueError(f"linear_act_max: x must have 1 .. 512 channels, got {K}")
    if conv.weight.device != x.device:
        raise ValueError(f"linear_act_max: conv lives on {conv.weight.device}, x on {x.device}")
    x = f32c(x, "linear_act_max: x")
    Wt, shift = _folded_t(conv, bn)
    out = torch.empty(B, C, dtype=torch.float32, device=x.device)
    ws_bytes = ops().tgn_linear_act_max_workspace_bytes(B, N, K, C)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    ops().tgn_linear_act_max(B, N, K, C, x, Wt, shift, _ACTS[act], float(slope), out, ws, ws_bytes, stream())
    return out


def _pointwise(x, conv, bn, relu):
    """A narrow 1x1 convolution in eval mode with the BatchNorm folded, (B, K, N) -> (B, C, N): one GEMM per scan, so that a
    scan's bits do not depend on the batch."""
    W, t = fold.affine(conv, bn)
    y = torch.empty(x.shape[0], W.shape[0], x.shape[2], dtype=torch.float32, device=x.device)
    for b in range(x.shape[0]):
        torch.matmul(W, x[b], out=y[b])
    y.add_(t[:, None])
    return y.relu_() if relu else y


def _per_scan_mm(A, x):
    """torch.bmm(A (B, C, K), x (B, K, N)) as one GEMM per scan (see _pointwise)."""
    y = torch.empty(x.shape[0], A.shape[1], x.shape[2], dtype=torch.float32, device=x.device)
    for b in range(x.shape[0]):
        torch.matmul(A[b], x[b], out=y[b])
    return y


class _STN(nn.Module):
    """pointnet_utils.py:10-85: the transform regressor, (B, cin, N) -> (B, k, k) = identity + fc(max over the points)."""

    def __init__(self, cin, k):
        super().__init__()
        self.conv1 = nn.Conv1d(cin, 64, 1)
        self.conv2 = nn.Conv1d(64, 128, 1)
        self.conv3 = nn.Conv1d(128, 1024, 1)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc3 = nn.Linear(256, k * k)
        self.relu = nn.ReLU()
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.bn4 = nn.LayerNorm(512)
        self.bn5 = nn.LayerNorm(256)
        self._side = k

    def _fc(self, g):
        k = self._side
        g = F.relu(self.bn4(self.fc1(g)))
        g = F.relu(self.bn5(self.fc2(g)))
        g = self.fc3(g) + torch.eye(k, dtype=torch.float32, device=g.device).reshape(1, k * k)
        return g.view(-1, k, k)

    def _fc_eval(self, g):
        """_fc in float64, one scan per GEMM: g (B, 1024) float32 -> (B, k, k) float32."""
        def build():
            return tuple(t.detach().double() for m in (self.fc1, self.bn4, self.fc2, self.bn5, self.fc3) for t in (m.weight, m.bias))
        w1, b1, lw4, lb4, w2, b2, lw5, lb5, w3, b3 = _derived.cached(
            self, "pointnet_fc64", _derived.sources(self.fc1, self.bn4, self.fc2, self.bn5, self.fc3), None, build)
        k = self._side
        eye = torch.eye(k, dtype=torch.float64, device=g.device).reshape(1, k * k)
        rows = []
        for b in range(g.shape[0]):
            r = g[b:b + 1].double()
            r = F.relu(F.layer_norm(F.linear(r, w1, b1), (512,), lw4, lb4, self.bn4.eps))
            r = F.relu(F.layer_norm(F.linear(r, w2, b2), (256,), lw5, lb5, self.bn5.eps))
            rows.append(F.linear(r, w3, b3) + eye)
        return torch.cat(rows).float().view(-1, k, k)

    def forward(self, x):
        if fold.frozen(self, x) and x.dtype == torch.float32:
            return self._forward_eval(x)
        return self._forward_train(x)

    def _forward_train(self, x):
        x = F.relu(self.bn1(self.conv1(x)))
        x = F.relu(self.bn2(self.conv2(x)))
        x = F.relu(self.bn3(self.conv3(x)))
        return self._fc(torch.max(x, 2)[0])

    def _forward_eval(self, x):
        require_cuda(x)
        h = _pointwise(_pointwise(x, self.conv1, self.bn1, True), self.conv2, self.bn2, True)
        return self._fc_eval(linear_act_max(h, self.conv3, self.bn3, "relu"))


class STN3d(_STN):
    def __init__(self, channel):
        super().__init__(channel, 3)


class STNkd(_STN):
    def __init__(self, k=64):
        super().__init__(k, k)
        self.k = k


class PointNetEncoder(nn.Module):
    """pointnet_utils.py:88-134.  forward(x (B, D, N)) -> (features, trans, trans_feat); features = the global feature
    (B, 1024 * scale) with global_feat, else [global feature repeated over the points, pointfeat] (B, 1088 * scale, N)."""

    def __init__(self, global_feat=True, feature_transform=False, channel=3, scale=1):
        super().__init__()
        self.stn = STN3d(channel)
        self.scale = scale
        self.conv1 = nn.Conv1d(channel, 64 * scale, 1)
        self.conv2 = nn.Conv1d(64 * scale, 128 * scale, 1)
        self.conv3 = nn.Conv1d(128 * scale, 1024 * scale, 1)
        self.bn1 = nn.BatchNorm1d(64 * scale)
        self.bn2 = nn.BatchNorm1d(128 * scale)
        self.bn3 = nn.BatchNorm1d(1024 * scale)
        self.global_feat = global_feat
        self.feature_transform = feature_transform
        if feature_transform:
            self.fstn = STNkd(k=64 * scale)

    def _assemble(self, g, pointfeat, trans, trans_feat):
        if self.global_feat:
            return g, trans, trans_feat
        rep = g.view(-1, 1024 * self.scale, 1).repeat(1, 1, pointfeat.shape[2])
        return torch.cat([rep, pointfeat], 1), trans, trans_feat

    def forward(self, x):
        if fold.frozen(self, x) and x.dtype == torch.float32:
            return self._assemble(*self._features_eval(x))
        return self._assemble(*self._features_train(x))

    def _features_train(self, x):
        """The reference's formulation up to the max: (global feature (B, 1024 * scale), pointfeat, trans, trans_feat)."""
        D = x.shape[1]
        trans = self.stn._forward_train(x)
        x = x.transpose(2, 1)
        moved = torch.bmm(x[:, :, :3], trans)
        x = torch.cat([moved, x[:, :, 3:]], dim=2) if D > 3 else moved
        x = F.relu(self.bn1(self.conv1(x.transpose(2, 1))))
        trans_feat = None
        if self.feature_transform:
            trans_feat = self.fstn._forward_train(x)
            x = torch.bmm(x.transpose(2, 1), trans_feat).transpose(2, 1)
        pointfeat = x
        x = F.relu(self.bn2(self.conv2(x)))
        x = self.bn3(self.conv3(x))
        return torch.max(x, 2)[0], pointfeat, trans, trans_feat

    def _features_eval(self, x):
        """The same four on the fused layers.  The 3 x 3 input transform moves into conv1's weight, per scan:
        W1 [T^T xyz; f] = [W1[:, :3] T^T, W1[:, 3:]] [xyz; f]."""
        require_cuda(x)
        x = x.contiguous()
        trans = self.stn._forward_eval(x)
        W1, t1 = fold.affine(self.conv1, self.bn1)
        W1 = torch.cat([torch.matmul(W1[:, :3], trans.transpose(1, 2)), W1[:, 3:].expand(x.shape[0], -1, -1)], dim=2)   # (B, C, D)
        h = _per_scan_mm(W1, x).add_(t1[:, None]).relu_()
        trans_feat = None
        if self.feature_transform:
            trans_feat = self.fstn._forward_eval(h)
            h = _per_scan_mm(trans_feat.transpose(1, 2), h)
        g = linear_act_max(_pointwise(h, self.conv2, self.bn2, True), self.conv3, self.bn3, "identity")
        return g, h, trans, trans_feat


def feature_transform_reguliarzer(trans):
    """pointnet_utils.py:137-143: mean over the batch of || T T^T - I ||_F."""
    eye = torch.eye(trans.shape[1], dtype=trans.dtype, device=trans.device)[None]
    return torch.mean(torch.norm(torch.bmm(trans, trans.transpose(2, 1)) - eye, dim=(1, 2)))


class get_model(nn.Module):
    """pointnet.py:9-35: the segmentation network, 17 classes, scale 2.  forward([x (B, 6, N), ...]) -> (log-probabilities
    (B, 17, N), trans_feat (B, 128, 128))."""

    def __init__(self):
        super().__init__()
        self.k = 17
        scale = 2
        self.feat = PointNetEncoder(global_feat=False, feature_transform=True, channel=6, scale=scale)
        self.conv1 = nn.Conv1d(1088 * scale, 512 * scale, 1)
        self.conv2 = nn.Conv1d(512 * scale, 256 * scale, 1)
        self.conv3 = nn.Conv1d(256 * scale, 128 * scale, 1)
        self.conv4 = nn.Conv1d(128 * scale, self.k, 1)
        self.bn1 = nn.BatchNorm1d(512 * scale)
        self.bn2 = nn.BatchNorm1d(256 * scale)
        self.bn3 = nn.BatchNorm1d(128 * scale)

    def forward(self, x_in):
        x = x_in[0]
        if fold.frozen(self, x) and x.dtype == torch.float32:
            return self._forward_eval(x)
        return self._forward_train(x)

    def _forward_train(self, x):
        """The reference's formulation in torch ops: autograd, any device, any floating dtype."""
        g, pointfeat, _, trans_feat = self.feat._features_train(x)
        x = torch.cat([g.unsqueeze(2).repeat(1, 1, x.shape[2]), pointfeat], 1)
        x = F.relu(self.bn1(self.conv1(x)))
        x = F.relu(self.bn2(self.conv2(x)))
        x = F.relu(self.bn3(self.conv3(x)))
        B, _, N = x.shape
        x = self.conv4(x).transpose(2, 1).contiguous()                        # the softmax over rows of 17, as the reference runs it
        return F.log_softmax(x.view(-1, self.k), dim=-1).view(B, N, self.k).permute(0, 2, 1), trans_feat

    def _forward_eval(self, x):
        g, pointfeat, _, trans_feat = self.feat._features_eval(x)
        B, ng = g.shape

        def build():
            W1, t1 = fold.affine(self.conv1, self.bn1)
            W4, t4 = fold.affine(self.conv4)
            return W1[:, ng:].contiguous(), W1[:, :ng].t().double(), t1.double(), W4.double(), t4.double()[:, None]
        W1p, W1g, t1, W4, t4 = _derived.cached(self, "pointnet_head", _derived.sources(self.conv1, self.bn1, self.conv4), ng, build)
        out = torch.empty(B, self.k, x.shape[2], dtype=torch.float32, device=x.device)
        for b in range(B):                                                    # one scan's (1024, N) activations at a time
            per_scan = torch.addmm(t1, g[b:b + 1].double(), W1g).float()      # (1, 1024): W[:, :2048] g + shift, once per scan
            h = torch.matmul(W1p, pointfeat[b:b + 1]).add_(per_scan[:, :, None]).relu_()
            h = _pointwise(h, self.conv2, self.bn2, True)
            h = _pointwise(h, self.conv3, self.bn3, True)
            out[b] = F.log_softmax(torch.matmul(W4, h[0].double()).add_(t4), dim=0)
        return out, trans_feat


class get_loss(nn.Module):
    """pointnet.py:37-46: nll_loss + mat_diff_loss_scale * feature_transform_reguliarzer(trans_feat)."""

    def __init__(self, mat_diff_loss_scale=0.001):
        super().__init__()
        self.mat_diff_loss_scale = mat_diff_loss_scale

    def forward(self, pred, target, trans_feat, weight):
        return F.nll_loss(pred, target, weight=weight) + feature_transform_reguliarzer(trans_feat) * self.mat_diff_loss_scale


class PointFirstModule(nn.Module):
    """pointnet.py:49-68: same constructor argument, parameter names and shapes, so the reference's checkpoints load with
    strict=True.  forward([features (B, 6, N), ...]) -> {"cls_pred": log-probabilities (B, 17, N)}."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.first_sem_model = get_model()

    def forward(self, inputs, test=False):
        cls_pred, _ = self.first_sem_model(inputs)
        return {"cls_pred": cls_pred}
