"""DGCNN (models/modules/dgcnn.py, the "dgcnn" branch of inference_pipeline_maker.py): the feature-space kNN, the edge features and
a state_dict-compatible mirror of DGCnnModule.

  knn(x, k)                 the reference's neighbour search (dgcnn.py:4-10) on tgn_feature_knn: no N x N matrix.  Rows hold the
                            k nearest points in ascending (direct-form fp32 distance, index) order -- see include/tgn_pointops.h
                            and DESIGN.md section 4 for how this differs from the expanded-form matmul + topk of the reference.
  get_graph_feature(...)    dgcnn.py:13-40 with the same signature and output ([x_j - x_i, x_i], (B, 2C, N, k)), on x's device.
  DGCnnModule(config)       dgcnn.py:43-143.  Eval mode (frozen: no gradient wanted) runs the fused EdgeConv kernels
                            (tgn_edgeconv2_max / tgn_edgeconv1_max) on per-point transforms, so neither the edge tensors nor
                            the N x N distances exist, and conv7 by the commuted split (W7[:, :1024] g once per scan).
                            Train mode is the reference's formulation on the new kNN (autograd through torch ops).
"""
import torch
import torch.nn as nn

from . import _derived, _lib, fold
from ._lib import f32c, ops, require_cuda, stream


def feature_knn(x, k):
    """x (B, D, N) float32 on the GPU -> (idx (B, N, k) int64, dist2 (B, N, k) float32): per point the k nearest points of its scan
    (itself included) in ascending (distance, index) order, distance = the direct form sum_c (x_i[c] - x_j[c])^2 in fp32, summed
    over c in order.  1 <= D <= 64, 1 <= k <= min(N, 32)."""
    require_cuda(x)
    if x.dim() != 3:
        raise ValueError(f"feature_knn: x must be (B, D, N), got {tuple(x.shape)}")
    x = x.float().contiguous()
    B, D, N = x.shape
    k = int(k)
    idx = torch.empty(B, N, max(k, 0), dtype=torch.long, device=x.device)
    dist = torch.empty(B, N, max(k, 0), dtype=torch.float32, device=x.device)
    ws_bytes = ops().tgn_feature_knn_workspace_bytes(B, N, k)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
    ops().tgn_feature_knn(B, N, D, k, x, idx, dist, ws, ws_bytes, stream())
    return idx, dist


def knn(x, k):
    """dgcnn.py:4-10: x (B, D, N) -> idx (B, N, k) int64, indices local to each scan."""
    return feature_knn(x, k)[0]


def get_graph_feature(x, k=20, idx=None, dim9=False):
    """dgcnn.py:13-40: (B, C, N) -> (B, 2C, N, k) edge features [x_j - x_i, x_i] (bit-equal to the reference's formula for the same
    idx), on x's device rather than a hard-coded 'cuda'."""
    batch_size = x.size(0)
    num_points = x.size(2)
    x = x.view(batch_size, -1, num_points)
    if idx is None:
        idx = knn(x, k=k)   # dim9 or not: the reference searches all channels either way
    idx_base = torch.arange(0, batch_size, device=x.device).view(-1, 1, 1) * num_points
    idx = (idx + idx_base).view(-1)
    _, num_dims, _ = x.size()
    x = x.transpose(2, 1).contiguous()
    feature = x.view(batch_size * num_points, -1)[idx, :]
    feature = feature.view(batch_size, num_points, k, num_dims)
    x = x.view(batch_size, num_points, 1, num_dims).repeat(1, 1, k, 1)
    return torch.cat((feature - x, x), dim=3).permute(0, 3, 1, 2).contiguous()


def _edge_first_layer(conv, bn):
    """Eval-mode BatchNorm folded into an edge layer's first 1x1 convolution, split for the commuted form
    W' [x_j - x_i ; x_i] + t = Wa' x_j + (Wb' - Wa') x_i + t: returns (Wa'^T, (Wb' - Wa')^T, t), the matrices (C, 64)."""
    W, t = fold.affine(conv, bn)
    C = W.shape[1] // 2
    Wa, Wb = W[:, :C], W[:, C:]
    return Wa.t().contiguous(), (Wb - Wa).t().contiguous(), t


def _second_layer(conv, bn):
    return fold.affine(conv, bn)


def edgeconv_max(x, idx, first, second=None, out=None, coff=0):
    """One fused EdgeConv level in eval mode: x (B, C, N) features, idx (B, N, K) neighbours, first = _edge_first_layer(...),
    second = _second_layer(...) or None (one-layer level).  Writes max_j lrelu(...) into out[:, coff:coff + 64] of a (B, Ctot, N)
    tensor (allocated (B, 64, N) when None) and returns out.  The per-point transforms P = Wa' x, Q = (Wb' - Wa') x + t are GEMMs."""
    require_cuda(x, idx)
    if not x.is_floating_point():
        raise TypeError(f"edgeconv_max: x must be a floating-point tensor, got {x.dtype}")
    B, C, N = x.shape
    K = idx.shape[-1]
    WaT, WdT, t1 = first
    if WaT.shape != (C, 64):
        raise ValueError(f"edgeconv_max: the fused kernels take 64 output channels from C = {C} inputs, got {tuple(WaT.shape)}")
    if out is not None:
        if out.dtype != torch.float32 or out.device != x.device:
            raise TypeError(f"edgeconv_max: out must be float32 on {x.device}, got {out.dtype} on {out.device}")
        if out.dim() != 3 or out.shape[0] != B or out.shape[2] != N or not 0 <= coff <= out.shape[1] - 64:
            raise ValueError(f"edgeconv_max: out must be ({B}, Ctot, {N}) with 0 <= coff <= Ctot - 64, got {tuple(out.shape)}, coff {coff}")
        if out.stride(2) != 1 or out.stride(1) != N:
            raise ValueError("edgeconv_max: out must be (B, Ctot, N) with rows of N contiguous floats")
    x = f32c(x, "edgeconv_max: x")                                    # one layout: the GEMMs below round by the layout they read
    xt = x.transpose(1, 2)                              # (B, N, C) view; the GEMMs read it in place
    P = torch.matmul(xt, WaT)                           # (B, N, 64), contiguous
    Q = torch.matmul(xt, WdT).add_(t1)
    idx = idx.contiguous()
    if idx.dtype != torch.long:
        idx = idx.long()
    if out is None:
        out, coff = torch.empty(B, 64, N, dtype=torch.float32, device=x.device), 0
    _lib.begin_index_check()
    if second is None:
        ops().tgn_edgeconv1_max(B, N, K, P, Q, idx, out, out.stride(0), coff, stream())
    else:
        W2, b2 = (t.float().contiguous() for t in second)
        ops().tgn_edgeconv2_max(B, N, K, P, Q, idx, W2, b2, out, out.stride(0), coff, stream())
    _lib.raise_on_index_error("DGCNN EdgeConv")
    return out


class DGCnnModule(nn.Module):
    """models/modules/dgcnn.py:43-143: same constructor argument, parameter names and shapes, so the reference's checkpoints load
    with strict=True.  forward([features (B, 6, N), ...]) -> {"cls_pred": (B, 17, N)}."""

    def __init__(self, config):
        super().__init__()
        drop_out_ratio = 0.5
        emb_dims = 1024
        self.k = 20
        input_dim = 6
        self.scale = 1
        s = self.scale
        self.bn1 = nn.BatchNorm2d(64 * s)
        self.bn2 = nn.BatchNorm2d(64 * s)
        self.bn3 = nn.BatchNorm2d(64 * s)
        self.bn4 = nn.BatchNorm2d(64 * s)
        self.bn5 = nn.BatchNorm2d(64 * s)
        self.bn6 = nn.BatchNorm1d(emb_dims * s)
        self.bn7 = nn.BatchNorm1d(512 * s)
        self.bn8 = nn.BatchNorm1d(256 * s)
        lrelu = lambda: nn.LeakyReLU(negative_slope=0.2)   # noqa: E731
        self.conv1 = nn.Sequential(nn.Conv2d(input_dim * 2, 64 * s, kernel_size=1, bias=False), self.bn1, lrelu())
        self.conv2 = nn.Sequential(nn.Conv2d(64 * s, 64 * s, kernel_size=1, bias=False), self.bn2, lrelu())
        self.conv3 = nn.Sequential(nn.Conv2d(64 * 2 * s, 64 * s, kernel_size=1, bias=False), self.bn3, lrelu())
        self.conv4 = nn.Sequential(nn.Conv2d(64 * s, 64 * s, kernel_size=1, bias=False), self.bn4, lrelu())
        self.conv5 = nn.Sequential(nn.Conv2d(64 * 2 * s, 64 * s, kernel_size=1, bias=False), self.bn5, lrelu())
        self.conv6 = nn.Sequential(nn.Conv1d(192 * s, emb_dims * s, kernel_size=1, bias=False), self.bn6, lrelu())
        self.conv7 = nn.Sequential(nn.Conv1d(1216 * s, 512 * s, kernel_size=1, bias=False), self.bn7, lrelu())
        self.conv8 = nn.Sequential(nn.Conv1d(512 * s, 256 * s, kernel_size=1, bias=False), self.bn8, lrelu())
        self.dp1 = nn.Dropout(p=drop_out_ratio)
        self.cls_conv = nn.Conv1d(256, 17, kernel_size=1, bias=False)
        self.offset_conv = nn.Conv1d(256, 3, kernel_size=1, bias=False)
        self.dist_conv = nn.Conv1d(256, 1, kernel_size=1, bias=False)
        nn.init.zeros_(self.offset_conv.weight)
        nn.init.zeros_(self.dist_conv.weight)
        self.last_idx = None   # the three levels' neighbour indices of the last forward (tests, diagnostics)

    def _folded(self):
        def build():
            return (_edge_first_layer(self.conv1[0], self.bn1), _second_layer(self.conv2[0], self.bn2),
                    _edge_first_layer(self.conv3[0], self.bn3), _second_layer(self.conv4[0], self.bn4),
                    _edge_first_layer(self.conv5[0], self.bn5))
        src = _derived.sources(self.conv1[0], self.bn1, self.conv2[0], self.bn2, self.conv3[0], self.bn3, self.conv4[0], self.bn4,
                               self.conv5[0], self.bn5)
        return _derived.cached(self, "dgcnn_edge_eval", src, None, build)

    def _head(self, feats):
        """conv6 .. cls_conv over the (B, 192, N) concatenation [x1, x2, x3]; conv7 by the commuted split: its first 1024 input
        channels see the global feature g repeated over the points, so W7[:, :1024] g is computed once per scan and broadcast."""
        g = self.conv6(feats).max(dim=-1, keepdim=True)[0]                  # (B, 1024, 1)
        W7 = self.conv7[0].weight.reshape(self.conv7[0].out_channels, -1)
        y = torch.matmul(W7[:, 1024:], feats) + torch.matmul(W7[:, :1024], g)
        x = self.conv7[2](self.conv7[1](y))
        x = self.dp1(self.conv8(x))
        return self.cls_conv(x)

    def forward(self, x_in):
        x = x_in[0]
        if fold.frozen(self, x) and x.dtype == torch.float32:
            return {"cls_pred": self._forward_eval(x)}
        return {"cls_pred": self._forward_train(x)}

    def _forward_train(self, x):
        k = self.k
        idx1 = knn(x.detach(), k)
        x1 = self.conv2(self.conv1(get_graph_feature(x, k=k, idx=idx1))).max(dim=-1, keepdim=False)[0]
        idx2 = knn(x1.detach(), k)
        x2 = self.conv4(self.conv3(get_graph_feature(x1, k=k, idx=idx2))).max(dim=-1, keepdim=False)[0]
        idx3 = knn(x2.detach(), k)
        x3 = self.conv5(get_graph_feature(x2, k=k, idx=idx3)).max(dim=-1, keepdim=False)[0]
        self.last_idx = (idx1, idx2, idx3)
        return self._head(torch.cat((x1, x2, x3), dim=1))

    def _forward_eval(self, x, idx=None):
        """Fused eval forward.  idx: None (the kNN runs) or the three levels' (B, N, k) neighbour indices to use instead."""
        require_cuda(x)
        x = x.contiguous()
        B, _, N = x.shape
        f1, s2, f3, s4, f5 = self._folded()
        feats = torch.empty(B, 192, N, dtype=torch.float32, device=x.device)
        used = []
        level_in = x
        with _lib.deferred_index_check("DGCnnModule forward"):   # one read of the error word for the three levels
            for lvl, (first, second) in enumerate(((f1, s2), (f3, s4), (f5, None))):
                ii = knn(level_in, self.k) if idx is None else idx[lvl]
                used.append(ii)
                edgeconv_max(level_in, ii, first, second, out=feats, coff=64 * lvl)
                if lvl < 2:
                    level_in = feats[:, 64 * lvl:64 * (lvl + 1)].contiguous()
        self.last_idx = tuple(used)
        return self._head(feats)
