"""fold.py on the CPU: eval-mode BatchNorm folded into the layer in front of it, and the kernel layouts built on top of it.

Every comparison is bit for bit (torch.equal on the int32 view of the float32 operands): the formula restated here is the one the
eval paths have always used, one fp32 operation per product and sum, so a fold that drifts by one rounding fails.
"""
import pytest
import torch
import torch.nn as nn

from toothgroupnetwork_amd import dgcnn, fold, nets, point_transformer as PT, pointnet, pointnet2_utils as U
from toothgroupnetwork_amd.sa_fused import pack_first_layer


def same_bits(got, want):
    return (got.dtype == want.dtype == torch.float32 and got.shape == want.shape and got.is_contiguous()
            and torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32)))


def randomise(mod, seed):
    """Seeded-random statistics and affine parameters for every BatchNorm of `mod`, which goes to eval mode."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 1.5 + 0.5)
                m.weight.copy_(torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(torch.randn(m.bias.shape, generator=g))
    return mod.eval()


def scale_shift(bn):
    scale = (bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)).float()
    return scale, (bn.bias.detach() - bn.running_mean * scale).float()


def weight2d(layer):
    return layer.weight.detach().reshape(layer.weight.shape[0], -1).float()


LAYERS = {"linear": (lambda b: nn.Linear(12, 7, bias=b), nn.BatchNorm1d), "conv1d": (lambda b: nn.Conv1d(12, 7, 1, bias=b), nn.BatchNorm1d),
          "conv2d": (lambda b: nn.Conv2d(12, 7, 1, bias=b), nn.BatchNorm2d)}


@pytest.mark.parametrize("norm", ["default", "random", "none"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("kind", sorted(LAYERS))
def test_affine_is_the_fold_formula(kind, bias, norm):
    """W' = W * scale[:, None]; b' = bias * scale + shift, shift alone without a bias; without a BatchNorm the layer's own weight and
    bias, zeros where it has none."""
    torch.manual_seed(5)
    make, Norm = LAYERS[kind]
    layer = make(bias)
    bn = None if norm == "none" else Norm(7).eval()
    if norm == "random":
        randomise(bn, 6)
    W, b = fold.affine(layer, bn)
    if bn is None:
        assert same_bits(W, weight2d(layer))
        assert same_bits(b, layer.bias.detach() if bias else torch.zeros(7))
        return
    s, t = scale_shift(bn)
    assert all(same_bits(g, w) for g, w in zip(fold.scale_shift(bn), (s, t)))
    assert same_bits(W, weight2d(layer) * s[:, None])
    assert same_bits(b, layer.bias.detach().float() * s + t if bias else t)
    x = torch.randn(9, 12)
    want = bn(layer(x[:, :, None, None] if kind == "conv2d" else x[:, :, None] if kind == "conv1d" else x)).detach().reshape(9, 7)
    assert torch.allclose(torch.nn.functional.linear(x, W, b), want, atol=1e-5)


def test_head_fold_is_two_affine_layers():
    """nets.fold_head at the head's smallest shape (32 -> 16 -> 3)"""
    torch.manual_seed(7)
    conv1, bn1, conv2 = nn.Conv1d(32, 16, 1), randomise(nn.BatchNorm1d(16), 8), nn.Conv1d(16, 3, 1)
    s, t = scale_shift(bn1)
    want = (conv1.weight.detach().squeeze(-1).float() * s[:, None], conv1.bias.detach().float() * s + t,
            conv2.weight.detach().squeeze(-1).float(), conv2.bias.detach().float())
    got = nets.fold_head(conv1, bn1, conv2)
    assert len(got) == 4 and all(same_bits(g, w) for g, w in zip(got, want))


def test_feature_propagation_stack_fold():
    """pointnet2_utils.fold_fp_stack over two layers, one without a bias (where the earlier fold carried a zero bias through)"""
    torch.manual_seed(9)
    convs = nn.ModuleList([nn.Conv1d(10, 12, 1), nn.Conv1d(12, 6, 1, bias=False)])
    bns = randomise(nn.ModuleList([nn.BatchNorm1d(12), nn.BatchNorm1d(6)]), 10)
    got = U.fold_fp_stack(convs, bns)
    assert len(got) == 2
    for (W, b), conv, bn in zip(got, convs, bns):
        sc, sh = scale_shift(bn)
        bias = conv.bias.detach().float() if conv.bias is not None else torch.zeros_like(sh)
        assert same_bits(W, conv.weight.detach().squeeze(-1).float() * sc[:, None]) and same_bits(b, bias * sc + sh)


def test_dgcnn_edge_layers_split_the_folded_weight():
    """dgcnn._edge_first_layer (12 -> 64: Wa'^T, (Wb' - Wa')^T, t) and _second_layer (64 -> 64)"""
    torch.manual_seed(11)
    conv1, bn1 = nn.Conv2d(12, 64, 1, bias=False), randomise(nn.BatchNorm2d(64), 12)
    conv2, bn2 = nn.Conv2d(64, 64, 1, bias=False), randomise(nn.BatchNorm2d(64), 13)
    s, t = scale_shift(bn1)
    W = weight2d(conv1) * s[:, None]
    Wa, Wb = W[:, :6], W[:, 6:]
    got = dgcnn._edge_first_layer(conv1, bn1)
    assert len(got) == 3 and all(same_bits(g, w) for g, w in zip(got, (Wa.t(), (Wb - Wa).t(), t)))
    s2, t2 = scale_shift(bn2)
    W2, b2 = dgcnn._second_layer(conv2, bn2)
    assert same_bits(W2, weight2d(conv2) * s2[:, None]) and same_bits(b2, t2)


@pytest.mark.parametrize("with_bn", [True, False])
def test_pointnet_transposed_fold(with_bn):
    """pointnet._folded_t (64 -> 128): the folded weight as (K, C) rows"""
    torch.manual_seed(14)
    conv, bn = nn.Conv1d(64, 128, 1), (randomise(nn.BatchNorm1d(128), 15) if with_bn else None)
    Wt, b = pointnet._folded_t(conv, bn)
    W, bias = weight2d(conv), conv.bias.detach().float()
    if with_bn:
        s, t = scale_shift(bn)
        W, bias = W * s[:, None], bias * s + t
    assert same_bits(Wt, W.t()) and same_bits(b, bias)


def test_pt_attention_layer_fold():
    """point_transformer._fold_pt_layer (c = 32, share_planes = 8): the ten operands of tgn_pt_attention_forward"""
    torch.manual_seed(16)
    layer = randomise(PT.PointTransformerLayer(32, 32, 8, 16), 17)
    lp0, bnp, lp3 = layer.linear_p[0], layer.linear_p[1], layer.linear_p[3]
    bnw0, lw2, bnw3, lw5 = layer.linear_w[0], layer.linear_w[2], layer.linear_w[3], layer.linear_w[5]
    sp, tp = scale_shift(bnp)
    a1, t1 = scale_shift(bnw0)
    s3, t3 = scale_shift(bnw3)
    f = lambda t: t.detach().float().contiguous()                                # noqa: E731
    want = dict(Wp1=f(lp0.weight * sp[:, None]), bp1=f(lp0.bias * sp + tp), Wp2=f(lp3.weight), bp2=f(lp3.bias), a1=f(a1), t1=f(t1),
                Ww1=f(lw2.weight * s3[:, None]), bw1=f(lw2.bias * s3 + t3), Ww2=f(lw5.weight), bw2=f(lw5.bias))
    got = PT._fold_pt_layer(lp0, bnp, lp3, bnw0, lw2, bnw3, lw5)
    assert sorted(got) == sorted(want)
    for k in want:
        assert same_bits(got[k], want[k]), k
    memo = PT.fold_pt_layer(layer)                                               # the memoised entry point: the same ten operands
    assert sorted(memo) == sorted(want) and all(same_bits(memo[k], want[k]) for k in want)


def test_transition_down_operands():
    """point_transformer.fold_transition_down (c = 8 -> 16, stride 4): pack_first_layer of the bias-free linear layer with the
    BatchNorm's scale and shift, columns [xyz, features]"""
    torch.manual_seed(18)
    td = randomise(PT.TransitionDown(8, 16, 4, 16), 19)
    s, t = scale_shift(td.bn)
    f = pack_first_layer(td.linear.weight.detach().float(), None, s, t, 8, True)
    got = PT.fold_transition_down(td, 8)
    assert len(got) == 3 and all(same_bits(g, w) for g, w in zip(got, (f["Wt"], f["Wxs"], f["b"])))
    assert got[0].shape == (11, 16) and got[1].shape == (3, 16) and same_bits(got[2], t)
