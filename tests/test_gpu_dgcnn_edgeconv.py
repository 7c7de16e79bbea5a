"""GPU: the fused EdgeConv levels of DGCNN (tgn_edgeconv2_max, tgn_edgeconv1_max through dgcnn.edgeconv_max) held to a float64 error
bound scaled by their terms, and get_graph_feature against the reference's formula.

The kernels do not compute what the reference computes (dgcnn.py:13-40 and the conv1 .. conv5 blocks): BatchNorm is folded into the
weights (dgcnn._edge_first_layer / _second_layer), the first layer is commuted with the gather,
W' [x_j - x_i ; x_i] + t = Wa' x_j + (Wb' - Wa') x_i + t = P_j + Q_i with P and Q per point, and the second layer runs on fp32 MFMA.
As in tests/test_gpu_sa_forward_bounds.py, each test restates that algorithm in float64 and returns for every output the value and the
magnitude M, the sum of the absolute values of the terms the algorithm adds:
  first layer    M1 = |Wa'| |x_j| + (|Wb'| + |Wa'|) |x_i| + |t terms|   (Wb' - Wa' is formed in fp32)
  second layer   M2 = |W2'| (|h1| + M1) + |b2' terms|     (layer 1's bound through the 1-Lipschitz LeakyReLU)
  max over k     M_out = max_j M
and asserts |got - want| <= C u M, C = 8 max(1, sqrt(n / 16)), n the longest fp32 chain (2C + 2 for the first layer, 64 for the
second); that test's derivation applies unchanged, LeakyReLU(0.2) being 1-Lipschitz like ReLU."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

U_RND = 2.0 ** -24


def chain_const(n):
    return 8.0 * max(1.0, math.sqrt(n / 16.0))


def _bn_fold64(conv, bn):
    C = conv.out_channels
    W = conv.weight.detach().double().reshape(C, -1)
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    mu, beta = bn.running_mean.double(), bn.bias.detach().double()
    return W * s[:, None], beta - s * mu, beta.abs() + (s * mu).abs()


def _layers(C, dev, seed):
    g = torch.Generator().manual_seed(seed)
    conv1, bn1 = torch.nn.Conv2d(2 * C, 64, 1, bias=False), torch.nn.BatchNorm2d(64)
    conv2, bn2 = torch.nn.Conv2d(64, 64, 1, bias=False), torch.nn.BatchNorm2d(64)
    for bn in (bn1, bn2):
        bn.weight.data = 0.5 + torch.rand(64, generator=g)
        bn.bias.data = 0.2 * torch.randn(64, generator=g)
        bn.running_mean.copy_(0.3 * torch.randn(64, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(64, generator=g))
    for conv in (conv1, conv2):
        conv.weight.data = torch.randn(conv.weight.shape, generator=g) / math.sqrt(conv.in_channels)
    return [m.to(dev).eval() for m in (conv1, bn1, conv2, bn2)]


def edge_level64(x, idx, conv1, bn1, conv2=None, bn2=None):
    """(want, M) of one level in float64: x (B, C, N), idx (B, N, K) -> (B, 64, N) each."""
    B, C, N = x.shape
    W1, t1, t1m = _bn_fold64(conv1, bn1)
    Wa, Wd = W1[:, :C], W1[:, C:] - W1[:, :C]
    xd = x.double()
    P, Pm = torch.einsum("oc,bcn->bon", Wa, xd), torch.einsum("oc,bcn->bon", Wa.abs(), xd.abs())
    Q = torch.einsum("oc,bcn->bon", Wd, xd) + t1[None, :, None]
    Qm = torch.einsum("oc,bcn->bon", W1[:, :C].abs() + W1[:, C:].abs(), xd.abs()) + t1m[None, :, None]   # Wb' - Wa' is a sum too
    flat = (idx + torch.arange(B, device=x.device).view(-1, 1, 1) * N).reshape(-1)

    def gather(T):                                          # (B, 64, N) -> (B, 64, N, K) of the neighbours
        return T.permute(0, 2, 1).reshape(B * N, -1)[flat].view(B, N, -1, 64).permute(0, 3, 1, 2)
    pre = gather(P) + Q[..., None]
    M1 = gather(Pm) + Qm[..., None]
    h1 = torch.nn.functional.leaky_relu(pre, 0.2)
    if conv2 is None:
        return h1.max(-1)[0], M1.max(-1)[0], 2 * C + 2
    W2, t2, t2m = _bn_fold64(conv2, bn2)
    y = torch.einsum("oc,bcnk->bonk", W2, h1) + t2[None, :, None, None]
    M2 = torch.einsum("oc,bcnk->bonk", W2.abs(), h1.abs() + M1) + t2m[None, :, None, None]
    return torch.nn.functional.leaky_relu(y, 0.2).max(-1)[0], M2.max(-1)[0], max(64, 2 * C + 2)


@pytest.mark.parametrize("C", [6, 64])
@pytest.mark.parametrize("two", [True, False])
@pytest.mark.parametrize("K", [20, 7, 32])
def test_fused_edgeconv_within_the_term_scaled_bound(dev, C, two, K):
    from toothgroupnetwork_amd import dgcnn
    B, N = 1, 24000
    g = torch.Generator().manual_seed(C * 100 + K)
    x = torch.randn(B, C, N, generator=g).to(dev)
    idx = torch.randint(0, N, (B, N, K), generator=g)
    idx[..., K // 2:] = idx[..., :K - K // 2]                 # ragged neighbour sets with repeated indices
    idx = idx.to(dev)
    conv1, bn1, conv2, bn2 = _layers(C, dev, seed=C + K)
    first = dgcnn._edge_first_layer(conv1, bn1)
    second = dgcnn._second_layer(conv2, bn2) if two else None
    out = torch.full((B, 192, N), float("nan"), device=dev)
    dgcnn.edgeconv_max(x, idx, first, second, out=out, coff=64)
    got = out[:, 64:128].double()
    assert torch.isnan(out[:, :64]).all() and torch.isnan(out[:, 128:]).all()      # only its channel slice is written
    want, M, n = edge_level64(x, idx, conv1, bn1, *((conv2, bn2) if two else ()))
    ratio = ((got - want).abs() / (U_RND * M)).max().item()
    print(f"\nedgeconv C={C} K={K} two={two}: worst |got - want| / (u M) = {ratio:.2f} (bound {chain_const(n):.1f})")
    assert ratio <= chain_const(n)


def test_fused_edgeconv_batch_two_reads_its_own_scan(dev):
    from toothgroupnetwork_amd import dgcnn
    B, N, C, K = 2, 3000, 64, 20
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, C, N, generator=g).to(dev)
    idx = dgcnn.knn(x, K)
    conv1, bn1, conv2, bn2 = _layers(C, dev, seed=1)
    out = dgcnn.edgeconv_max(x, idx, dgcnn._edge_first_layer(conv1, bn1), dgcnn._second_layer(conv2, bn2))
    want, M, n = edge_level64(x, idx, conv1, bn1, conv2, bn2)
    assert ((out.double() - want).abs() <= chain_const(n) * U_RND * M).all()


def test_fused_edgeconv_raises_on_a_bad_index(dev):
    from toothgroupnetwork_amd import dgcnn
    x = torch.randn(1, 6, 100, device=dev)
    idx = torch.randint(0, 100, (1, 100, 20), device=dev)
    idx[0, 5, 3] = 100
    conv1, bn1, conv2, bn2 = _layers(6, dev, seed=2)
    with pytest.raises(IndexError):
        dgcnn.edgeconv_max(x, idx, dgcnn._edge_first_layer(conv1, bn1), dgcnn._second_layer(conv2, bn2))
    idx[0, 5, 3] = -1
    with pytest.raises(IndexError):
        dgcnn.edgeconv_max(x, idx, dgcnn._edge_first_layer(conv1, bn1))


def reference_graph_feature(x, k=20, idx=None):
    """dgcnn.py:13-40 verbatim in substance (with the device taken from x)."""
    batch_size, num_points = x.size(0), x.size(2)
    x = x.view(batch_size, -1, num_points)
    idx_base = torch.arange(0, batch_size, device=x.device).view(-1, 1, 1) * num_points
    idx = (idx + idx_base).view(-1)
    _, num_dims, _ = x.size()
    x = x.transpose(2, 1).contiguous()
    feature = x.view(batch_size * num_points, -1)[idx, :].view(batch_size, num_points, k, num_dims)
    x = x.view(batch_size, num_points, 1, num_dims).repeat(1, 1, k, 1)
    return torch.cat((feature - x, x), dim=3).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("C", [6, 64])
def test_get_graph_feature_bit_equal_to_the_reference_formula(dev, C):
    from toothgroupnetwork_amd import dgcnn
    x = torch.randn(2, C, 2048, device=dev)
    idx = dgcnn.knn(x, 20)
    got = dgcnn.get_graph_feature(x, k=20)
    assert got.shape == (2, 2 * C, 2048, 20)
    assert torch.equal(got, reference_graph_feature(x, 20, idx))
    assert torch.equal(dgcnn.get_graph_feature(x, k=20, idx=idx, dim9=True), got)
