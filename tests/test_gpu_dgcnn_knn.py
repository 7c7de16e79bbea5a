"""GPU: DGCNN's feature-space kNN (tgn_feature_knn, dgcnn.knn) against its contract and against exact and reference top-k sets.

The contract (include/tgn_pointops.h): row i holds the k smallest fp32 direct-form distances acc = acc + t*t, t = x_i[c] - x_j[c],
c = 0..D-1 in order, every operation rounded, in ascending (distance, index) order.  `contract_knn` restates it with torch elementwise
operations (one multiply and one add per channel, never fused) and a stable sort, so the kernel must match it bit for bit, indices
and distances, whatever its splits and merges.

Against the float64 exact top k.  t = fl(x_i - x_j) = (x_i - x_j)(1 + e1), t*t gains one more rounding, and a recursive sum of D
non-negative terms gains at most (D - 1) roundings of a partial sum no larger than the total: |d_fp32 - d| <= ((D - 1) + 3) u d
+ O(u^2) <= (D + 3) u d, u = 2^-24.  Two rows' k-th and (k+1)-th distances can therefore trade places only when their float64 gap is
at most (D + 3) u (d_k + d_k+1) <= 2 (D + 3) u d_k+1; elsewhere the index SETS must be equal.

Against the reference's expanded form -|x_i|^2 + 2 x_i.x_j - |x_j|^2 (dgcnn.py:4-10, matmul + topk, restated in torch on the GPU):
each of the three terms carries a relative error of at most (D + 2) u of its magnitude (a D-term dot product), so the distance is
off by at most (D + 2) u (|x_i|^2 + 2 |x_i||x_j| + |x_j|^2) <= 2 (D + 2) u (|x_i|^2 + |x_j|^2); rows whose float64 gap lies within
twice the largest such error over the row's candidates are left out, the rest must have equal sets."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U_RND = 2.0 ** -24


def contract_knn(x, k, rows=512):
    """(idx, dist2) of the contract, by torch elementwise operations and sort(stable=True)."""
    B, D, N = x.shape
    idx = torch.empty(B, N, k, dtype=torch.long, device=x.device)
    dist = torch.empty(B, N, k, dtype=torch.float32, device=x.device)
    for b in range(B):
        for r0 in range(0, N, rows):
            r1 = min(N, r0 + rows)
            acc = torch.zeros(r1 - r0, N, dtype=torch.float32, device=x.device)
            for c in range(D):
                t = x[b, c, r0:r1, None] - x[b, c, None, :]
                acc = acc + t * t
            d, i = torch.sort(acc, dim=1, stable=True)
            idx[b, r0:r1], dist[b, r0:r1] = i[:, :k], d[:, :k]
    return idx, dist


def exact_rows(x, k, rows=512):
    """float64 distances: the (k+1) smallest per row (values) and the k-set (sorted indices)."""
    B, D, N = x.shape
    xd = x.double()
    sets, vals = [], []
    for b in range(B):
        for r0 in range(0, N, rows):
            r1 = min(N, r0 + rows)
            d = ((xd[b, :, r0:r1, None] - xd[b, :, None, :]) ** 2).sum(0)
            v, i = torch.topk(d, min(k + 1, N), dim=1, largest=False, sorted=True)
            sets.append(i[:, :k].sort(dim=1)[0])
            vals.append(v)
    return torch.cat(sets).view(B, N, k), torch.cat(vals).view(B, N, -1)


def reference_knn(x, k):
    """dgcnn.py:4-10 as the reference writes it (fp32 matmul + topk)."""
    inner = -2 * torch.matmul(x.transpose(2, 1), x)
    xx = torch.sum(x ** 2, dim=1, keepdim=True)
    pairwise_distance = -xx - inner - xx.transpose(2, 1)
    return pairwise_distance.topk(k=k, dim=-1)[1]


def _scan(B, N, D, seed, kind="arch"):
    from toothgroupnetwork_amd import synth
    if D == 6 and kind == "arch":
        return torch.from_numpy(np.ascontiguousarray(synth.scan_batch(B, N, "arch", seed=seed).transpose(0, 2, 1)))
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, D, N, generator=g)


def _check_contract(x, k):
    from toothgroupnetwork_amd import dgcnn
    got_i, got_d = dgcnn.feature_knn(x, k)
    want_i, want_d = contract_knn(x, k)
    torch.cuda.synchronize()
    assert got_i.dtype == torch.long and got_i.shape == (x.shape[0], x.shape[2], k)
    bad = (got_i != want_i).any(dim=-1)
    assert not bad.any(), f"{int(bad.sum())} rows differ, first at {bad.nonzero()[0].tolist()}"
    assert torch.equal(got_d.view(torch.int32), want_d.view(torch.int32))
    assert torch.equal(dgcnn.knn(x, k), got_i)    # deterministic
    return got_i, got_d


@pytest.mark.parametrize("B,N,D,k", [(2, 24000, 6, 20), (1, 24000, 64, 20)])
def test_knn_bit_equal_to_the_contract_at_network_shapes(dev, B, N, D, k):
    _check_contract(_scan(B, N, D, seed=B + D).to(dev), k)


@pytest.mark.parametrize("N", [20, 21, 1000])
def test_knn_short_clouds(dev, N):
    _check_contract(_scan(2, N, 3, seed=N).to(dev), 20)


@pytest.mark.parametrize("D", [1, 3, 64])
@pytest.mark.parametrize("k", [1, 20, 32])
def test_knn_dimensions_and_k(dev, D, k):
    x = _scan(1, 3000, D, seed=7 * D + k).to(dev)
    idx, dist = _check_contract(x, k)
    # every point is its own neighbour at distance 0 (the first one unless a lower-index duplicate exists)
    assert (dist[..., 0] == 0).all()
    if D >= 3:
        assert torch.equal(idx[..., 0], torch.arange(3000, device=dev).expand(1, -1))


def test_knn_duplicated_vertices_tie_at_zero_in_index_order(dev):
    """Raw scans hold duplicated vertices: ties at distance 0 come in ascending index order, so a lower-index copy precedes i."""
    from toothgroupnetwork_amd import synth
    pts = synth.lattice_cloud(16, dup=600, seed=2)                   # 4 096 lattice points + 600 copies, shuffled
    x = torch.from_numpy(np.ascontiguousarray(pts.T[None])).to(dev)
    idx, dist = _check_contract(x, 20)
    n_zero = (dist == 0).sum(-1)
    assert (n_zero >= 2).sum() >= 600
    first_zero = torch.where(dist == 0, idx, torch.full_like(idx, 1 << 40)).min(-1)[0]
    assert torch.equal(idx[..., 0], first_zero)


def test_knn_on_a_non_default_stream(dev):
    from toothgroupnetwork_amd import dgcnn
    x = _scan(2, 5000, 64, seed=11).to(dev)
    want_i, want_d = contract_knn(x, 20)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got_i, got_d = dgcnn.feature_knn(x, 20)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(got_i, want_i) and torch.equal(got_d, want_d)


@pytest.mark.parametrize("B,N,D", [(2, 24000, 6), (1, 24000, 64)])
def test_knn_sets_equal_the_exact_top_k_outside_the_fp32_bound(dev, B, N, D):
    from toothgroupnetwork_amd import dgcnn
    k = 20
    x = _scan(B, N, D, seed=3 + D).to(dev)
    got = dgcnn.knn(x, k).sort(dim=-1)[0]
    want, vals = exact_rows(x, k)
    gap = vals[..., k] - vals[..., k - 1]
    close = gap <= 2 * (D + 3) * U_RND * vals[..., k]
    differ = (got != want).any(-1)
    print(f"\nknn B={B} N={N} D={D}: {int(close.sum())} rows within the fp32 bound, {int(differ.sum())} differing sets")
    assert not (differ & ~close).any(), int((differ & ~close).sum())


@pytest.mark.parametrize("B,N,D", [(2, 24000, 6), (1, 24000, 64)])
def test_knn_sets_equal_the_reference_expanded_form_outside_its_bound(dev, B, N, D):
    from toothgroupnetwork_amd import dgcnn
    k = 20
    x = _scan(B, N, D, seed=5 + D).to(dev)
    got = dgcnn.knn(x, k).sort(dim=-1)[0]
    ref = reference_knn(x, k).sort(dim=-1)[0]
    _, vals = exact_rows(x, k)
    sq = (x.double() ** 2).sum(1)                                       # (B, N)
    err = 2 * (D + 2) * U_RND * (sq + sq.max(dim=1, keepdim=True)[0])   # per row: the largest error over its candidates
    close = (vals[..., k] - vals[..., k - 1]) <= 2 * err
    differ = (got != ref).any(-1)
    print(f"\nknn vs expanded form B={B} N={N} D={D}: {int(close.sum())} rows within its bound, {int(differ.sum())} differing sets")
    assert not (differ & ~close).any(), int((differ & ~close).sum())
    assert close.float().mean() < 0.5                                   # the comparison covers most rows


def test_knn_refuses_what_it_does_not_support(dev):
    from toothgroupnetwork_amd import dgcnn
    x = torch.randn(1, 6, 100, device=dev)
    with pytest.raises(RuntimeError, match="bad arguments"):
        dgcnn.knn(x[..., :10], 20)                                      # k > N, as torch.topk refuses
    with pytest.raises(RuntimeError, match="bad arguments"):
        dgcnn.knn(torch.randn(1, 65, 100, device=dev), 20)              # D > 64
    with pytest.raises(RuntimeError, match="bad arguments"):
        dgcnn.knn(x, 33)                                                # k > 32
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dgcnn.knn(x.cpu(), 20)
