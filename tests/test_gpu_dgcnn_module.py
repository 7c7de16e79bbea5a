"""GPU: the DGCNN mirror (dgcnn.DGCnnModule) at the inference shape, 24 000 points.

  * Each level's neighbour indices are the contract kNN (tests/test_gpu_dgcnn_knn.py) of the features that level received.
  * cls_pred of the fused eval forward lies within 2x of what the reference's own formulation in fp32 (dgcnn.py:94-143: materialised
    edge tensors, Conv2d + BatchNorm + LeakyReLU, the 1216-channel conv7) achieves against the same formulation in float64, both
    on the indices the module used (so the comparison is of arithmetic, not of neighbour choice), with a floor of 1e-5.
  * Train mode (BatchNorm batch statistics over the (B, N, k) edges) runs the reference formulation on the new kNN: its loss and
    gradients equal that formulation's on the same indices, and the parameters all receive a gradient.
  * inference.InferencePipeLine(DGCnnModule) labels every vertex of a synthetic OBJ."""
import copy
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_gpu_dgcnn_knn import contract_knn

sys.path.insert(0, GOLDEN)
from seeded import seeded_fill  # noqa: E402

pytestmark = pytest.mark.gpu

# Gradients are held to GRAD_TOL of their norm.  conv6's global max over the points and the max over the neighbours send each
# channel's gradient to ONE element; where two candidates lie within fp32 noise of each other, a different summation order (conv7 in
# two sums here, a CPU GEMM in the fixture) can pick the other one and move the early layers' gradients by ~1e-3 of their norm
# (measured: up to 1.1e-2 against the CPU reference, at bn3.bias), while the loss agrees to 1e-5.  A gradient that is zero but for
# rounding (bn6.bias: BatchNorm's shift ahead of a max, norm ~1e-7) is held to FLOOR times the largest gradient norm instead.
GRAD_TOL, FLOOR = 3e-2, 1e-3


def _err(got, want):
    got, want = got.double(), want.double()
    return float(((got - want).abs() / (1.0 + want.abs())).max())


def reference_forward(net, x, idx):
    """dgcnn.py:94-143 on given neighbour indices (the module's own submodules, any dtype)."""
    from toothgroupnetwork_amd.dgcnn import get_graph_feature
    k = net.k
    x1 = net.conv2(net.conv1(get_graph_feature(x, k=k, idx=idx[0]))).max(dim=-1)[0]
    x2 = net.conv4(net.conv3(get_graph_feature(x1, k=k, idx=idx[1]))).max(dim=-1)[0]
    x3 = net.conv5(get_graph_feature(x2, k=k, idx=idx[2])).max(dim=-1)[0]
    x = torch.cat((x1, x2, x3), dim=1)
    g = net.conv6(x).max(dim=-1, keepdim=True)[0].repeat(1, 1, x.shape[-1])
    x = net.conv8(net.conv7(torch.cat((g, x), dim=1)))
    return net.cls_conv(net.dp1(x))


def _net(dev, seed=81):
    from toothgroupnetwork_amd import nets
    net = nets.DGCnnModule({})
    seeded_fill(net, seed)
    return net.to(dev).eval()


def _scan(dev, B=1, N=24000, seed=4):
    from toothgroupnetwork_amd import synth
    return torch.from_numpy(np.ascontiguousarray(synth.scan_batch(B, N, "arch", seed=seed).transpose(0, 2, 1))).to(dev)


def test_eval_forward_indices_and_accuracy_at_24000_points(dev, monkeypatch):
    from toothgroupnetwork_amd import dgcnn
    net = _net(dev)
    x = _scan(dev)
    seen = []
    real_knn = dgcnn.knn
    monkeypatch.setattr(dgcnn, "knn", lambda feats, k: (seen.append(feats.clone()), real_knn(feats, k))[1])
    with torch.no_grad():
        got = net([x])["cls_pred"]
    assert got.shape == (1, 17, 24000) and got.dtype == torch.float32
    assert len(seen) == 3 and len(net.last_idx) == 3
    for lvl, (feats, idx) in enumerate(zip(seen, net.last_idx)):
        assert feats.shape == (1, 6 if lvl == 0 else 64, 24000)
        assert torch.equal(idx, contract_knn(feats, 20)[0]), f"level {lvl}"
    idx = net.last_idx
    with torch.no_grad():
        r32 = reference_forward(net, x, idx)
        net64 = copy.deepcopy(net).double()
        r64 = reference_forward(net64, x.double(), idx)
    e, own = _err(got, r64), _err(r32, r64)
    print(f"\nDGCnnModule eval at 24 000 points: fused vs float64 {e:.3g}, reference formulation fp32 vs float64 {own:.3g}")
    assert e <= max(1e-5, 2.0 * own), (e, own)


def test_eval_forward_batch_of_two_equals_two_single_scans(dev):
    net = _net(dev)
    x = _scan(dev, B=2, N=4096, seed=6)
    with torch.no_grad():
        both = net([x])["cls_pred"]
        idx_both = net.last_idx
        one = net([x[1:2]])["cls_pred"]
        idx_one = net.last_idx
    for a, b in zip(idx_both, idx_one):
        assert torch.equal(a[1:2], b)
    # the same indices and the same per-point arithmetic; only the GEMMs' blocking may differ with the batch size
    assert _err(both[1:2], one) <= 1e-5


def test_train_mode_matches_the_reference_formulation(dev):
    net = _net(dev).train()
    net.dp1.eval()                                        # dropout off: the comparison is deterministic
    x = _scan(dev, B=2, N=2048, seed=8)
    labels = torch.randint(0, 17, (2, 2048), device=dev)
    out = net([x])["cls_pred"]
    loss = torch.nn.functional.cross_entropy(out, labels)
    loss.backward()
    grads = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    # every parameter but the two heads the reference computes and never returns (dgcnn.py:129-130) receives a gradient
    assert sorted(n for n, _ in net.named_parameters() if n not in grads) == ["dist_conv.weight", "offset_conv.weight"]
    assert all(torch.isfinite(g).all() for g in grads.values())
    ref = _net(dev).train()                               # the same seeded weights; train mode normalises by batch statistics
    ref.dp1.eval()
    out_r = reference_forward(ref, x, net.last_idx)
    loss_r = torch.nn.functional.cross_entropy(out_r, labels)
    loss_r.backward()
    assert torch.allclose(loss, loss_r, rtol=1e-5, atol=0)      # (conv7 split in two sums: fp32 order only)
    top = max(float(p.grad.double().norm()) for p in ref.parameters() if p.grad is not None)
    for n, p in ref.named_parameters():
        if n not in grads:
            assert p.grad is None
            continue
        norm = max(float(p.grad.double().norm()), FLOOR * top)     # fp32 order only, held to the gradient's norm (GRAD_TOL)
        assert float((grads[n] - p.grad).double().abs().max()) <= GRAD_TOL * norm, n


def test_inference_pipeline_labels_every_vertex(dev, tmp_path):
    from toothgroupnetwork_amd import inference, synth
    path = tmp_path / "scan.obj"
    path.write_text(synth.obj_text(300, 150, 11, "plain", with_tail=False))
    net = _net(dev, seed=82)
    got = inference.InferencePipeLine(net)(str(path))
    n_vertices = sum(1 for line in path.read_text().splitlines() if line.startswith("v "))
    assert got["sem"].shape == (n_vertices,)
    assert np.array_equal(got["ins"], got["sem"])
    assert set(np.unique(got["sem"]).tolist()) <= set(inference.fdi_from_classes(np.arange(17)).tolist())


# ---- against the reference's own module on CPU (tests/golden/make_golden_r8_dgcnn.py) ----------------------------------------------
@pytest.fixture(scope="module")
def r8():
    import os
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r8_dgcnn.npz")))


def _fixture_inputs(r8, dev):
    import make_golden_r8_dgcnn as M
    from crop_cases import digest
    x = M.scans()
    assert digest(x) == str(r8["input_digest"])
    net = _net(dev, seed=M.SEED)
    assert seeded_fill(net, M.SEED) == r8["params"].tolist()       # the reference's parameter names and shapes, in its order
    return M, torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dev), net.to(dev)


def _sets(r8, key, M, dev):
    from crop_cases import unpack_sets
    return torch.from_numpy(unpack_sets(r8[key])).view(M.B, M.N, M.K).to(dev)


def test_eval_forward_matches_the_reference_module_on_its_indices(dev, r8):
    M, x, net = _fixture_inputs(r8, dev)
    idx = [_sets(r8, f"eval_idx{lvl}", M, dev) for lvl in range(3)]
    with torch.no_grad():
        got = net.eval()._forward_eval(x, idx=idx)[:, :, ::2]
    want = torch.from_numpy(r8["eval_cls_64"])
    e, own = _err(got.cpu(), want), _err(torch.from_numpy(r8["eval_cls_32"]), want)
    print(f"\nDGCnnModule eval vs the reference module (CPU): fused vs float64 {e:.3g}, reference fp32 vs float64 {own:.3g}")
    assert e <= max(1e-5, 2.0 * own), (e, own)


def test_train_step_matches_the_reference_module(dev, r8, monkeypatch):
    from toothgroupnetwork_amd import dgcnn
    M, x, net = _fixture_inputs(r8, dev)
    served = iter([_sets(r8, f"train_idx{lvl}", M, dev) for lvl in range(3)])
    monkeypatch.setattr(dgcnn, "knn", lambda feats, k: next(served))
    net.train()
    net.dp1.eval()
    gt = torch.from_numpy(M.labels()).to(dev)
    pred = net([x, gt])["cls_pred"]
    loss = torch.nn.functional.cross_entropy(pred, gt.view(M.B, -1) + 1)      # tgn_loss.tooth_class_loss (tgn_loss.py:355-367)
    loss.backward()
    assert abs(float(loss) - float(r8["train_loss"])) <= 1e-5 * abs(float(r8["train_loss"]))
    worst = 0.0
    top = max(float(v) for k, v in r8.items() if k.startswith("gradnorm::"))
    for name, p in net.named_parameters():
        if f"grad::{name}" not in r8:
            assert p.grad is None, name
            continue
        g = p.grad.reshape(-1).double().cpu()
        norm = float(r8[f"gradnorm::{name}"])
        assert abs(float(g.norm()) - norm) <= GRAD_TOL * max(norm, FLOOR * top), name
        sample = g[::M.grad_stride(g.numel())]
        d = float((sample - torch.from_numpy(r8[f"grad::{name}"]).double()).abs().max()) / max(norm, FLOOR * top)
        worst = max(worst, d)
        assert d <= GRAD_TOL, (name, d)
    print(f"\nDGCnnModule train step vs the reference module (CPU): loss {float(loss):.6f}, worst gradient sample error / norm {worst:.2e}")
