"""GPU: the PointNet mirror (pointnet.PointFirstModule) against the reference's own module on CPU
(tests/golden/make_golden_r15_pointnet.py).

  * The fused eval forward lies within 2x of what the reference's fp32 pass achieves against its float64 pass (floor 1e-5): the
    criterion tests/test_gpu_dgcnn_module.py uses for a fused network against the reference's own fp32 noise.
  * It calls the fused linear + max kernel exactly three times (128 -> 1024 twice, 256 -> 2048) and never builds a tensor of 2048 or
    2176 channels by N.
  * A batch of two equals its two scans alone.
  * Train mode is the reference's formulation: loss and gradients equal the fixture's, every parameter receives a gradient.
  * A state_dict with the reference's keys loads with strict=True, and inference.InferencePipeLine labels every vertex of an OBJ.
  * The wrapper pointnet.linear_act_max casts and packs what is not packed float32 and names the argument it refuses.

Measured on one MI355X: e = 1.47e-5 for the log-probabilities (bound 1.66e-5 = 2 x own, own = 8.28e-6) and 1.03e-6 for trans_feat; with
the eval path's float64 pieces in fp32, and for the reference's own formulation in fp32 on the same GPU, e = 2.7e-5."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
from seeded import seeded_fill  # noqa: E402

pytestmark = pytest.mark.gpu

# the project's values for a global max that routes each channel's gradient to ONE point (tests/test_gpu_dgcnn_module.py)
GRAD_TOL, FLOOR = 3e-2, 1e-3


def _err(got, want):
    got, want = got.double(), want.double()
    return float(((got - want).abs() / (1.0 + want.abs())).max())


@pytest.fixture(scope="module")
def r15():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r15_pointnet.npz")))


def _fixture_inputs(r15, dev):
    import make_golden_r15_pointnet as M
    from crop_cases import digest
    from toothgroupnetwork_amd import nets
    x = M.scans()
    assert digest(x) == str(r15["input_digest"])
    net = nets.PointFirstModule({})
    assert seeded_fill(net, M.SEED) == r15["params"].tolist()
    return M, torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dev), net.to(dev)


class _Spy:
    """Records every call of pointnet.linear_act_max, and every torch.cat / Tensor.repeat result's shape."""

    def __init__(self, monkeypatch):
        from toothgroupnetwork_amd import pointnet
        self.calls, self.built = [], []
        real, real_cat, real_repeat = pointnet.linear_act_max, torch.cat, torch.Tensor.repeat

        def spy(x, conv, bn, act, slope=0.0):
            out = real(x, conv, bn, act, slope)
            self.calls.append((tuple(x.shape), conv.in_channels, conv.out_channels, act, x.clone(), out.clone()))
            return out

        def cat(*a, **k):
            out = real_cat(*a, **k)
            self.built.append(tuple(out.shape))
            return out

        def repeat(t, *a):
            out = real_repeat(t, *a)
            self.built.append(tuple(out.shape))
            return out
        monkeypatch.setattr(pointnet, "linear_act_max", spy)
        monkeypatch.setattr(torch, "cat", cat)
        monkeypatch.setattr(torch.Tensor, "repeat", repeat)


def test_eval_forward_matches_the_reference_module(dev, r15):
    M, x, net = _fixture_inputs(r15, dev)
    net.eval()
    with torch.no_grad():
        logp, trans_feat = net.first_sem_model([x])
        out = net([x])["cls_pred"]
    assert torch.equal(out, logp) and logp.shape == (M.B, 17, M.N) and logp.dtype == torch.float32
    assert trans_feat.shape == (M.B, 128, 128)
    own = float(r15["own"])
    e = _err(logp[:, :, ::2].cpu(), torch.from_numpy(r15["eval_cls_64"]))
    et = _err(trans_feat.cpu(), torch.from_numpy(r15["eval_trans_64"]))
    print(f"\nPointFirstModule eval vs the reference module (CPU, float64): log-probs e = {e:.3g}, trans_feat {et:.3g}; "
          f"reference fp32 vs float64 own = {own:.3g} (trans_feat {float(r15['own_trans']):.3g})")
    assert e <= max(1e-5, 2.0 * own), (e, own)
    assert et <= max(1e-5, 2.0 * own), (et, own)


def test_eval_forward_runs_three_fused_layers_and_no_wide_tensor(dev, r15, monkeypatch):
    M, x, net = _fixture_inputs(r15, dev)
    net.eval()
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        net([x])
    assert [(c[0], c[1], c[2], c[3]) for c in spy.calls] == [((M.B, 128, M.N), 128, 1024, "relu"), ((M.B, 128, M.N), 128, 1024, "relu"),
                                                            ((M.B, 256, M.N), 256, 2048, "identity")]
    assert [tuple(c[5].shape) for c in spy.calls] == [(M.B, 1024), (M.B, 1024), (M.B, 2048)]
    wide = [s for s in spy.built if len(s) == 3 and s[1] in (2048, 2176) and s[2] == M.N]
    assert wide == [], spy.built
    # the same spy does see them in the reference's formulation
    spy.built.clear()
    with torch.no_grad():
        net.first_sem_model._forward_train(x)
    assert (M.B, 2048, M.N) in spy.built and (M.B, 2176, M.N) in spy.built and len(spy.calls) == 3


def test_eval_forward_batch_of_two_equals_two_single_scans(dev, r15, monkeypatch):
    _, x, net = _fixture_inputs(r15, dev)
    net.eval()
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        both = net([x])["cls_pred"]
        singles = [net([x[b:b + 1]])["cls_pred"] for b in range(2)]
    assert len(spy.calls) == 9
    for b in range(2):
        assert _err(both[b:b + 1], singles[b]) <= 1e-5
        for layer in range(3):
            assert torch.equal(spy.calls[layer][5][b:b + 1], spy.calls[3 + 3 * b + layer][5]), (b, layer)


def test_train_step_matches_the_reference_module(dev, r15):
    M, x, net = _fixture_inputs(r15, dev)
    net.train()
    gt = torch.from_numpy(M.labels()).to(dev)
    pred = net([x, gt])["cls_pred"]
    loss = torch.nn.functional.cross_entropy(pred, gt.view(M.B, -1) + 1)      # tgn_loss.tooth_class_loss (tgn_loss.py:355-367)
    loss.backward()
    print(f"\nPointFirstModule train step: loss {float(loss):.6f}, fixture {float(r15['train_loss']):.6f}")
    assert abs(float(loss) - float(r15["train_loss"])) <= 1e-5 * abs(float(r15["train_loss"]))
    worst = 0.0
    top = max(float(v) for k, v in r15.items() if k.startswith("gradnorm::"))
    for name, p in net.named_parameters():
        assert p.grad is not None and f"grad::{name}" in r15, name
        g = p.grad.reshape(-1).double().cpu()
        norm = float(r15[f"gradnorm::{name}"])
        assert abs(float(g.norm()) - norm) <= GRAD_TOL * max(norm, FLOOR * top), name
        sample = g[::M.grad_stride(g.numel())]
        d = float((sample - torch.from_numpy(r15[f"grad::{name}"]).double()).abs().max()) / max(norm, FLOOR * top)
        worst = max(worst, d)
        assert d <= GRAD_TOL, (name, d)
    print(f"worst gradient sample error / norm {worst:.2e}")


def test_a_reference_checkpoint_loads_strictly(dev, r15):
    from toothgroupnetwork_amd import nets
    sd = {}
    g = torch.Generator().manual_seed(3)
    for entry in r15["params"].tolist():
        name, shape = entry.rsplit(":", 1)
        sd[name] = torch.rand([int(s) for s in shape.split("x")], generator=g) + 0.5
        if name.endswith(".running_mean"):
            sd[name[:-len("running_mean")] + "num_batches_tracked"] = torch.tensor(7)
    net = nets.PointFirstModule({})
    net.load_state_dict(sd, strict=True)
    net.to(dev)
    for name, t in net.state_dict().items():
        assert torch.equal(t.cpu(), sd[name]), name


def test_inference_pipeline_labels_every_vertex(dev, tmp_path):
    from toothgroupnetwork_amd import inference, nets, synth
    path = tmp_path / "scan.obj"
    path.write_text(synth.obj_text(300, 150, 11, "plain", with_tail=False))
    net = nets.PointFirstModule({})
    seeded_fill(net, 152)
    got = inference.InferencePipeLine(net.to(dev).eval())(str(path))
    n_vertices = sum(1 for line in path.read_text().splitlines() if line.startswith("v "))
    assert got["sem"].shape == (n_vertices,)
    assert np.array_equal(got["ins"], got["sem"])
    assert set(np.unique(got["sem"]).tolist()) <= set(inference.fdi_from_classes(np.arange(17)).tolist())


def test_wrapper_packs_its_input_and_names_what_it_refuses(dev):
    from toothgroupnetwork_amd import pointnet
    g = torch.Generator().manual_seed(5)
    conv, bn = torch.nn.Conv1d(70, 100, 1), torch.nn.BatchNorm1d(100)
    seeded_fill(conv, 1), seeded_fill(bn, 2)
    conv, bn = conv.to(dev), bn.to(dev).eval()
    base = torch.randn(2, 300, 2 * 70 + 1, generator=g, dtype=torch.float64).to(dev)
    x = base.transpose(1, 2)[:, 1::2]                              # (2, 70, 300) float64, strided, offset
    assert not x.is_contiguous()
    packed = x.float().contiguous()
    with torch.no_grad():
        for act, slope, f in (("identity", 0.0, lambda y: y), ("relu", 0.0, torch.relu),
                              ("leaky_relu", 0.2, lambda y: torch.nn.functional.leaky_relu(y, 0.2))):
            got = pointnet.linear_act_max(x, conv, bn, act, slope)
            assert got.dtype == torch.float32 and got.shape == (2, 100)
            assert torch.equal(got, pointnet.linear_act_max(packed, conv, bn, act, slope)), act
            want = f(bn(conv(packed))).max(dim=2)[0]
            assert _err(got, want) <= 1e-5, act
        with pytest.raises(ValueError, match="linear_act_max: x must be"):
            pointnet.linear_act_max(packed[0], conv, bn, "relu")
        with pytest.raises(ValueError, match="linear_act_max: x has 60 channels"):
            pointnet.linear_act_max(packed[:, :60], conv, bn, "relu")
        with pytest.raises(TypeError, match="linear_act_max: x must be a floating-point"):
            pointnet.linear_act_max(packed.long(), conv, bn, "relu")
        with pytest.raises(ValueError, match="linear_act_max: act must be"):
            pointnet.linear_act_max(packed, conv, bn, "gelu")
        with pytest.raises(TypeError, match="linear_act_max: bn must be"):
            pointnet.linear_act_max(packed, conv, torch.nn.LayerNorm(100).to(dev), "relu")
        with pytest.raises(TypeError, match="linear_act_max: conv must be"):
            pointnet.linear_act_max(packed, torch.nn.Linear(70, 100).to(dev), bn, "relu")
