"""GPU: tgnet's two-stage boundary network (nets.PointTransformerSeg(block_num=2), inference_pipeline_maker.py:43-54) against the reference's
class run on CPU (tests/golden/make_golden_r16_tgnet.py): the reference's seeded weights load strictly, and the eval forward at N = 1024
lies within the bound tests/test_gpu_r4_parity.py applies to the five-stage network -- the distance from the float64 evaluation of the
same network, against the reference's own float32 distance from it on the same entries (root mean square within 2x, maximum within
4x, floors 1e-6 and 1e-5).  The bound is that test's function, imported, not a new one."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_gpu_r4_parity import _within_reference_noise

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r16_tgnet.npz")))


@pytest.fixture(scope="module")
def net(dev):
    from toothgroupnetwork_amd import nets
    net = nets.PointTransformerSeg(c=6, k=10, planes=(16, 32), blocks=(2, 3), stride=(1, 1), nsample=(36, 24), block_num=2)
    net.load_state_dict(torch.load(os.path.join(GOLDEN, "tgnet_boundary_weights.pt")), strict=True)
    return net.to(dev).eval()


@pytest.mark.parametrize("B", [1, 2])
def test_boundary_network_forward_within_the_reference_noise(dev, fx, net, B):
    from toothgroupnetwork_amd import synth
    N, seed = (int(v) for v in fx["net_scan"])
    scans = synth.scan_batch(2, N, "arch", seed=seed)[:B]
    feats = torch.from_numpy(np.ascontiguousarray(scans.transpose(0, 2, 1))).to(dev)
    with torch.no_grad():
        cls, offset, _, x1 = net([feats])
    assert tuple(cls.shape) == (B, 10, N) and tuple(x1.shape) == (B * N, 16) and (offset is None) == (B == 2)
    got = {"cls": cls.cpu().numpy()[:, :, ::2], "x1": x1.cpu().numpy()[::4]}
    if offset is not None:
        got["offset"] = offset.cpu().numpy()[:, :, ::2]
    tag = f"b{B}"
    report = {n_: _within_reference_noise(n_, v, fx[f"net_{tag}_{n_}_32"], fx[f"net_{tag}_{n_}_64"]) for n_, v in got.items()}
    print(f"\ntwo-stage PointTransformerSeg at {N} points, B = {B}: (drop-in vs exact, reference fp32 vs exact) {report}")
