"""Host-side checks of the DGCNN mirror (no GPU): the state_dict against the reference's own DGCnnModule (build container only), and
the kNN's argument checks, which refuse before any launch."""
import os
import sys

import pytest
import torch

REFERENCE = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "models")), reason="reference checkout not present")
def test_dgcnn_state_dict_equals_the_reference(monkeypatch):
    from toothgroupnetwork_amd import nets
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.setattr(sys, "path", [repo, REFERENCE] + [p for p in sys.path if p not in (repo, REFERENCE)])
    before = set(sys.modules)
    try:
        import models.modules.dgcnn as RD
        ref = RD.DGCnnModule({})
    finally:                                      # the reference's packages must not shadow the repo's
        for name in set(sys.modules) - before:
            del sys.modules[name]
    ours = nets.DGCnnModule({})
    want = [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    got = [(k, tuple(v.shape)) for k, v in ours.state_dict().items()]
    assert got == want
    ours.load_state_dict(ref.state_dict(), strict=True)


def test_dgcnn_module_layout():
    from toothgroupnetwork_amd import dgcnn, nets
    assert nets.DGCnnModule is dgcnn.DGCnnModule
    m = dgcnn.DGCnnModule({})
    assert m.k == 20
    assert m.conv1[0].weight.shape == (64, 12, 1, 1) and m.conv7[0].weight.shape == (512, 1216, 1)
    assert m.cls_conv.weight.shape == (17, 256, 1)


def test_knn_refuses_cpu_tensors():
    from toothgroupnetwork_amd import dgcnn
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dgcnn.knn(torch.zeros(1, 6, 64), 20)
