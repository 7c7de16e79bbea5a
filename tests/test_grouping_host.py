"""Host-side checks of the two-stage tgnet_fps mirror (no GPU): the missing-centroid error and, in the build container, the state_dict
against the reference's own GroupingNetworkModule."""
import os
import sys
import types

import pytest
import torch

REFERENCE = "/root/reference"
CONFIG = {"model_parameter": {"input_feat": 6, "stride": [1, 4, 4, 4, 4], "nsample": [36, 24, 24, 24, 24], "blocks": [2, 3, 4, 6, 3],
                              "block_num": 5, "planes": [32, 64, 128, 256, 512], "crop_sample_size": 3072}}


def test_tooth_crops_without_labels_or_centroids_raises_before_any_launch(monkeypatch):
    from toothgroupnetwork_amd import _lib, crops
    monkeypatch.setattr(_lib, "require_cuda", lambda *t: None)
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    with pytest.raises(ValueError, match="DBSCAN"):
        crops.tooth_crops(torch.zeros(1, 6, 100))


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "models")), reason="reference checkout not present")
def test_grouping_network_state_dict_equals_the_reference(monkeypatch):
    from toothgroupnetwork_amd import nets
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.setattr(sys, "path", [repo, REFERENCE] + [p for p in sys.path if p not in (repo, REFERENCE)])
    monkeypatch.setitem(sys.modules, "open3d", types.ModuleType("open3d"))
    monkeypatch.setitem(sys.modules, "trimesh", types.ModuleType("trimesh"))
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: self)     # the reference moves its second network to CUDA
    before = set(sys.modules)
    try:
        import models.modules.grouping_network_module as GM
        ref = GM.GroupingNetworkModule(CONFIG)
    finally:                                      # the reference's packages (external_libs among them) must not shadow the repo's
        for name in set(sys.modules) - before:
            del sys.modules[name]
    ours = nets.GroupingNetworkModule(CONFIG)
    want = [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    got = [(k, tuple(v.shape)) for k, v in ours.state_dict().items()]
    assert got == want
    ours.load_state_dict(ref.state_dict(), strict=True)
