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


def test_tooth_crops_validates_its_arguments_before_any_launch(monkeypatch):
    import numpy as np
    from toothgroupnetwork_amd import _lib, crops
    feats, lab = torch.zeros(1, 6, 100), torch.zeros(1, 100, dtype=torch.int64)
    monkeypatch.setattr(_lib, "require_cuda", lambda *t: None)
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    for k in (0, 101):
        with pytest.raises(ValueError, match=rf"k = {k} must satisfy 1 <= k <= min\(N, 4096\) = 100"):
            crops.tooth_crops(feats, lab, k=k)
    with pytest.raises(ValueError, match="1 <= k"):
        crops.tooth_crops(feats, centroids=[np.zeros((2, 3))], k=101)
    with pytest.raises(TypeError, match="int32 or int64"):
        crops.tooth_crops(feats, lab.float(), k=8)
    with pytest.raises(ValueError, match="labels must be"):                # int32 is accepted: the shape check is what fails
        crops.tooth_crops(feats, lab.int()[:, :99], k=8)
    with pytest.raises(ValueError, match=r"feats must be \(B, C >= 3, N\)"):
        crops.tooth_crops(feats[:, :2], lab, k=8)
    # past the label checks tooth_crops takes the library handle and the stream, then stacks the centroids: all still host work
    monkeypatch.setattr(_lib, "lib", lambda: object())                     # any launch through it is an AttributeError
    monkeypatch.setattr(_lib, "stream", lambda: None)
    with pytest.raises(ValueError, match="centroids must be a list of 1 per-scan"):
        crops.tooth_crops(feats, centroids=[np.zeros((2, 3))] * 2, k=8)
    with pytest.raises(ValueError, match="no tooth"):
        crops.tooth_crops(feats, centroids=[np.zeros((0, 3))], k=8)
    seen = {}                                                              # a flat centroid entry is reshaped to (-1, 3) and accepted

    def stop_at_the_launch(feats_, scan, cent, k):
        seen.update(scan=scan, cent=cent, k=k)
        raise KeyboardInterrupt

    monkeypatch.setattr(crops, "crop_knn", stop_at_the_launch)
    with pytest.raises(KeyboardInterrupt):
        crops.tooth_crops(feats, centroids=[np.arange(6.0)], k=8)
    assert seen["cent"].dtype == torch.float32 and seen["cent"].tolist() == [[0, 1, 2], [3, 4, 5]]
    assert seen["scan"].dtype == torch.int32 and seen["scan"].tolist() == [0, 0] and seen["k"] == 8


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
