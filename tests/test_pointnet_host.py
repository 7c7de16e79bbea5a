"""CPU: the PointNet mirror (toothgroupnetwork_amd/pointnet.py) against the reference's own module
(tests/golden/make_golden_r15_pointnet.py): parameter names and shapes, the train formulation's arithmetic on CPU tensors, the
refusal of an eval forward on CPU tensors, and the two new symbols in the ctypes table."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
from seeded import seeded_fill  # noqa: E402


@pytest.fixture(scope="module")
def r15():
    return dict(np.load(os.path.join(GOLDEN, "reference_cpu_r15_pointnet.npz")))


def _fixture_net_and_input(r15):
    import make_golden_r15_pointnet as M
    from crop_cases import digest
    from toothgroupnetwork_amd import nets
    x = M.scans()
    assert digest(x) == str(r15["input_digest"])
    net = nets.PointFirstModule({})
    names = seeded_fill(net, M.SEED)
    return names, net, torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1)))


def test_state_dict_names_and_shapes_equal_the_reference_modules(r15):
    names, net, _ = _fixture_net_and_input(r15)
    assert names == r15["params"].tolist()
    assert len(names) == 94           # 70 parameters + 12 BatchNorms' running mean and variance
    assert len(list(net.named_parameters())) == 70


def test_train_formulation_on_cpu_matches_the_reference_eval_pass(r15):
    _, net, x = _fixture_net_and_input(r15)
    net.eval()
    with torch.no_grad():
        logp, trans_feat = net.first_sem_model._forward_train(x)
    assert logp.shape == (2, 17, 2048) and trans_feat.shape == (2, 128, 128)
    d = float((logp[:, :, ::2] - torch.from_numpy(r15["eval_cls_32"])).abs().max())
    dt = float((trans_feat - torch.from_numpy(r15["eval_trans_32"])).abs().max())
    print(f"\nPointNet train formulation on CPU vs the reference's fp32 eval pass: log-probs {d:.3g}, trans_feat {dt:.3g}")
    assert d <= 1e-5
    assert dt <= 1e-5
    # a forward that wants a gradient takes the same method: BatchNorm in eval mode, parameters requiring grad
    out = net([x[:1, :, :64]])["cls_pred"]
    assert out.requires_grad and out.shape == (1, 17, 64)


def test_eval_forward_refuses_cpu_tensors(r15):
    from toothgroupnetwork_amd import pointnet
    _, net, x = _fixture_net_and_input(r15)
    net.eval()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            net([x])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pointnet.linear_act_max(torch.zeros(1, 128, 8), net.first_sem_model.feat.stn.conv3, net.first_sem_model.feat.stn.bn3, "relu")


def test_ctypes_table_carries_the_new_symbols():
    from toothgroupnetwork_amd import _lib
    assert len(_lib.SIGNATURES["tgn_linear_act_max_workspace_bytes"][1]) == 4
    assert len(_lib.SIGNATURES["tgn_linear_act_max"][1]) == 13
    L = _lib.lib()
    # one scan at C = 1024 is cut into enough point chunks to fill the chip; a refused shape needs no workspace
    assert L.tgn_linear_act_max_workspace_bytes(1, 24000, 128, 1024) >= 32 * 1024 * 4
    assert L.tgn_linear_act_max_workspace_bytes(1, 0, 128, 1024) == 0
    assert L.tgn_linear_act_max_workspace_bytes(1, 1, 128, 1024) == 1024 * 4


def test_drop_in_module_reexports_the_mirrors():
    import external_libs.pointnet2_utils.pointnet_utils as D
    from toothgroupnetwork_amd import nets, pointnet
    assert D.PointNetEncoder is pointnet.PointNetEncoder and D.feature_transform_reguliarzer is pointnet.feature_transform_reguliarzer
    assert D.STN3d is pointnet.STN3d and D.STNkd is pointnet.STNkd
    assert nets.PointFirstModule is pointnet.PointFirstModule
    t = torch.eye(4)[None].repeat(2, 1, 1) * 2.0
    assert float(pointnet.feature_transform_reguliarzer(t)) == pytest.approx(6.0)     # || 4 I - I ||_F = 3 * 2
