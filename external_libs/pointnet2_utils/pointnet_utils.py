"""Drop-in for the reference's ``external_libs/pointnet2_utils/pointnet_utils.py``.

Importer in the reference (unchanged): ``models/modules/pointnet.py:6``.  Implementation: ``toothgroupnetwork_amd.pointnet``.
"""
from toothgroupnetwork_amd.pointnet import (  # noqa: F401
    PointNetEncoder,
    STN3d,
    STNkd,
    feature_transform_reguliarzer,
)
