"""Drop-in `models` package.  The reference's models/__init__.py:1-9 re-exports seven classes; all seven are here: vanilla
PointNet (models/pointnet.py), PointTransformer (models/point_transformer.py) and the five built on the set-abstraction
backbone (plus the von-Mises models the training scripts import from their submodules).  PointNetPlusPlusCls is the classifier of the
reference's PointNet++Demo.py, which lives outside its models package."""
from .pointnet import PointNet
from .point_transformer import PointTransformer
from .pointnet_pp import PointNetPP
from .Pointnet_pp_xyz import PointNetPPXYZ
from .Pointnet_pp_xyz_Schedmit import PointNetPPXYZ_Schedmit
from .pointnet_pp_8dir import PointNetPP8Dir, PointNetSetAbstraction, DIRS_8
from .pointnet_pp_Fwd import PointNetPPFwd
from .pointnet_pp_vonMises import PointNetPPVonMises
from .pointnet_pp_mvM import PointNetPPMvM
from .pointnet_pp_cls import PointNetPlusPlusCls, SimpleSetAbstraction, SimpleSetAbstractionGroupAll, get_loss

__all__ = ["PointNet", "PointTransformer", "PointNetPP", "PointNetPPXYZ", "PointNetPPXYZ_Schedmit", "PointNetPP8Dir", "PointNetPPFwd",
           "PointNetSetAbstraction", "DIRS_8", "PointNetPPVonMises", "PointNetPPMvM",
           "PointNetPlusPlusCls", "SimpleSetAbstraction", "SimpleSetAbstractionGroupAll", "get_loss"]
