"""models/pointnet_pp_cls.py -- drop-in for the reference's textbook PointNet++ classifier (PointNet++Demo.py:74-245):
SimpleSetAbstraction, SimpleSetAbstractionGroupAll, PointNetPlusPlusCls, get_loss.

The parameter containers are the reference's (mlp_convs / mlp_bns of nn.Conv2d / nn.BatchNorm2d, fc1 / bn1 / dropout1 / fc2 / bn2 /
dropout2 / fc3) in its construction order, so state_dict keys, shapes and the seeded default initialisation are identical and a
reference checkpoint loads with load_state_dict(strict=True).  forward() runs on the HIP kernels: a level is true farthest-point
sampling (ops.farthest_point_sample, PointNet++Demo.py:8-29), the radius query (ops.ball_query, :49-70) and
ops.set_abstraction(..., neighbour_idx=...) with train-mode BatchNorm and the running-statistics update; the head is ops.fc_block
twice, a plain linear layer, ops.log_softmax; the loss is ops.nll_loss.  Inputs are GPU float32 tensors; there is no CPU fallback.

The first index of each farthest-point run is drawn as the reference draws it -- torch.randint on the host generator, once per
level -- unless `start=` injects it.  The per-point input features of the first level (the normals, D = 3) are input data: they
are detached, no gradient flows to them.  The whole-cloud level's mean coordinate (:172) is used by nothing and is not produced.
"""
import torch
import torch.nn as nn

from pnpp_hip import ops
from pnpp_hip.lengths import fps_starts, ragged_lengths


class _Level(nn.Module):
    """mlp_convs / mlp_bns in the reference's order; `convs` / `bns` are the same containers under the names the library's
    set-abstraction code (ops.set_abstraction, pnpp_hip.inference) reads."""

    group_all = False

    def __init__(self, in_channel, mlp):
        super().__init__()
        last_channel = in_channel + 3
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        for out_channel in mlp:
            self.mlp_convs.append(nn.Conv2d(last_channel, out_channel, 1))
            self.mlp_bns.append(nn.BatchNorm2d(out_channel))
            last_channel = out_channel

    @property
    def convs(self):
        return self.mlp_convs

    @property
    def bns(self):
        return self.mlp_bns

    def forward(self, xyz, points, start=None):
        """The reference's channels-first interface: xyz (B,3,N), points (B,D,N) or None -> new_xyz (B,3,S), new_points (B,C,S)."""
        pts = None if points is None else points.transpose(1, 2)
        new_xyz, new_points = self.rows(xyz.transpose(1, 2), pts, start)
        return new_xyz.transpose(1, 2).contiguous(), new_points.transpose(1, 2).contiguous()


class SimpleSetAbstraction(_Level):
    """PointNet++Demo.py:74-129: npoint farthest-point centres, up to nsample members within `radius` of each (padded with the first
    member), 1x1 conv + BatchNorm + ReLU x len(mlp), max over the neighbourhood."""

    sampler = "fps"

    def __init__(self, npoint, radius, nsample, in_channel, mlp):
        super().__init__(in_channel, mlp)
        self.npoint = npoint
        self.radius = radius
        self.nsample = nsample

    @property
    def grouper(self):
        return ("ball", self.radius)

    def _centres(self, xyz, start=None, lengths=None):
        return ops.farthest_point_sample(xyz, self.npoint, start, lengths=lengths)

    def rows(self, xyz, points, start=None, lengths=None):
        """xyz (B,N,3), points (B,N,D) or None -> new_xyz (B,S,3), new_points (B,S,C); start (B,) injects the first centre index.
        lengths (B,): a ragged batch -- cloud b is its first lengths[b] rows (any length from 1: farthest-point sampling may revisit
        points and the radius query pads its lists); sampling and query read them, the level's output is uniform.  Without `start`
        the first index of cloud b is torch.randint(0, lengths[b]) on the host generator, which reads a device `lengths` back once."""
        if lengths is not None:   # checked / uploaded once for the sampling and the query
            dev = ragged_lengths(lengths, xyz.shape[0], xyz.shape[1], xyz.device)
            if start is None:
                start = fps_starts(lengths)
            lengths = dev
        centre = self._centres(xyz, start, lengths)
        nbr = ops.ball_query(self.radius, self.nsample, xyz, ops.index_points(xyz, centre), lengths=lengths)
        return ops.set_abstraction(xyz, points, centre, self.nsample, False, self.training, self.mlp_convs, self.mlp_bns,
                                   neighbour_idx=nbr)


class SimpleSetAbstractionGroupAll(_Level):
    """PointNet++Demo.py:131-173: the whole cloud as one group (absolute coordinates), same MLP, max over the points."""

    group_all = True
    npoint = nsample = None

    def rows(self, xyz, points, start=None):
        return ops.set_abstraction(xyz, points, None, None, True, self.training, self.mlp_convs, self.mlp_bns)


class PointNetPlusPlusCls(nn.Module):
    """PointNet++Demo.py:177-235.  The level sizes default to the reference's (512 / 0.2 / 32, 128 / 0.4 / 64, whole cloud) and can
    be overridden by keyword: sa1=(npoint, radius, nsample), sa2=(npoint, radius, nsample)."""

    def __init__(self, num_classes=40, normal_channel=True, sa1=(512, 0.2, 32), sa2=(128, 0.4, 64)):
        super().__init__()
        in_channel = 3
        self.normal_channel = normal_channel
        self.sa1 = SimpleSetAbstraction(npoint=sa1[0], radius=sa1[1], nsample=sa1[2], in_channel=in_channel, mlp=[64, 64, 128])
        self.sa2 = SimpleSetAbstraction(npoint=sa2[0], radius=sa2[1], nsample=sa2[2], in_channel=128, mlp=[128, 128, 256])
        self.sa3 = SimpleSetAbstractionGroupAll(in_channel=256, mlp=[256, 512, 1024])

        self.fc1 = nn.Linear(1024, 512)
        self.bn1 = nn.BatchNorm1d(512)
        self.dropout1 = nn.Dropout(p=0.4)
        self.fc2 = nn.Linear(512, 256)
        self.bn2 = nn.BatchNorm1d(256)
        self.dropout2 = nn.Dropout(p=0.4)
        self.fc3 = nn.Linear(256, num_classes)

    def split_input(self, x):
        """x (B, 6, N) channels-first (coordinates, then normals) -> xyz (B,N,3), points (B,N,3) as rows, detached."""
        ops._need_gpu(x, "x")
        want = 6 if self.normal_channel else 3
        if x.dim() != 3 or x.shape[1] != want:
            raise ValueError(f"expected input (B, {want}, N), got {tuple(x.shape)}")
        if not self.normal_channel:
            # the reference builds sa1 for three feature channels whatever normal_channel says (:185); its forward then fails in
            # the first convolution (6 input channels, 3 given).  Same parameters here, and the same refusal.
            raise ValueError("normal_channel=False: the first level's convolution has 6 input channels and cannot take 3 "
                             "(PointNet++Demo.py:185)")
        rows = x.detach().transpose(1, 2)
        return rows[:, :, :3].contiguous(), rows[:, :, 3:].contiguous()

    def forward(self, x, start=None, drop_masks=None, lengths=None):
        """x (B, 6, N) -> (B, num_classes) log-probabilities.  start = (sa1 start indices (B,), sa2 start indices (B,)) and
        drop_masks = ((B,512), (B,256)) keep-masks inject the random draws (parity runs).  lengths (B,): a ragged batch -- cloud b
        is x[b, :, :lengths[b]] (SimpleSetAbstraction.rows); only the first level reads them."""
        xyz, points = self.split_input(x)
        B = xyz.size(0)
        s1, s2 = start if start is not None else (None, None)
        m1, m2 = drop_masks if drop_masks is not None else (None, None)
        t = self.training
        l1_xyz, l1_points = self.sa1.rows(xyz, points, s1, lengths=lengths)
        l2_xyz, l2_points = self.sa2.rows(l1_xyz, l1_points, s2)
        _, l3_points = self.sa3.rows(l2_xyz, l2_points)
        h = l3_points.view(B, -1)
        h = ops.fc_block(h, self.fc1, self.bn1, relu=True, dropout=self.dropout1, training=t, mask=m1)
        h = ops.fc_block(h, self.fc2, self.bn2, relu=True, dropout=self.dropout2, training=t, mask=m2)
        return ops.log_softmax(ops.fc_block(h, self.fc3, training=t))


class get_loss(nn.Module):
    """PointNet++Demo.py:239-245: F.nll_loss(pred, target)."""

    def forward(self, pred, target):
        return ops.nll_loss(pred, target)
