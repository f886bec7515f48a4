"""models/pointnet.py -- drop-in for the reference's vanilla PointNet (models/pointnet.py: STN3d, STNkd, PointNetEncoder, PointNet).

The parameter containers are declared in the reference's order with its names, so state_dict keys and shapes and the seeded
default initialisation are identical.  forward() runs on the HIP kernels:
  - the narrow per-point layers (D -> 64 -> 128, and 64 -> 64 -> 128 in the feature T-Net) are ops.fc_block over the B*N point rows
    (Conv1d with kernel 1 + BatchNorm1d over (B, N) is a linear layer + BatchNorm over rows); the input rows are padded to a
    multiple of 4 columns with zeros, the first layer's weight likewise;
  - each trunk's last layer 128 -> 1024 with its max over the points is the pooled wide layer, which stores nothing of size
    B*N x 1024; the per-point layers in front of it and the pooled layer are one ops.pn_trunk node, which keeps only its input
    rows and the narrow layers' pre-BatchNorm outputs (their outputs are recomputed in the backward pass);
  - the transforms x @ trans and x @ trans_feat are ops.pn_transform (the D = 6 extra columns pass through), the T-Nets'
    `fc3(x) + iden` is ops.pn_add_identity, the head's relu(bn2(dropout(fc2(x)))) is fc_block + ops.pn_bn_relu, and
    global_feat=False's repeat + cat is ops.pn_concat.
Inputs are GPU float32 tensors; there is no CPU fallback.  PointNet.forward(x, return_transforms=True) also returns `trans` and
`trans_feat` (the reference drops them), for ops.feature_transform_regularizer in the loss.  Nothing of a forward pass is kept
on the module: a tensor held there would keep the step's autograd graph -- and its gradient-accumulation nodes, bound to the
stream they were created on -- alive into the next step, which breaks a hipGraph capture that follows eager steps.

Ragged batches: every forward() takes lengths=(B,) integers, 1 <= lengths[b] <= N; cloud b is the first lengths[b] points of its
row and the padding may hold anything (NaN included).  The first ops.pn_transform packs the valid rows, cloud after cloud, and all
per-point work runs on the M = sum(lengths) packed rows: every per-point BatchNorm takes its statistics over exactly those rows,
each cloud's max runs over its own rows, the gradient at padding is an exact zero, and global_feat=False returns zeros in the
padding columns.  Eval mode: row b is what the call on x[b:b+1, :, :lengths[b]] returns.  M is data dependent, so a ragged
TRAINING step is eager only (a device lengths tensor costs one read-back per forward; a list or CPU tensor none) unless the
lengths are fixed across replays; the forward-only Predictor keeps padded shapes and stays capturable.  The trunks need M > 32.
Without lengths nothing changes.
"""
import types

import torch
import torch.nn as nn

from pnpp_hip import ops
from pnpp_hip.lengths import packed_lengths


def _pad4(d: int) -> int:
    return (d + 3) // 4 * 4


def _check_channels(D: int, channel: int) -> None:
    """The reference's Conv1d refuses an input whose channel count differs from the module's (zero padding must not hide one)."""
    if D != channel:
        raise ValueError(f"expected input with {channel} channels, got {D}")


def _first_layer(conv: nn.Conv1d, width: int):
    """conv1 with its input columns zero-padded to `width` (the fc launchers read rows of a multiple of 4 floats)."""
    w = conv.weight
    if w.shape[1] == width:
        return conv
    wp = ops.pn_transform(w.view(1, w.shape[0], w.shape[1]), None, width)
    return types.SimpleNamespace(weight=wp, bias=conv.bias)


def _packed(lengths, B: int, N: int, device):
    """None, or the batch's PackedLengths, built once per forward and handed to every operator"""
    return None if lengths is None else packed_lengths(lengths, B, N, device)


def _tnet_rows(m: nn.Module, rows: torch.Tensor, B: int, N: int, k: int, lengths=None) -> torch.Tensor:
    """The T-Net on (B*N, width) point rows -- with lengths, the sum(lengths) packed rows -> (B, k, k)."""
    t = m.training
    g = ops.pn_trunk(rows, B, N, [(_first_layer(m.conv1, rows.shape[1]), m.bn1), (m.conv2, m.bn2)], (m.conv3, m.bn3), True, t,
                     lengths=lengths)
    g = ops.fc_block(g, m.fc1, m.bn4, relu=True, training=t)
    g = ops.fc_block(g, m.fc2, m.bn5, relu=True, training=t)
    return ops.pn_add_identity(ops.fc_block(g, m.fc3, training=t), k)


class STN3d(nn.Module):
    def __init__(self, channel: int):
        super(STN3d, self).__init__()
        self.conv1 = nn.Conv1d(channel, 64, 1)
        self.conv2 = nn.Conv1d(64, 128, 1)
        self.conv3 = nn.Conv1d(128, 1024, 1)
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc3 = nn.Linear(256, 9)
        self.bn4 = nn.BatchNorm1d(512)
        self.bn5 = nn.BatchNorm1d(256)
        self.relu = nn.ReLU()

    def forward(self, x: torch.Tensor, lengths=None) -> torch.Tensor:
        """x (B, D, N) -> (B, 3, 3).  lengths (B,): cloud b is x[b, :, :lengths[b]]."""
        B, D, N = x.shape
        _check_channels(D, self.conv1.in_channels)
        lengths = _packed(lengths, B, N, x.device)
        return _tnet_rows(self, ops.pn_transform(x.transpose(1, 2), None, _pad4(D), lengths=lengths), B, N, 3, lengths)


class STNkd(nn.Module):
    def __init__(self, k: int = 64):
        super(STNkd, self).__init__()
        self.k = k
        self.conv1 = nn.Conv1d(k, 64, 1)
        self.conv2 = nn.Conv1d(64, 128, 1)
        self.conv3 = nn.Conv1d(128, 1024, 1)
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc3 = nn.Linear(256, k * k)
        self.bn4 = nn.BatchNorm1d(512)
        self.bn5 = nn.BatchNorm1d(256)
        self.relu = nn.ReLU()

    def forward(self, x: torch.Tensor, lengths=None) -> torch.Tensor:
        """x (B, k, N) -> (B, k, k).  lengths (B,): cloud b is x[b, :, :lengths[b]]."""
        B, D, N = x.shape
        _check_channels(D, self.k)
        lengths = _packed(lengths, B, N, x.device)
        return _tnet_rows(self, ops.pn_transform(x.transpose(1, 2), None, _pad4(D), lengths=lengths), B, N, self.k, lengths)


class PointNetEncoder(nn.Module):
    def __init__(self, global_feat: bool = True, feature_transform: bool = False, channel: int = 3):
        super(PointNetEncoder, self).__init__()
        self.stn = STN3d(channel)
        self.conv1 = nn.Conv1d(channel, 64, 1)
        self.conv2 = nn.Conv1d(64, 128, 1)
        self.conv3 = nn.Conv1d(128, 1024, 1)
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.global_feat = global_feat
        self.feature_transform = feature_transform
        if self.feature_transform:
            self.fstn = STNkd(k=64)

    def forward(self, x: torch.Tensor, lengths=None):
        """x (B, D, N), D >= 3 (the first three columns are coordinates) -> (global (B, 1024) or (B, 1088, N), trans (B, 3, 3),
        trans_feat (B, 64, 64) or None).  lengths (B,): cloud b is x[b, :, :lengths[b]]; the (B, 1088, N) output is zero in the
        padding columns."""
        B, D, N = x.shape
        _check_channels(D, self.conv1.in_channels)
        t = self.training
        xr = x.transpose(1, 2)                               # (B, N, D) view, read in place
        width = _pad4(D)
        if lengths is not None:
            return self._forward_ragged(xr, B, N, width, _packed(lengths, B, N, x.device))
        trans = _tnet_rows(self.stn, ops.pn_transform(xr, None, width), B, N, 3)
        rows = ops.pn_transform(xr, trans, width)             # [xyz @ trans, extra columns, zero padding]
        h = ops.fc_block(rows, _first_layer(self.conv1, width), self.bn1, relu=True, training=t)
        trans_feat = None
        if self.feature_transform:
            trans_feat = _tnet_rows(self.fstn, h, B, N, 64)
            h = ops.pn_transform(h.view(B, N, 64), trans_feat, 64)
        pointfeat = h                                         # (B*N, 64) rows
        g = ops.pn_trunk(h, B, N, [(self.conv2, self.bn2)], (self.conv3, self.bn3), False, t)
        if self.global_feat:
            return g, trans, trans_feat
        return ops.pn_concat(g, pointfeat, N), trans, trans_feat

    def _forward_ragged(self, xr, B, N, width, pk):
        """forward() on the packed valid rows: the same operators, every (B*N, .) array replaced by its (sum(lengths), .) packing"""
        t = self.training
        trans = _tnet_rows(self.stn, ops.pn_transform(xr, None, width, lengths=pk), B, N, 3, pk)
        rows = ops.pn_transform(xr, trans, width, lengths=pk)
        h = ops.fc_block(rows, _first_layer(self.conv1, width), self.bn1, relu=True, training=t)
        trans_feat = None
        if self.feature_transform:
            trans_feat = _tnet_rows(self.fstn, h, B, N, 64, pk)
            h = ops.pn_transform(h, trans_feat, 64, lengths=pk, B=B, N=N)
        g = ops.pn_trunk(h, B, N, [(self.conv2, self.bn2)], (self.conv3, self.bn3), False, t, lengths=pk)
        if self.global_feat:
            return g, trans, trans_feat
        return ops.pn_concat(g, h, N, lengths=pk), trans, trans_feat


class PointNet(nn.Module):
    def __init__(self, feature_transform: bool = True):
        super(PointNet, self).__init__()
        self.encoder = PointNetEncoder(global_feat=True, feature_transform=feature_transform, channel=3)
        self.fc1 = nn.Linear(1024, 512)
        self.bn1 = nn.BatchNorm1d(512)
        self.fc2 = nn.Linear(512, 256)
        self.bn2 = nn.BatchNorm1d(256)
        self.dropout = nn.Dropout(p=0.4)
        self.fc3 = nn.Linear(256, 3)
        self.relu = nn.ReLU()

    def forward(self, x: torch.Tensor, drop_mask=None, return_transforms: bool = False, lengths=None):
        """x (B, D, N) or (B, N, 3|6) -> (B, 3), or (out, trans (B, 3, 3), trans_feat (B, 64, 64) | None) with
        return_transforms.  drop_mask (B, 256) of {0,1} replaces the dropout draw (parity runs); the dropout comes before bn2,
        as in the reference's relu(bn2(dropout(fc2(x)))).  lengths (B,): a ragged batch, cloud b its first lengths[b] points (the
        module docstring); the head, on B rows, is unchanged."""
        if x.dim() == 3 and x.shape[2] in (3, 6):
            x = x.transpose(1, 2)
        g, trans, trans_feat = self.encoder(x) if lengths is None else self.encoder(x, lengths=lengths)
        t = self.training
        h = ops.fc_block(g, self.fc1, self.bn1, relu=True, training=t)
        h = ops.fc_block(h, self.fc2, None, relu=False, dropout=self.dropout, training=t, mask=drop_mask)
        h = ops.pn_bn_relu(h, self.bn2, training=t)
        out = ops.fc_block(h, self.fc3, training=t)
        return (out, trans, trans_feat) if return_transforms else out
