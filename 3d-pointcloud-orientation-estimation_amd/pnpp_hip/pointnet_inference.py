"""Forward-only inference for the vanilla PointNet models (models/pointnet.py): what Predictor(model) is for a PointNet or a
PointNetEncoder.

    predictor = Predictor(model)                         # folds the eval-mode BatchNorms, once
    out = predictor(x)                                   # PointNet: model.eval()(x) under torch.no_grad()
    out, trans, trans_feat = predictor(x, return_transforms=True)
    feat, trans, trans_feat = Predictor(encoder)(x)      # PointNetEncoder: its own triple

A trunk (the input T-Net `stn`, the feature T-Net `fstn`, the `encoder`) runs as ONE launch of pnpp_pn_infer plus a small finishing
pass: the per-point layers and the max over the cloud's points stay on the chip, the T-Net transforms are applied inside the launch,
nothing of size B*N x C is written for C > 64 (PointNetEncoder(global_feat=False) writes its 64-wide point features, which are
part of its output).  The BatchNorm head blocks (`stn.fc1`, `stn.fc2`, `fstn.fc1`, `fstn.fc2`, and PointNet's `fc1`, `fc2` -- whose
relu(bn2(dropout(fc2(x)))) has the identity for dropout in eval mode, so bn2 folds into fc2) run as a linear + ReLU on folded
parameters.  A trunk the kernel refuses (pnpp_pn_infer_supported: a width that is not a multiple of 32, ...) and a head block
without running statistics run the library's existing eval path on a private copy of the model.  `plan` says which is which,
`last_plan` what the latest call ran.

Same contract as the set-abstraction Predictor: a snapshot (refresh() folds again), not differentiable, nothing written to the
model, no CPU fallback.  Sizes that model.eval() itself refuses (B * N <= 32 point rows) RUN here when every trunk is fused: the
kernel takes any B >= 1, N >= 1; a trunk on the eval path raises the same ValueError as the model.  Non-finite inputs are outside
the contract: the fused max is a plain fmax over the rows, which drops a NaN beside a number (the eval path's scan skips NaN rows
too; torch.max would propagate them).

Ragged batches: predictor(x, lengths=(B,)) takes cloud b as the first lengths[b] points of its row, whatever the padding holds;
row b of every output is what the call on x[b:b+1, :, :lengths[b]] returns, and global_feat=False's (B, 1088, N) output is zero in
the padding columns.  A fused trunk keeps every buffer at its padded shape and reads the lengths on the device (pnpp_pn_infer_ragged:
tiles beyond a cloud's length leave at once), so the call has static shapes, makes no synchronisation with a device lengths tensor
and stays capturable; a trunk on the eval path packs its rows and reads the row count back.
"""
from __future__ import annotations

import copy
import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .inference import Predictor, _tracked, planes_to_float32
from .lengths import packed_lengths


class PointNetPredictor(Predictor):
    """Forward-only evaluation of models.pointnet.PointNet / PointNetEncoder (feature transform on or off, channel 3 or 6,
    global_feat either way); built by Predictor(model)."""

    def __init__(self, model: nn.Module):
        from models.pointnet import PointNet, PointNetEncoder
        if not isinstance(model, (PointNet, PointNetEncoder)):
            raise TypeError(f"PointNetPredictor takes a PointNet or a PointNetEncoder, not {type(model).__name__}")
        self._bind(model)
        self._whole = isinstance(model, PointNet)
        self._blobs: Dict[str, torch.Tensor] = {}
        self._snap: Optional[nn.Module] = None
        lib = L.lib()
        enc = self._enc(model)
        for name in self._trunk_names(enc):
            d = self._trunk_desc(enc, name, 1, 1)
            nbytes = lib.pnpp_pn_infer_weights_bytes(C.byref(d)) if d is not None else 0
            if nbytes:
                self._blobs[name] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                self.plan[name] = "fused"
            else:
                self.plan[name] = "eval-path"
            if name != "encoder":
                for fc, bn in (("fc1", "bn4"), ("fc2", "bn5")):
                    self._plan_head(f"{name}.{fc}", getattr(getattr(enc, name), fc), getattr(getattr(enc, name), bn))
        if self._whole:
            self._plan_head("fc1", model.fc1, model.bn1)
            self._plan_head("fc2", model.fc2, model.bn2)
        self.last_plan.update(self.plan)
        self.refresh()

    # ---- construction ----------------------------------------------------------------------------------------------------
    def _enc(self, model):
        return model.encoder if self._whole else model

    @staticmethod
    def _trunk_names(enc) -> List[str]:
        return ["stn"] + (["fstn"] if enc.feature_transform else []) + ["encoder"]

    @staticmethod
    def _trunk_layers(enc, name) -> List[Tuple[nn.Module, nn.Module]]:
        """the (conv, bn) chain of a trunk, from the point rows to the pooled layer"""
        if name == "stn":
            return [(enc.stn.conv1, enc.stn.bn1), (enc.stn.conv2, enc.stn.bn2), (enc.stn.conv3, enc.stn.bn3)]
        if name == "fstn":
            f = enc.fstn
            return [(enc.conv1, enc.bn1), (f.conv1, f.bn1), (f.conv2, f.bn2), (f.conv3, f.bn3)]
        return [(enc.conv1, enc.bn1), (enc.conv2, enc.bn2), (enc.conv3, enc.bn3)]

    def _trunk_desc(self, enc, name, B, N):
        layers = self._trunk_layers(enc, name)
        if len(layers) > L.PNPP_MAX_LAYERS or not _tracked(*[bn for _, bn in layers]):
            return None
        if any(not isinstance(c, nn.Conv1d) or c.kernel_size != (1,) or c.bias is None for c, _ in layers):
            return None
        if len({bn.eps for _, bn in layers}) != 1:
            return None
        widths = [c.weight.shape[0] for c, _ in layers]
        if any(layers[l + 1][0].weight.shape[1] != widths[l] for l in range(len(layers) - 1)):
            return None
        d = L.PnInferDesc()
        d.B, d.N, d.D, d.L = B, N, layers[0][0].weight.shape[1], len(layers)
        for l, w in enumerate(widths):
            d.C[l] = w
        d.input_transform = 0 if name == "stn" else 1
        d.transform_after = 0 if (name == "encoder" and enc.feature_transform) else -1
        d.relu_last = 0 if name == "encoder" else 1
        d.eps = float(layers[0][1].eps)
        return d

    @torch.no_grad()
    def refresh(self) -> None:
        """Fold the model's current parameters and running statistics again (after training steps, load_state_dict, ...)."""
        lib = L.lib()
        # the whole model is copied: the plain linear layers (fc3 of the T-Nets and of the head) and whatever runs the eval path read it
        self._snap = copy.deepcopy(self.model).requires_grad_(False).eval()
        enc = self._enc(self.model)
        with torch.cuda.device(self.device):
            for name, blob in self._blobs.items():
                convs, bns = zip(*self._trunk_layers(enc, name))
                self._fold_chain(lib.pnpp_pn_infer_fold, self._trunk_desc(enc, name, 1, 1), convs, bns, blob)
            for name, f in self._heads.items():
                self._fold_head(f, *self._head_modules(self.model, name))

    def _head_modules(self, model, name):
        if "." in name:
            tnet, fc = name.split(".")
            m = getattr(self._enc(model), tnet)
            return getattr(m, fc), getattr(m, {"fc1": "bn4", "fc2": "bn5"}[fc])
        return getattr(model, name), getattr(model, {"fc1": "bn1", "fc2": "bn2"}[name])

    def folded_layer(self, trunk: str, layer: int):
        """(W' (C_l, Cin_l), b' (C_l), the zero padding columns) of a fused trunk's layer as float32 tensors: the documented view of
        its blob (pnpp_pn_infer_weights_layout)."""
        enc = self._enc(self.model)
        d = self._trunk_desc(enc, trunk, 1, 1)
        conv = self._trunk_layers(enc, trunk)[layer][0]
        woff, ld, boff = C.c_size_t(), C.c_int(), C.c_size_t()
        L.check(L.lib().pnpp_pn_infer_weights_layout(C.byref(d), layer, C.byref(woff), C.byref(ld), C.byref(boff)))
        blob = self._blobs[trunk]
        c, cin = conv.weight.shape[0], conv.weight.shape[1]
        w = planes_to_float32(blob, woff.value, c, ld.value)
        b = blob[boff.value:boff.value + 4 * c].view(torch.float32)
        return w[:, :cin].clone(), b.clone(), w[:, cin:].clone()

    # ---- one call --------------------------------------------------------------------------------------------------------
    def _fused_trunk(self, name, d, xr, trans, trans_feat, want_feat, fresh_out, pk=None):
        B, N = d.B, d.N
        a = L.PnInferArgs()
        a.x = xr.data_ptr()
        a.stride_b, a.stride_n, a.stride_c = xr.stride()
        a.trans, a.trans_feat = ops._p(trans), ops._p(trans_feat)
        a.weights = self._blobs[name].data_ptr()
        a.scratch = self._buf(name + ".scratch", (L.lib().pnpp_pn_infer_scratch_bytes(C.byref(d)),), torch.uint8).data_ptr()
        c = d.C[d.L - 1]
        out = torch.empty(B, c, device=self.device, dtype=torch.float32) if fresh_out else self._buf(name + ".out", (B, c), torch.float32)
        a.out = out.data_ptr()
        feat = None
        if want_feat:
            feat = self._buf(name + ".feat", (B * N, d.C[0]), torch.float32)
            a.feat_out, a.feat_layer = feat.data_ptr(), 0
        if pk is None:
            L.check(L.lib().pnpp_pn_infer(C.byref(d), C.byref(a), ops._stream()))
        else:   # feat keeps its padded (B*N, 64) rows, zero beyond each cloud's length
            L.check(L.lib().pnpp_pn_infer_ragged(C.byref(d), C.byref(a), pk.offs_dev.data_ptr(), ops._stream()))
        return out, feat

    def _eval_trunk(self, name, xr, trans, trans_feat, pk=None):
        """the trunk through the library's existing eval-mode operators, as models/pointnet.py runs it, on the snapshot's parameters:
        -> (pooled (B, C), the 64-wide point features the encoder's global_feat=False output carries or None; packed rows with pk)"""
        from models.pointnet import _first_layer, _pad4
        enc = self._enc(self._snap)
        B, N, D = xr.shape
        width = _pad4(D)
        if pk is not None:
            pk = packed_lengths(pk, B, N, xr.device)   # this path allocates by the packed row count
        if name == "stn":
            m = enc.stn
            rows = ops.pn_transform(xr, None, width, lengths=pk)
            return ops.pn_trunk(rows, B, N, [(_first_layer(m.conv1, width), m.bn1), (m.conv2, m.bn2)], (m.conv3, m.bn3), True, False,
                                lengths=pk), None
        rows = ops.pn_transform(xr, trans, width, lengths=pk)
        h = ops.fc_block(rows, _first_layer(enc.conv1, width), enc.bn1, relu=True, training=False)
        if name == "fstn":
            m = enc.fstn
            return ops.pn_trunk(h, B, N, [(m.conv1, m.bn1), (m.conv2, m.bn2)], (m.conv3, m.bn3), True, False, lengths=pk), None
        if trans_feat is not None:
            h = ops.pn_transform(h.view(B, N, 64), trans_feat, 64) if pk is None else ops.pn_transform(h, trans_feat, 64, lengths=pk, B=B, N=N)
        return ops.pn_trunk(h, B, N, [(enc.conv2, enc.bn2)], (enc.conv3, enc.bn3), False, False, lengths=pk), h

    def _trunk(self, name, xr, trans=None, trans_feat=None, want_feat=False, fresh_out=False, pk=None):
        B, N, _ = xr.shape
        d = self._trunk_desc(self._enc(self.model), name, B, N) if name in self._blobs else None
        if d is not None and not L.lib().pnpp_pn_infer_supported(C.byref(d)):
            d = None
        self.last_plan[name] = "fused" if d is not None else "eval-path"
        if d is None:
            return self._eval_trunk(name, xr, trans, trans_feat, pk)
        return self._fused_trunk(name, d, xr, trans, trans_feat, want_feat, fresh_out, pk)

    def _eval_head(self, name, x):
        fc, bn = self._head_modules(self._snap, name)
        if name == "fc2":   # the model head's relu(bn2(dropout(fc2(x)))), dropout the identity
            return ops.pn_bn_relu(ops.fc_block(x, fc, None, relu=False, training=False), bn, training=False)
        return ops.fc_block(x, fc, bn, relu=True, training=False)

    def _head(self, name, x):
        self.last_plan[name] = self.plan[name]
        return self._run_head(name, x, self._eval_head)

    def _tnet(self, name, xr, trans, k, pk=None):
        g, _ = self._trunk(name, xr, trans, pk=pk)
        g = self._head(f"{name}.fc2", self._head(f"{name}.fc1", g))
        fc3 = getattr(self._enc(self._snap), name).fc3
        return ops.pn_add_identity(ops.fc_block(g, fc3, training=False), k)

    def _encode(self, x, lengths=None):
        from models.pointnet import _check_channels
        enc = self._enc(self.model)
        ops._need_gpu(x, "x")
        if x.dtype != torch.float32:
            raise TypeError(f"x must be float32, got {x.dtype}")
        if x.dim() != 3:
            raise ValueError(f"expected a (B, D, N) input, got {tuple(x.shape)}")
        B, D, N = x.shape
        _check_channels(D, enc.conv1.in_channels)
        xr = x.transpose(1, 2)   # (B, N, D) view, read in place through its strides
        if not (xr.is_contiguous() or x.is_contiguous()):
            xr = xr.contiguous()
        pk = None if lengths is None else packed_lengths(lengths, B, N, self.device, need_total=False)
        trans = self._tnet("stn", xr, None, 3, pk)
        trans_feat = self._tnet("fstn", xr, trans, 64, pk) if enc.feature_transform else None
        # the encoder's pooled feature is returned by a Predictor of a PointNetEncoder: not a reused buffer then
        g, feat = self._trunk("encoder", xr, trans, trans_feat, want_feat=not enc.global_feat, fresh_out=not self._whole, pk=pk)
        if enc.global_feat:
            return g, trans, trans_feat
        if pk is None:
            return ops.pn_concat(g, feat, N), trans, trans_feat
        # a fused trunk tapped padded rows, the eval path returned packed ones
        return ops.pn_concat(g, feat, N, lengths=pk, pf_padded=self.last_plan["encoder"] == "fused"), trans, trans_feat

    @torch.no_grad()
    def __call__(self, x: torch.Tensor, return_transforms: bool = False, lengths=None):
        """PointNet: x (B, D, N) or (B, N, 3|6) -> (B, 3), or (out, trans, trans_feat | None) with return_transforms.
        PointNetEncoder: x (B, D, N) -> (global (B, 1024) | (B, 1088, N), trans, trans_feat | None).
        lengths (B,): a ragged batch, cloud b its first lengths[b] points (the module docstring)."""
        ops._need_gpu(x, "x")
        with torch.cuda.device(self.device):
            if not self._whole:
                return self._encode(x, lengths)
            if x.dim() == 3 and x.shape[2] in (3, 6):
                x = x.transpose(1, 2)
            g, trans, trans_feat = self._encode(x, lengths)
            h = self._head("fc2", self._head("fc1", g))
            out = ops.fc_block(h, self._snap.fc3, training=False)
            return (out, trans, trans_feat) if return_transforms else out
