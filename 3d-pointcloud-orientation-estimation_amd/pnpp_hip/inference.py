"""Forward-only inference for the PointNet++ set-abstraction models.

    predictor = Predictor(model)            # folds the eval-mode BatchNorms into the weights in front of them, once
    mu, kappa = predictor(xyz)              # what model.eval()(xyz) returns under torch.no_grad()

A level runs as ONE launch (pnpp_sa_infer: gather -> 3 x (product + bias + ReLU) -> max, nothing of size M x C leaves the
chip); the BatchNorm head blocks run as a plain linear + ReLU on folded parameters.  Whatever the fused kernel does not take
(pnpp_sa_infer_supported: K other than 16 or a multiple of 32 up to 256, other layer counts, the LayerNorm head of PointNetPPMvM, the output maps) goes
through the library's existing eval-mode entry points, unchanged.  `predictor.plan` says which is which at the sizes the model's
constructor arguments imply; the choice is made again from each call's sizes (a level planned "fused" whose input a call makes
unsupported runs the eval path for that call), and `predictor.last_plan` says what the latest call ran.

A Predictor is a SNAPSHOT of the model's parameters and running statistics at construction (folded weights for what is fused,
private copies of the levels and of every other submodule for whatever runs the eval path): call refresh() after the model has been trained further or loaded from a checkpoint.
The copies hold the fused levels' parameters a second time beside their folded planes (about 7 MB for the BASELINE models): the price
of a level staying a snapshot when a call's sizes send it to the eval path.
It is not differentiable (model.eval() remains the path with a backward pass), keeps nothing between calls but the folded weights and reusable index / activation buffers, and never writes to the model.

`Predictor` itself is the base class and the factory: it holds what every model family shares (the device check, the reusable
buffers, held_tensors() / persistent_bytes(), the fold of a conv + BatchNorm chain and of a head block, the bf16-plane view) and
Predictor(model) builds the family's subclass.  The set-abstraction models get the SetAbstractionPredictor below; a PointNetPlusPlusCls
(models/pointnet_pp_cls.py) the ClsPredictor below: the same levels and head blocks, farthest-point sampling + radius query in
front of each level's launch, and fc3 + log_softmax as one launch (pnpp_linear_log_softmax).  A vanilla PointNet / PointNetEncoder
(models/pointnet.py) gets the PointNetPredictor of pnpp_hip.pointnet_inference: the same contract, one launch per trunk
(pnpp_pn_infer).  A PointTransformer (models/point_transformer.py) gets the TransformerPredictor of pnpp_hip.transformer_inference:
one launch per encoder layer beside its attention (pnpp_pt_infer_tail); Predictor(model, attention="split" | "float32") chooses the
attention kernel there.
"""
from __future__ import annotations

import copy
import ctypes as C
import types
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import _lib as L
from . import ops, sampling
from .lengths import device_and_draw_lengths, fps_starts, ragged_lengths


class _Folded:
    """weight / bias of a folded nn.Linear + nn.BatchNorm1d block, shaped like the nn.Linear that ops.fc_block reads"""

    def __init__(self, n_out: int, n_in: int, device):
        self.weight = torch.empty(n_out, n_in, device=device, dtype=torch.float32)
        self.bias = torch.empty(n_out, device=device, dtype=torch.float32)


class _Proxy:
    """Stands in for `self` in the model class's own forward(): every attribute is the model's, methods are re-bound to the proxy,
    `training` is False, and the two methods that hold the backbone (`trunk`, `_global_feat`) are the Predictor's."""

    def __init__(self, predictor):
        object.__setattr__(self, "_pred", predictor)

    training = False

    def __getattr__(self, name):
        snap = self._pred._snap
        if name in snap:
            return snap[name]
        model = self._pred.model
        fn = getattr(type(model), name, None)
        if isinstance(fn, types.FunctionType):
            return types.MethodType(fn, self)
        return getattr(model, name)

    def __setattr__(self, name, value):
        raise AttributeError("a Predictor does not write to its model")

    def trunk(self, xyz, centres=None, drop_mask=None, lengths=None):
        return self._pred._trunk(xyz, centres, lengths)

    def _global_feat(self, pts, centres=None, drop_masks=(None, None), lengths=None):
        return self._pred._trunk(pts, centres, lengths)


def _ball(grouper):
    kind, radius = grouper if isinstance(grouper, tuple) else tuple(grouper.split(":"))
    if kind != "ball":
        raise ValueError(f"unknown grouper '{grouper}'")
    return float(radius)


def _tracked(*bns) -> bool:
    return all(isinstance(b, nn.BatchNorm1d) and b.track_running_stats and b.affine for b in bns)


def planes_to_float32(blob: torch.Tensor, offset: int, rows: int, ld: int) -> torch.Tensor:
    """the (rows, ld) float32 matrix that the three bf16 planes at `offset` of a uint8 blob sum to"""
    # three bf16 planes (W' = high + middle + low, exactly), each fragment-major [rows/32][ld/16][2][32][8]:
    # rows n = 32 cb + r, columns k = 16 ks + 8 h + j
    w = blob[offset:offset + 6 * rows * ld].view(torch.bfloat16).view(3, rows // 32, ld // 16, 2, 32, 8)
    w = w.permute(0, 1, 4, 2, 3, 5).reshape(3, rows, ld).float()
    return (w[0] + w[1]) + w[2]


class Predictor:
    """What the forward-only Predictors of every model family share, and their factory: Predictor(model, ...) builds the
    SetAbstractionPredictor, ClsPredictor, PointNetPredictor or TransformerPredictor that takes the model.  A subclass checks its
    model type, calls _bind(), plans (`plan`, `_blobs`, `_heads`) and folds in refresh() into `_blobs`, `_heads` and `_snap`."""

    def __new__(cls, model=None, *args, **kwargs):
        if cls is not Predictor:
            return object.__new__(cls)
        from models.pointnet import PointNet, PointNetEncoder
        if isinstance(model, (PointNet, PointNetEncoder)):
            from .pointnet_inference import PointNetPredictor
            return object.__new__(PointNetPredictor)
        from models.point_transformer import PointTransformer
        if isinstance(model, PointTransformer):
            from .transformer_inference import TransformerPredictor
            return object.__new__(TransformerPredictor)
        from models.pointnet_pp_cls import PointNetPlusPlusCls
        if isinstance(model, PointNetPlusPlusCls):   # the textbook classifier: other samplers, other head tail
            return object.__new__(ClsPredictor)
        from models.pointnet_pp_8dir import BackboneBNHead
        from models.pointnet_pp_mvM import PointNetPPMvM
        if isinstance(model, (BackboneBNHead, PointNetPPMvM)):
            return object.__new__(SetAbstractionPredictor)
        raise TypeError(f"Predictor takes a PointNet++ set-abstraction model, a PointNetPlusPlusCls, a PointNet, a PointNetEncoder or "
                        f"a PointTransformer, not {type(model).__name__}")

    # ---- construction ----------------------------------------------------------------------------------------------------
    def _bind(self, model: nn.Module) -> None:
        p = next(model.parameters())
        if not p.is_cuda:
            raise RuntimeError(f"the model is on '{p.device}': the pnpp HIP operators run on an AMD GPU only "
                               "(no CPU fallback exists in this package)")
        self.model = model
        self.device = p.device
        self._bufs: Dict[tuple, torch.Tensor] = {}
        self._heads: Dict[str, _Folded] = {}
        self.plan: Dict[str, str] = {}
        self.last_plan: Dict[str, str] = {}   # what the latest call ran (a call's sizes can refuse what was planned "fused")

    @torch.no_grad()
    def orientation(self, *args, num: int = 360, rel_height: float = 0.1, density: bool = False, **kwargs):
        """self(*args, **kwargs) decoded on the device: the von-Mises parameters of a PointNetPPVonMises (one peak) or the mixture of
        a PointNetPPMvM -> pnpp_hip.decode.Orientation(angle, modes, heights, n_modes, density), one more launch and no read-back."""
        from models.pointnet_pp_mvM import PointNetPPMvM
        from models.pointnet_pp_vonMises import PointNetPPVonMises
        from . import decode
        if not isinstance(self.model, (PointNetPPVonMises, PointNetPPMvM)):
            raise TypeError(f"Predictor.orientation decodes the von-Mises outputs of a PointNetPPVonMises or a PointNetPPMvM, "
                            f"not those of a {type(self.model).__name__}")
        out = self(*args, **kwargs)
        with torch.cuda.device(self.device):
            return decode.decode(*out, num=num, rel_height=rel_height, density=density)

    def _plan_head(self, name: str, fc, bn) -> None:
        if _tracked(bn) and isinstance(fc, nn.Linear) and fc.bias is not None:
            self._heads[name] = _Folded(fc.weight.shape[0], fc.weight.shape[1], self.device)
            self.plan[name] = "fused"
        else:
            self.plan[name] = "eval-path"

    @staticmethod
    def _fold_chain(entry, desc, convs, bns, blob: torch.Tensor) -> None:
        """pnpp_sa_infer_fold / pnpp_pn_infer_fold (`entry`) of a conv + BatchNorm chain into its blob"""
        a = L.SaFwdArgs()
        keep = []   # the contiguous float32 tensors whose pointers the call reads
        for field, ts in (("conv_w", [c.weight for c in convs]), ("conv_b", [c.bias for c in convs]),
                          ("bn_w", [b.weight for b in bns]), ("bn_b", [b.bias for b in bns]),
                          ("bn_rm", [b.running_mean for b in bns]), ("bn_rv", [b.running_var for b in bns])):
            ts = [ops._f32(t.detach(), field) for t in ts]
            keep += ts
            setattr(a, field, ops._ptr_array(ts))
        L.check(entry(C.byref(desc), C.byref(a), blob.data_ptr(), ops._stream()))

    @staticmethod
    def _fold_head(f: _Folded, fc, bn) -> None:
        ts = [ops._f32(t.detach(), "head parameter") for t in (fc.weight, fc.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)]
        L.check(L.lib().pnpp_fc_infer_fold(f.weight.shape[0], f.weight.shape[1], *[t.data_ptr() for t in ts], float(bn.eps),
                                           f.weight.data_ptr(), f.bias.data_ptr(), ops._stream()))

    def _blob_tensors(self) -> List[torch.Tensor]:
        return list(self._blobs.values())

    def _snap_modules(self) -> List[nn.Module]:
        return [self._snap]

    def held_tensors(self) -> List[torch.Tensor]:
        """the device tensors the Predictor holds between calls: folded weights, the reusable index / activation buffers, the
        folded head blocks, the snapshot's parameters and buffers"""
        ts = self._blob_tensors() + list(self._bufs.values())
        for f in self._heads.values():
            ts += [f.weight, f.bias]
        for m in self._snap_modules():
            ts += list(m.parameters()) + list(m.buffers())
        return ts

    def persistent_bytes(self) -> int:
        """device memory the Predictor holds between calls"""
        return sum(t.numel() * t.element_size() for t in self.held_tensors())

    # ---- one call --------------------------------------------------------------------------------------------------------
    def _buf(self, tag: str, shape, dtype) -> torch.Tensor:
        key = (tag, tuple(shape), dtype)
        t = self._bufs.get(key)
        if t is None:
            for k in [k for k in self._bufs if k[0] == tag]:   # one buffer per role: a new shape replaces the old one
                del self._bufs[k]
            t = torch.empty(*shape, dtype=dtype, device=self.device)
            self._bufs[key] = t
        return t

    def _run_head(self, name: str, x, eval_block):
        f = self._heads.get(name)
        if f is not None:     # folded linear + BatchNorm1d: y = relu(x W'^T + b'); eval-mode dropout is the identity
            return ops.fc_block(x, f, None, relu=True, training=False)
        return eval_block(name, x)


class SetAbstractionPredictor(Predictor):
    """Forward-only evaluation of a BackboneBNHead model (PointNetPPVonMises, PointNetPP8Dir, PointNetPP, PointNetPPFwd,
    PointNetPPXYZ, PointNetPPXYZ_Schedmit) or of PointNetPPMvM: predictor(xyz, centres=None) == model.eval()(xyz, centres=centres)
    under no_grad -- same tuple structure, shapes and dtypes, same sampler / grouper per level, same draws from the host generator."""

    def __init__(self, model: nn.Module):
        from models.pointnet_pp_8dir import BackboneBNHead
        from models.pointnet_pp_mvM import PointNetPPMvM
        if not isinstance(model, (BackboneBNHead, PointNetPPMvM)):
            raise TypeError(f"SetAbstractionPredictor takes a PointNet++ set-abstraction model, not {type(model).__name__}")
        # the model class's own forward() is run on a proxy whose backbone entry is the Predictor's: it must have one
        if not any(callable(getattr(type(model), n, None)) for n in ("trunk", "_global_feat")):
            raise TypeError(f"{type(model).__name__} reaches its backbone through neither trunk() nor _global_feat()")
        self._build(model)

    def _build(self, model: nn.Module) -> None:
        self._bind(model)
        self._levels = [model.sa1, model.sa2, model.sa3]
        self._names = ["sa1", "sa2", "sa3"]
        self._blobs: Dict[str, torch.Tensor] = {}
        self._snap: Dict[str, nn.Module] = {}   # private copies of the submodules that are not folded (refresh())
        lib = L.lib()
        prev_npoint = None
        for name, sa in zip(self._names, self._levels):
            d = self._nominal_desc(sa, prev_npoint)
            nbytes = lib.pnpp_sa_infer_weights_bytes(C.byref(d)) if d is not None else 0
            if nbytes:
                self._blobs[name] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                self.plan[name] = "fused"
            else:
                self.plan[name] = "eval-path"
            prev_npoint = sa.npoint
        for i in (1, 2):
            self._plan_head(f"fc{i}", getattr(model, f"fc{i}"), getattr(model, f"bn{i}", None))
        self.last_plan.update(self.plan)
        self.refresh()

    # ---- construction ----------------------------------------------------------------------------------------------------
    @staticmethod
    def _channels(sa):
        return [c.weight.shape[0] for c in sa.convs]

    def _desc(self, sa, B, N, S, K):
        eps = sa.bns[0].eps
        return ops._sa_desc(B, N, S, K, sa.convs[0].weight.shape[1] - 3, self._channels(sa), sa.group_all, False, eps, 0.1)

    def _nominal_desc(self, sa, prev_npoint):
        """the level's descriptor at the sizes its constructor arguments imply (the blob depends on D and the channels only)"""
        if len(sa.convs) > L.PNPP_MAX_LAYERS or any(not bn.track_running_stats for bn in sa.bns):
            return None
        if sa.group_all:
            if prev_npoint is None:
                return None
            return self._desc(sa, 1, prev_npoint, 1, prev_npoint)
        return self._desc(sa, 1, max(sa.npoint, sa.nsample), sa.npoint, sa.nsample)

    @torch.no_grad()
    def refresh(self) -> None:
        """Fold the model's current parameters and running statistics again (after training steps, load_state_dict, ...)."""
        lib = L.lib()
        prev_npoint = None
        # every level is copied, fused ones too: a call whose sizes the kernel refuses runs the eval path on the snapshot
        folded = set(self._heads) | {"bn" + k[2:] for k in self._heads}
        self._snap = {name: copy.deepcopy(child).requires_grad_(False) for name, child in self.model.named_children()
                      if name not in folded}
        with torch.cuda.device(self.device):
            for name, sa in zip(self._names, self._levels):
                if name in self._blobs:
                    self._fold_chain(lib.pnpp_sa_infer_fold, self._nominal_desc(sa, prev_npoint), sa.convs, sa.bns, self._blobs[name])
                prev_npoint = sa.npoint
            for name, f in self._heads.items():
                self._fold_head(f, getattr(self.model, name), getattr(self.model, "bn" + name[2:]))

    def folded_layer(self, level: str, layer: int):
        """(W' (C_l, Cin_l), b' (C_l)) of a fused level as float32 tensors: the documented view of its blob (pnpp_sa_infer_weights_layout)."""
        sa = self._levels[self._names.index(level)]
        prev = self._levels[self._names.index(level) - 1].npoint if sa.group_all else None
        d = self._nominal_desc(sa, prev)
        woff, ld, boff = C.c_size_t(), C.c_int(), C.c_size_t()
        L.check(L.lib().pnpp_sa_infer_weights_layout(C.byref(d), layer, C.byref(woff), C.byref(ld), C.byref(boff)))
        blob = self._blobs[level]
        c = self._channels(sa)[layer]
        cin = sa.convs[layer].weight.shape[1]
        w = planes_to_float32(blob, woff.value, c, ld.value)
        b = blob[boff.value:boff.value + 4 * c].view(torch.float32)
        return w[:, :cin].clone(), b.clone(), w[:, cin:].clone()

    def _snap_modules(self):
        return list(self._snap.values())

    # ---- one call --------------------------------------------------------------------------------------------------------
    def _takes(self, i: int, B: int, N: int) -> Optional[L.SaDesc]:
        """the level's descriptor at this call's sizes when the fused kernel takes it, else None"""
        name, sa = self._names[i], self._levels[i]
        if name not in self._blobs:
            return None
        d = self._desc(sa, B, N, 1, N) if sa.group_all else self._desc(sa, B, N, sa.npoint, sa.nsample)
        return d if L.lib().pnpp_sa_infer_supported(C.byref(d)) else None

    def _fused(self, i: int, d, xyz, points, centre, nbr):
        name = self._names[i]
        B, S, K = d.B, d.S, d.K
        a = L.SaInferArgs()
        a.xyz, a.points = xyz.data_ptr(), ops._p(points)
        if not d.group_all:
            a.centre_idx = centre.data_ptr()
            if nbr is not None:
                a.neighbour_idx = nbr.data_ptr()
            else:
                a.idx_out = self._buf(name + ".idx", (B, S, K), torch.int32).data_ptr()
        a.weights = self._blobs[name].data_ptr()
        new_xyz = self._buf(name + ".new_xyz", (B, S, 3), torch.float32)
        out = self._buf(name + ".out", (B, S, d.C[2]), torch.float32)
        a.new_xyz, a.out = new_xyz.data_ptr(), out.data_ptr()
        L.check(L.lib().pnpp_sa_infer(C.byref(d), C.byref(a), ops._stream()))
        return new_xyz, out

    @staticmethod
    def _neighbours(sa, xyz, centre, lengths):
        """the neighbour lists a level needs handed to it: the radius query's, or -- a ragged level 1 -- the ragged kNN's (the
        level's own search knows no lengths); None: the level searches for itself"""
        if sa.grouper != "knn":
            return ops.ball_query(_ball(sa.grouper), sa.nsample, xyz, ops.index_points(xyz, centre), lengths=lengths)
        if lengths is not None:
            return ops.knn(ops.index_points(xyz, centre), xyz, sa.nsample, lengths=lengths)
        return None

    def _eval_level(self, i, xyz, points, centre, lengths=None):
        """the level through the library's existing eval-mode forward (PointNetSetAbstraction.forward with training = False):
        sizes, sampler and grouper are the model's, the parameters the snapshot's"""
        sa = self._levels[i]
        w = self._snap[self._names[i]]
        if sa.group_all:
            return ops.set_abstraction(xyz, points, None, None, True, False, w.convs, w.bns)
        if centre is None:
            centre = sa._centres(xyz)
        nbr = self._neighbours(sa, xyz, centre, lengths)
        return ops.set_abstraction(xyz, points, centre, sa.nsample, False, False, w.convs, w.bns, neighbour_idx=nbr)

    def _level(self, i: int, xyz, points, centre=None, lengths=None):
        """lengths: the device tensor of a ragged level 1 (the centres are then given: drawn by the caller from the lengths)"""
        sa = self._levels[i]
        B, N, _ = xyz.shape
        d = self._takes(i, B, N)
        self.last_plan[self._names[i]] = "fused" if d is not None else "eval-path"
        if d is None:
            return self._eval_level(i, xyz, points, centre, lengths)
        if sa.group_all:
            return self._fused(i, d, xyz, points, None, None)
        if centre is None:
            centre = sa._centres(xyz)
        centre = ops._i32(centre, "centre_idx")
        nbr = self._neighbours(sa, xyz, centre, lengths)
        if nbr is not None:
            nbr = ops._i32(nbr, "neighbour_idx")
        return self._fused(i, d, xyz, points, centre, nbr)

    def _levels12(self, xyz, centres, lengths=None):
        """sa1 + sa2 with the draws of BackboneBNHead.levels12 / stacked_levels, in their order; lengths (B,): a ragged batch"""
        sa1, sa2 = self._levels[0], self._levels[1]
        B, N, _ = xyz.shape
        c1, c2 = centres if centres is not None else (None, None)
        draw_lengths = lengths
        if lengths is not None and not sa1.group_all:
            lengths, draw_lengths = device_and_draw_lengths(lengths, B, N, xyz.device, sa1.min_length(), sa1.sampler)
        if centres is None and sa1.sampler == "device" and sa2.sampler == "device" and not sa1.group_all and not sa2.group_all:
            c1, c2 = sampling.device_random_centres_pair(B, N, sa1.npoint, sa1.npoint, sa2.npoint, xyz.device, lengths=lengths)
        pair_ok = (not sa1.group_all and not sa2.group_all and sa1.grouper == "knn" and sa2.grouper == "knn"
                   and (c1 is not None or sa1.sampler != "fps") and (c2 is not None or sa2.sampler != "fps")
                   and sa1.npoint <= N and sa2.npoint <= sa1.npoint and sa1.nsample <= N and sa2.nsample <= sa1.npoint)
        if pair_ok:
            # the same draws whichever path each level takes (stacked_levels draws both before either level runs)
            if c1 is None:
                c1 = sa1._centres(xyz, draw_lengths)
            if c2 is None:
                c2 = sa2._centres(xyz[:, :sa1.npoint])
        elif c1 is None and lengths is not None:
            c1 = sa1._centres(xyz, draw_lengths)
        d1 = self._takes(0, B, N) if pair_ok else None
        d2 = self._takes(1, B, sa1.npoint) if pair_ok else None
        if d1 is not None and d2 is not None:   # both neighbour searches in one launch, then the two level launches
            self.last_plan["sa1"] = self.last_plan["sa2"] = "fused"
            c1, c2 = ops._i32(c1, "centre_idx"), ops._i32(c2, "centre_idx")
            idx1 = self._buf("sa1.idx", (B, d1.S, d1.K), torch.int32)
            idx2 = self._buf("sa2.idx", (B, d2.S, d2.K), torch.int32)
            nx1 = self._buf("sa1.new_xyz", (B, d1.S, 3), torch.float32)
            nx2 = self._buf("sa2.new_xyz", (B, d2.S, 3), torch.float32)
            tail = (c1.data_ptr(), c2.data_ptr(), idx1.data_ptr(), nx1.data_ptr(), idx2.data_ptr(), nx2.data_ptr(), ops._stream())
            if lengths is not None:
                L.check(L.lib().pnpp_sa_infer_group_pair_ragged(C.byref(d1), C.byref(d2), xyz.data_ptr(), lengths.data_ptr(), *tail))
            else:
                L.check(L.lib().pnpp_sa_infer_group_pair(C.byref(d1), C.byref(d2), xyz.data_ptr(), *tail))
            l1_xyz, l1_pts = self._fused(0, d1, xyz, None, c1, idx1)
            return self._fused(1, d2, l1_xyz, l1_pts, c2, idx2)
        l1_xyz, l1_pts = self._level(0, xyz, None, c1, lengths)
        return self._level(1, l1_xyz, l1_pts, c2)

    def _eval_head(self, name, x):
        m = _Proxy(self)   # unfolded head blocks come from the snapshot
        norm = getattr(m, "bn" + name[2:], None) or getattr(m, "ln" + name[2:], None)
        return ops.fc_block(x, getattr(m, name), norm, relu=True, dropout=m.drop, training=False)

    def _trunk(self, xyz, centres, lengths=None):
        xyz = ops._f32(xyz, "xyz")
        B = xyz.size(0)
        l2_xyz, l2_pts = self._levels12(xyz, centres, lengths)
        x = self._level(2, l2_xyz, l2_pts)[1].reshape(B, -1)
        for name in ("fc1", "fc2"):
            x = self._run_head(name, x, self._eval_head)
        return x

    @torch.no_grad()
    def __call__(self, xyz: torch.Tensor, centres=None, lengths=None):
        """lengths (B,): a ragged batch, as model.eval()(xyz, centres=centres, lengths=lengths) -- row b is the result for
        xyz[b:b+1, :lengths[b]] given the same draws; the pair route, a level-1 launch on the ragged kernel's neighbour lists and
        the eval-path fall-back all take it."""
        ops._need_gpu(xyz, "xyz")
        with torch.cuda.device(self.device):
            if lengths is None:
                return type(self.model).forward(_Proxy(self), xyz, centres=centres)
            return type(self.model).forward(_Proxy(self), xyz, centres=centres, lengths=lengths)


class ClsPredictor(SetAbstractionPredictor):
    """Forward-only evaluation of PointNetPlusPlusCls: predictor(x, start=None) == model.eval()(x, start=start) under no_grad.
    Each level is farthest-point sampling, the radius query and one pnpp_sa_infer launch on the neighbour lists; fc1 / bn1 and
    fc2 / bn2 are folded; fc3 + log_softmax is one launch on the snapshot's fc3 (plan["fc3"]).  Same draws from the host generator as
    the model: one torch.randint per level unless `start` injects them."""

    def __init__(self, model: nn.Module):
        from models.pointnet_pp_cls import PointNetPlusPlusCls
        if not isinstance(model, PointNetPlusPlusCls):
            raise TypeError(f"ClsPredictor takes a PointNetPlusPlusCls, not {type(model).__name__}")
        self._build(model)
        self.plan["fc3"] = self.last_plan["fc3"] = "fused"

    def _eval_head(self, name, x):
        return ops.fc_block(x, self._snap[name], self._snap["bn" + name[2:]], relu=True, training=False)

    @torch.no_grad()
    def __call__(self, x: torch.Tensor, start=None, lengths=None):
        """lengths (B,): a ragged batch, as model.eval()(x, start=start, lengths=lengths)"""
        ops._need_gpu(x, "x")
        with torch.cuda.device(self.device):
            xyz, points = self.model.split_input(x)
            s1, s2 = start if start is not None else (None, None)
            sa1, sa2 = self._levels[0], self._levels[1]
            if lengths is not None:   # checked / uploaded once; the start draws of SimpleSetAbstraction.rows
                dev = ragged_lengths(lengths, xyz.size(0), xyz.size(1), xyz.device)
                if s1 is None:
                    s1 = fps_starts(lengths)
                lengths = dev
            l1_xyz, l1_pts = self._level(0, xyz, points, sa1._centres(xyz, s1, lengths), lengths)
            l2_xyz, l2_pts = self._level(1, l1_xyz, l1_pts, sa2._centres(l1_xyz, s2))
            h = self._level(2, l2_xyz, l2_pts)[1].reshape(xyz.size(0), -1)
            for name in ("fc1", "fc2"):
                h = self._run_head(name, h, self._eval_head)
            return ops.linear_log_softmax(h, self._snap["fc3"])
