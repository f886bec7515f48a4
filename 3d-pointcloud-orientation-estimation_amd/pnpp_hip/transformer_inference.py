"""Forward-only inference for the point transformer (models/point_transformer.py): what Predictor(model) is for a PointTransformer.

    predictor = Predictor(model)            # splits the weights into their bf16 planes, once
    out = predictor(xyz)                    # what model.eval()(xyz) returns under torch.no_grad(): (B, n_pts, in_dim) -> (B, 3)

Everything of an encoder layer behind its attention is row-local (out_proj, residual, LayerNorm, the feed-forward block, residual,
LayerNorm, the next layer's in_proj) and runs as ONE launch (pnpp_pt_infer_tail): the dim_feedforward-wide hidden activation is
produced and consumed on the chip and no tensor with that many columns is allocated.  A forward is pnpp_pt_infer_head, then per
layer the attention + pnpp_pt_infer_tail, then pnpp_pt_infer_pool: 2 + 2 * depth launches.  The stages are "head",
"layers.0" ... "layers.{depth-1}" and "pool"; `plan` says for each whether it runs "fused" or on the "eval-path", `last_plan` what
the latest call ran.

The attention has two forms, chosen by Predictor(model, attention=...): "split" is pnpp_attention_infer, both products on the bf16
matrix instruction from exact three-way splits of the float32 operands (no log-sum-exp, no dropout mask, no workspace); "float32" is
the training kernel pnpp_attention_fwd with lse = NULL and mask = NULL.  `attention` says which one the Predictor was built with,
`last_attention` which one the latest fused call ran: a call whose sizes pnpp_attention_infer_supported refuses runs the float32
kernel.  Without the keyword the form is DEFAULT_ATTENTION below.  A model the kernels refuse (pnpp_pt_infer_supported: another
width, head count or feed-forward size that is no multiple of 64, pre-norm, GELU, ...) runs transformer.point_transformer_forward
on a private eval-mode copy.

A ragged batch is predictor(xyz, lengths): xyz (B, n_pts, in_dim) padded, cloud b = rows 0 .. lengths[b] - 1 (a list, a CPU tensor, or
an int32 device tensor used as it is, without a synchronisation -- pnpp_hip.transformer.ragged_lengths); row b of the result is what
the call on xyz[b:b+1, :lengths[b]] alone returns, whatever the padding rows hold.  The same kernels run in their ragged forms, in both
attention forms; every row of the reused buffers is written on every call, so nothing stale reaches a later kernel.

Same contract as the other Predictors: a snapshot (refresh() folds again), not differentiable, nothing written to the model,
evaluated in eval mode whatever model.training says, any n_pts >= 1 (padded to a multiple of 128 inside), no CPU fallback.
"""
from __future__ import annotations

import copy
import ctypes as C
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .inference import Predictor, planes_to_float32

# the form Predictor(model) runs: per launch at 8 x 4096 pnpp_attention_infer takes 318 us against 553 us for pnpp_attention_fwd
# (kernel trace), far outside the spread of the timing windows
DEFAULT_ATTENTION = "split"

_MATRICES = {"in_proj": L.PT_IN_PROJ, "out_proj": L.PT_OUT_PROJ, "linear1": L.PT_LINEAR1, "linear2": L.PT_LINEAR2,
             "norm1": L.PT_NORM1, "norm2": L.PT_NORM2, "input_proj": L.PT_INPUT_PROJ}


def _layer_tensors(layer) -> Dict[str, torch.Tensor]:
    att = layer.self_attn
    return {"in_proj_w": att.in_proj_weight, "in_proj_b": att.in_proj_bias, "out_proj_w": att.out_proj.weight, "out_proj_b": att.out_proj.bias,
            "linear1_w": layer.linear1.weight, "linear1_b": layer.linear1.bias, "linear2_w": layer.linear2.weight, "linear2_b": layer.linear2.bias,
            "norm1_w": layer.norm1.weight, "norm1_b": layer.norm1.bias, "norm2_w": layer.norm2.weight, "norm2_b": layer.norm2.bias}


def _is_relu(layer) -> bool:
    code = getattr(layer, "activation_relu_or_gelu", None)
    if code is not None:
        return code == 1
    return layer.activation is torch.nn.functional.relu or isinstance(layer.activation, nn.ReLU)


class TransformerPredictor(Predictor):
    """Forward-only evaluation of models.point_transformer.PointTransformer; built by Predictor(model)."""

    ATTENTION_FORMS = ("split", "float32")

    def __init__(self, model: nn.Module, attention: str = DEFAULT_ATTENTION):
        from models.point_transformer import PointTransformer
        if not isinstance(model, PointTransformer):
            raise TypeError(f"TransformerPredictor takes a PointTransformer, not {type(model).__name__}")
        if attention not in self.ATTENTION_FORMS:
            raise ValueError(f"attention={attention!r}: the forms are {', '.join(repr(a) for a in self.ATTENTION_FORMS)}")
        self.attention = attention
        self.last_attention: Optional[str] = None   # what the latest fused call ran
        self._bind(model)
        self.depth = len(model.transformer.layers)
        self.stages = ["head"] + [f"layers.{l}" for l in range(self.depth)] + ["pool"]
        self._snap: Optional[nn.Module] = None
        self._blobs: List[torch.Tensor] = []   # one per layer: no allocation larger than a layer's planes
        d = self._desc(1, 128, 1)
        nbytes = L.lib().pnpp_pt_infer_weights_bytes(C.byref(d)) if d is not None else 0
        self.refused = None if nbytes else (self._why or L.last_error())   # why the kernels do not take the model
        if nbytes:
            self._blobs = [torch.empty(nbytes, dtype=torch.uint8, device=self.device) for _ in range(self.depth)]
        self.plan.update({s: "fused" if nbytes else "eval-path" for s in self.stages})
        self.last_plan.update(self.plan)
        self.refresh()

    # ---- construction ----------------------------------------------------------------------------------------------------
    def _desc(self, B: int, N: int, n_valid: int) -> Optional[L.PtInferDesc]:
        """the model's descriptor at these sizes, or None (self._why says why) when its structure is not the reference's"""
        m = self.model
        layers = list(m.transformer.layers)
        self._why = None
        if not layers or not isinstance(m.input_proj, nn.Linear) or not isinstance(m.fc_out, nn.Linear):
            self._why = "input_proj / fc_out are not nn.Linear or there is no encoder layer"
            return None
        if m.input_proj.bias is None or m.fc_out.bias is None:
            self._why = "input_proj / fc_out without bias"
            return None
        E, F = m.input_proj.out_features, None
        for l, layer in enumerate(layers):
            att = layer.self_attn
            if layer.norm_first or att.in_proj_weight is None or not att.batch_first or not _is_relu(layer):
                self._why = f"layers.{l}: only the post-norm, ReLU, packed in_proj, batch_first encoder layer of the reference"
                return None
            if not all(isinstance(x, nn.Linear) for x in (layer.linear1, layer.linear2)) or not isinstance(layer.norm1, nn.LayerNorm):
                self._why = f"layers.{l}: linear1 / linear2 / norm1 are not the reference's modules"
                return None
            ts = _layer_tensors(layer)
            if any(t is None for t in ts.values()):
                self._why = f"layers.{l}: a bias or LayerNorm parameter is missing"
                return None
            F = layer.linear1.out_features if F is None else F
            shapes = {"in_proj_w": (3 * E, E), "out_proj_w": (E, E), "linear1_w": (F, E), "linear2_w": (E, F), "norm1_w": (E,), "norm2_w": (E,)}
            if any(tuple(ts[k].shape) != s for k, s in shapes.items()) or att.num_heads != layers[0].self_attn.num_heads:
                self._why = f"layers.{l}: parameter shapes differ from (E={E}, F={F}) or the head count changes between layers"
                return None
            if layer.norm1.eps != layers[0].norm1.eps or layer.norm2.eps != layers[0].norm1.eps:
                self._why = f"layers.{l}: the LayerNorms' eps differ"
                return None
        if m.fc_out.in_features != E:
            self._why = "fc_out does not take the embedding"
            return None
        d = L.PtInferDesc()
        d.B, d.N, d.n_valid, d.in_dim = B, N, n_valid, m.input_proj.in_features
        d.E, d.H, d.F, d.depth, d.eps = E, layers[0].self_attn.num_heads, F, len(layers), float(layers[0].norm1.eps)
        return d

    @torch.no_grad()
    def refresh(self) -> None:
        """Split the model's current parameters again (after training steps, load_state_dict, ...)."""
        # the whole model is copied: fc_out is read from the copy, and a refused model or call runs the eval path on it
        self._snap = copy.deepcopy(self.model).requires_grad_(False).eval()
        if not self._blobs:
            return
        d = self._desc(1, 128, 1)
        iw, ib = ops._f32(self.model.input_proj.weight.detach(), "input_proj.weight"), ops._f32(self.model.input_proj.bias.detach(), "input_proj.bias")
        with torch.cuda.device(self.device):
            for l, layer in enumerate(self.model.transformer.layers):
                params = L.PtInferLayerParams()
                keep = []   # the contiguous float32 tensors whose pointers the call reads
                for name, t in _layer_tensors(layer).items():
                    t = ops._f32(t.detach(), name)
                    keep.append(t)
                    setattr(params, name, t.data_ptr())
                L.check(L.lib().pnpp_pt_infer_fold(C.byref(d), l, C.byref(params), iw.data_ptr(), ib.data_ptr(), self._blobs[l].data_ptr(),
                                                   ops._stream()))

    def folded(self, layer: int, name: str):
        """(matrix, bias) of the blob as float32 tensors, the documented view (pnpp_pt_infer_weights_layout): for "in_proj", "out_proj",
        "linear1", "linear2" the matrix its three bf16 planes sum to; for "norm1", "norm2" the LayerNorm's (weight, bias); for
        "input_proj" (layer 0) the (E, 8) matrix, zero beyond in_dim."""
        if not self._blobs:
            raise RuntimeError(f"nothing is folded: {self.refused}")
        d = self._desc(1, 128, 1)
        woff, ld, boff = C.c_size_t(), C.c_int(), C.c_size_t()
        L.check(L.lib().pnpp_pt_infer_weights_layout(C.byref(d), layer, _MATRICES[name], C.byref(woff), C.byref(ld), C.byref(boff)))
        blob, E = self._blobs[layer], d.E

        def f32(off, n):
            return blob[off:off + 4 * n].view(torch.float32).clone()
        if name in ("norm1", "norm2"):
            return f32(woff.value, E), f32(boff.value, E)
        if name == "input_proj":
            return f32(woff.value, E * ld.value).view(E, ld.value), f32(boff.value, E)
        rows = {"in_proj": 3 * E, "linear1": d.F}.get(name, E)
        return planes_to_float32(blob, woff.value, rows, ld.value), f32(boff.value, rows)

    def _blob_tensors(self):
        return list(self._blobs)

    # ---- one call --------------------------------------------------------------------------------------------------------
    def _sizes(self, xyz):
        """(descriptor | None, B, n_pts, N) of a call"""
        xyz = ops._f32(xyz, "xyz")
        if xyz.dim() != 3 or xyz.shape[1] < 1:
            raise ValueError(f"expected a (B, n_pts, in_dim) input with n_pts >= 1, got {tuple(xyz.shape)}")
        B, n_pts, K = xyz.shape
        if K != self.model.input_proj.in_features:
            raise ValueError(f"the model takes {self.model.input_proj.in_features} input columns, got {K}")
        N = (n_pts + 127) // 128 * 128
        d = self._desc(B, N, n_pts) if self._blobs else None
        if d is not None and not L.lib().pnpp_pt_infer_supported(C.byref(d)):
            d = None
        return xyz, d, B, n_pts, N

    def _buffers(self, d):
        M = d.B * d.N
        x = self._buf("x", (2, M, d.E), torch.float32)            # ping-pong: a layer's input and output
        qkv = self._buf("qkv", (M, 3 * d.E), torch.float32)
        att = self._buf("attention", (M, d.E), torch.float32)
        part = self._buf("partial", (L.lib().pnpp_pt_infer_scratch_bytes(C.byref(d)),), torch.uint8)
        return x, qkv, att, part

    def _split_supported(self, d) -> bool:
        return bool(L.lib().pnpp_attention_infer_supported(d.B, d.N, d.n_valid, d.H, d.E // d.H))

    def _attention_form(self, d) -> str:
        """the form this call runs: the Predictor's own, or "float32" where the split kernel does not take the call's sizes"""
        return "split" if self.attention == "split" and self._split_supported(d) else "float32"

    def _attention(self, d, qkv, att, form, lengths=None):
        lib, hd = L.lib(), d.E // d.H
        if lengths is None:
            if form == "split":
                L.check(lib.pnpp_attention_infer(qkv.data_ptr(), d.B, d.N, d.n_valid, d.H, hd, att.data_ptr(), ops._stream()))
            else:
                L.check(lib.pnpp_attention_fwd(qkv.data_ptr(), d.B, d.N, d.n_valid, d.H, hd, None, 0.0, att.data_ptr(), None, ops._stream()))
        elif form == "split":
            L.check(lib.pnpp_attention_infer_ragged(qkv.data_ptr(), d.B, d.N, d.n_valid, lengths.data_ptr(), d.H, hd, att.data_ptr(), ops._stream()))
        else:
            L.check(lib.pnpp_attention_fwd_ragged(qkv.data_ptr(), d.B, d.N, d.n_valid, lengths.data_ptr(), d.H, hd, None, 0.0, att.data_ptr(), None,
                                                  ops._stream()))
        self.last_attention = form

    def _pool(self, d, part, w, b, lengths=None):
        out = torch.empty(d.B, w.shape[0], device=self.device, dtype=torch.float32)
        if lengths is None:
            L.check(L.lib().pnpp_pt_infer_pool(C.byref(d), part.data_ptr(), w.data_ptr(), b.data_ptr(), w.shape[0], out.data_ptr(), ops._stream()))
        else:
            L.check(L.lib().pnpp_pt_infer_pool_ragged(C.byref(d), lengths.data_ptr(), part.data_ptr(), w.data_ptr(), b.data_ptr(), w.shape[0],
                                                      out.data_ptr(), ops._stream()))
        return out

    @torch.no_grad()
    def __call__(self, xyz: torch.Tensor, lengths=None) -> torch.Tensor:
        ops._need_gpu(xyz, "xyz")
        with torch.cuda.device(self.device):
            xyz, d, B, n_pts, N = self._sizes(xyz.detach())
            from . import transformer
            if lengths is not None:
                lengths = transformer.ragged_lengths(lengths, B, n_pts, xyz.device)
            self.last_plan = {s: "fused" if d is not None else "eval-path" for s in self.stages}
            if d is None:
                return transformer.point_transformer_forward(self._snap, xyz, lengths)
            lib, st = L.lib(), ops._stream()
            blobs = [b.data_ptr() for b in self._blobs] + [None]
            x, qkv, att, part = self._buffers(d)
            form = self._attention_form(d)
            if lengths is None:
                L.check(lib.pnpp_pt_infer_head(C.byref(d), xyz.data_ptr(), blobs[0], x[0].data_ptr(), qkv.data_ptr(), st))
            else:
                L.check(lib.pnpp_pt_infer_head_ragged(C.byref(d), lengths.data_ptr(), xyz.data_ptr(), blobs[0], x[0].data_ptr(), qkv.data_ptr(), st))
            for l in range(self.depth):
                self._attention(d, qkv, att, form, lengths)
                args = (l, x[l & 1].data_ptr(), att.data_ptr(), blobs[l], blobs[l + 1], x[(l + 1) & 1].data_ptr(), qkv.data_ptr(), part.data_ptr(), st)
                if lengths is None:
                    L.check(lib.pnpp_pt_infer_tail(C.byref(d), *args))
                else:
                    L.check(lib.pnpp_pt_infer_tail_ragged(C.byref(d), lengths.data_ptr(), *args))
            fc = self._snap.fc_out
            return self._pool(d, part, fc.weight, fc.bias, lengths)

    # ---- single stages (parity tests, tools) -------------------------------------------------------------------------------
    @torch.no_grad()
    def head(self, xyz: torch.Tensor):
        """pnpp_pt_infer_head alone: -> (x0 (B, N, E), qkv_0 (B, N, 3E)) with N = n_pts rounded up to 128; views of reused buffers"""
        with torch.cuda.device(self.device):
            xyz, d, B, n_pts, N = self._sizes(xyz.detach())
            if d is None:
                raise RuntimeError(f"the fused kernels do not take this model or call: {self.refused or L.last_error()}")
            x, qkv, _, _ = self._buffers(d)
            L.check(L.lib().pnpp_pt_infer_head(C.byref(d), xyz.data_ptr(), self._blobs[0].data_ptr(), x[0].data_ptr(), qkv.data_ptr(), ops._stream()))
            return x[0].view(B, N, d.E), qkv.view(B, N, 3 * d.E)

    @torch.no_grad()
    def attend(self, qkv_in: torch.Tensor):
        """the attention alone on qkv_in (B, n_pts, 3E) float32, a layer's in_proj output: -> (B, N, E) with N = n_pts rounded up to 128,
        a view of a reused buffer.  Rows beyond n_pts are padded with zeros here; the output's rows beyond n_pts are finite and mean
        nothing.  Runs the form a call of these sizes runs (`last_attention`)."""
        with torch.cuda.device(self.device):
            if qkv_in.dim() != 3 or qkv_in.shape[1] < 1:
                raise ValueError(f"expected a (B, n_pts, 3E) input with n_pts >= 1, got {tuple(qkv_in.shape)}")
            B, n_pts, E3 = qkv_in.shape
            N = (n_pts + 127) // 128 * 128
            d = self._desc(B, N, n_pts) if self._blobs else None
            if d is None or not L.lib().pnpp_pt_infer_supported(C.byref(d)):
                raise RuntimeError(f"the fused kernels do not take this model or call: {self.refused or L.last_error()}")
            if E3 != 3 * d.E:
                raise ValueError(f"the model's qkv rows have {3 * d.E} columns, got {E3}")
            _, qkv, att, _ = self._buffers(d)
            qkv.zero_()
            qkv.view(B, N, E3)[:, :n_pts] = ops._f32(qkv_in, "qkv")
            self._attention(d, qkv, att, self._attention_form(d))
            return att.view(B, N, d.E)

    @torch.no_grad()
    def tail(self, layer: int, x_in: torch.Tensor, o_in: torch.Tensor):
        """pnpp_pt_infer_tail of one layer alone on x_in, o_in (B, n_pts, E): the layer's input and its attention output (rows beyond
        n_pts are padded with zeros here).  -> (x_next (B, N, E), qkv_next (B, N, 3E)), or in the last layer (x_next, the mean of
        x_next over each cloud's n_pts points (B, E), from the partial sums through pnpp_pt_infer_pool with an identity fc)."""
        with torch.cuda.device(self.device):
            B, n_pts, E = x_in.shape
            N = (n_pts + 127) // 128 * 128
            d = self._desc(B, N, n_pts) if self._blobs else None
            if d is None or not L.lib().pnpp_pt_infer_supported(C.byref(d)):
                raise RuntimeError(f"the fused kernels do not take this model or call: {self.refused or L.last_error()}")
            x, qkv, att, part = self._buffers(d)
            x[0].zero_(), att.zero_()
            x[0].view(B, N, E)[:, :n_pts] = ops._f32(x_in, "x")
            att.view(B, N, E)[:, :n_pts] = ops._f32(o_in, "o")
            nxt = self._blobs[layer + 1].data_ptr() if layer < self.depth - 1 else None
            L.check(L.lib().pnpp_pt_infer_tail(C.byref(d), layer, x[0].data_ptr(), att.data_ptr(), self._blobs[layer].data_ptr(), nxt,
                                               x[1].data_ptr(), qkv.data_ptr(), part.data_ptr(), ops._stream()))
            if layer < self.depth - 1:
                return x[1].view(B, N, E), qkv.view(B, N, 3 * E)
            eye = torch.eye(E, device=self.device, dtype=torch.float32)
            return x[1].view(B, N, E), self._pool(d, part, eye, torch.zeros(E, device=self.device, dtype=torch.float32))
