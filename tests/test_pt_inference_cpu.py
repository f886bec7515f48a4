"""CPU-side checks of the forward-only path of the point transformer: the pnpp_pt_infer_* additions to the C ABI (argument validation
happens before any launch, so it runs without a GPU), the descriptor queries and the Python surface's refusal to run off-GPU."""
import ctypes
import os
import subprocess
import tempfile
import textwrap

import pytest
import torch

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from pnpp_hip import build, _lib
    build.build()
    return _lib.lib()


def _desc(B=8, N=4096, n_valid=None, in_dim=3, E=64, H=4, F=2048, depth=6):
    from pnpp_hip import _lib
    d = _lib.PtInferDesc()
    d.B, d.N, d.n_valid, d.in_dim, d.E, d.H, d.F, d.depth, d.eps = B, N, N if n_valid is None else n_valid, in_dim, E, H, F, depth, 1e-5
    return d


def test_predictor_of_a_cpu_point_transformer_has_no_cpu_fallback():
    from pnpp_hip import Predictor
    from models.point_transformer import PointTransformer
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Predictor(PointTransformer())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Predictor(PointTransformer(depth=2))
    with pytest.raises(TypeError, match="PointTransformer"):   # the message names the new family as well
        Predictor(torch.nn.Linear(3, 3))


def test_reference_shape_is_taken(lib):
    for N in (128, 256, 4096):
        for B in (1, 3):
            assert lib.pnpp_pt_infer_supported(ctypes.byref(_desc(B=B, N=N))) == 1, (B, N, lib.pnpp_last_error())
    for n_valid in range(1, 129):
        assert lib.pnpp_pt_infer_supported(ctypes.byref(_desc(B=3, N=128, n_valid=n_valid))) == 1, n_valid
    for kw in (dict(in_dim=1), dict(in_dim=8), dict(F=64), dict(depth=1)):
        assert lib.pnpp_pt_infer_supported(ctypes.byref(_desc(**kw))) == 1, kw
    d = _desc()
    assert lib.pnpp_pt_infer_scratch_bytes(ctypes.byref(d)) == 8 * (4096 // 32) * 64 * 4   # one row per 32 points, nothing per point


@pytest.mark.parametrize("kw, field", [(dict(E=128), b"E=128"), (dict(H=2), b"H=2"), (dict(N=100), b"N=100"), (dict(F=96), b"F=96"),
                                       (dict(in_dim=9), b"in_dim=9"), (dict(N=128, n_valid=0), b"n_valid=0")])
def test_refused_descriptors_name_the_field(lib, kw, field):
    d = _desc(**kw)
    assert lib.pnpp_pt_infer_supported(ctypes.byref(d)) == 0
    assert field in lib.pnpp_last_error(), lib.pnpp_last_error()
    assert lib.pnpp_pt_infer_weights_bytes(ctypes.byref(d)) == 0
    assert lib.pnpp_pt_infer_scratch_bytes(ctypes.byref(d)) == 0
    woff, ld, boff = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t()
    assert lib.pnpp_pt_infer_weights_layout(ctypes.byref(d), 0, 0, ctypes.byref(woff), ctypes.byref(ld), ctypes.byref(boff)) != 0


def test_weights_layout_is_aligned_disjoint_and_inside(lib):
    from pnpp_hip import _lib
    d = _desc()
    nbytes = lib.pnpp_pt_infer_weights_bytes(ctypes.byref(d))
    E, F = 64, 2048
    assert nbytes >= 6 * (3 * E * E + E * E + 2 * E * F) + 4 * (3 * E + E + F + E + 4 * E)
    assert nbytes == lib.pnpp_pt_infer_weights_bytes(ctypes.byref(_desc(B=1, N=128, n_valid=5)))   # independent of the call's sizes
    shape = {_lib.PT_IN_PROJ: (3 * E, E), _lib.PT_OUT_PROJ: (E, E), _lib.PT_LINEAR1: (F, E), _lib.PT_LINEAR2: (E, F)}
    for layer in range(d.depth):
        spans = []
        for m in range(7):
            woff, ld, boff = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t()
            assert lib.pnpp_pt_infer_weights_layout(ctypes.byref(d), layer, m, ctypes.byref(woff), ctypes.byref(ld), ctypes.byref(boff)) == 0
            assert woff.value % 16 == 0 and boff.value % 16 == 0
            if m in shape:      # three bf16 planes, float32 bias
                rows, cols = shape[m]
                assert ld.value == cols
                spans += [(woff.value, woff.value + 6 * rows * cols), (boff.value, boff.value + 4 * rows)]
            elif m == _lib.PT_INPUT_PROJ:
                assert ld.value == 8
                spans += [(woff.value, woff.value + 4 * E * 8), (boff.value, boff.value + 4 * E)]
            else:
                spans += [(woff.value, woff.value + 4 * E), (boff.value, boff.value + 4 * E)]
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans
        assert spans[0][0] >= 0 and spans[-1][1] <= nbytes
    woff, ld, boff = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t()
    for layer, m in ((d.depth, 0), (-1, 0), (0, 7), (0, -1)):
        assert lib.pnpp_pt_infer_weights_layout(ctypes.byref(d), layer, m, ctypes.byref(woff), ctypes.byref(ld), ctypes.byref(boff)) == _lib.PNPP_ERR_ARG


def test_struct_layouts_match_c():
    from pnpp_hip import _lib
    src = textwrap.dedent('''
        #include <stdio.h>
        #include "pnpp_hip.h"
        int main(void) { printf("%zu %zu\\n", sizeof(pnpp_pt_infer_desc), sizeof(pnpp_pt_infer_layer_params)); return 0; }
    ''')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        sizes = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [ctypes.sizeof(_lib.PtInferDesc), ctypes.sizeof(_lib.PtInferLayerParams)]


def test_null_pointers_are_argument_errors(lib):
    from pnpp_hip import _lib
    d = _desc(B=2, N=256, depth=2)
    dp = ctypes.byref(d)
    assert lib.pnpp_pt_infer_supported(None) == 0
    assert lib.pnpp_pt_infer_weights_bytes(None) == 0 and lib.pnpp_pt_infer_scratch_bytes(None) == 0
    assert lib.pnpp_pt_infer_weights_layout(dp, 0, 0, None, None, None) == _lib.PNPP_ERR_ARG
    assert lib.pnpp_pt_infer_head(dp, None, None, None, None, None) == _lib.PNPP_ERR_ARG
    assert b"null" in lib.pnpp_last_error()
    assert lib.pnpp_pt_infer_head(None, 8, 8, 8, 8, None) == _lib.PNPP_ERR_ARG
    assert lib.pnpp_pt_infer_head(dp, 8, 8, 8, None, None) == _lib.PNPP_ERR_ARG
    assert lib.pnpp_pt_infer_tail(dp, 0, None, None, None, None, None, None, None, None) == _lib.PNPP_ERR_ARG
    assert b"null" in lib.pnpp_last_error()
    assert lib.pnpp_pt_infer_tail(dp, 0, 8, 16, 8, None, 24, 8, None, None) == _lib.PNPP_ERR_ARG     # a middle layer needs the next blob
    assert b"weights_next" in lib.pnpp_last_error()
    assert lib.pnpp_pt_infer_tail(dp, 1, 8, 16, 8, None, 24, None, None, None) == _lib.PNPP_ERR_ARG  # the last layer needs the scratch
    assert b"scratch" in lib.pnpp_last_error()
    assert lib.pnpp_pt_infer_tail(dp, 2, 8, 16, 8, 8, 24, 8, 8, None) == _lib.PNPP_ERR_ARG           # no such layer
    assert lib.pnpp_pt_infer_tail(dp, 0, 8, 16, 8, 8, 8, 8, 8, None) == _lib.PNPP_ERR_ARG            # in place
    assert b"alias" in lib.pnpp_last_error()
    assert lib.pnpp_pt_infer_pool(dp, None, None, None, 3, None, None) == _lib.PNPP_ERR_ARG
    assert b"null" in lib.pnpp_last_error()
    assert lib.pnpp_pt_infer_pool(dp, 8, 8, 8, 0, 8, None) == _lib.PNPP_ERR_ARG
    q = _lib.PtInferLayerParams()
    assert lib.pnpp_pt_infer_fold(dp, 0, None, 8, 8, 8, None) == _lib.PNPP_ERR_ARG
    assert lib.pnpp_pt_infer_fold(dp, 0, ctypes.byref(q), 8, 8, 8, None) == _lib.PNPP_ERR_ARG
    assert b"null parameter pointer in layer 0" in lib.pnpp_last_error()
    for name, _ in q._fields_:
        setattr(q, name, 8)
    assert lib.pnpp_pt_infer_fold(dp, 0, ctypes.byref(q), None, None, 8, None) == _lib.PNPP_ERR_ARG
    assert b"input_proj" in lib.pnpp_last_error()
    refused = _desc(E=128)
    assert lib.pnpp_pt_infer_head(ctypes.byref(refused), 8, 8, 8, 8, None) == _lib.PNPP_ERR_ARG and b"E=128" in lib.pnpp_last_error()
