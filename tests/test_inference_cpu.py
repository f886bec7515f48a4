"""CPU-side checks of the forward-only inference path: the additions to the C ABI (argument validation happens before any launch,
so it runs without a GPU), the descriptor query and the Python surface's refusal to run off-GPU."""
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


def _desc(B, N, S, K, D, channels, group_all=False):
    from pnpp_hip import _lib
    d = _lib.SaDesc()
    d.B, d.N, d.S, d.K, d.D, d.L = B, N, S, K, D, len(channels)
    for i, c in enumerate(channels):
        d.C[i] = c
    d.group_all, d.training, d.eps, d.momentum = int(group_all), 0, 1e-5, 0.1
    return d


BASELINE_LEVELS = [
    dict(B=32, N=1024, S=128, K=32, D=0, channels=[64, 64, 128]),
    dict(B=32, N=128, S=32, K=32, D=128, channels=[128, 128, 256]),
    dict(B=32, N=32, S=1, K=32, D=256, channels=[256, 512, 1024], group_all=True),
]


def test_infer_args_layout_matches_c():
    from pnpp_hip import _lib
    src = textwrap.dedent('''
        #include <stdio.h>
        #include "pnpp_hip.h"
        int main(void) { printf("%zu\\n", sizeof(pnpp_sa_infer_args)); return 0; }
    ''')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        size = int(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    assert size == ctypes.sizeof(_lib.SaInferArgs)


def test_infer_null_pointers_are_argument_errors(lib):
    from pnpp_hip import _lib
    d = _desc(**BASELINE_LEVELS[0])
    assert lib.pnpp_sa_infer(ctypes.byref(d), None, None) == _lib.PNPP_ERR_ARG
    a = _lib.SaInferArgs()
    assert lib.pnpp_sa_infer(ctypes.byref(d), ctypes.byref(a), None) == _lib.PNPP_ERR_ARG
    assert b"null" in lib.pnpp_last_error()
    assert lib.pnpp_sa_infer(None, ctypes.byref(a), None) == _lib.PNPP_ERR_ARG
    assert lib.pnpp_sa_infer_fold(ctypes.byref(d), None, None, None) == _lib.PNPP_ERR_ARG
    assert lib.pnpp_fc_infer_fold(512, 1024, None, None, None, None, None, None, 1e-5, None, None, None) == _lib.PNPP_ERR_ARG
    assert lib.pnpp_sa_infer_group_pair(ctypes.byref(d), ctypes.byref(d), None, None, None, None, None, None, None, None) == _lib.PNPP_ERR_ARG


@pytest.mark.parametrize("level", range(3))
def test_baseline_levels_are_taken(lib, level):
    d = _desc(**BASELINE_LEVELS[level])
    assert lib.pnpp_sa_infer_supported(ctypes.byref(d)) == 1
    nbytes = lib.pnpp_sa_infer_weights_bytes(ctypes.byref(d))
    ch, cin = BASELINE_LEVELS[level]["channels"], BASELINE_LEVELS[level]["D"] + 3
    assert nbytes >= 4 * (ch[0] * cin + ch[1] * ch[0] + ch[2] * ch[1] + sum(ch))
    end = 0
    for l in range(3):   # the documented view: layers in order, nothing overlaps, everything inside the blob
        woff, ld, boff = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t()
        assert lib.pnpp_sa_infer_weights_layout(ctypes.byref(d), l, ctypes.byref(woff), ctypes.byref(ld), ctypes.byref(boff)) == 0
        assert ld.value >= (cin if l == 0 else ch[l - 1]) and ld.value % 8 == 0
        assert woff.value >= end and boff.value >= woff.value + 4 * ch[l] * ld.value
        end = boff.value + 4 * ch[l]
    assert end <= nbytes
    # B, N and S do not enter the answer: any batch, any cloud, partial last tiles
    for B, N, S in ((1, 10000, 128), (36, 777, 33)):
        kw = dict(BASELINE_LEVELS[level])
        if kw.get("group_all"):
            kw.update(B=B)
        else:
            kw.update(B=B, N=N, S=S)
        d2 = _desc(**kw)
        assert lib.pnpp_sa_infer_supported(ctypes.byref(d2)) == 1
        assert lib.pnpp_sa_infer_weights_bytes(ctypes.byref(d2)) == nbytes


def test_refused_descriptors_name_the_reason(lib):
    kw = dict(BASELINE_LEVELS[0])
    kw["K"] = 24
    d = _desc(**kw)
    assert lib.pnpp_sa_infer_supported(ctypes.byref(d)) == 0
    assert b"K=24" in lib.pnpp_last_error()
    assert lib.pnpp_sa_infer_weights_bytes(ctypes.byref(d)) == 0
    kw = dict(BASELINE_LEVELS[1])
    kw["channels"] = [128, 128]
    d = _desc(**kw)
    assert lib.pnpp_sa_infer_supported(ctypes.byref(d)) == 0
    assert b"3 layers" in lib.pnpp_last_error()
    kw = dict(BASELINE_LEVELS[1])
    kw["channels"] = [128, 2048, 256]
    d = _desc(**kw)
    assert lib.pnpp_sa_infer_supported(ctypes.byref(d)) == 0
    assert b"multiple of 32 up to 1024" in lib.pnpp_last_error()
    d = _desc(B=4, N=1024, S=1, K=1024, D=0, channels=[64, 64, 128], group_all=True)   # whole-cloud pooling over 1024 rows
    assert lib.pnpp_sa_infer_supported(ctypes.byref(d)) == 0
    assert lib.pnpp_sa_infer_weights_bytes(ctypes.byref(d)) == 0


def test_predictor_has_no_cpu_fallback():
    import pnpp_hip
    from pnpp_hip.inference import Predictor
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    assert pnpp_hip.Predictor is Predictor
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Predictor(PointNetPPVonMises())
    with pytest.raises(TypeError):
        Predictor(torch.nn.Linear(3, 3))
