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


# ---- the plan's edges (the shapes tests/test_gpu_sa_infer_bands.py launches, and one step beyond them) ----------------------------------
def _band_desc(c, **over):
    kw = dict(B=c["B"], N=c["N"], S=c["S"], K=c["K"], D=c["D"], channels=c["ch"], group_all=c.get("group_all", False))
    kw.update(over)
    return _desc(**kw)


def _layout(lib, d):
    """[(w_offset, w_ld, b_offset)] of the three layers"""
    out = []
    for l in range(3):
        woff, ld, boff = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t()
        assert lib.pnpp_sa_infer_weights_layout(ctypes.byref(d), l, ctypes.byref(woff), ctypes.byref(ld), ctypes.byref(boff)) == 0
        out.append((woff.value, ld.value, boff.value))
    return out


def _up(x, a):
    return (x + a - 1) // a * a


def _blob_by_hand(D, ch):
    """per layer three bf16 planes of C_l x ld_l, then C_l floats, every piece on a 256-byte boundary -> ([(woff, ld, boff)], bytes)"""
    off, out = 0, []
    for l in range(3):
        ld = _up(D + 3, 16) if l == 0 else ch[l - 1]
        woff = off
        boff = _up(woff + ch[l] * ld * 3 * 2, 256)
        off = _up(boff + ch[l] * 4, 256)
        out.append((woff, ld, boff))
    return out, off


def test_every_band_case_is_taken_and_its_lds_is_what_the_table_says(lib):
    from sa_infer_bands_cases import CASES, plan_lds
    for name, c in CASES.items():
        d = _band_desc(c)
        assert lib.pnpp_sa_infer_supported(ctypes.byref(d)) == 1, (name, lib.pnpp_last_error())
        assert plan_lds(c) <= 160 * 1024, name
        if "lds" in c:
            assert plan_lds(c) == c["lds"], name
        if c["tm"] == 64:   # TM = 64 only where 64 rows fit 80 KiB, on more than 32 rows of neighbourhoods of at most 32
            assert plan_lds(c) <= 80 * 1024 and c["B"] * c["S"] * c["K"] > 32 and c["K"] <= 32, name
        else:
            assert 2 * plan_lds(c) > 80 * 1024 or c["B"] * c["S"] * c["K"] <= 32 or c["K"] > 32, name
        want, nbytes = _blob_by_hand(c["D"], c["ch"])
        assert _layout(lib, d) == want and lib.pnpp_sa_infer_weights_bytes(ctypes.byref(d)) == nbytes, name


@pytest.mark.parametrize("D,channels,need", [(0, [544, 320, 320], 168960), (798, [32, 64, 128], 165888)], ids=["C1-320", "D798"])
def test_one_step_past_the_largest_tile_is_refused_for_lds(lib, D, channels, need):
    for K in (32, 64):   # the narrow kernel's 32-row tile and the wide kernel's
        d = _desc(B=2, N=100, S=3, K=K, D=D, channels=channels)
        assert lib.pnpp_sa_infer_supported(ctypes.byref(d)) == 0
        err = lib.pnpp_last_error()
        assert b"LDS" in err and str(need).encode() in err, err
        assert lib.pnpp_sa_infer_weights_bytes(ctypes.byref(d)) == 0
        woff, ld, boff = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t()
        assert lib.pnpp_sa_infer_weights_layout(ctypes.byref(d), 0, ctypes.byref(woff), ctypes.byref(ld), ctypes.byref(boff)) != 0


@pytest.mark.parametrize("K", [48, 288])
def test_k_between_and_beyond_the_tiles_is_refused(lib, K):
    d = _desc(B=2, N=300, S=3, K=K, D=0, channels=[64, 64, 128])
    assert lib.pnpp_sa_infer_supported(ctypes.byref(d)) == 0
    assert b"K=%d" % K in lib.pnpp_last_error()
    assert lib.pnpp_sa_infer_weights_bytes(ctypes.byref(d)) == 0
    d = _desc(B=2, N=K, S=1, K=K, D=0, channels=[64, 64, 128], group_all=True)
    assert lib.pnpp_sa_infer_supported(ctypes.byref(d)) == 0
    assert b"K=%d" % K in lib.pnpp_last_error()


@pytest.mark.parametrize("channels", [[96, 96, 160], [544, 288, 320], [128, 160, 288], [32, 32, 32]], ids=lambda c: "-".join(map(str, c)))
def test_blob_layout_at_odd_widths_and_d14(lib, channels):
    D = 14
    d = _desc(B=2, N=100, S=5, K=32, D=D, channels=channels)
    lay, nbytes = _layout(lib, d), lib.pnpp_sa_infer_weights_bytes(ctypes.byref(d))
    assert lay[0][1] == 32 == _up(D + 3, 16)
    assert [ld for _, ld, _ in lay[1:]] == channels[:2]
    assert all(woff % 256 == 0 and boff % 256 == 0 for woff, _, boff in lay)
    pieces = [_up(c * ld * 3 * 2, 256) + _up(c * 4, 256) for c, (_, ld, _) in zip(channels, lay)]
    assert nbytes == sum(pieces)
    assert [woff for woff, _, _ in lay] == [0, pieces[0], pieces[0] + pieces[1]]
    assert [boff - woff for woff, _, boff in lay] == [_up(c * ld * 3 * 2, 256) for c, (_, ld, _) in zip(channels, lay)]
    # the blob belongs to the weights: B, N, S and K do not enter (K = 64 .. 256 are the wide kernel's, K = 16 the narrow one's)
    for B, N, S, K in ((1, 40, 1, 32), (7, 333, 33, 16), (2, 300, 3, 64), (5, 300, 2, 256)):
        d2 = _desc(B=B, N=N, S=S, K=K, D=D, channels=channels)
        assert lib.pnpp_sa_infer_supported(ctypes.byref(d2)) == 1, lib.pnpp_last_error()
        assert _layout(lib, d2) == lay and lib.pnpp_sa_infer_weights_bytes(ctypes.byref(d2)) == nbytes
    dg = _desc(B=3, N=224, S=1, K=224, D=D, channels=channels, group_all=True)
    assert _layout(lib, dg) == lay and lib.pnpp_sa_infer_weights_bytes(ctypes.byref(dg)) == nbytes


def test_predictor_has_no_cpu_fallback():
    import pnpp_hip
    from pnpp_hip.inference import Predictor
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    assert pnpp_hip.Predictor is Predictor
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Predictor(PointNetPPVonMises())
    with pytest.raises(TypeError):
        Predictor(torch.nn.Linear(3, 3))
