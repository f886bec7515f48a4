"""CPU-side checks of the forward-only path of the vanilla PointNet models: the pnpp_pn_infer_* additions to the C ABI (argument
validation happens before any launch, so it runs without a GPU), the descriptor queries, the Python surface's refusal to run
off-GPU, and the eval-mode fixture's own consistency."""
import ctypes
import os
import subprocess
import tempfile
import textwrap

import numpy as np
import pytest
import torch

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from pnpp_hip import build, _lib
    build.build()
    return _lib.lib()


def _desc(B, N, D, channels, input_transform=0, transform_after=-1, relu_last=1):
    from pnpp_hip import _lib
    d = _lib.PnInferDesc()
    d.B, d.N, d.D, d.L = B, N, D, len(channels)
    for i, c in enumerate(channels[:_lib.PNPP_MAX_LAYERS]):
        d.C[i] = c
    d.input_transform, d.transform_after, d.relu_last, d.eps = input_transform, transform_after, relu_last, 1e-5
    return d


def _trunks(D):
    """the trunk shapes of DESIGN section 11's table, with and without the feature transform"""
    return {
        "stn": dict(D=D, channels=[64, 128, 1024]),
        "fstn": dict(D=D, channels=[64, 64, 128, 1024], input_transform=1),
        "encoder": dict(D=D, channels=[64, 128, 1024], input_transform=1, relu_last=0),
        "encoder+ft": dict(D=D, channels=[64, 128, 1024], input_transform=1, transform_after=0, relu_last=0),
    }


def test_predictor_of_a_cpu_pointnet_has_no_cpu_fallback():
    from pnpp_hip import Predictor
    from models.pointnet import PointNet, PointNetEncoder
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Predictor(PointNet())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Predictor(PointNetEncoder(global_feat=False, feature_transform=True, channel=6))
    with pytest.raises(TypeError):
        Predictor(torch.nn.Linear(3, 3))


def test_struct_layouts_match_c():
    from pnpp_hip import _lib
    src = textwrap.dedent('''
        #include <stdio.h>
        #include "pnpp_hip.h"
        int main(void) { printf("%zu %zu\\n", sizeof(pnpp_pn_infer_desc), sizeof(pnpp_pn_infer_args)); return 0; }
    ''')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        sizes = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [ctypes.sizeof(_lib.PnInferDesc), ctypes.sizeof(_lib.PnInferArgs)]


def test_null_pointers_are_argument_errors(lib):
    from pnpp_hip import _lib
    d = _desc(32, 1024, **_trunks(3)["stn"])
    assert lib.pnpp_pn_infer(ctypes.byref(d), None, None) == _lib.PNPP_ERR_ARG
    assert b"null" in lib.pnpp_last_error()
    a = _lib.PnInferArgs()
    assert lib.pnpp_pn_infer(ctypes.byref(d), ctypes.byref(a), None) == _lib.PNPP_ERR_ARG
    assert b"null" in lib.pnpp_last_error()
    assert lib.pnpp_pn_infer(None, ctypes.byref(a), None) == _lib.PNPP_ERR_ARG
    assert lib.pnpp_pn_infer_fold(ctypes.byref(d), None, None, None) == _lib.PNPP_ERR_ARG
    assert b"null" in lib.pnpp_last_error()
    assert lib.pnpp_pn_infer_supported(None) == 0
    assert lib.pnpp_pn_infer_weights_bytes(None) == 0 and lib.pnpp_pn_infer_scratch_bytes(None) == 0
    assert lib.pnpp_pn_infer_weights_layout(ctypes.byref(d), 0, None, None, None) == _lib.PNPP_ERR_ARG
    # everything but the transform the descriptor asks for: still an argument error, before any launch
    d2 = _desc(32, 1024, **_trunks(3)["encoder+ft"])
    a.x = a.weights = a.scratch = a.out = 8
    assert lib.pnpp_pn_infer(ctypes.byref(d2), ctypes.byref(a), None) == _lib.PNPP_ERR_ARG
    assert b"trans is null" in lib.pnpp_last_error()
    a.trans = 8
    assert lib.pnpp_pn_infer(ctypes.byref(d2), ctypes.byref(a), None) == _lib.PNPP_ERR_ARG
    assert b"trans_feat is null" in lib.pnpp_last_error()
    a.trans_feat, a.feat_out, a.feat_layer = 8, 8, 1   # layer 1 is 128 wide: nothing wider than 64 is written per point
    assert lib.pnpp_pn_infer(ctypes.byref(d2), ctypes.byref(a), None) == _lib.PNPP_ERR_ARG
    assert b"at most 64 wide" in lib.pnpp_last_error()


@pytest.mark.parametrize("D", [3, 6])
@pytest.mark.parametrize("trunk", ["stn", "fstn", "encoder", "encoder+ft"])
def test_every_trunk_is_taken_at_any_size(lib, trunk, D):
    kw = _trunks(D)[trunk]
    ch = kw["channels"]
    sizes = ((32, 1024), (1, 1), (36, 777), (2, 10000))
    d = _desc(*sizes[0], **kw)
    assert lib.pnpp_pn_infer_supported(ctypes.byref(d)) == 1, lib.pnpp_last_error()
    nbytes = lib.pnpp_pn_infer_weights_bytes(ctypes.byref(d))
    cins = [D] + ch[:-1]
    assert nbytes >= sum(6 * c * ci + 4 * c for c, ci in zip(ch, cins))
    end = 0
    for l in range(len(ch)):   # the documented view: layers in order, nothing overlaps, everything inside the blob
        woff, ld, boff = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t()
        assert lib.pnpp_pn_infer_weights_layout(ctypes.byref(d), l, ctypes.byref(woff), ctypes.byref(ld), ctypes.byref(boff)) == 0
        assert ld.value >= cins[l] and ld.value % 16 == 0
        assert woff.value >= end and boff.value >= woff.value + 6 * ch[l] * ld.value   # three bf16 planes
        end = boff.value + 4 * ch[l]
    assert end <= nbytes
    woff, ld, boff = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t()
    assert lib.pnpp_pn_infer_weights_layout(ctypes.byref(d), len(ch), ctypes.byref(woff), ctypes.byref(ld), ctypes.byref(boff)) != 0
    for B, N in sizes[1:]:
        d2 = _desc(B, N, **kw)
        assert lib.pnpp_pn_infer_supported(ctypes.byref(d2)) == 1, (B, N)
        assert lib.pnpp_pn_infer_weights_bytes(ctypes.byref(d2)) == nbytes
        # the per-call workspace: one partial row per 32 points and cloud (+ the planes of the feature transform), nothing per point
        sb = lib.pnpp_pn_infer_scratch_bytes(ctypes.byref(d2))
        planes = B * 3 * 64 * 64 * 2 if kw.get("transform_after", -1) >= 0 else 0
        assert 0 < sb <= B * ((N + 31) // 32) * ch[-1] * 4 + 256 + planes
        assert sb < max(B * N, 64) * 128 * 4


def test_refused_descriptors_name_the_reason(lib):
    kw = dict(_trunks(3)["encoder"])
    for channels, msg in (([64, 48, 1024], b"multiple of 32 up to 1024"), ([64, 2048, 1024], b"multiple of 32 up to 1024"),
                          ([64, 64, 64, 128, 1024], b"2 to 4 layers"), ([1024], b"2 to 4 layers")):
        kw["channels"] = channels
        d = _desc(32, 1024, **kw)
        assert lib.pnpp_pn_infer_supported(ctypes.byref(d)) == 0, channels
        assert msg in lib.pnpp_last_error(), (channels, lib.pnpp_last_error())
        assert lib.pnpp_pn_infer_weights_bytes(ctypes.byref(d)) == 0 and lib.pnpp_pn_infer_scratch_bytes(ctypes.byref(d)) == 0
    d = _desc(32, 1024, 3, [128, 128, 1024], input_transform=1, transform_after=0)   # the feature transform is 64 x 64
    assert lib.pnpp_pn_infer_supported(ctypes.byref(d)) == 0 and b"64 x 64" in lib.pnpp_last_error()
    d = _desc(32, 1024, 3, [64, 128, 1024], transform_after=2)                       # behind the pooled layer
    assert lib.pnpp_pn_infer_supported(ctypes.byref(d)) == 0 and b"transform_after=2" in lib.pnpp_last_error()
    d = _desc(32, 1024, 2, [64, 128, 1024], input_transform=1)                       # a 3 x 3 transform of 2 columns
    assert lib.pnpp_pn_infer_supported(ctypes.byref(d)) == 0 and b"D >= 3" in lib.pnpp_last_error()
    for B, N in ((0, 1024), (32, 0), (1 << 20, 1 << 12)):
        d = _desc(B, N, **_trunks(3)["stn"])
        assert lib.pnpp_pn_infer_supported(ctypes.byref(d)) == 0, (B, N)


def test_fixture_is_what_the_tool_describes(golden):
    """tests/golden/pointnet_infer.npz (tools/make_golden_pointnet_infer.py): the seeded initialisation of this package's modules is
    the reference's at the stored positions, the BatchNorm values are bfloat16-representable and in the ranges the tool draws from."""
    from models.pointnet import PointNet, PointNetEncoder
    z = golden("pointnet_infer.npz")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "pointnet_infer.npz")) < 400 * 1024
    for tag in ("ft", "noft", "enc6"):
        torch.manual_seed(int(z[f"{tag}.seed"]))
        m = PointNetEncoder(False, True, 6) if tag == "enc6" else PointNet(tag == "ft")
        ws = []
        for i, (n, p) in enumerate(m.named_parameters()):
            if p.dim() > 1:
                g = torch.Generator().manual_seed(i)
                ws.append(p.detach().flatten()[torch.randint(0, p.numel(), (min(8, p.numel()),), generator=g)])
        assert np.array_equal(torch.cat(ws).numpy(), z[f"{tag}.ws"]), f"{tag}: the seeded initialisation has drifted from the reference's"
        nbn = sum(4 * b.num_features for b in m.modules() if isinstance(b, torch.nn.BatchNorm1d))
        bits = z["ft.bn" if tag == "enc6" else f"{tag}.bn"]
        assert bits.dtype == np.uint16 and bits.size >= nbn and (tag == "enc6" or bits.size == nbn)
    bn = torch.from_numpy(z["ft.bn"].view(np.int16).copy()).view(torch.bfloat16).float()
    assert torch.isfinite(bn).all()
    rv = bn[3 * 64:4 * 64]   # stn.bn1: [weight, bias, running_mean, running_var] of 64 channels
    assert float(rv.min()) >= 0.049 and float(rv.max()) <= 2.01
    assert z["ft.x"].shape == (8, 300, 3) and z["noft.x"].shape == (8, 300, 3) and z["enc6.x"].shape[1:] == (6, 300)
    assert z["ft.trans_feat"].dtype == np.float32 and z["ft.global"].shape == (8, 1024) and "noft.trans_feat" not in z.files
