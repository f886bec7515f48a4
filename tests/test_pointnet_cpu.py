"""CPU-side checks of the vanilla PointNet drop-in (models/pointnet.py): the reference's parameter counts and state_dict
contract, the package exports, no CPU fallback, the ctypes mirrors of the new C structs and argument validation of the new
entry points before any launch."""
import ctypes
import os

import pytest
import torch

from conftest import ROOT


def _n(m):
    return sum(p.numel() for p in m.parameters())


def test_parameter_counts_match_reference():
    from models.pointnet import PointNet, PointNetEncoder, STN3d, STNkd
    assert _n(PointNet()) == 3461964
    assert _n(PointNet(False)) == 1604620
    assert _n(STN3d(3)) == 803081
    assert _n(STN3d(6)) == 803273
    assert _n(STNkd()) == 1857344
    assert _n(PointNetEncoder(True, True, 6)) == 2803913
    sd = PointNet().state_dict()
    assert len(sd) == 111
    assert tuple(sd["encoder.fstn.fc3.weight"].shape) == (4096, 256)
    assert tuple(sd["encoder.conv3.weight"].shape) == (1024, 128, 1)
    assert "encoder.fstn.bn3.num_batches_tracked" in sd
    assert "encoder.fstn.conv1.weight" not in PointNet(False).state_dict()


def test_seeded_initialisation_is_reproducible():
    from models.pointnet import PointNet
    torch.manual_seed(4)
    a = PointNet().state_dict()
    torch.manual_seed(4)
    b = PointNet().state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_package_exports():
    from models import PointNet, PointTransformer
    import models
    assert "PointNet" in models.__all__ and "PointTransformer" in models.__all__
    assert PointNet.__module__ == "models.pointnet" and PointTransformer.__module__ == "models.point_transformer"


def test_no_cpu_fallback():
    from models.pointnet import PointNet, PointNetEncoder, STN3d
    from pnpp_hip import ops
    for call in (lambda: PointNet()(torch.randn(2, 16, 3)), lambda: PointNetEncoder()(torch.randn(2, 3, 16)),
                 lambda: STN3d(3)(torch.randn(2, 3, 16)), lambda: ops.feature_transform_regularizer(torch.eye(3).expand(2, 3, 3))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_struct_layouts_match_c():
    import subprocess, tempfile, textwrap
    from pnpp_hip import _lib
    src = textwrap.dedent('''
        #include <stdio.h>
        #include "pnpp_hip.h"
        int main(void) { printf("%zu %zu %zu\\n", sizeof(pnpp_pn_pool_desc), sizeof(pnpp_pn_pool_fwd_args),
            sizeof(pnpp_pn_pool_bwd_args)); return 0; }
    ''')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        sizes = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [ctypes.sizeof(t) for t in (_lib.PnPoolDesc, _lib.PnPoolFwdArgs, _lib.PnPoolBwdArgs)]


@pytest.fixture(scope="module")
def lib():
    from pnpp_hip import _lib, build
    build.build()
    return _lib.lib()


def _desc(B=2, N=16, K=128, C=1024, relu=1, training=1):
    from pnpp_hip import _lib
    d = _lib.PnPoolDesc()
    d.B, d.N, d.K, d.C, d.relu, d.training, d.eps, d.momentum = B, N, K, C, relu, training, 1e-5, 0.1
    return d


def test_pool_descriptor_validation(lib):
    from pnpp_hip import _lib
    ok = _desc()
    assert lib.pnpp_pn_pool_saved_bytes(ctypes.byref(ok)) > 0
    assert lib.pnpp_pn_pool_scratch_bytes(ctypes.byref(ok)) > 0
    # far smaller than the (B*N) x C activation it replaces at the full size
    big = _desc(B=32, N=1024)
    assert lib.pnpp_pn_pool_saved_bytes(ctypes.byref(big)) < 32 * 1024 * 1024 * 4 // 100
    for bad, word in ((_desc(K=130), b"K=130"), (_desc(K=6), b"K=6"), (_desc(C=100), b"C=100"), (_desc(C=2048), b"C=2048"),
                      (_desc(B=0), b"B=0"), (_desc(relu=2), b"relu"), (_desc(B=1, N=1), b"more than 1 value")):
        assert lib.pnpp_pn_pool_saved_bytes(ctypes.byref(bad)) == 0
        assert word in lib.pnpp_last_error()
        assert lib.pnpp_pn_pool_forward(ctypes.byref(bad), ctypes.byref(_lib.PnPoolFwdArgs()), None) == _lib.PNPP_ERR_ARG
    assert _desc(B=1, N=1, training=0) and lib.pnpp_pn_pool_saved_bytes(ctypes.byref(_desc(B=1, N=1, training=0))) > 0
    assert lib.pnpp_pn_pool_forward(ctypes.byref(ok), ctypes.byref(_lib.PnPoolFwdArgs()), None) == _lib.PNPP_ERR_ARG
    assert b"null" in lib.pnpp_last_error()
    assert lib.pnpp_pn_pool_backward(ctypes.byref(ok), ctypes.byref(_lib.PnPoolBwdArgs()), None) == _lib.PNPP_ERR_ARG
    assert lib.pnpp_pn_pool_saved_route(ctypes.byref(ok), None) is None


def test_other_entry_points_reject_bad_arguments(lib):
    from pnpp_hip import _lib
    E = _lib.PNPP_ERR_ARG
    p = 64   # never dereferenced: every call below fails validation first
    assert lib.pnpp_pn_transform(None, 0, 0, 0, None, 1, 1, 3, 3, 4, p, None) == E
    assert lib.pnpp_pn_transform(p, 0, 0, 0, p, 1, 1, 65, 3, 68, p, None) == E and b"D=65" in lib.pnpp_last_error()
    assert lib.pnpp_pn_transform(p, 0, 0, 0, p, 1, 1, 3, 4, 4, p, None) == E and b"k=4" in lib.pnpp_last_error()
    assert lib.pnpp_pn_transform(p, 0, 0, 0, p, 1, 1, 6, 3, 4, p, None) == E
    assert lib.pnpp_pn_transform(p, 0, 0, 0, p, 0, 1, 3, 3, 4, p, None) == E
    assert lib.pnpp_pn_transform_bwd(p, 0, 0, 0, None, p, 1, 1, 3, 3, 4, p, p, None) == E
    assert lib.pnpp_pn_regularizer(p, 2, 65, p, p, None) == E
    assert lib.pnpp_pn_regularizer(None, 2, 3, p, p, None) == E
    assert lib.pnpp_pn_regularizer_bwd(p, p, p, 0, 3, p, None) == E
    assert lib.pnpp_pn_add_identity(p, 0, 3, p, None) == E
    assert lib.pnpp_pn_concat(p, p, 2, 0, 1024, 64, p, None) == E
    assert lib.pnpp_pn_concat_bwd(None, 2, 4, 1024, 64, p, p, None) == E
    assert lib.pnpp_pn_bn_relu(p, 1, 8, p, p, p, p, None, 1, 1e-5, 0.1, p, p, p, None) == E
    assert b"more than 1 value" in lib.pnpp_last_error()
    assert lib.pnpp_pn_bn_relu_bwd(p, p, p, 0, 8, p, p, p, 1, p, p, p, None) == E


@pytest.mark.parametrize("tag", ["ft", "noft", "enc6"])
def test_seeded_initialisation_matches_reference_capture(golden, tag):
    """torch.manual_seed(s) gives the reference's weights (tests/golden/pointnet.npz holds samples of the reference's own
    initialisation, tools/make_golden_pointnet.py)."""
    import numpy as np
    from models.pointnet import PointNet, PointNetEncoder
    g = golden("pointnet.npz")
    torch.manual_seed(int(g[f"{tag}.seed"]))
    m = PointNetEncoder(global_feat=False, feature_transform=True, channel=6) if tag == "enc6" else PointNet(tag == "ft")
    for n, p in m.named_parameters():
        got = p.detach().flatten()[torch.from_numpy(g[f"{tag}.gp.{n}"])].double().numpy()
        assert np.array_equal(got, g[f"{tag}.init.{n}"]), n


def test_channel_count_mismatch_is_refused():
    """Extra input columns are not silently dropped: PointNet() (3 channels) refuses (B, N, 6) like the reference's Conv1d."""
    from models.pointnet import PointNet, PointNetEncoder, STN3d
    with pytest.raises(ValueError, match="3 channels, got 6"):
        PointNet()(torch.randn(2, 16, 6))
    with pytest.raises(ValueError, match="6 channels, got 3"):
        PointNetEncoder(channel=6)(torch.randn(2, 3, 16))
    with pytest.raises(ValueError, match="3 channels, got 4"):
        STN3d(3)(torch.randn(2, 4, 16))


def test_recompute_and_bounds_validation(lib):
    from pnpp_hip import _lib
    E = _lib.PNPP_ERR_ARG
    d = _lib.FcDesc()
    d.M, d.K, d.N, d.norm, d.relu, d.training, d.eps, d.momentum, d.drop_scale = 32, 64, 64, _lib.NORM_BATCH, 1, 1, 1e-5, 0.1, 1.0
    assert lib.pnpp_fc_recompute_output(ctypes.byref(d), 64, None, 64, None) == E          # 32 rows: the epilogue form keeps no z
    d.M, d.norm = 4096, _lib.NORM_NONE
    assert lib.pnpp_fc_recompute_output(ctypes.byref(d), 64, None, 64, None) == E
    d.norm = _lib.NORM_BATCH
    assert lib.pnpp_fc_recompute_output(ctypes.byref(d), None, None, 64, None) == E
    assert lib.pnpp_pn_pool_saved_bytes(ctypes.byref(_desc(B=70000, N=2))) == 0 and b"65535" in lib.pnpp_last_error()
    assert lib.pnpp_pn_transform(64, 0, 0, 0, None, 70000, 2, 3, 3, 4, 64, None) == E and b"65535" in lib.pnpp_last_error()
    assert lib.pnpp_pn_pool_saved_ypre(ctypes.byref(_desc()), None) is None
