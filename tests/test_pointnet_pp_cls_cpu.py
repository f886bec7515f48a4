"""CPU-side checks of the PointNet++ classifier port (models/pointnet_pp_cls.py): the drop-in surface against the reference's
recorded state_dict layout, the widened answer of pnpp_sa_infer_supported, argument validation of the new loss entries (it happens
before any launch, so it runs without a GPU) and the refusal to run off-GPU."""
import ctypes

import pytest
import torch


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


def _sa2(K, B=8):
    return _desc(B, 512, 128, K, 128, [128, 128, 256])


def _sa3(N, B=8):
    return _desc(B, N, 1, N, 256, [256, 512, 1024], group_all=True)


def test_state_dict_matches_the_reference(golden):
    from models import PointNetPlusPlusCls
    g = golden("pointnet_pp_cls.npz")
    m = PointNetPlusPlusCls()
    sd = m.state_dict()
    assert list(sd.keys()) == [str(n) for n in g["cls.sd.names"]]
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in g["cls.sd.shapes"]]
    assert sum(p.numel() for p in m.parameters()) == int(g["cls.n_params"])
    assert tuple(sd["sa1.mlp_convs.0.weight"].shape) == (64, 6, 1, 1)
    for k in ("sa2.mlp_bns.1.running_var", "fc3.weight", "bn1.num_batches_tracked"):
        assert k in sd
    # the reference's defaults, and the keyword override the tests use to run small
    assert (m.sa1.npoint, m.sa1.radius, m.sa1.nsample, m.sa2.npoint, m.sa2.radius, m.sa2.nsample) == (512, 0.2, 32, 128, 0.4, 64)
    small = PointNetPlusPlusCls(num_classes=5, sa1=(16, 0.3, 8), sa2=(4, 0.6, 8))
    assert small.sa2.nsample == 8 and small.fc3.weight.shape == (5, 256)
    assert list(small.state_dict().keys()) == list(sd.keys())


@pytest.mark.parametrize("K", [64, 96, 128, 256])
def test_wide_neighbourhoods_are_taken(lib, K):
    nbytes = {}
    for what, mk in (("plain", _sa2), ("group_all", _sa3)):
        d = mk(K)
        assert lib.pnpp_sa_infer_supported(ctypes.byref(d)) == 1, (what, lib.pnpp_last_error())
        nbytes[what] = lib.pnpp_sa_infer_weights_bytes(ctypes.byref(d))
        assert nbytes[what] == lib.pnpp_sa_infer_weights_bytes(ctypes.byref(mk(32))), "the blob depends on D and the channels only"
        assert nbytes[what] == lib.pnpp_sa_infer_weights_bytes(ctypes.byref(mk(K, B=300)))
    assert nbytes["plain"] > 0 and nbytes["group_all"] > 0


@pytest.mark.parametrize("K", [24, 48, 1024])
def test_other_neighbourhoods_are_refused(lib, K):
    for mk in (_sa2, _sa3):
        d = mk(K)
        assert lib.pnpp_sa_infer_supported(ctypes.byref(d)) == 0
        assert f"K={K}".encode() in lib.pnpp_last_error()
        assert lib.pnpp_sa_infer_weights_bytes(ctypes.byref(d)) == 0


def test_loss_entries_argument_errors(lib):
    from pnpp_hip import _lib
    E = _lib.PNPP_ERR_ARG
    p = 256   # any non-null pointer: validation comes before the launch
    assert lib.pnpp_log_softmax(None, 4, 40, p, None) == E and b"null" in lib.pnpp_last_error()
    assert lib.pnpp_log_softmax(p, 4, 40, None, None) == E
    assert lib.pnpp_log_softmax(p, 0, 40, p, None) == E and b"M=0" in lib.pnpp_last_error()
    assert lib.pnpp_log_softmax(p, 4, -1, p, None) == E
    assert lib.pnpp_log_softmax_bwd(p, None, 4, 40, p, None) == E and b"null" in lib.pnpp_last_error()
    assert lib.pnpp_log_softmax_bwd(p, p, 4, 0, p, None) == E
    assert lib.pnpp_nll_loss(p, None, 4, 40, p, p, 1, None) == E and b"null" in lib.pnpp_last_error()
    assert lib.pnpp_nll_loss(p, p, 4, 40, p, None, 0, None) == E   # the out-of-range count is always written
    assert lib.pnpp_nll_loss(p, p, 0, 40, p, p, 1, None) == E
    assert lib.pnpp_nll_loss_bwd(None, p, 4, 40, p, None) == E and b"null" in lib.pnpp_last_error()
    assert lib.pnpp_nll_loss_bwd(p, p, 4, 0, p, None) == E
    assert lib.pnpp_linear_log_softmax(p, p, None, 4, 256, 40, p, None) == E
    assert lib.pnpp_linear_log_softmax(p, p, p, 4, 256, 2000, p, None) == E and b"C=2000" in lib.pnpp_last_error()


def test_no_cpu_fallback():
    from pnpp_hip import ops
    from pnpp_hip.inference import Predictor
    from models import PointNetPlusPlusCls, get_loss
    m = PointNetPlusPlusCls(num_classes=5, sa1=(16, 0.3, 8), sa2=(4, 0.6, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.rand(2, 6, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.log_softmax(torch.randn(3, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nll_loss(torch.randn(3, 5), torch.zeros(3, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        get_loss()(torch.randn(3, 5), torch.zeros(3, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Predictor(m)
