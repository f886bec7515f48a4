"""Ragged batches of the PointNet++ models, the part that needs no GPU: the nine `*_ragged` entry points are declared, bound and
exported and refuse bad arguments before any launch (a null `lengths` first, then their uniform twins' cases); the lengths helpers
both model families share validate host values, with the minimum a model's first level needs."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 4096      # a non-null "device pointer": every call below is refused before anything could read it

NAMES = ["pnpp_knn_ragged", "pnpp_fps_ragged", "pnpp_ball_query_ragged", "pnpp_sample_random_ragged", "pnpp_sample_random_dev_ragged",
         "pnpp_sample_random_dev2_ragged", "pnpp_knn_pair_ragged", "pnpp_sa_group_pair_ragged", "pnpp_sa_infer_group_pair_ragged"]


@pytest.fixture(scope="module")
def lib():
    from pnpp_hip import build, _lib
    build.build()
    return _lib.lib()


def _descs(N=64, S1=16, K1=8, S2=8, K2=4, N2=None):
    from pnpp_hip import _lib
    d1, d2 = _lib.SaDesc(), _lib.SaDesc()
    d1.B, d1.N, d1.S, d1.K, d1.D, d1.L = 2, N, S1, K1, 0, 3
    d2.B, d2.N, d2.S, d2.K, d2.D, d2.L = 2, S1 if N2 is None else N2, S2, K2, 128, 3
    d1.C[0], d1.C[1], d1.C[2] = 64, 64, 128
    d2.C[0], d2.C[1], d2.C[2] = 128, 128, 256
    d1.eps = d2.eps = 1e-5
    d1.momentum = d2.momentum = 0.1
    return d1, d2


def _calls(lib, lengths, B=2, N=64, k=8, npoint=16, ptr=PTR, d=None):
    """the nine ragged entry points at small legal sizes; `lengths` is the argument under test"""
    d1, d2 = d if d is not None else _descs(N=N)
    r1, r2 = ctypes.byref(d1), ctypes.byref(d2)
    return {
        "knn_ragged": lambda: lib.pnpp_knn_ragged(ptr, ptr, B, 4, N, lengths, k, ptr, None),
        "fps_ragged": lambda: lib.pnpp_fps_ragged(ptr, B, N, lengths, npoint, ptr, ptr, None),
        "ball_query_ragged": lambda: lib.pnpp_ball_query_ragged(ptr, ptr, B, 4, N, lengths, 0.2, k, ptr, None),
        "sample_random_ragged": lambda: lib.pnpp_sample_random_ragged(1, 2, B, N, lengths, npoint, ptr, None),
        "sample_random_dev_ragged": lambda: lib.pnpp_sample_random_dev_ragged(1, ptr, 2, B, N, lengths, npoint, ptr, None),
        "sample_random_dev2_ragged": lambda: lib.pnpp_sample_random_dev2_ragged(1, ptr, 2, B, N, lengths, npoint, ptr, npoint, 8, ptr, None),
        "knn_pair_ragged": lambda: lib.pnpp_knn_pair_ragged(ptr, B, N, lengths, ptr, npoint, k, ptr, ptr, ptr, 8, 4, ptr, ptr, None, None),
        "sa_group_pair_ragged": lambda: lib.pnpp_sa_group_pair_ragged(r1, r2, ptr, lengths, ptr, ptr, ptr, ptr, ptr, ptr, None),
        "sa_infer_group_pair_ragged": lambda: lib.pnpp_sa_infer_group_pair_ragged(r1, r2, ptr, lengths, ptr, ptr, ptr, ptr, ptr, ptr, None),
    }


def test_symbols_declared_bound_and_exported(lib):
    from pnpp_hip import _lib
    text = open(os.path.join(ROOT, "include", "pnpp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pnpp_[a-z0-9_]+)\s*\(", text))
    for n in NAMES:
        assert n in declared, f"{n} is not declared in include/pnpp_hip.h"
        assert n in _lib.SIGNATURES, f"{n} is not bound in _lib.SIGNATURES"
        assert hasattr(lib, n), f"{n} is not exported"
        twin = n[:-len("_ragged")]
        assert len(_lib.SIGNATURES[n][1]) == len(_lib.SIGNATURES[twin][1]) + 1, f"{n} is its twin plus the lengths pointer"
    assert lib.pnpp_abi_version() == 5


def test_null_lengths_is_refused(lib):
    from pnpp_hip import _lib
    calls = _calls(lib, None)
    assert len(calls) == 9
    for name, call in calls.items():
        assert call() == _lib.PNPP_ERR_ARG, name
        msg = lib.pnpp_last_error().decode()
        assert "null lengths" in msg and name in msg, (name, msg)


def test_the_twins_argument_checks_hold_before_any_launch(lib):
    from pnpp_hip import _lib
    ARG, RANGE = _lib.PNPP_ERR_ARG, _lib.PNPP_ERR_RANGE
    for name, call in _calls(lib, PTR, ptr=None).items():                    # null data pointers
        assert call() == ARG, name
        assert "null" in lib.pnpp_last_error().decode(), name
    flat = {k: v for k, v in _calls(lib, PTR, B=0).items() if "sa_" not in k}  # non-positive size (the descriptor calls carry B inside)
    for name, call in flat.items():
        assert call() == ARG, name
        assert "non-positive" in lib.pnpp_last_error().decode(), name
    # k > N, like torch.topk; more centres than points
    big = _calls(lib, PTR, N=6, k=8, npoint=4, d=_descs(N=6, S1=4, K1=8, S2=2, K2=2))
    for name in ("knn_ragged", "sa_group_pair_ragged", "sa_infer_group_pair_ragged"):
        assert big[name]() == RANGE, name
    assert lib.pnpp_knn_pair_ragged(PTR, 2, 6, PTR, PTR, 4, 8, PTR, PTR, PTR, 2, 2, PTR, PTR, None, None) == RANGE
    many = _calls(lib, PTR, N=8, k=4, npoint=16)
    for name in ("sample_random_ragged", "sample_random_dev_ragged", "sample_random_dev2_ragged"):
        assert many[name]() == RANGE, name
    assert lib.pnpp_knn_ragged(PTR, PTR, 1, 4, 500, PTR, 200, PTR, None) == ARG      # nsample over the kernel maximum
    assert lib.pnpp_sample_random_dev_ragged(1, None, 2, 2, 64, PTR, 16, PTR, None) == ARG and b"counter" in lib.pnpp_last_error()
    assert lib.pnpp_sample_random_ragged(1, 2, 2, 1 << 20, PTR, 16, PTR, None) == ARG and b"too large" in lib.pnpp_last_error()
    assert lib.pnpp_fps_ragged(PTR, 2, 1 << 20, PTR, 16, PTR, PTR, None) == ARG and b"exceeds" in lib.pnpp_last_error()
    d1, d2 = _descs(N2=17)                                                     # level 2 must take level 1's centres
    for fn in (lib.pnpp_sa_group_pair_ragged, lib.pnpp_sa_infer_group_pair_ragged):
        assert fn(ctypes.byref(d1), ctypes.byref(d2), PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, None) == ARG
        assert b"level 1's" in lib.pnpp_last_error()


def test_shared_lengths_helper_with_a_minimum():
    from pnpp_hip.lengths import check_lengths, ragged_lengths
    from pnpp_hip import transformer
    assert transformer.check_lengths is check_lengths and transformer.ragged_lengths is ragged_lengths   # the old names still import
    ok = check_lengths([128, 300, 200], 3, 300, minimum=128)
    assert ok.dtype == torch.int32 and ok.tolist() == [128, 300, 200] and not ok.is_cuda
    assert check_lengths(torch.tensor([7, 8], dtype=torch.int64), 2, 8).dtype == torch.int32           # minimum defaults to 1
    with pytest.raises(ValueError, match="integer dtype"):
        check_lengths(torch.tensor([128.0, 200.0]), 2, 300, minimum=128)
    with pytest.raises(ValueError, match=r"shape \(3,\)"):
        check_lengths([128, 200], 3, 300, minimum=128)
    with pytest.raises(ValueError, match=r"shape \(2,\)"):
        check_lengths(torch.full((2, 1), 200, dtype=torch.int32), 2, 300, minimum=128)
    with pytest.raises(ValueError, match=r"lengths\[2\] = 301: cloud 2"):
        check_lengths([128, 300, 301], 3, 300, minimum=128)
    with pytest.raises(ValueError, match=r"lengths\[1\] = 127: cloud 1 must hold between 128 and n_pts = 300"):
        check_lengths([128, 127, 300], 3, 300, minimum=128)
    with pytest.raises(ValueError, match=r"lengths\[0\] = 0: cloud 0 must hold between 1 and"):
        check_lengths([0, 5], 2, 10)
    up = ragged_lengths([40, 64], 2, 64, "cpu", minimum=32)                    # host values: validated, then moved to the device
    assert up.dtype == torch.int32 and up.tolist() == [40, 64]
    with pytest.raises(ValueError, match=r"lengths\[0\] = 31"):
        ragged_lengths([31, 64], 2, 64, "cpu", minimum=32)


def test_minimum_length_of_a_models_first_level():
    from pnpp_hip.lengths import sa_minimum_length
    from models.pointnet_pp_8dir import PointNetSetAbstraction
    from models.pointnet_pp_cls import PointNetPlusPlusCls
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    assert sa_minimum_length("randperm", "knn", 128, 32) == 128 and sa_minimum_length("device", "knn", 16, 32) == 32
    assert sa_minimum_length("fps", "knn", 128, 32) == 32
    assert sa_minimum_length("fps", ("ball", 0.2), 512, 32) == 1 and sa_minimum_length("fps", "ball:0.2", 512, 32) == 1
    assert PointNetPPVonMises(sampler="device").sa1.min_length() == 128
    assert PointNetSetAbstraction(64, 32, 0, [32, 32, 64], sampler="fps", grouper="knn").min_length() == 32
    cls = PointNetPlusPlusCls()
    assert sa_minimum_length(cls.sa1.sampler, cls.sa1.grouper, cls.sa1.npoint, cls.sa1.nsample) == 1


def test_models_with_lengths_have_no_cpu_fallback_and_refuse_the_ring():
    from models.pointnet_pp_mvM import PointNetPPMvM
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    with pytest.raises(ValueError, match=r"lengths\[1\] = 100: cloud 1 must hold between 128"):
        PointNetPPVonMises()(torch.rand(2, 200, 3), lengths=[200, 100])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PointNetPPVonMises()(torch.rand(2, 200, 3), lengths=[200, 150])
    for m in (PointNetPPVonMises(), PointNetPPMvM()):
        m.use_presampled(object())
        with pytest.raises(ValueError, match="use_presampled"):
            m(torch.rand(2, 200, 3), lengths=[200, 150])
