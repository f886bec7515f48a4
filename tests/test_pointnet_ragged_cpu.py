"""Ragged batches of the vanilla PointNet, the part that needs no GPU: the nine `*_ragged` entry points are declared, bound and
exported and refuse bad arguments before any launch; the packed-offsets helper is right for hand-written cases and rejects bad
lengths; the models, the operators and the Predictor take `lengths`; pn_trunk refuses a batch of at most 32 valid points."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 4096      # a non-null "device pointer": every call below is refused before anything could read it

NAMES = ["pnpp_pn_pool_saved_bytes_ragged", "pnpp_pn_pool_scratch_bytes_ragged", "pnpp_pn_pool_forward_ragged",
         "pnpp_pn_pool_backward_ragged", "pnpp_pn_transform_ragged", "pnpp_pn_transform_bwd_ragged", "pnpp_pn_concat_ragged",
         "pnpp_pn_concat_bwd_ragged", "pnpp_pn_infer_ragged"]
HELPERS = ["pnpp_pn_offsets"]


@pytest.fixture(scope="module")
def lib():
    from pnpp_hip import build, _lib
    build.build()
    return _lib.lib()


def _pool_desc(B=2, N=64, K=128, C=128, training=1):
    from pnpp_hip import _lib
    d = _lib.PnPoolDesc()
    d.B, d.N, d.K, d.C, d.relu, d.training, d.eps, d.momentum = B, N, K, C, 1, training, 1e-5, 0.1
    return d


def test_symbols_declared_bound_and_exported(lib):
    from pnpp_hip import _lib
    text = open(os.path.join(ROOT, "include", "pnpp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pnpp_[a-z0-9_]+)\s*\(", text))
    for n in NAMES:
        assert n in declared, f"{n} is not declared in include/pnpp_hip.h"
        assert n in _lib.SIGNATURES, f"{n} is not bound in _lib.SIGNATURES"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n[:-len("_ragged")] in _lib.SIGNATURES, f"{n} has no uniform twin"
    for n in HELPERS:
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert lib.pnpp_pn_offsets(None, 2, 64, PTR, PTR, None) == _lib.PNPP_ERR_ARG and b"null pointer" in lib.pnpp_last_error()
    assert lib.pnpp_pn_offsets(PTR, 0, 64, PTR, PTR, None) == _lib.PNPP_ERR_ARG and b"B=0" in lib.pnpp_last_error()
    assert lib.pnpp_abi_version() == 5


def test_pool_entry_points_check_offsets_and_row_count(lib):
    from pnpp_hip import _lib
    ARG = _lib.PNPP_ERR_ARG
    d = _pool_desc()
    fa, ba = _lib.PnPoolFwdArgs(), _lib.PnPoolBwdArgs()
    for f in ("a", "w", "b", "gamma", "beta", "rm", "rv", "out", "saved", "scratch"):
        setattr(fa, f, PTR)
    for f in ("a", "w", "gamma", "dout", "saved", "scratch", "da", "dw", "db", "dgamma", "dbeta"):
        setattr(ba, f, PTR)
    r = ctypes.byref(d)
    assert lib.pnpp_pn_pool_forward_ragged(r, ctypes.byref(fa), None, 100, None) == ARG and b"null offsets" in lib.pnpp_last_error()
    assert lib.pnpp_pn_pool_backward_ragged(r, ctypes.byref(ba), None, 100, None) == ARG and b"null offsets" in lib.pnpp_last_error()
    # the packed row count: at least one row per cloud, at most the padded B * N, more than one when training
    assert lib.pnpp_pn_pool_forward_ragged(r, ctypes.byref(fa), PTR, 1, None) == ARG and b"M_total=1" in lib.pnpp_last_error()
    assert lib.pnpp_pn_pool_forward_ragged(r, ctypes.byref(fa), PTR, 129, None) == ARG and b"M_total=129" in lib.pnpp_last_error()
    assert lib.pnpp_pn_pool_saved_bytes_ragged(r, 0) == 0 and lib.pnpp_pn_pool_scratch_bytes_ragged(r, 129) == 0
    one = _pool_desc(B=1, N=8)
    assert lib.pnpp_pn_pool_saved_bytes_ragged(ctypes.byref(one), 1) == 0 and b"more than 1 value" in lib.pnpp_last_error()
    one.training = 0
    assert lib.pnpp_pn_pool_saved_bytes_ragged(ctypes.byref(one), 1) > 0
    # the workspaces have the uniform call's layout
    assert lib.pnpp_pn_pool_saved_bytes_ragged(r, 77) == lib.pnpp_pn_pool_saved_bytes(r) > 0
    assert lib.pnpp_pn_pool_scratch_bytes_ragged(r, 77) == lib.pnpp_pn_pool_scratch_bytes(r) > 0
    # the existing limits on K, C and B
    for bad in (_pool_desc(K=130), _pool_desc(C=96), _pool_desc(B=70000, N=1)):
        assert lib.pnpp_pn_pool_saved_bytes_ragged(ctypes.byref(bad), bad.B) == 0
        assert lib.pnpp_pn_pool_forward_ragged(ctypes.byref(bad), ctypes.byref(fa), PTR, bad.B, None) == ARG


def test_transform_concat_and_infer_refuse_null_offsets(lib):
    from pnpp_hip import _lib
    ARG = _lib.PNPP_ERR_ARG
    assert lib.pnpp_pn_transform_ragged(PTR, 0, 192, 3, 1, None, None, 2, 64, 3, 0, 4, PTR, None) == ARG
    assert b"null offsets" in lib.pnpp_last_error()
    assert lib.pnpp_pn_transform_bwd_ragged(PTR, 0, 192, 3, 1, None, PTR, None, 2, 64, 3, 0, 4, PTR, None, None) == ARG
    assert b"null offsets" in lib.pnpp_last_error()
    assert lib.pnpp_pn_concat_ragged(PTR, PTR, 0, None, 2, 64, 1024, 64, PTR, None) == ARG and b"null offsets" in lib.pnpp_last_error()
    assert lib.pnpp_pn_concat_bwd_ragged(PTR, None, 2, 64, 1024, 64, PTR, PTR, None) == ARG and b"null offsets" in lib.pnpp_last_error()
    # the twins' checks hold too
    assert lib.pnpp_pn_transform_ragged(PTR, 0, 192, 3, 1, None, PTR, 2, 64, 65, 0, 68, PTR, None) == ARG
    assert b"width D=65" in lib.pnpp_last_error()
    assert lib.pnpp_pn_concat_ragged(PTR, PTR, 0, PTR, 0, 64, 1024, 64, PTR, None) == ARG and b"non-positive" in lib.pnpp_last_error()
    d = _lib.PnInferDesc()
    d.B, d.N, d.D, d.L = 2, 64, 3, 3
    d.C[0], d.C[1], d.C[2] = 64, 128, 1024
    d.input_transform, d.transform_after, d.relu_last, d.eps = 0, -1, 1, 1e-5
    a = _lib.PnInferArgs()
    a.x, a.weights, a.scratch, a.out = PTR, PTR, PTR, PTR
    assert lib.pnpp_pn_infer_ragged(ctypes.byref(d), ctypes.byref(a), None, None) == ARG and b"null offsets" in lib.pnpp_last_error()


def test_packed_offsets_by_hand():
    from pnpp_hip.lengths import PackedLengths, packed_lengths, packed_offsets
    assert packed_offsets([320, 1, 63, 64, 257]) == [0, 320, 321, 384, 448, 705]
    assert packed_offsets([1]) == [0, 1]
    assert packed_offsets(torch.tensor([4, 4, 4])) == [0, 4, 8, 12]            # lengths == N: the uniform rows b * N
    pk = packed_lengths([320, 1, 63, 64, 257], 5, 320, "cpu")
    assert isinstance(pk, PackedLengths) and pk.M_total == 705
    assert pk.lens_dev.dtype == torch.int32 and pk.lens_dev.tolist() == [320, 1, 63, 64, 257]
    assert pk.offs_dev.dtype == torch.int32 and pk.offs_dev.tolist() == [0, 320, 321, 384, 448, 705]
    assert packed_lengths(pk, 5, 320, "cpu") is pk                              # built once per forward, passed through
    pk = packed_lengths(torch.tensor([2, 7], dtype=torch.int64), 2, 7, "cpu")
    assert pk.offs_dev.tolist() == [0, 2, 9] and pk.M_total == 9
    with pytest.raises(ValueError, match="packed for 2 clouds"):
        packed_lengths(pk, 3, 7, "cpu")


def test_bad_lengths_are_rejected_naming_the_cloud():
    from pnpp_hip.lengths import packed_lengths
    with pytest.raises(ValueError, match=r"lengths\[1\] = 0: cloud 1 must hold between 1 and n_pts = 64"):
        packed_lengths([64, 0, 3], 3, 64, "cpu")
    with pytest.raises(ValueError, match=r"lengths\[2\] = 65: cloud 2 must hold between 1 and n_pts = 64"):
        packed_lengths([64, 1, 65], 3, 64, "cpu")
    with pytest.raises(ValueError, match=r"shape \(3,\), one entry per cloud"):
        packed_lengths([64, 1], 3, 64, "cpu")
    with pytest.raises(ValueError, match=r"shape \(3,\), one entry per cloud"):
        packed_lengths(torch.ones(3, 1, dtype=torch.int32), 3, 64, "cpu")
    with pytest.raises(ValueError, match="integer dtype"):
        packed_lengths(torch.tensor([64.0, 1.0, 3.0]), 3, 64, "cpu")


def test_signatures_take_lengths():
    from models.pointnet import PointNet, PointNetEncoder, STN3d, STNkd
    from pnpp_hip import ops
    from pnpp_hip.pointnet_inference import PointNetPredictor
    for cls in (STN3d, STNkd, PointNetEncoder, PointNet):
        p = inspect.signature(cls.forward).parameters
        assert "lengths" in p and p["lengths"].default is None, cls.__name__
    assert list(inspect.signature(PointNet.forward).parameters) == ["self", "x", "drop_mask", "return_transforms", "lengths"]
    assert list(inspect.signature(PointNetPredictor.__call__).parameters) == ["self", "x", "return_transforms", "lengths"]
    for fn in (ops.pn_transform, ops.pn_pool, ops.pn_trunk, ops.pn_concat):
        p = inspect.signature(fn).parameters
        assert "lengths" in p and p["lengths"].default is None, fn.__name__


def test_trunk_refuses_at_most_32_valid_rows_and_bad_lengths_before_the_gpu():
    import torch.nn as nn
    from models.pointnet import PointNet
    from pnpp_hip import ops
    conv, bn = nn.Conv1d(128, 1024, 1), nn.BatchNorm1d(1024)
    with pytest.raises(ValueError, match=r"lengths of the 4 clouds sum to 32 point rows; the per-point layers need more than 32"):
        ops.pn_trunk(torch.zeros(32, 128), 4, 100, [], (conv, bn), True, True, lengths=[10, 10, 10, 2])
    with pytest.raises(ValueError, match=r"lengths\[3\] = 101: cloud 3"):
        ops.pn_trunk(torch.zeros(131, 128), 4, 100, [], (conv, bn), True, True, lengths=[10, 10, 10, 101])
    m = PointNet(True)
    with pytest.raises(ValueError, match=r"lengths\[1\] = 0: cloud 1"):
        m(torch.rand(2, 3, 50), lengths=[50, 0])
    with pytest.raises(ValueError, match=r"lengths\[0\] = 51: cloud 0"):
        m.encoder.stn(torch.rand(2, 3, 50), lengths=[51, 2])
    with pytest.raises(RuntimeError, match="GPU|cuda|CPU fallback"):              # valid lengths: on to the kernels, which need a GPU
        m(torch.rand(2, 3, 50), lengths=[50, 20])
