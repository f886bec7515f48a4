"""Ragged batches of the point transformer, the part that needs no GPU: the new entry points refuse bad arguments before any launch,
the lengths are validated on the host by one helper, DeviceCloudBank.padded hands out padded clouds with their lengths, and the model
still refuses to run off the GPU."""
import ctypes

import numpy as np
import pytest
import torch

PTR = 4096      # a non-null "device pointer": every call below is refused before anything could read it


@pytest.fixture(scope="module")
def lib():
    from pnpp_hip import build, _lib
    build.build()
    return _lib.lib()


def _desc(N=128, n_valid=100):
    from pnpp_hip import _lib
    d = _lib.PtInferDesc()
    d.B, d.N, d.n_valid, d.in_dim, d.E, d.H, d.F, d.depth, d.eps = 2, N, n_valid, 3, 64, 4, 2048, 6, 1e-5
    return d


def _attention_calls(lib, B, N, nv, lengths):
    """the five ragged attention entry points at these sizes, every other pointer non-null"""
    fwd = (PTR, B, N, nv, lengths, 4, 16, None, 0.0, PTR, PTR, None)
    bwd = (PTR, PTR, PTR, PTR, B, N, nv, lengths, 4, 16, None, None, 0.0, PTR, PTR, None)
    return {"attention_fwd_ragged": lambda: lib.pnpp_attention_fwd_ragged(*fwd),
            "attention_bwd_ragged": lambda: lib.pnpp_attention_bwd_ragged(*bwd),
            "attention_split_fwd_ragged": lambda: lib.pnpp_attention_split_fwd_ragged(*fwd),
            "attention_split_bwd_ragged": lambda: lib.pnpp_attention_split_bwd_ragged(*bwd),
            "attention_infer_ragged": lambda: lib.pnpp_attention_infer_ragged(PTR, B, N, nv, lengths, 4, 16, PTR, None)}


def _pt_calls(lib, d, lengths):
    r = ctypes.byref(d)
    return {"pt_infer_head_ragged": lambda: lib.pnpp_pt_infer_head_ragged(r, lengths, PTR, PTR, PTR, PTR, None),
            "pt_infer_tail_ragged": lambda: lib.pnpp_pt_infer_tail_ragged(r, lengths, 0, PTR, PTR + 4096, PTR, PTR, PTR + 8192, PTR, PTR, None),
            "pt_infer_pool_ragged": lambda: lib.pnpp_pt_infer_pool_ragged(r, lengths, PTR, PTR, PTR, 3, PTR, None)}


def _refused(lib, calls, *words):
    from pnpp_hip import _lib
    for name, call in calls.items():
        assert call() == _lib.PNPP_ERR_ARG, name
        msg = lib.pnpp_last_error().decode()
        assert msg and all(w in msg for w in words), (name, msg)


def test_null_lengths_is_refused(lib):
    calls = {**_attention_calls(lib, 2, 128, 100, None), **_pt_calls(lib, _desc(), None),
             "mean_points_ragged": lambda: lib.pnpp_mean_points_ragged(PTR, 2, 128, None, 64, PTR, None),
             "mean_points_bwd_ragged": lambda: lib.pnpp_mean_points_bwd_ragged(PTR, 2, 128, None, 64, PTR, None)}
    assert len(calls) == 10
    _refused(lib, calls, "null lengths")
    for name in calls:                                        # the message names the entry point
        calls[name]()
        assert name in lib.pnpp_last_error().decode(), name


def test_size_rules_hold_before_any_launch(lib):
    _refused(lib, _attention_calls(lib, 2, 200, 100, PTR), "multiple of 128")
    _refused(lib, _pt_calls(lib, _desc(N=200), PTR), "multiple of 128")
    for nv in (0, 129):
        _refused(lib, _attention_calls(lib, 2, 128, nv, PTR), "n_valid", "1..N=128")
        _refused(lib, _pt_calls(lib, _desc(n_valid=nv), PTR), "n_valid", "1..N=128")
    _refused(lib, {"mean_points_ragged": lambda: lib.pnpp_mean_points_ragged(PTR, 0, 128, PTR, 64, PTR, None),
                   "mean_points_bwd_ragged": lambda: lib.pnpp_mean_points_bwd_ragged(PTR, 2, 128, PTR, 0, PTR, None)}, "non-positive")


def test_lengths_validation_helper():
    from pnpp_hip.transformer import check_lengths
    ok = check_lengths([5, 1, 300], 3, 300)
    assert ok.dtype == torch.int32 and ok.tolist() == [5, 1, 300] and not ok.is_cuda
    assert check_lengths(torch.tensor([7, 8], dtype=torch.int64), 2, 8).dtype == torch.int32
    with pytest.raises(ValueError, match=r"shape \(3,\)"):
        check_lengths([1, 2], 3, 10)
    with pytest.raises(ValueError, match=r"shape \(2,\)"):
        check_lengths(torch.ones(2, 1, dtype=torch.int32), 2, 10)
    with pytest.raises(ValueError, match="integer dtype"):
        check_lengths(torch.tensor([1.0, 2.0]), 2, 10)
    with pytest.raises(ValueError, match=r"lengths\[1\] = 0: cloud 1"):
        check_lengths([3, 0, 4], 3, 10)
    with pytest.raises(ValueError, match=r"lengths\[2\] = 11: cloud 2"):
        check_lengths(torch.tensor([3, 10, 11], dtype=torch.int32), 3, 10)


def test_bank_padded_on_a_cpu_bank():
    from dataloader_common import DeviceCloudBank
    rng = np.random.default_rng(0)
    sizes = [5, 40, 17, 1, 23]
    clouds = [rng.standard_normal((n, 3)).astype(np.float32) for n in sizes]
    bank = DeviceCloudBank(clouds, "cpu")
    for ids in ([2, 0, 3], torch.tensor([4, 2]), [1]):
        xyz, lengths = bank.padded(ids)
        ids = [int(i) for i in ids]
        longest = max(sizes[i] for i in ids)
        assert xyz.shape == (len(ids), longest, 3) and xyz.dtype == torch.float32 and xyz.is_contiguous()
        assert lengths.dtype == torch.int32 and lengths.tolist() == [sizes[i] for i in ids]
        for row, i in enumerate(ids):
            assert np.array_equal(xyz[row, :sizes[i]].numpy(), clouds[i])
            assert bool((xyz[row, sizes[i]:] == 0).all())
    assert bank.draws == 0                                    # no sampling, no draw counted
    with pytest.raises(IndexError):
        bank.padded([5])


def test_model_with_lengths_has_no_cpu_fallback():
    from models.point_transformer import PointTransformer
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PointTransformer()(torch.rand(2, 64, 3), lengths=[64, 10])
