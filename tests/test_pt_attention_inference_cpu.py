"""CPU-side checks of the Predictor's split-product attention (csrc/attention_infer_kernels.hip): the two additions to the C ABI are
exported and bound, their argument validation runs before any launch (so it runs without a GPU) and names the refused field, and the
Python surface rejects an unknown attention form before it looks for a device."""
import ctypes

import pytest

from conftest import ROOT  # noqa: F401  (puts the package on sys.path)


@pytest.fixture(scope="module")
def lib():
    from pnpp_hip import build, _lib
    build.build()
    return _lib.lib()


def test_symbols_are_exported_and_bound(lib):
    from pnpp_hip import _lib
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pnpp_attention_infer", "pnpp_attention_infer_supported"):
        assert name in _lib.SIGNATURES, name
        assert hasattr(h, name), f"{name} is not exported"
    res, args = _lib.SIGNATURES["pnpp_attention_infer"]
    assert res is ctypes.c_int and len(args) == 8      # qkv, B, N, n_valid, H, head_dim, out, stream
    res, args = _lib.SIGNATURES["pnpp_attention_infer_supported"]
    assert res is ctypes.c_int and args == [ctypes.c_int] * 5
    assert lib.pnpp_abi_version() == 5


def test_shapes_taken(lib):
    for B, N, n_valid, H in ((1, 128, 1, 1), (1, 128, 128, 4), (8, 4096, 4096, 4), (32, 1024, 1000, 4), (3, 256, 129, 8), (65535, 128, 5, 65535)):
        assert lib.pnpp_attention_infer_supported(B, N, n_valid, H, 16) == 1, (B, N, n_valid, H, lib.pnpp_last_error())


def test_null_pointers_are_argument_errors(lib):
    from pnpp_hip import _lib
    assert lib.pnpp_attention_infer(None, 2, 256, 200, 4, 16, None, None) == _lib.PNPP_ERR_ARG
    assert b"null" in lib.pnpp_last_error()
    assert lib.pnpp_attention_infer(None, 2, 256, 200, 4, 16, 8, None) == _lib.PNPP_ERR_ARG
    assert lib.pnpp_attention_infer(8, 2, 256, 200, 4, 16, None, None) == _lib.PNPP_ERR_ARG
    assert b"null" in lib.pnpp_last_error()


@pytest.mark.parametrize("kw, field", [(dict(head_dim=32), b"head_dim=32"), (dict(N=100), b"N=100"), (dict(n_valid=0), b"n_valid=0"),
                                       (dict(n_valid=257), b"n_valid=257"), (dict(B=0), b"B=0"), (dict(H=0), b"H=0"), (dict(N=0), b"N=0"),
                                       (dict(B=65536), b"B=65536")])
def test_refused_shapes_name_the_field(lib, kw, field):
    from pnpp_hip import _lib
    a = dict(B=2, N=256, n_valid=200, H=4, head_dim=16)
    a.update(kw)
    assert lib.pnpp_attention_infer_supported(a["B"], a["N"], a["n_valid"], a["H"], a["head_dim"]) == 0
    assert field in lib.pnpp_last_error(), lib.pnpp_last_error()
    # the call refuses the same shape before it launches anything: the pointers are never dereferenced
    assert lib.pnpp_attention_infer(8, a["B"], a["N"], a["n_valid"], a["H"], a["head_dim"], 16, None) == _lib.PNPP_ERR_ARG
    assert field in lib.pnpp_last_error(), lib.pnpp_last_error()


def test_unknown_attention_form_is_a_value_error():
    """checked as far as it goes without a device: the keyword is validated in front of the device check, a known form reaches it"""
    from pnpp_hip import Predictor
    from pnpp_hip.transformer_inference import TransformerPredictor
    from models.point_transformer import PointTransformer
    model = PointTransformer(depth=2)
    for cls in (Predictor, TransformerPredictor):
        with pytest.raises(ValueError, match="attention='fast'"):
            cls(model, attention="fast")
        for form in ("split", "float32"):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                cls(model, attention=form)
    assert TransformerPredictor.ATTENTION_FORMS == ("split", "float32")
