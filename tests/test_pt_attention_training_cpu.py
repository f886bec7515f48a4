"""CPU-side checks of the training attention on the bf16 matrix pipe (csrc/attention_train_kernels.hip): the three additions to the C ABI
are exported, declared and bound with the argument lists of the float32 entries they mirror, their argument validation runs before any
launch (so it runs without a GPU) and names the refused field, and the Python surface (attention(form=), PointTransformer.set_attention)
rejects an unknown form and leaves the state_dict alone."""
import ctypes
import os
import re

import pytest

from conftest import ROOT  # noqa: F401  (puts the package on sys.path)

NAMES = ("pnpp_attention_split_fwd", "pnpp_attention_split_bwd", "pnpp_attention_split_supported")


@pytest.fixture(scope="module")
def lib():
    from pnpp_hip import build, _lib
    build.build()
    return _lib.lib()


def test_symbols_are_exported_declared_and_bound(lib):
    from pnpp_hip import build, _lib
    h = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(build.INCLUDE, "pnpp_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert hasattr(h, name), f"{name} is not exported"
        assert re.search(r"^int %s\(" % name, header, re.M), f"{name} is not declared in pnpp_hip.h"
    # the argument lists of the float32 entries
    assert _lib.SIGNATURES["pnpp_attention_split_fwd"] == _lib.SIGNATURES["pnpp_attention_fwd"]
    assert _lib.SIGNATURES["pnpp_attention_split_bwd"] == _lib.SIGNATURES["pnpp_attention_bwd"]
    assert _lib.SIGNATURES["pnpp_attention_split_supported"] == _lib.SIGNATURES["pnpp_attention_infer_supported"]
    assert lib.pnpp_abi_version() == 5


def test_shapes_taken(lib):
    for B, N, n_valid, H in ((1, 128, 1, 1), (1, 128, 128, 4), (8, 4096, 4096, 4), (32, 1024, 1000, 4), (3, 256, 129, 8), (65535, 128, 5, 65535)):
        assert lib.pnpp_attention_split_supported(B, N, n_valid, H, 16) == 1, (B, N, n_valid, H, lib.pnpp_last_error())


@pytest.mark.parametrize("kw, field", [(dict(head_dim=32), b"head_dim=32"), (dict(head_dim=8), b"head_dim=8"), (dict(N=100), b"N=100"),
                                       (dict(N=192), b"N=192"), (dict(n_valid=0), b"n_valid=0"), (dict(n_valid=257), b"n_valid=257"),
                                       (dict(B=0), b"B=0"), (dict(H=0), b"H=0"), (dict(B=65536), b"B=65536")])
def test_refused_shapes_name_the_field(lib, kw, field):
    from pnpp_hip import _lib
    a = dict(B=2, N=256, n_valid=200, H=4, head_dim=16)
    a.update(kw)
    assert lib.pnpp_attention_split_supported(a["B"], a["N"], a["n_valid"], a["H"], a["head_dim"]) == 0
    assert field in lib.pnpp_last_error(), lib.pnpp_last_error()
    # both calls refuse the same shape before they launch anything: the pointers are never dereferenced
    assert lib.pnpp_attention_split_fwd(8, a["B"], a["N"], a["n_valid"], a["H"], a["head_dim"], None, 0.0, 16, 24, None) == _lib.PNPP_ERR_ARG
    assert field in lib.pnpp_last_error(), lib.pnpp_last_error()
    assert lib.pnpp_attention_split_bwd(8, 8, 8, 8, a["B"], a["N"], a["n_valid"], a["H"], a["head_dim"], None, None, 0.0, 16, 24,
                                        None) == _lib.PNPP_ERR_ARG
    assert field in lib.pnpp_last_error(), lib.pnpp_last_error()


def test_argument_errors_are_those_of_the_float32_entries(lib):
    from pnpp_hip import _lib
    assert lib.pnpp_attention_split_fwd(None, 2, 256, 200, 4, 16, None, 0.0, None, None, None) == _lib.PNPP_ERR_ARG
    assert b"null" in lib.pnpp_last_error()
    assert lib.pnpp_attention_split_fwd(8, 2, 256, 200, 4, 16, None, 1.0, 16, None, None) == _lib.PNPP_ERR_ARG
    assert b"p=1" in lib.pnpp_last_error()
    assert lib.pnpp_attention_split_bwd(8, 8, 8, 8, 2, 256, 200, 4, 16, 8, None, 0.1, 16, 24, None) == _lib.PNPP_ERR_ARG
    assert b"both mask orientations" in lib.pnpp_last_error()
    assert lib.pnpp_attention_split_bwd(8, 8, 8, None, 2, 256, 200, 4, 16, None, None, 0.0, 16, 24, None) == _lib.PNPP_ERR_ARG
    assert b"null" in lib.pnpp_last_error()


def test_unknown_form_is_a_value_error():
    import torch
    from pnpp_hip import transformer as T
    with pytest.raises(ValueError, match="form='nope'"):
        T.attention(torch.zeros(1, 128, 48), 1, form="nope")
    assert T.ATTENTION_FORMS == ("float32", "split")


def test_set_attention_is_a_plain_attribute():
    from models.point_transformer import PointTransformer
    model = PointTransformer(depth=2)
    keys = list(model.state_dict().keys())
    assert model.attention_form == "float32"
    assert model.set_attention("split") is model and model.attention_form == "split"
    assert list(model.state_dict().keys()) == keys
    assert not any("attention_form" in n for n, _ in list(model.named_parameters()) + list(model.named_buffers()))
    with pytest.raises(ValueError, match="form='nope'"):
        model.set_attention("nope")
    assert model.attention_form == "split"
    assert model.set_attention("float32").attention_form == "float32"
