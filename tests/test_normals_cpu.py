"""Surface normals without a GPU: the numpy restatement on hand-made inputs, every refusal of the C entry points (they come before any
launch), the header / binding pair, and the loader's unchanged default."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import normals_ref as R


@pytest.fixture(scope="module")
def h():
    from pnpp_hip import build, _lib
    build.build()
    return _lib.lib()


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_ref_exact_plane_gives_z():
    xyz = R.plane(200, 3)[None]
    idx = R.knn_bruteforce(xyz, 16)
    n, c, ill, tie = R.normals_ref(xyz, idx, None, "none")
    assert not ill.any()
    assert np.array_equal(n, np.broadcast_to(np.array([0.0, 0.0, 1.0]), n.shape))     # canonical sign: +z
    assert np.all(c == 0.0)
    view = np.array([[0.0, 0.0, 5.0]], np.float32)
    assert np.array_equal(R.normals_ref(xyz, idx, view, "toward")[0], n)              # the viewpoint is above the plane
    assert np.array_equal(R.normals_ref(xyz, idx, view, "away")[0], -n)


def test_ref_triangle_k3():
    tri = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 1.0]]], np.float32)
    idx = np.array([[[0, 1, 2], [1, 0, 2], [2, 1, 0]]])
    n, c, ill, _ = R.normals_ref(tri, idx, None, "none")
    want = np.cross(tri[0, 1] - tri[0, 0], tri[0, 2] - tri[0, 0]).astype(np.float64)
    want /= np.linalg.norm(want)
    want *= np.sign(want[np.argmax(np.abs(want))])
    assert not ill.any()
    assert np.abs(n - want[None, None, :]).max() < 1e-15
    assert np.abs(c).max() < 1e-15


def test_ref_identical_points_give_zeros():
    xyz = np.tile(np.array([[0.3, -1.5, 2.0]], np.float32), (1, 8, 1))
    idx = np.tile(np.arange(5)[None, None, :], (1, 8, 1))
    n, c, ill, tie = R.normals_ref(xyz, idx, np.zeros((1, 3), np.float32), "away")
    assert np.all(n == 0.0) and np.all(c == 0.0) and ill.all() and not tie.any()


def test_ref_orientation_and_masks():
    xyz = R.sphere(256, 11)[None]
    idx = R.knn_bruteforce(xyz, 16)
    centre = np.zeros((1, 3), np.float32)
    n_out = R.normals_ref(xyz, idx, centre, "away")[0]
    n_in = R.normals_ref(xyz, idx, centre, "toward")[0]
    assert np.all((n_out[0] * xyz[0]).sum(-1) > 0.0) and np.array_equal(n_in, -n_out)
    assert np.abs(np.linalg.norm(n_out, axis=-1) - 1.0).max() < 1e-14
    c = R.normals_ref(xyz, idx, centre, "away")[1]
    assert np.all(c >= 0.0) and np.all(c <= 1.0 / 3.0 + 1e-15)


def test_case_table_families_exclude_little():
    """The gates of the GPU tests leave out ill-conditioned points and sign ties; the seeded families must keep that under 2 %."""
    for name, c in R.CASES.items():
        xyz = R.batch(c["families"], c["N"], R.SEED)
        assert xyz.dtype == np.float32 and xyz.shape == (len(c["families"]), c["N"], 3)
        idx = R.knn_bruteforce(xyz, c["k"])
        if c["orient"] == "centroid":
            ref, mode = xyz.astype(np.float64).mean(1).astype(np.float32), "away"
        elif c["orient"] is None:
            ref, mode = None, "none"
        else:
            ref, mode = np.tile(np.array(c["orient"], np.float32), (xyz.shape[0], 1)), "toward"
        _, _, ill, tie = R.normals_ref(xyz, idx, ref, mode)
        assert (ill | tie).mean() <= R.MAX_EXCLUDED, name


# ---- the C entry points' refusals -----------------------------------------------------------------------------------------------------
def _call(h, ragged, xyz=8, B=1, N=64, k=16, orient=0, ref=None, out=8, stride=3, curv=None, idx=None, lengths=8):
    if ragged:
        return h.pnpp_estimate_normals_ragged(xyz, B, N, lengths, k, orient, ref, out, stride, curv, idx, None)
    return h.pnpp_estimate_normals(xyz, B, N, k, orient, ref, out, stride, curv, idx, None)


@pytest.mark.parametrize("ragged", [False, True])
def test_refusals(h, ragged):
    from pnpp_hip import _lib
    ARG, RANGE = _lib.PNPP_ERR_ARG, _lib.PNPP_ERR_RANGE
    table = [
        (dict(xyz=None), ARG, b"null pointer"),
        (dict(out=None), ARG, b"null pointer"),
        (dict(B=0), ARG, b"non-positive size"),
        (dict(N=0), ARG, b"non-positive size"),
        (dict(N=-3), ARG, b"non-positive size"),
        (dict(k=2), ARG, b"k=2 outside the supported range 3..128"),
        (dict(k=129, N=500), ARG, b"k=129 outside the supported range 3..128"),
        (dict(k=16, N=15), RANGE, b"selected index k out of range (k=16 > N=15)"),
        (dict(stride=4), ARG, b"output stride 4 is neither 3"),
        (dict(stride=0), ARG, b"output stride 0 is neither 3"),
        (dict(orient=3), ARG, b"unknown orientation mode 3"),
        (dict(orient=-1), ARG, b"unknown orientation mode -1"),
        (dict(orient=_lib.NORMALS_AWAY, ref=None), ARG, b"needs a reference point per cloud"),
        (dict(orient=_lib.NORMALS_TOWARD, ref=None), ARG, b"needs a reference point per cloud"),
        (dict(B=70000), ARG, b"exceeds grid limit"),
    ]
    for kw, code, words in table:
        assert _call(h, ragged, **kw) == code, kw
        assert words in h.pnpp_last_error(), (kw, h.pnpp_last_error())
    if ragged:
        assert _call(h, True, lengths=None) == ARG
        assert b"null lengths" in h.pnpp_last_error()


def test_header_and_binding(h):
    from pnpp_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "pnpp_hip.h")).read()
    for name in ("pnpp_estimate_normals", "pnpp_estimate_normals_ragged"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.SIGNATURES and hasattr(h, name)
    assert len(_lib.SIGNATURES["pnpp_estimate_normals_ragged"][1]) == len(_lib.SIGNATURES["pnpp_estimate_normals"][1]) + 1
    for name, value in (("NONE", 0), ("AWAY", 1), ("TOWARD", 2)):
        assert re.search(r"#define PNPP_NORMALS_%s %d\b" % (name, value), hdr) and getattr(_lib, "NORMALS_" + name) == value
    assert h.pnpp_abi_version() == 5


def test_built_from_index_kernels():
    from pnpp_hip import build
    assert "knn_kernels.hip" in build.SOURCES
    src = open(os.path.join(build.CSRC, "knn_kernels.hip")).read()
    assert "knn_normals_kernel" in src and "pnpp_estimate_normals_ragged" in src


# ---- Python surface ---------------------------------------------------------------------------------------------------------------
def test_no_cpu_fallback_and_exports():
    import pnpp_hip
    from pnpp_hip import normals, ops
    assert "normals" in pnpp_hip.__all__
    assert set(normals.__all__) == {"estimate_normals", "with_normals", "reference_points"}
    x = torch.rand(1, 32, 3)
    for fn in (normals.estimate_normals, normals.with_normals, normals.reference_points):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.estimate_normals(x, 8)


def test_bankloader_default_unchanged():
    from dataloader_common import BankLoader, DeviceCloudBank
    clouds = [np.random.default_rng(i).random((20 + i, 3)).astype(np.float32) for i in range(3)]
    bank = DeviceCloudBank(clouds, "cpu")
    loader = BankLoader(bank, [torch.arange(3)], num_points=16, batch=2, shuffle=False)
    assert loader.normals is None and loader.channels_first is False and loader.normals_orient == "centroid" and len(loader) == 2
    assert BankLoader(bank, [torch.arange(3)], 16, 2, False, normals=8, channels_first=True).normals == 8
    for bad in (2, 17, 129):
        with pytest.raises(ValueError, match="normals="):
            BankLoader(bank, [torch.arange(3)], 16, 2, False, normals=bad)
