"""Yaw symmetry without a GPU: the numpy restatement against float64 and on clouds whose answer is known, the classification of the
seeded families, symmetric_targets on CPU tensors, every refusal of the C entry points (they come before any launch) and the header /
binding pair."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import symmetry_ref as R


@pytest.fixture(scope="module")
def h():
    from pnpp_hip import build, _lib
    build.build()
    return _lib.lib()


def _parity_cases():
    return [(B, N, G) for N in R.PARITY_N for G in R.PARITY_G for B in R.PARITY_B] + [(1, N, 3) for N in R.TILE_N]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
F32_WORST_MEASURED = 1.85   # units of 2^-24 R^2, over the parity case table (B=3, N=2, G=1, cloud 1); DESIGN section 20 records it
F32_GATE = 4 * F32_WORST_MEASURED


def test_float32_against_float64():
    """The only place float64 judges the arithmetic: worst |D32 - D64| (and |nu32 - nu64|) over the parity case table, in units of
    2^-24 R^2 with R the largest centred coordinate of the cloud.  Measured worst 1.85; the gate is four times that."""
    worst = 0.0
    for B, N, G in _parity_cases():
        x = R.parity_cloud(B, N)
        for b in range(B):
            c, table = R.centroid(x[b]), R.grid_table(G)
            D32, nu32 = R.profile(x[b], c, table)
            D64, nu64 = R.profile(x[b], c, table, np.float64)
            radius = max(np.abs(x[b][:, 0] - c[0]).max(), np.abs(x[b][:, 1]).max(), np.abs(x[b][:, 2] - c[2]).max())
            unit = 2.0 ** -24 * float(radius) ** 2
            worst = max(worst, np.abs(D32.astype(np.float64) - D64).max() / unit, abs(float(nu32) - nu64) / unit)
    print(f"float32 against float64: worst {worst:.3f} x 2^-24 R^2 (gate {F32_GATE:.2f})")
    assert worst <= F32_GATE


def test_exact_properties():
    for name in R.NAMES:
        x = R.family(name, 96, 5)
        D, nu = R.profile(x, R.centroid(x), R.grid_table(12))
        assert D[0] == 0.0 and nu > 0.0
        S = R.symmetric(D)
        assert np.array_equal(S, S[(12 - np.arange(12)) % 12])
    x, c = R.lattice()
    for G in (4, 72):
        D, nu = R.profile(x, c, R.grid_table(G))
        assert np.all(D[[0, G // 4, G // 2, 3 * G // 4]] == 0.0) and nu == 1.0
    one = np.array([[0.25, -1.5, 3.0]], np.float32)
    D, nu = R.profile(one, R.centroid(one), R.grid_table(8))
    assert nu == 0.0 and np.all(D == 0.0) and R.decide(D, nu)[0] == 0


def test_grid_table_is_the_library_table():
    from pnpp_hip import symmetry
    for G in (1, 2, 3, 4, 8, 24, 72, 360):
        t = symmetry.grid_table(G, "cpu").numpy()
        assert np.array_equal(t, R.grid_table(G))
        for q in range(4):
            if (q * G) % 4 == 0:
                assert tuple(t[q * G // 4]) == ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[q]


def test_decision_on_hand_made_profiles():
    D = np.ones(12, np.float32)
    D[0] = 0.0
    assert R.decide(D, 1.0)[0] == 0                                   # S = 2 everywhere <= 2.6
    assert R.decide(D * 2, 1.0)[0] == 1
    two = D * 2
    two[6] = 1.0
    assert R.decide(two, 1.0)[0] == 2
    four = two.copy()
    four[[3, 9]] = 1.0
    order, count, angles = R.decide(four, 1.0)
    assert order == 4 and count == 4 and np.array_equal(angles[:4], np.float32(2 * np.pi * np.arange(4) / 4)) and np.all(angles[4:] == 0)
    assert R.decide(four, 1.0, orders=(2, 3))[0] == 2
    assert R.decide(four, 1.0, orders=(8,))[0] == 1                   # 8 does not divide 12


def test_classification_of_the_families():
    """N = 1024, G = 24, tol = 1.3.  A case is admitted only if the float64 restatement puts every true-symmetry score <= 1.15 and every
    other candidate order's worst score >= 1.5; every one of the three seeds of every family has to be (the GPU tests use all fifteen)."""
    for name, want in R.FAMILIES.items():
        for seed in R.CLASS_SEEDS:
            xyz, ok, worst_true, least_false = R.admitted(name, seed)
            print(f"{name} seed {seed}: true symmetries <= {worst_true:.3f}, other orders >= {least_false:.3f}")
            assert ok, (name, seed, worst_true, least_false)
            D, nu = R.profile(xyz, R.centroid(xyz), R.grid_table(R.CLASS_G))
            assert R.decide(D, nu)[0] == want, (name, seed)


# ---- symmetric_targets -----------------------------------------------------------------------------------------------------------------
def _angle_set_equal(a, b, tol=1e-6):
    if len(a) != len(b):
        return False
    left = list(b)
    for v in a:
        hit = [w for w in left if abs((v - w + math.pi) % (2 * math.pi) - math.pi) <= tol]
        if not hit:
            return False
        left.remove(hit[0])
    return True


def test_symmetric_targets_match_multi_peak_gt():
    import synthetic
    from pnpp_hip.symmetry import symmetric_targets
    _, mu, _, fwd = synthetic.rotated_clouds(12, 8, seed=3)
    for order in (1, 2, 4):
        K = torch.full((12,), order)
        want = synthetic.multi_peak_gt(fwd, K, 4, 8.0)
        vm, K_gt = symmetric_targets(mu, K, kappa=8.0, max_K=4)
        assert vm.shape == (12, 4, 3) and vm.dtype == torch.float32 and K_gt.dtype == torch.int32 and torch.equal(K_gt, K.int())
        for b in range(12):
            assert _angle_set_equal(vm[b, :order, 0].tolist(), want[b, :order, 0].tolist()), (order, b)
            assert torch.all(vm[b, :order, 1] == 8.0) and torch.allclose(vm[b, :order, 2], torch.full((order,), 1.0 / order))
            assert torch.all(vm[b, order:] == 0.0)
            assert torch.all(vm[b, :order, 0] > -math.pi) and torch.all(vm[b, :order, 0] <= math.pi)
        assert torch.equal(vm[:, 0, 0], mu)


def test_symmetric_targets_k0_row():
    from pnpp_hip.symmetry import symmetric_targets
    mu = torch.tensor([0.5, -2.0, 3.0, 1.0])
    vm, K = symmetric_targets(mu, torch.tensor([0, 6, 8, 3]), kappa=8.0, max_K=4)
    assert K.tolist() == [1, 1, 1, 3]
    for b in range(3):                                                # continuous, and two orders above max_K: one peak at mu, kappa 0
        assert vm[b, 0].tolist() == [float(mu[b]), 0.0, 1.0] and torch.all(vm[b, 1:] == 0.0)
    assert vm[3, :3, 1].tolist() == [8.0, 8.0, 8.0] and torch.all(vm[3, 3] == 0.0)
    with pytest.raises(ValueError):
        symmetric_targets(mu, torch.tensor([1, 2]))


# ---- the C entry points' refusals ------------------------------------------------------------------------------------------------------
def _profile(h, ragged, xyz=8, B=1, N=64, lengths=8, centre=8, table=8, G=8, ws=8, nbytes=None, nd=None, ni=None):
    if nbytes is None:
        nbytes = h.pnpp_yaw_workspace_bytes(max(B, 1), max(N, 1), max(G, 1))
    if ragged:
        return h.pnpp_yaw_profile_ragged(xyz, B, N, lengths, centre, table, G, ws, nbytes, nd, ni, None)
    return h.pnpp_yaw_profile(xyz, B, N, centre, table, G, ws, nbytes, nd, ni, None)


@pytest.mark.parametrize("ragged", [False, True])
def test_profile_refusals(h, ragged):
    from pnpp_hip import _lib
    table = [
        (dict(xyz=None), b"yaw_profile: null pointer"),
        (dict(centre=None), b"yaw_profile: null pointer"),
        (dict(table=None), b"yaw_profile: null pointer"),
        (dict(ws=None), b"yaw_profile: null pointer"),
        (dict(nd=8), b"nearest distances and indices come together"),
        (dict(ni=8), b"nearest distances and indices come together"),
        (dict(N=0), b"non-positive size (B=1 N=0)"),
        (dict(N=-2), b"non-positive size (B=1 N=-2)"),
        (dict(B=0), b"non-positive size (B=0 N=64)"),
        (dict(G=0), b"non-positive number of angles (G=0)"),
        (dict(G=-1), b"non-positive number of angles (G=-1)"),
        (dict(B=70000), b"exceeds grid limit"),
        (dict(nbytes=0), b"workspace too small (0 bytes"),
        (dict(N=257, nbytes=h.pnpp_yaw_workspace_bytes(1, 256, 8)), b"workspace too small"),
    ]
    for kw, words in table:
        assert _profile(h, ragged, **kw) == _lib.PNPP_ERR_ARG, kw
        assert words in h.pnpp_last_error(), (kw, h.pnpp_last_error())
    if ragged:
        assert _profile(h, True, lengths=None) == _lib.PNPP_ERR_ARG
        assert b"yaw_profile_ragged: null lengths" in h.pnpp_last_error()


def _symmetry(h, ws=8, nbytes=None, B=1, N=64, lengths=None, G=24, tol=1.3, orders=(2, 3, 4, 6, 8), n_orders=None, distance=8, floor=8,
              score=8, order=8, count=8, angles=8, stride=8):
    if nbytes is None:
        nbytes = h.pnpp_yaw_workspace_bytes(max(B, 1), max(N, 1), max(G, 1))
    arr = None if orders is None else (ctypes.c_int32 * max(len(orders), 1))(*orders)
    n = (0 if orders is None else len(orders)) if n_orders is None else n_orders
    return h.pnpp_yaw_symmetry(ws, nbytes, B, N, lengths, G, tol, arr, n, distance, floor, score, order, count, angles, stride, None)


def test_symmetry_refusals(h):
    from pnpp_hip import _lib
    table = [
        (dict(ws=None), b"yaw_symmetry: null pointer"),
        (dict(distance=None), b"yaw_symmetry: null pointer"),
        (dict(floor=None), b"yaw_symmetry: null pointer"),
        (dict(score=None), b"yaw_symmetry: null pointer"),
        (dict(angles=None), b"yaw_symmetry: null pointer"),
        (dict(N=0), b"non-positive size (B=1 N=0)"),
        (dict(B=-1), b"non-positive size (B=-1 N=64)"),
        (dict(G=0), b"non-positive number of angles (G=0)"),
        (dict(tol=float("nan")), b"is not a finite, non-negative number"),
        (dict(tol=float("inf")), b"is not a finite, non-negative number"),
        (dict(tol=-0.5), b"tol=-0.5 is not a finite, non-negative number"),
        (dict(orders=(2, 1)), b"candidate order 1 is below 2"),
        (dict(orders=(0,)), b"candidate order 0 is below 2"),
        (dict(orders=(2, 5)), b"candidate order 5 does not divide G=24"),
        (dict(G=9, orders=(2,)), b"candidate order 2 does not divide G=9"),
        (dict(orders=tuple([2] * 17)), b"17 candidate orders (at most 16"),
        (dict(orders=None, n_orders=2), b"2 candidate orders (at most 16"),
        (dict(stride=7), b"angle stride 7 is below the largest candidate order 8"),
        (dict(nbytes=8), b"workspace too small (8 bytes"),
        (dict(B=70000), b"exceeds grid limit"),
    ]
    for kw, words in table:
        assert _symmetry(h, **kw) == _lib.PNPP_ERR_ARG, kw
        assert words in h.pnpp_last_error(), (kw, h.pnpp_last_error())
    assert h.pnpp_yaw_workspace_bytes(0, 64, 8) == 0 and b"non-positive size" in h.pnpp_last_error()
    assert h.pnpp_yaw_workspace_bytes(1, 64, 0) == 0
    # part[b][query chunk][slot] float64: slots = the G angles and the floor, rounded up to whole angle blocks
    assert h.pnpp_yaw_workspace_bytes(3, 257, 8) == 3 * 2 * 16 * 8
    assert h.pnpp_yaw_workspace_bytes(1, 256, 7) == 1 * 1 * 8 * 8


def test_header_and_binding(h):
    from pnpp_hip import _lib, build
    hdr = open(os.path.join(ROOT, "include", "pnpp_hip.h")).read()
    for name in ("pnpp_yaw_profile", "pnpp_yaw_profile_ragged", "pnpp_yaw_symmetry"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.SIGNATURES and hasattr(h, name)
    assert len(_lib.SIGNATURES["pnpp_yaw_profile_ragged"][1]) == len(_lib.SIGNATURES["pnpp_yaw_profile"][1]) + 1
    for name, value in (("ANGLE_BLOCK", R.ANGLE_BLOCK), ("TILE", R.TILE), ("QUERIES", 256), ("MAX_ORDERS", 16)):
        assert re.search(r"#define PNPP_YAW_%s %d\b" % (name, value), hdr) and getattr(_lib, "YAW_" + name) == value
    assert h.pnpp_abi_version() == 5
    assert build.SOURCES["symmetry_kernels.hip"] == ["-ffp-contract=off"]
    src = open(os.path.join(build.CSRC, "symmetry_kernels.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "yaw_profile_kernel" in src and "yaw_symmetry_kernel" in src
    assert "atomic" not in src


# ---- Python surface --------------------------------------------------------------------------------------------------------------------
def test_no_cpu_fallback_and_exports():
    import pnpp_hip
    from pnpp_hip import ops, symmetry
    assert "symmetry" in pnpp_hip.__all__
    assert {"yaw_profile", "yaw_symmetry", "symmetric_targets", "YawProfile", "YawSymmetry"} <= set(symmetry.__all__)
    x = torch.rand(1, 32, 3)
    for fn in (symmetry.yaw_profile, symmetry.yaw_symmetry):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.yaw_profile(x, torch.zeros(1, 3), torch.zeros(4, 2))
    from dataloader_common import DeviceCloudBank
    assert callable(DeviceCloudBank.symmetry)
