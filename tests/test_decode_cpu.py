"""CPU-side checks of orientation decoding (pnpp_hip/decode.py, csrc/decode_kernels.hip): the float64 restatement the GPU tests
compare with reproduces the reference's own mvm_density_on_grid, the histogram -> statistics code on hand-made histograms, the
argument refusals of the two C entries (they happen before any launch) and their header / binding symmetry."""
import os
import re

import numpy as np
import pytest

import decode_ref as R
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from pnpp_hip import build, _lib
    build.build()
    return _lib.lib()


def test_decode_ref_density_equals_the_reference(golden):
    g = golden("mvm_decode.npz")
    for num in (int(n) for n in g["nums"]):
        assert np.abs(R.grid(num) - g[f"theta_{num}"]).max() <= 1e-12
        d = R.density(g["mu"], g["kappa"], g["weight"], num=num)
        assert d.shape == g[f"density_{num}"].shape
        assert np.abs(d - g[f"density_{num}"]).max() <= 1e-12, num


def test_decode_ref_hand_made_rows():
    """The restatement on rows whose answer is known without it."""
    o = R.decode([[0.0, np.pi]], [[20.0, 20.0]], [[0.6, 0.4]], num=360)
    assert o["n_modes"][0] == 2 and abs(o["modes"][0, 0]) < 1e-7 and abs(abs(o["modes"][0, 1]) - np.pi) < 1e-7
    th = R.grid(360)[100]                                                                  # exactly on a grid point
    o = R.decode(np.float64([[th]]), [[30.0]], None, num=360)
    assert o["n_modes"][0] == 1 and abs(o["angle"][0] - th) < 1e-7
    o = R.decode([[1.0, 1.2]], [[8.0, 8.0]], [[0.5, 0.5]], num=360)                        # 0.2 rad apart at kappa 8: one mode
    assert o["n_modes"][0] == 1 and abs(o["angle"][0] - 1.1) < 1e-6
    near = np.pi / 4 + 0.01                                                                # beside grid point 1 of 8
    o = R.decode([[near, 2.0]], [[500.0, 1e-6]], [[0.5, 0.5]], num=9)                      # finite at kappa 500, the flat one is cut
    assert o["n_modes"][0] == 1 and abs(o["angle"][0] - near) < 1e-6 and np.isfinite(o["heights"][0, 0])
    o = R.decode([[0.3, 2.0]], [[0.0, 0.0]], [[0.5, 0.5]], num=360)                        # flat
    assert o["n_modes"][0] == 0 and np.isnan(o["angle"][0])
    o = R.decode([[0.3, 2.0]], [[9.0, 9.0]], [[0.5, 0.5]], counts=[1], num=360)
    assert o["n_modes"][0] == 1 and abs(o["angle"][0] - 0.3) < 1e-6


def _acc(n_labels=1):
    from pnpp_hip.decode import STRIDE
    return np.zeros(n_labels * STRIDE + 1, np.int64)


def test_summary_median_and_p90_bin_edges():
    from pnpp_hip.decode import BINS, STRIDE, summarize
    a = _acc()
    a[0], a[3], a[19] = 5, 4, 1                      # top1: five errors in [0, 0.5), four in [1.5, 2), one in [9.5, 10)
    a[BINS + 44] = 10                                # cover: all ten in [22, 22.5)
    a[2 * BINS], a[2 * BINS + 1], a[2 * BINS + 2] = 10, 2, 9
    a[2 * BINS + 3], a[2 * BINS + 4] = 17_500_000, 222_000_000
    a[-1] = 12
    s = summarize(a, 1)
    o = s["overall"]
    assert s["samples"] == 12 and o == s["labels"][0]
    assert o["n"] == 10 and o["excluded"] == 2 and o["count_ok_rate"] == 9 / 12
    t = o["top1"]
    assert t["median"] == 0.5      # the 5th of 10 sorted errors is in bin 0: its upper edge
    assert t["p90"] == 2.0         # the 9th is in bin 3
    assert t["mean"] == 1.75
    assert t["within_5"] == 0.9 and t["within_10"] == 1.0 and t["within_22.5"] == 1.0
    c = o["cover"]
    assert c["median"] == 22.5 and c["p90"] == 22.5 and c["within_10"] == 0.0 and c["within_22.5"] == 1.0 and c["mean"] == 22.2
    a = _acc()
    a[7] = 11                                        # an odd count: the median is the 6th
    a[8] = 10
    a[2 * BINS] = 21
    t = summarize(a, 1)["overall"]["top1"]
    assert t["median"] == 4.0 and t["p90"] == 4.5    # ceil(10.5) = 11th is still bin 7; ceil(18.9) = 19th is bin 8
    a = _acc()
    a[BINS - 1] = 1                                  # 180 degrees sits in the last bin
    a[2 * BINS] = 1
    assert summarize(a, 1)["overall"]["top1"]["median"] == 180.0
    with pytest.raises(ValueError, match="expected n_labels"):
        summarize(np.zeros(STRIDE), 1)


def test_summary_empty_label_and_all_excluded():
    from pnpp_hip.decode import BINS, STRIDE, summarize
    a = _acc(3)
    a[2 * STRIDE + 2] = 4                            # label 2: four errors in [1, 1.5); label 0 empty; label 1 all excluded
    a[2 * STRIDE + BINS + 2] = 4
    a[2 * STRIDE + 2 * BINS] = 4
    a[2 * STRIDE + 2 * BINS + 3] = a[2 * STRIDE + 2 * BINS + 4] = 5_000_000
    a[STRIDE + 2 * BINS + 1] = 6
    a[-1] = 10
    s = summarize(a, 3)
    empty, excl, full = s["labels"]
    assert empty["n"] == 0 and empty["excluded"] == 0 and empty["count_ok_rate"] is None
    assert all(v is None for v in empty["top1"].values()) and all(v is None for v in empty["cover"].values())
    assert excl["n"] == 0 and excl["excluded"] == 6 and excl["count_ok_rate"] == 0.0 and excl["top1"]["median"] is None
    assert full["n"] == 4 and full["top1"]["median"] == 1.5 and full["top1"]["mean"] == 1.25 and full["top1"]["within_5"] == 1.0
    o = s["overall"]
    assert o["n"] == 4 and o["excluded"] == 6 and o["top1"]["p90"] == 1.5 and o["count_ok_rate"] == 0.0


P = 64   # a non-null pointer: validation never dereferences


def _dec(lib, mu=P, kappa=P, weight=P, counts=None, B=2, K=4, num=360, rel=0.1, modes=P, heights=P, n_modes=P, angle=P, density=None):
    return lib.pnpp_mvm_decode(mu, kappa, weight, counts, B, K, num, rel, modes, heights, n_modes, angle, density, None)


def _ev(lib, modes=P, n_modes=P, angle=P, B=2, K=4, mu_gt=None, kappa_gt=None, vm_gt=None, K_gt=None, Kmax=0, labels=None, n_labels=1,
        acc=P, sample_err=None, capacity=0, top1=None, cover=None, ok=None):
    return lib.pnpp_orient_eval(modes, n_modes, angle, B, K, mu_gt, kappa_gt, vm_gt, K_gt, Kmax, labels, n_labels, acc, sample_err,
                                capacity, top1, cover, ok, None)


def test_decode_argument_refusals(lib):
    from pnpp_hip import _lib
    E = _lib.PNPP_ERR_ARG
    assert lib.pnpp_abi_version() == 5
    for kw, words in (({"mu": None}, b"mvm_decode: null pointer"), ({"n_modes": None}, b"mvm_decode: null pointer"),
                      ({"B": 0}, b"B=0"), ({"K": 0}, b"K=0 (1 <= K <= 8)"), ({"K": 9}, b"K=9 (1 <= K <= 8)"),
                      ({"weight": None}, b"null weight takes K=1, got K=4"),
                      ({"num": 2}, b"num=2 (a grid of num - 1 points, 2 <= num - 1 <= 1024)"), ({"num": 1026}, b"num=1026"),
                      ({"rel": -0.5}, b"rel_height=-0.5"), ({"rel": 1.5}, b"rel_height=1.5")):
        assert _dec(lib, **kw) == E, kw
        assert words in lib.pnpp_last_error(), (kw, lib.pnpp_last_error())


def test_orient_eval_argument_refusals(lib):
    from pnpp_hip import _lib
    E = _lib.PNPP_ERR_ARG
    single, multi = {"mu_gt": P, "kappa_gt": P}, {"vm_gt": P, "K_gt": P, "Kmax": 4}
    for kw, words in (({"modes": None, **single}, b"orient_eval: null pointer"), ({"B": 0, **single}, b"B=0"),
                      ({"K": 9, **single}, b"K=9 (1 <= K <= 8)"), ({}, b"either mu_gt and kappa_gt or vm_gt and K_gt"),
                      ({**single, **multi}, b"either mu_gt and kappa_gt or vm_gt and K_gt"),
                      ({"mu_gt": P}, b"mu_gt and kappa_gt go together"), ({"vm_gt": P, "Kmax": 4}, b"vm_gt and K_gt go together"),
                      ({**multi, "Kmax": 9}, b"Kmax=9 (1 <= Kmax <= 8)"), ({**single, "acc": None}, b"no output requested"),
                      ({**single, "n_labels": 65}, b"n_labels=65 (1 <= n_labels <= 64)"), ({**single, "n_labels": 0}, b"n_labels=0"),
                      ({**single, "acc": None, "top1": P, "sample_err": P, "capacity": 8}, b"needs the accumulator"),
                      ({**single, "sample_err": P, "capacity": 0}, b"capacity=0")):
        assert _ev(lib, **kw) == E, kw
        assert words in lib.pnpp_last_error(), (kw, lib.pnpp_last_error())


def test_python_surface_refuses_before_any_launch():
    import torch
    from pnpp_hip import decode, ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decode.decode(torch.zeros(2, 4), torch.ones(2, 4), torch.full((2, 4), 0.25))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.orient_eval(torch.zeros(2, 4), torch.zeros(2, dtype=torch.int32), torch.zeros(2), mu_gt=torch.zeros(2), kappa_gt=torch.ones(2))
    with pytest.raises(ValueError, match="n_labels=65"):
        decode.AngularErrors(n_labels=65)
    assert decode.Orientation._fields == ("angle", "modes", "heights", "n_modes", "density")


def test_header_and_binding_agree_on_the_new_entries(lib):
    from pnpp_hip import _lib, build
    hdr = open(os.path.join(ROOT, "include", "pnpp_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    ctype = {"float": _lib._f, "int": _lib._i, "int64_t": _lib.C.c_int64}
    for name in ("pnpp_mvm_decode", "pnpp_orient_eval"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in include/pnpp_hip.h"
        params = [p.strip() for p in m.group(1).split(",")]
        want = [_lib._fp if "*" in p else ctype[p.split()[-2]] for p in params]
        res, args = _lib.SIGNATURES[name]
        assert res is _lib._i and args == want, name
        assert hasattr(lib, name)
    assert "decode_kernels.hip" in build.SOURCES
    for macro, value in (("PNPP_ORIENT_BINS", _lib.ORIENT_BINS), ("PNPP_ORIENT_STRIDE", _lib.ORIENT_STRIDE),
                         ("PNPP_ORIENT_MAX_LABELS", _lib.ORIENT_MAX_LABELS)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), hdr), macro


def test_seeded_cases_have_no_near_ties():
    """What the GPU tests rely on: on their seeded inputs float64 itself decides the order and the count of the modes for all but
    NEAR_TIE_CAP of the samples (here: for all of them)."""
    total = near = 0
    for B, K, num in R.SHAPES:
        o = R.decode(*R.random_case(B, K, R.case_seed(B, K, num)), num=num)
        total, near = total + B, near + int(o["near_tie"].sum())
        assert o["near_tie"].sum() <= R.NEAR_TIE_CAP * B, (B, K, num)
        assert (o["n_modes"] >= 1).all() and (o["n_modes"] <= K).all()
    assert total == 408 and near == 0
