"""Single-view scan simulation, what can be checked without a GPU: the C ABI's refusals and struct layout, the host-side validation,
the operator's DEFINITION (tests/view_ref.py, the numpy restatement) against ground truth it does not use -- analytic normals of
spheres and boxes --, the stream ids of the three families of draws, and the loader plumbing."""
import ctypes
import math
import os
import subprocess
import tempfile
import textwrap

import numpy as np
import pytest
import torch

import view_ref as vr
from conftest import ROOT


@pytest.fixture(scope="module")
def libpath():
    from pnpp_hip import build
    return build.build()


# ---- (a) refusals ---------------------------------------------------------------------------------------------------------
def _desc(L, **kw):
    d = L.ViewDesc()
    d.G, d.splat, d.thickness, d.elev_lo, d.elev_hi, d.drop, d.min_keep, d.flags = 32, 1, 0.1, -0.5, 1.0, 0.0, 1, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_errors_without_gpu(libpath):
    """Every refusal happens before a launch, so none of these touches a device."""
    from pnpp_hip import _lib as L
    h = L.lib()

    def call(d, xin=8, xout=16, lin=None, lout=24, idx=None, B_=2, N_=64, C_=3, params=32):
        return h.pnpp_view_clouds(1, 2, xin, xout, lin, lout, idx, B_, N_, C_, None if d is None else ctypes.byref(d), params, None)

    def refused(word, *a, **kw):
        assert call(*a, **kw) == L.PNPP_ERR_ARG
        assert word in h.pnpp_last_error(), h.pnpp_last_error()

    for name in ("xin", "xout", "lout", "params"):
        refused(b"null", _desc(L), **{name: None})
    refused(b"null", None)
    refused(b"out of place", _desc(L), xin=16, xout=16)
    for bad in (0, 1, 2, 4, 5, 7):
        refused(b"C=", _desc(L), C_=bad)
    for bad in (0, -1, 65536):
        refused(b"B=", _desc(L), B_=bad)
    for bad in (0, -5, 2 ** 24 + 1, 2 ** 32):
        refused(b"N=", _desc(L), N_=bad)
    for bad in (0, -1, 129):
        refused(b"G=", _desc(L, G=bad))
    for bad in (-1, 3):
        refused(b"splat", _desc(L, splat=bad))
    for bad in (-0.1, float("inf"), float("nan")):
        refused(b"thickness", _desc(L, thickness=bad))
    for lo, hi in ((0.5, 0.25), (-1.6, 0.0), (0.0, 1.6), (float("nan"), 1.0), (0.0, float("nan"))):
        refused(b"elevation", _desc(L, elev_lo=lo, elev_hi=hi))
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        refused(b"drop", _desc(L, drop=bad))
    for bad in (-1, 65):
        refused(b"min_keep", _desc(L, min_keep=bad))
    refused(b"unknown flag", _desc(L, flags=4))
    refused(b"not both", _desc(L, flags=3, view_dirs=40))
    refused(b"go together", _desc(L, flags=1))                   # the flag without the pointer
    refused(b"go together", _desc(L, view_dirs=40))              # the pointer without a flag


def test_view_desc_layout_matches_c(libpath):
    from pnpp_hip import _lib as L
    src = textwrap.dedent('''
        #include <stdio.h>
        #include <stddef.h>
        #include "pnpp_hip.h"
        int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(pnpp_view_desc), offsetof(pnpp_view_desc, drop), offsetof(pnpp_view_desc, flags),
                                offsetof(pnpp_view_desc, view_dirs)); return 0; }
    ''')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        sizes = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [ctypes.sizeof(L.ViewDesc), L.ViewDesc.drop.offset, L.ViewDesc.flags.offset, L.ViewDesc.view_dirs.offset]


def test_plan_refuses_what_the_library_refuses():
    from pnpp_hip import ops
    shape = (4, 100, 3)
    assert ops.view_plan(shape) == (10, 1, 0.1, ops.VIEW_ELEVATION, 0.0, 1, 0)
    assert [ops.view_resolution(n) for n in (1, 2, 4, 5, 1024, 1025, 16384, 10 ** 6)] == [1, 2, 2, 3, 32, 33, 128, 128]
    assert [vr.resolution(n) for n in (1, 2, 4, 5, 1024, 1025, 16384, 10 ** 6)] == [1, 2, 2, 3, 32, 33, 128, 128]
    assert ops.view_plan((4, 100, 6), resolution=128, splat=2, thickness=0.0, drop=0.5, min_keep=100)[:2] == (128, 2)
    assert ops.view_plan(shape, view_dirs=torch.zeros(4, 3))[-1] == 1 and ops.view_plan(shape, angles=torch.zeros(4, 2))[-1] == 2
    bad = [
        dict(xyz_shape=(4, 100, 4)), dict(xyz_shape=(4, 100)), dict(xyz_shape=(0, 100, 3)), dict(xyz_shape=(4, 0, 3)),
        dict(xyz_shape=(65536, 1, 3)), dict(xyz_shape=(1, 2 ** 24 + 1, 3)),
        dict(resolution=0), dict(resolution=129), dict(splat=-1), dict(splat=3), dict(splat=0.5),
        dict(thickness=-0.1), dict(thickness=float("inf")), dict(thickness=float("nan")),
        dict(elevation=(0.5, 0.25)), dict(elevation=(-2.0, 0.0)), dict(elevation=(0.0, 2.0)), dict(elevation=0.3),
        dict(drop=-0.1), dict(drop=1.0), dict(drop=float("nan")), dict(min_keep=-1), dict(min_keep=101),
        dict(lengths=torch.zeros(3, dtype=torch.int32)), dict(lengths=torch.zeros(4)), dict(lengths=[1, 2, 3, 4]),
        dict(view_dirs=torch.zeros(4, 2)), dict(view_dirs=torch.zeros(3, 3)), dict(view_dirs=torch.zeros(4, 3, dtype=torch.float64)),
        dict(angles=torch.zeros(4, 3)), dict(view_dirs=torch.zeros(4, 3), angles=torch.zeros(4, 2)),
    ]
    for kw in bad:
        kw = dict(kw)
        with pytest.raises(ValueError):
            ops.view_plan(kw.pop("xyz_shape", shape), **kw)


# ---- (b) the definition against independent ground truth ------------------------------------------------------------------
def _sphere(rng, n):
    p = rng.standard_normal((n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    return p.astype(np.float32), p


def _box(rng, n, half=(1.0, 0.6, 0.4)):
    """Uniform on the surface of a box: a face by its area, a point on it; the normal is the face's."""
    half = np.asarray(half)
    area = np.array([half[1] * half[2], half[0] * half[2], half[0] * half[1]])
    axis = rng.choice(3, n, p=area / area.sum())
    sign = rng.choice([-1.0, 1.0], n)
    p = rng.uniform(-1, 1, (n, 3)) * half
    nrm = np.zeros((n, 3))
    p[np.arange(n), axis] = sign * half[axis]
    nrm[np.arange(n), axis] = sign
    return p.astype(np.float32), nrm


def _quality(family, n, G, thickness, clouds=8, seed=0):
    rng = np.random.default_rng(seed)
    phi, eps = rng.uniform(0, 2 * np.pi, clouds), rng.uniform(-0.5, 1.0, clouds)
    v, r, u = vr.basis(np.cos(phi), np.sin(phi), np.cos(eps), np.sin(eps))
    back_kept, front_dropped, kept = [], [], []
    for b in range(clouds):
        pts, nrm = family(rng, n)
        mask, _ = vr.visible(pts, v[b], r[b], u[b], G, 1, thickness)
        facing = nrm @ v[b].astype(np.float64)
        front, back = facing > 0.15, facing < -0.15
        back_kept.append(mask[back].mean())
        front_dropped.append(1.0 - mask[front].mean())
        kept.append(mask.mean())
    return float(np.mean(back_kept)), float(np.mean(front_dropped)), (float(min(kept)), float(max(kept)))


@pytest.fixture(scope="module")
def quality():
    """The restatement on 8 spheres and 8 boxes of 1024 points, computed once."""
    return {"sphere": _quality(_sphere, 1024, 32, 0.1, seed=11), "box": _quality(_box, 1024, 32, 0.1, seed=12)}


def test_hidden_side_goes_and_facing_side_stays(quality):
    """N = 1024, resolution 32, splat 1, thickness 0.1, azimuth uniform, elevation in [-0.5, 1.0]; front is n . v > 0.15, back
    n . v < -0.15.  Gates: twice the figures of the sketch this operator was specified from (0.056 back kept, 0.144 front dropped)."""
    for name, (bk, fd, kept) in quality.items():
        print(f"{name}: back kept {bk:.4f}  front dropped {fd:.4f}  kept fraction {kept[0]:.3f} .. {kept[1]:.3f}")
    bk = np.mean([q[0] for q in quality.values()])
    fd = np.mean([q[1] for q in quality.values()])
    print(f"all 16: back kept {bk:.4f}  front dropped {fd:.4f}")
    assert bk <= 0.12 and fd <= 0.30
    for name, (b, f, _) in quality.items():
        assert b <= 0.12 and f <= 0.30, name


def test_restatement_properties():
    """Survivors keep their order, the padding is exact zeros and -1, a finer thickness keeps a subset, thickness 0 keeps each cell's
    nearest point, identical points all stay, the floor passes a cloud through, and thinning only ever removes."""
    rng = np.random.default_rng(3)
    pts, _ = _sphere(rng, 300)
    xyz = np.stack([pts, pts[::-1]])
    v, r, u = vr.basis(*(np.array([t, t]) for t in (math.cos(0.7), math.sin(0.7), math.cos(0.3), math.sin(0.3))))
    out, kept, idx, cell, passed = vr.view(xyz, v, r, u, G=16)
    assert not passed.any() and (kept > 60).all() and (kept < 240).all() and (cell > 0).all()
    for b in range(2):
        k = kept[b]
        assert (np.diff(idx[b, :k]) > 0).all() and (idx[b, k:] == -1).all() and not out[b, k:].any()
        assert out[b, :k].tobytes() == xyz[b, idx[b, :k]].tobytes()
    assert set(idx[0, :kept[0]]) == {299 - i for i in idx[1, :kept[1]]}          # the order of the rows does not decide who is seen
    thin_mask, _ = vr.visible(pts, v[0], r[0], u[0], 16, 1, 0.02)
    wide_mask, _ = vr.visible(pts, v[0], r[0], u[0], 16, 1, 0.1)
    assert (wide_mask | ~thin_mask).all() and thin_mask.sum() < wide_mask.sum()
    front, _ = vr.visible(pts, v[0], r[0], u[0], 16, 0, 0.0)
    assert 1 <= front.sum() <= 16 * 16
    same = np.tile(pts[:1], (50, 1))[None]
    o, k, i, c, p = vr.view(same, v[:1], r[:1], u[:1], G=8)
    assert k[0] == 50 and c[0] == 0 and not p[0] and o.tobytes() == same.tobytes()
    o, k, i, c, p = vr.view(xyz, v, r, u, G=16, min_keep=299)
    assert p.all() and (k == 300).all() and o.tobytes() == xyz.tobytes() and (i == np.arange(300)).all()
    o2, k2, i2, _, _ = vr.view(xyz, v, r, u, seed=5, stream_id=vr.STREAM_BASE | 1, G=16, drop=0.9)
    assert (k2 <= kept).all() and (k2 < kept).any()
    for b in range(2):
        assert set(i2[b, :k2[b]]) <= set(idx[b, :kept[b]])
    o0 = vr.view(xyz, v, r, u, seed=5, stream_id=vr.STREAM_BASE | 1, G=16, drop=0.0)
    assert o0[0].tobytes() == out.tobytes()


def test_drawn_directions():
    phi, eps = vr.drawn_angles(7, vr.STREAM_BASE | 1, 4096, (-0.5, 1.0))
    assert (phi >= 0).all() and (phi < 2 * np.pi).all() and (eps >= np.float32(-0.5)).all() and (eps < 1.0).all()
    assert abs(np.exp(1j * phi).mean()) <= 5.0 / math.sqrt(4096)
    assert abs(eps.mean() - 0.25) <= 5.0 * 1.5 / math.sqrt(12 * 4096)
    v, r, u = vr.basis(np.cos(phi), np.sin(phi), np.cos(eps), np.sin(eps))
    for a, b in ((v, r), (v, u), (r, u)):
        assert np.abs((a.astype(np.float64) * b).sum(1)).max() <= 4e-7
    assert np.abs(np.cross(u.astype(np.float64), r) - v).max() <= 4e-7         # u x r = v: orthonormal, v out of the image
    dirs = np.array([[0, 1, 0], [0, -2, 0], [0, 0, -1], [3, 0, 0], [0, 0, 0], [np.nan, 0, 1]], np.float32)
    vd, rd, ud = vr.basis(*vr.angles_of_dirs(dirs))
    want = np.array([[0, 1, 0], [0, -1, 0], [0, 0, -1], [1, 0, 0], [0, 0, -1], [0, 0, -1]], np.float32)
    assert np.abs(vd - want).max() == 0


# ---- (c) streams, (d) resampling and the plumbing -------------------------------------------------------------------------
def test_stream_ids_of_the_three_families_are_disjoint(monkeypatch):
    from pnpp_hip import augment, ops, views
    assert views.STREAM_BASE == vr.STREAM_BASE == 1 << 62 and views.RESAMPLE_BASE == vr.RESAMPLE_BASE == (1 << 62) | (1 << 61)
    assert augment.STREAM_BASE == 1 << 63
    seen = []
    monkeypatch.setattr(ops, "view_clouds", lambda xyz, seed, stream, *a, **k: seen.append(("view", stream)) or
                        (xyz, torch.ones(xyz.shape[0], dtype=torch.int32), torch.zeros(xyz.shape[0], 8)))
    monkeypatch.setattr(ops, "subsample_points", lambda seed, stream, bank, lengths, num: seen.append(("draw", stream)) or bank[:, :num])
    sv = views.SingleView(seed=3, resample=4)
    for _ in range(3):
        assert sv(torch.zeros(2, 9, 3)).shape == (2, 4, 3)
    assert sv.draws == 3 and sv.last_params.shape == (2, 8)
    assert seen == [(k, base | i) for i in (1, 2, 3) for k, base in (("view", 1 << 62), ("draw", (1 << 62) | (1 << 61)))]
    calls = [1, 2, 3, 1 << 20, (1 << 61) - 1]                       # the bank counts its draws up from 1, like the two others
    fam = {"bank": set(calls), "view": {views.STREAM_BASE | i for i in calls}, "resample": {views.RESAMPLE_BASE | i for i in calls},
           "augment": {augment.STREAM_BASE | i for i in calls}}
    names = list(fam)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert not fam[a] & fam[b], (a, b)
    top = lambda s: {x >> 61 for x in s}                            # the three top bits tell the families apart for every i < 2^61
    assert [top(fam[n]) for n in names] == [{0}, {2}, {3}, {4}]
    w = [vr.cloud_words(3, base | 1, 4)[0] for base in (0, views.STREAM_BASE, views.RESAMPLE_BASE, augment.STREAM_BASE)]
    assert len({x.tobytes() for x in w}) == 4


def test_resample_takes_xyz_only_and_refusals_count_no_draw():
    from pnpp_hip.views import SingleView
    sv = SingleView(resample=16)
    with pytest.raises(ValueError, match="resample"):
        sv.view(torch.zeros(2, 40, 6))
    with pytest.raises(ValueError):
        sv.view(torch.zeros(2, 40, 3), index=True)
    with pytest.raises(ValueError):
        SingleView(resample=0)
    with pytest.raises(ValueError):
        SingleView(elevation=(1.0, 0.0))
    with pytest.raises(ValueError):
        SingleView(drop=1.0)
    plain = SingleView(min_keep=32)
    with pytest.raises(ValueError):
        plain.view(torch.zeros(2, 16, 3))                           # min_keep above N
    with pytest.raises(ValueError):
        plain.view(torch.zeros(2, 40, 3), view_dirs=torch.zeros(3, 3))
    assert sv.draws == 0 and plain.draws == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        plain.view(torch.zeros(2, 40, 6))


class _StandInView:
    """Keeps the first half of every cloud; ragged unless resample is set."""

    def __init__(self, resample=None):
        self.resample, self.calls = resample, 0

    def __call__(self, xyz):
        self.calls += 1
        if self.resample is not None:
            return xyz[:, :self.resample] + 1.0
        half = xyz.clone()
        half[:, xyz.shape[1] // 2:] = 0
        return half, torch.full((xyz.shape[0],), xyz.shape[1] // 2, dtype=torch.int32)


class _StandInAugment:
    def __init__(self):
        self.lengths = []

    def __call__(self, xyz, *targets, kinds, counts=None, lengths=None):
        self.lengths.append(lengths)
        return (xyz * 2.0, *targets)


def test_view_loader_plumbing():
    from pnpp_hip import trainer
    xyz, mu = torch.rand(10, 6, 3), torch.rand(10, 2)
    plain = trainer.SyntheticLoader([xyz, mu], 4, False, "cpu")
    uniform = trainer.ViewLoader(plain, _StandInView(resample=3))
    assert len(uniform) == len(plain) == 3
    for got, want in zip(uniform, plain):
        assert len(got) == 3 and torch.equal(got[0], want[0][:, :3] + 1.0) and all(torch.equal(g, w) for g, w in zip(got[1:], want[1:]))
    ragged = list(trainer.ViewLoader(plain, _StandInView()))
    assert [len(b) for b in ragged] == [4, 4, 4] and ragged[2][-1].tolist() == [3, 3] and torch.equal(ragged[0][1], mu[:4])
    aug = _StandInAugment()
    both = list(trainer.AugmentedLoader(uniform, aug, ("vm",)))                 # the augmentation goes around the view
    assert torch.equal(both[0][0], (xyz[:4, :3] + 1.0) * 2.0)


def test_bank_loader_with_and_without_a_view():
    import dataloader_common as dc
    rng = np.random.default_rng(3)
    cl = [rng.standard_normal((n, 3)).astype(np.float32) for n in (15, 17, 17, 13, 16, 17)]
    mu = torch.arange(6, dtype=torch.float32)

    def loader(**kw):
        bank = dc.DeviceCloudBank(cl, "cpu", seed=1)
        bank.asked = []
        bank.sample = lambda ids, num: bank.asked.append(num) or bank.padded(ids)[0][:, :num]   # a CPU bank hands out its clouds
        return bank, dc.BankLoader(bank, [mu], 5, 4, True, seed=9, **kw)

    bank0, plain = loader()
    bank1, same = loader(view=None, view_points=99)
    plain, same = list(plain), list(same)
    assert bank0.asked == bank1.asked == [5, 5] and all(len(b) == 2 for b in plain)
    assert all(torch.equal(x, y) for a, b in zip(plain, same) for x, y in zip(a, b))
    bank2, viewed = loader(view=_StandInView(resample=5))
    viewed = list(viewed)
    assert bank2.asked == [10, 10]                                               # view_points defaults to 2 num_points
    order = torch.randperm(6, generator=torch.Generator().manual_seed(9))
    assert torch.equal(viewed[0][0], bank2.padded(order[:4])[0][:, :5] + 1.0) and torch.equal(viewed[0][1], mu[order[:4]])
    aug = _StandInAugment()
    bank3, ragged = loader(view=_StandInView(), view_points=12, augment=aug, kinds=("angle",))
    ragged = list(ragged)
    assert bank3.asked == [12, 12] and [len(b) for b in ragged] == [3, 3]
    assert ragged[0][2].tolist() == [6] * 4 and ragged[1][2].tolist() == [6] * 2 and all(l is b[2] for l, b in zip(aug.lengths, ragged))
    assert not ragged[0][0][:, 6:].any() and ragged[0][0][:, :6].abs().sum() > 0
    with pytest.raises(ValueError):
        loader(view=_StandInView(resample=7))                                    # resample must be num_points
    with pytest.raises(ValueError):
        loader(view=_StandInView(), normals=4)                                   # normals need the uniform batch


def test_scripts_take_the_views_switch(monkeypatch):
    import train_8dir_KL
    import train_multi_peaks_vonMises_KL
    import train_single_peak_vonMises_KL
    for mod in (train_single_peak_vonMises_KL, train_multi_peaks_vonMises_KL, train_8dir_KL):
        monkeypatch.delenv("PNPP_VIEWS", raising=False)
        assert mod._parser().parse_args([]).views is False
        assert mod._parser().parse_args(["--views", "--synthetic", "64"]).views is True
        assert mod._parser().parse_args(["--views", "--augment"]).augment is True
        monkeypatch.setenv("PNPP_VIEWS", "1")
        assert mod._parser().parse_args([]).views is True
