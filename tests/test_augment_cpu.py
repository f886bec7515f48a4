"""Device-side yaw augmentation, what can be checked without a GPU: the conventions on the CPU restatement (tests/augment_ref.py:
a target moved by the rule equals the target recomputed from the rotated axis), the float32 rotation's error bound, the seeds the
GPU tests use, the C ABI's argument checks and struct layout, and the host-side validation and loader plumbing."""
import ctypes
import math
import os
import subprocess
import tempfile
import textwrap

import numpy as np
import pytest
import torch

import augment_ref as ar
from conftest import ROOT

SEED, STREAM = 20240611, ar.STREAM_BASE | 1      # the seeds of tests/test_gpu_augment.py
B, N = 64, 257


@pytest.fixture(scope="module")
def clouds():
    import synthetic
    xyz, mu, kappa, fwd = synthetic.rotated_clouds(B, N, seed=5)
    th, c, s, _ = ar.cloud_params(SEED, STREAM, B)
    return {"xyz": xyz.numpy(), "mu": mu.numpy(), "kappa": kappa.numpy(), "fwd": fwd.numpy(), "th": th, "c": c, "s": s}


def _mu_of_axis(f):
    f = np.asarray(f, np.float64)
    return np.arctan2(f[..., 0], -f[..., 2])


def _axis_f64(f, th):
    """R f in float64 with the exact angle."""
    f = np.asarray(f, np.float64)
    c, s = np.cos(th), np.sin(th)
    return np.stack([c * f[:, 0] + s * f[:, 2], f[:, 1], c * f[:, 2] - s * f[:, 0]], 1)


def test_angle_rule_equals_recomputation(clouds):
    """mu' = wrap(mu - theta) is atan2 of the rotated forward axis, to the float32 rounding of the input mu."""
    got = ar.shift_angles(clouds["mu"], clouds["th"])
    want = _mu_of_axis(_axis_f64(clouds["fwd"], clouds["th"]))
    err = ar.angular_distance(got, want).max()
    print("single peak: max angular distance", err)
    assert err <= 1e-6
    assert (got > -np.pi).all() and (got <= np.float32(np.pi)).all()
    vm = ar.vm_table(np.stack([clouds["mu"], clouds["kappa"]], 1), clouds["th"])
    assert vm[:, 0].tobytes() == got.tobytes() and vm[:, 1].tobytes() == clouds["kappa"].tobytes()


@pytest.mark.parametrize("K", [0, 1, 2, 4])
def test_multi_peak_rule_equals_recomputation(clouds, K):
    import synthetic
    counts = np.full(B, K)
    vm = synthetic.multi_peak_gt(torch.from_numpy(clouds["fwd"]), torch.from_numpy(counts)).numpy()
    got = ar.vm_table(vm, clouds["th"], counts)
    rotated = torch.from_numpy(_axis_f64(clouds["fwd"], clouds["th"]).astype(np.float32))
    want = synthetic.multi_peak_gt(rotated, torch.from_numpy(counts)).numpy()
    err = ar.angular_distance(got[:, :K, 0], want[:, :K, 0]).max() if K else 0.0
    print("multi peak K =", K, "max angular distance", err)
    assert err <= 1e-6
    assert got[:, :, 1:].tobytes() == vm[:, :, 1:].tobytes()                     # kappa and weight are copied
    assert got[:, K:].tobytes() == vm[:, K:].tobytes() and not got[:, K:].any()   # the zero padding stays exact zeros


def test_dir8_labels_from_rotated_axis(clouds):
    import synthetic
    from models.pointnet_pp_8dir import DIRS_8
    f = clouds["fwd"].copy()
    f[7] = 0.0                                                     # a symmetric class: no forward axis
    got = ar.dir8(f, clouds["c"], clouds["s"], DIRS_8.numpy())
    assert np.abs(got.astype(np.float64).sum(1) - 1.0).max() <= 2e-7
    assert got[7].tobytes() == np.full(8, 0.125, np.float32).tobytes()
    keep = np.arange(B) != 7
    want = synthetic.dir8_soft_labels(torch.from_numpy(_axis_f64(f, clouds["th"])), DIRS_8.double()).numpy()
    assert np.abs(got[keep] - want[keep]).max() <= 1e-6


def test_float32_rotation_error_bound(clouds):
    """Three roundings (two products, one sum) of at most 2^-24 relative each plus the rounding of c and s (2^-25 absolute each,
    |c|, |s| <= 1): |x' - exact| <= 2^-23 (|x| + |z|), at every element; the same for z'."""
    x, z = clouds["xyz"][..., 0], clouds["xyz"][..., 2]
    gx, gz = ar.rotate_f32(clouds["c"][:, None], clouds["s"][:, None], x, z)
    c, s = np.cos(clouds["th"])[:, None], np.sin(clouds["th"])[:, None]
    x64, z64 = x.astype(np.float64), z.astype(np.float64)
    bound = 2.0 ** -23 * (np.abs(x64) + np.abs(z64))
    ex, ez = np.abs(gx - (c * x64 + s * z64)), np.abs(gz - (c * z64 - s * x64))
    print("rotation: max error", max(ex.max(), ez.max()), "bound at that scale", bound.max())
    assert (ex <= bound).all() and (ez <= bound).all()
    assert np.abs(clouds["c"] - np.cos(clouds["th"])).max() <= 2.0 ** -24 and np.abs(clouds["s"] - np.sin(clouds["th"])).max() <= 2.0 ** -24


def test_seeds_give_uniform_angles_and_both_wrap_cases(clouds):
    th = ar.theta(SEED, STREAM, 4096)
    assert (th >= 0).all() and (th < 2 * np.pi).all()
    for h in (1, 2):
        r = abs(np.exp(1j * h * th).mean())
        print("harmonic", h, "mean resultant length", r)
        assert r <= 5.0 / math.sqrt(4096)
    wraps = clouds["mu"].astype(np.float64) - clouds["th"] <= -np.pi
    assert wraps.any() and (~wraps).any()
    assert not np.array_equal(ar.theta(SEED, STREAM, 8), ar.theta(SEED, 1, 8))   # a bank draw of the same number: other words


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pnpp_hip import build, _lib
    build.build()
    return _lib


def _desc(L, flags=1, n_targets=0):
    d = L.AugmentDesc()
    d.flags, d.scale_lo, d.scale_hi, d.sigma, d.clip, d.n_targets = flags, 0.8, 1.25, 0.01, 0.05, n_targets
    for t in d.targets:
        t.kind, t.rows, t.cols, t.inp, t.out = L.AUG_ANGLE, 1, 1, 8, 16
    return d


def test_argument_errors_without_gpu(lib):
    """Every refusal happens before a launch, so none of these touches a device."""
    L, h = lib, lib.lib()

    def call(d, xin=8, xout=16, B_=2, N_=4, C_=3, params=32):
        return h.pnpp_augment_clouds(1, 2, xin, xout, None, B_, N_, C_, None if d is None else ctypes.byref(d), params, None)

    assert call(_desc(L), xin=None) == L.PNPP_ERR_ARG and b"null" in h.pnpp_last_error()
    assert call(_desc(L), xout=None) == L.PNPP_ERR_ARG
    assert call(_desc(L), params=None) == L.PNPP_ERR_ARG
    assert call(None) == L.PNPP_ERR_ARG
    for bad_c in (0, 4, 5, 7):
        assert call(_desc(L), C_=bad_c) == L.PNPP_ERR_ARG
    assert b"C=" in h.pnpp_last_error()
    assert call(_desc(L, n_targets=5)) == L.PNPP_ERR_ARG and b"n_targets" in h.pnpp_last_error()
    d = _desc(L, n_targets=2)
    d.targets[1].kind = 4
    assert call(d) == L.PNPP_ERR_ARG and b"kind" in h.pnpp_last_error()
    d = _desc(L, n_targets=1)
    d.targets[0].inp = None
    assert call(d) == L.PNPP_ERR_ARG
    d = _desc(L, n_targets=1)
    d.targets[0].kind = L.AUG_DIR8                                    # dirs8 missing
    d.targets[0].cols = 3
    assert call(d) == L.PNPP_ERR_ARG
    for lo, hi in ((1.25, 0.8), (0.0, 1.0), (-1.0, 1.0), (float("nan"), 1.0)):
        d = _desc(L, flags=L.AUG_YAW | L.AUG_SCALE)
        d.scale_lo, d.scale_hi = lo, hi
        assert call(d) == L.PNPP_ERR_ARG and b"scale" in h.pnpp_last_error()
    for sigma, clip in ((-0.01, 0.05), (0.01, -0.05)):
        d = _desc(L, flags=L.AUG_YAW | L.AUG_JITTER)
        d.sigma, d.clip = sigma, clip
        assert call(d) == L.PNPP_ERR_ARG and b"jitter" in h.pnpp_last_error()
    assert call(_desc(L, flags=8)) == L.PNPP_ERR_ARG
    assert call(_desc(L), N_=2 ** 32 - 1) == L.PNPP_ERR_ARG and b"32 bits" in h.pnpp_last_error()
    assert call(_desc(L), N_=2 ** 32) == L.PNPP_ERR_ARG
    assert call(_desc(L), N_=0) == L.PNPP_ERR_ARG and call(_desc(L), B_=0) == L.PNPP_ERR_ARG


def test_augment_desc_layout_matches_c(lib):
    src = textwrap.dedent('''
        #include <stdio.h>
        #include "pnpp_hip.h"
        int main(void) { printf("%zu %zu\\n", sizeof(pnpp_augment_desc), sizeof(pnpp_augment_target)); return 0; }
    ''')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        sizes = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [ctypes.sizeof(lib.AugmentDesc), ctypes.sizeof(lib.AugmentTarget)]


# ---- host-side validation and plumbing -----------------------------------------------------------------------------------
def test_plan_refuses_mismatches():
    from pnpp_hip import ops
    xyz = torch.zeros(4, 9, 3)
    ok = ops.augment_plan(xyz.shape, [torch.zeros(4), torch.zeros(4, 2), torch.zeros(4, 4, 3), torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64)],
                          ["angle", "vm", "vm", "dir8", "keep"])
    assert [None if p is None else p[:4] for p in ok] == [(0, 1, 1, (4,)), (1, 1, 2, (4, 2)), (1, 4, 3, (4, 4, 3)), (3, 1, 3, (4, 8)), None]
    bad = [
        (torch.zeros(4, 9, 4).shape, [], []),                               # C
        (torch.zeros(4, 9).shape, [], []),
        (xyz.shape, [torch.zeros(4)], []),                                  # one kind per target
        (xyz.shape, [torch.zeros(4)], ["yaw"]),                             # unknown kind
        (xyz.shape, [torch.zeros(5)], ["angle"]),                           # batch size
        (xyz.shape, [torch.zeros(4, 3)], ["vm"]),                           # (B,3) is no [mu, kappa] row
        (xyz.shape, [torch.zeros(4, 2, 4)], ["vm"]),
        (xyz.shape, [torch.zeros(4, 2)], ["axis"]),
        (xyz.shape, [torch.zeros(4, 2, 3)], ["dir8"]),
        (xyz.shape, [torch.zeros(4, 2, 2)], ["angle"]),
        (xyz.shape, [torch.zeros(4, dtype=torch.float64)], ["angle"]),
        (xyz.shape, [torch.zeros(4)] * 5, ["angle"] * 5),                   # more than one launch takes
    ]
    for shape, targets, kinds in bad:
        with pytest.raises(ValueError):
            ops.augment_plan(shape, targets, kinds)
    with pytest.raises(ValueError):
        ops.augment_plan(xyz.shape, [torch.zeros(4, 4, 3)], ["vm"], counts=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.augment_plan(xyz.shape, [torch.zeros(4, 4, 3)], ["vm"], counts=[None, None])
    for scale in ((1.25, 0.8), (0.0, 1.0)):
        with pytest.raises(ValueError):
            ops.augment_plan(xyz.shape, [], [], scale=scale)
    for jitter in ((-0.01, 0.05), (0.01, -1.0)):
        with pytest.raises(ValueError):
            ops.augment_plan(xyz.shape, [], [], jitter=jitter)


def test_augment_object_validates_on_the_host_and_needs_a_gpu():
    from pnpp_hip.augment import Augment, STREAM_BASE
    assert STREAM_BASE == ar.STREAM_BASE
    with pytest.raises(ValueError):
        Augment(scale=(2.0, 1.0))
    a = Augment(seed=3)
    with pytest.raises(ValueError):
        a(torch.zeros(2, 5, 3), torch.zeros(3), kinds=("angle",))
    assert a.draws == 0                                              # a refused call draws nothing
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        a(torch.zeros(2, 5, 3), torch.zeros(2), kinds=("angle",))


class _StandIn:
    """Records what a loader hands to its augmentation and marks the cloud."""

    def __init__(self):
        self.calls = []

    def __call__(self, xyz, *targets, kinds, counts=None, lengths=None):
        self.calls.append((kinds, counts, tuple(t.shape for t in targets)))
        return (xyz + 1.0, *targets)


def test_augmented_loader_plumbing():
    from pnpp_hip import trainer
    xyz, vm, K = torch.rand(10, 6, 3), torch.rand(10, 4, 3), torch.arange(10) % 3
    plain = trainer.SyntheticLoader([xyz, vm, K], 4, False, "cpu")
    aug = _StandIn()
    wrapped = trainer.AugmentedLoader(plain, aug, ("vm", "keep"), counts=1)
    assert len(wrapped) == len(plain) == 3
    for got, want in zip(wrapped, plain):
        assert len(got) == 4 and torch.equal(got[0], want[0] + 1.0)
        assert all(torch.equal(g, w) for g, w in zip(got[1:], want[1:]))
    assert [c[0] for c in aug.calls] == [("vm", "keep", "keep")] * 3           # the labels column is kept
    assert torch.equal(aug.calls[0][1], K[:4]) and aug.calls[2][2] == ((2, 4, 3), (2,), (2,))
    with pytest.raises(ValueError):
        list(trainer.AugmentedLoader(plain, aug, ("vm",)))                     # a target without a kind


def test_bank_loader_without_augment_is_unchanged():
    import dataloader_common as dc
    rng = np.random.default_rng(3)
    cl = [rng.standard_normal((n, 3)).astype(np.float32) for n in (5, 7, 7, 3, 6, 7)]
    mu = torch.arange(6, dtype=torch.float32)

    def loader(**kw):
        bank = dc.DeviceCloudBank(cl, "cpu", seed=1)
        bank.sample = lambda ids, num: bank.padded(ids)[0][:, :num]           # a CPU bank hands out its clouds, not a draw
        return dc.BankLoader(bank, [mu], 7, 4, True, seed=9, **kw)

    plain, same = list(loader()), list(loader(augment=None, kinds=None))
    assert len(plain) == 2 and [len(b) for b in plain] == [2, 2]
    order = torch.randperm(6, generator=torch.Generator().manual_seed(9))
    for i, (a, b) in enumerate(zip(plain, same)):
        ids = order[4 * i:4 * i + 4]
        assert torch.equal(a[1], mu[ids]) and all(torch.equal(x, y) for x, y in zip(a, b))
    aug = _StandIn()
    marked = list(loader(augment=aug, kinds=("angle",)))
    assert all(torch.equal(m[0], p[0] + 1.0) and torch.equal(m[1], p[1]) for m, p in zip(marked, plain))
    assert [c[0] for c in aug.calls] == [("angle",)] * 2
    with pytest.raises(ValueError):
        loader(augment=aug)                                                    # kinds missing


def test_scripts_take_the_augment_switch(capsys):
    import train_8dir_KL
    import train_multi_peaks_vonMises_KL
    import train_single_peak_vonMises_KL
    for mod in (train_single_peak_vonMises_KL, train_multi_peaks_vonMises_KL, train_8dir_KL):
        assert mod._parser().parse_args([]).augment is False
        assert mod._parser().parse_args(["--augment", "--synthetic", "64"]).augment is True
        assert mod._parser().parse_args(["--augment"]).synthetic == 0
    with pytest.raises(SystemExit):
        train_8dir_KL.main(["--augment"])                                      # dataset mode: the label files carry no axis
    assert "forward axis" in capsys.readouterr().err
