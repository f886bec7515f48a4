"""Orientation decoding and angular errors on the GPU (csrc/decode_kernels.hip through pnpp_hip.decode) against their float64
restatement tests/decode_ref.py.

Gates (they come from the number formats, not from the kernel):
  density   |got - ref| <= 1.2e-7 |ref| + 1e-12       one rounding of a float64 value to float32
  n_modes, order of the modes                         exact
  mode angles, on the circle: 5e-7 rad                1.2e-7 for the float32 rounding of an angle up to pi, the rest for value
                                                      sectioning's own resolution (flat top of a density at float64: ~5e-8 rad)
  heights   1e-6 relative
A sample is left out only where decode_ref itself reports a near-tie (NEAR_TIE_CAP of the samples at most)."""
import math

import numpy as np
import pytest
import torch

import decode_ref as R

pytestmark = pytest.mark.gpu

ANGLE_TOL, HEIGHT_TOL = 5e-7, 1e-6


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype).cuda()


def _circ(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return np.minimum(d, 2 * math.pi - d)


def _check_decode(mu, kappa, weight, counts=None, num=360, rel_height=0.1, what=""):
    """One decode call against the restatement; returns (device Orientation, restatement)."""
    from pnpp_hip import decode
    ref = R.decode(mu, kappa, weight, counts, num, rel_height)
    dref = R.density(mu, kappa, weight, counts, num)
    got = decode.decode(_dev(mu), _dev(kappa), _dev(weight), _dev(counts, torch.int32), num=num, rel_height=rel_height, density=True)
    torch.cuda.synchronize()
    B, K = np.shape(mu)
    dens = got.density.cpu().double().numpy()
    assert dens.shape == (B, num - 1) and got.modes.shape == (B, K) and got.n_modes.dtype == torch.int32
    derr = np.abs(dens - dref) - (1.2e-7 * np.abs(dref) + 1e-12)
    print(f"  {what} B={B} K={K} num={num}: density excess {derr.max():.2e}", end="")
    assert derr.max() <= 0.0
    keep = ~ref["near_tie"]
    assert (~keep).sum() <= R.NEAR_TIE_CAP * B, "decode_ref reports too many near-ties for these inputs"
    n = got.n_modes.cpu().numpy()
    modes, heights, angle = got.modes.cpu().double().numpy(), got.heights.cpu().double().numpy(), got.angle.cpu().double().numpy()
    assert np.array_equal(n[keep], ref["n_modes"][keep]), (n, ref["n_modes"])
    used = np.arange(K)[None, :] < ref["n_modes"][:, None]
    assert np.isnan(modes[~used & keep[:, None]]).all() and (heights[~used & keep[:, None]] == 0.0).all()
    sel = used & keep[:, None]
    aerr = _circ(modes[sel], ref["modes"][sel]).max() if sel.any() else 0.0
    herr = (np.abs(heights[sel] - ref["heights"][sel]) / ref["heights"][sel]).max() if sel.any() else 0.0
    print(f"  angle {aerr:.2e} rad  height {herr:.2e} rel")
    assert aerr <= ANGLE_TOL and herr <= HEIGHT_TOL
    assert np.array_equal(np.isnan(angle), n == 0)
    has = n > 0
    assert np.array_equal(angle[has], modes[has, 0])
    inside = modes[sel]
    assert (inside > -math.pi - 1e-6).all() and (inside <= math.pi + 1e-6).all()
    return got, ref


@pytest.mark.parametrize("B,K,num", R.SHAPES)
def test_decode_random_mixtures(B, K, num):
    mu, kappa, weight = R.random_case(B, K, R.case_seed(B, K, num))
    _check_decode(mu, kappa, weight, num=num, what="random")


def test_decode_hand_made_rows():
    f = np.float32
    on_grid = R.grid(360)[100]
    mu = f([[0.0, math.pi], [on_grid, 1.0], [1.0, 1.2], [0.3, 2.0], [-3.0, 3.0]])
    kappa = f([[20.0, 20.0], [30.0, 5.0], [8.0, 8.0], [0.0, 0.0], [400.0, 400.0]])
    weight = f([[0.6, 0.4], [1.0, 0.0], [0.5, 0.5], [0.5, 0.5], [0.3, 0.7]])
    got, ref = _check_decode(mu, kappa, weight, num=360, what="hand-made")
    assert ref["n_modes"].tolist() == [2, 1, 1, 0, 2]
    m = got.modes.cpu().numpy()
    assert abs(m[0, 0]) < 1e-6 and abs(abs(m[0, 1]) - math.pi) < 1e-6           # a peak at 0 and one at pi: the wrap
    assert abs(m[1, 0] - on_grid) < 1e-6                                         # a peak exactly on a grid point
    assert abs(m[2, 0] - 1.1) < 1e-5                                             # 0.2 rad apart at kappa 8: merged
    assert math.isnan(float(got.angle[3])) and int(got.n_modes[3]) == 0          # flat
    assert abs(m[4, 0] - 3.0) < 1e-4 and abs(m[4, 1] + 3.0) < 1e-4               # both sides of the cut at +-pi, the heavier first
    # kappa = 500 beside grid point 1 of 8, and a component that is flat to 1e-6: finite, and the flat one's mode is cut
    near = math.pi / 4 + 0.01
    got, ref = _check_decode(f([[near, 2.0]]), f([[500.0, 1e-6]]), f([[0.5, 0.5]]), num=9, what="kappa 500")
    assert ref["n_modes"].tolist() == [1] and abs(float(got.angle[0]) - near) < 1e-6
    assert torch.isfinite(got.density).all() and torch.isfinite(got.heights).all()
    # counts < K: the components beyond the count are not there
    mu, kappa, weight = R.random_case(5, 4, 77)
    counts = np.int32([1, 2, 3, 4, 0])
    got, ref = _check_decode(mu, kappa, weight, counts, num=65, what="counts")
    assert int(got.n_modes[4]) == 0 and float(got.density[4].abs().max()) == 0.0
    one, _ = _check_decode(mu[:1, :1], kappa[:1, :1], weight[:1, :1], num=65, what="counts=1 alone")
    assert torch.equal(one.modes[0, 0], got.modes[0, 0]) and torch.equal(one.density[0], got.density[0])


def test_decode_null_weight_is_the_single_peak_model():
    from pnpp_hip import decode
    mu, kappa, _ = R.random_case(33, 1, 5)
    got, ref = _check_decode(mu, kappa, None, num=360, what="null weight")
    assert ref["n_modes"].tolist() == [1] * 33
    assert float(_circ(got.angle.cpu().numpy(), mu[:, 0]).max()) <= ANGLE_TOL       # the mode of one von Mises is its mu
    flat = decode.decode(_dev(mu[:, 0]), _dev(kappa[:, 0]))                            # (B,) inputs: the single-peak head's outputs
    assert flat.modes.shape == (33, 1) and torch.equal(flat.angle, got.angle) and flat.density is None
    with pytest.raises(ValueError, match="null weight takes K=1"):
        decode.decode(_dev(np.zeros((2, 4), np.float32)), _dev(np.ones((2, 4), np.float32)))
    with pytest.raises(ValueError, match="num=2000"):
        decode.decode(_dev(mu), _dev(kappa), num=2000)


# ---- orient_eval ------------------------------------------------------------------------------------------------------------
def _eval_inputs(B=270, K=4, n_labels=64, seed=11):
    """Decoded random mixtures (on the device) with a multi-peak ground truth: K_gt in 0..4, some symmetric samples (every kappa 0),
    labels 0..63; samples whose errors sit within 1e-3 degrees of a histogram bin edge are left out (float64 decides their bin)."""
    from pnpp_hip import decode
    rng = np.random.default_rng(seed)
    mu, kappa, weight = R.random_case(B, K, seed)
    vm_gt = np.zeros((B, K, 3), np.float32)
    K_gt = rng.integers(0, K + 1, B).astype(np.int32)
    # ground truth near the predicted components (small errors) for half of the samples, anywhere for the rest
    vm_gt[:, :, 0] = np.where(rng.random((B, 1)) < 0.5, mu + rng.normal(0, 0.05, (B, K)), rng.uniform(-math.pi, math.pi, (B, K)))
    vm_gt[:, :, 1] = 8.0
    vm_gt[rng.random(B) < 0.1, :, 1] = 0.0
    vm_gt[:, :, 2] = 1.0 / K
    labels = (np.arange(B) % n_labels).astype(np.int32)
    ori = decode.decode(_dev(mu), _dev(kappa), _dev(weight))
    host = {k: getattr(ori, k).cpu().numpy() for k in ("modes", "n_modes", "angle")}
    ref = R.orient_eval(host["modes"], host["n_modes"], host["angle"], vm_gt=vm_gt, K_gt=K_gt, labels=labels, n_labels=n_labels)
    keep = ref["edge"] >= 1e-3
    assert (~keep).sum() <= R.NEAR_TIE_CAP * B
    sel = torch.as_tensor(keep).cuda()
    ori = decode.Orientation(ori.angle[sel], ori.modes[sel].contiguous(), ori.heights[sel].contiguous(), ori.n_modes[sel], None)
    vm_gt, K_gt, labels = vm_gt[keep], K_gt[keep], labels[keep]
    ref = R.orient_eval(host["modes"][keep], host["n_modes"][keep], host["angle"][keep], vm_gt=vm_gt, K_gt=K_gt, labels=labels,
                        n_labels=n_labels)
    return ori, _dev(vm_gt), _dev(K_gt), _dev(labels), ref


def _same_counts(acc, ref_acc, n_labels, n):
    """Every count exact; the two micro-degree sums to one unit per sample (they round a float64 product)."""
    from pnpp_hip.decode import BINS, STRIDE
    got, ref = np.asarray(acc, np.int64), np.asarray(ref_acc).astype(np.int64)
    sums = np.zeros(got.size, bool)
    for l in range(n_labels):
        sums[l * STRIDE + 2 * BINS + 3: l * STRIDE + 2 * BINS + 5] = True
    assert np.array_equal(got[~sums], ref[~sums])
    assert np.abs(got[sums] - ref[sums]).max() <= n


def test_orient_eval_errors_and_accumulator():
    from pnpp_hip import decode, ops
    from pnpp_hip.decode import STRIDE
    ori, vm_gt, K_gt, labels, ref = _eval_inputs()
    n = ori.modes.size(0)
    assert n > 256                                                                # more than one pass of the workgroup
    top1, cover, ok = ops.orient_eval(ori.modes, ori.n_modes, ori.angle, vm_gt=vm_gt, K_gt=K_gt)
    t, c = top1.cpu().double().numpy(), cover.cpu().double().numpy()
    excl = ref["top1"] < 0
    assert 0 < excl.sum() < n
    print(f"  orient_eval n={n} excluded={excl.sum()}: top1 {np.abs(t - ref['top1']).max():.2e} cover {np.abs(c - ref['cover']).max():.2e} deg")
    assert np.array_equal(t < 0, excl) and (t[excl] == -1.0).all() and (c[excl] == -1.0).all()
    assert np.abs(t - ref["top1"]).max() <= 1e-4 and np.abs(c - ref["cover"]).max() <= 1e-4
    assert np.array_equal(ok.cpu().numpy(), ref["count_ok"])

    m = decode.AngularErrors(n_labels=64, capacity=n + 7)
    m.update(ori, vm_gt=vm_gt, K_gt=K_gt, labels=labels)
    first = m.counts().copy()
    _same_counts(first, ref["acc"], 64, n)
    rows = m.sample_errors()
    assert rows.shape == (n, 2) and torch.equal(rows[:, 0], top1) and torch.equal(rows[:, 1], cover)
    s = m.summary()
    assert s["samples"] == n and s["overall"]["n"] == int((~excl).sum()) and s["overall"]["excluded"] == int(excl.sum())
    assert sum(e["n"] for e in s["labels"]) == s["overall"]["n"] and all(e["n"] + e["excluded"] > 0 for e in s["labels"])
    assert s["overall"]["count_ok_rate"] == float(ref["count_ok"].mean())
    assert abs(s["overall"]["top1"]["mean"] - ref["top1"][~excl].mean()) < 1e-4
    med = float(np.median(ref["top1"][~excl]))
    assert s["overall"]["top1"]["median"] - 0.5 <= med <= s["overall"]["top1"]["median"] + 0.5

    m.update(ori, vm_gt=vm_gt, K_gt=K_gt, labels=labels)                          # two updates add; the buffer overflows by n - 7 rows
    twice = m.counts()
    assert np.array_equal(twice, 2 * first)
    assert m.sample_errors().shape == (n + 7, 2) and torch.equal(m.sample_errors()[n:], rows[:7])
    m.reset()
    assert not m.counts().any() and m.sample_errors().shape == (0, 2)
    m.update(ori, vm_gt=vm_gt, K_gt=K_gt, labels=labels)                          # two runs are bit-identical
    assert np.array_equal(m.counts(), first) and torch.equal(m.sample_errors(), rows)
    assert first.size == 64 * STRIDE + 1

    out_of_table = decode.AngularErrors(n_labels=2)                               # a label outside the table is clamped into it
    out_of_table.update(ori, vm_gt=vm_gt, K_gt=K_gt, labels=labels)
    s2 = out_of_table.summary()
    assert s2["overall"] == s["overall"] and s2["labels"][0]["n"] + s2["labels"][0]["excluded"] == int((labels == 0).sum())


def test_orient_eval_single_peak_ground_truth():
    from pnpp_hip import decode
    B = 40
    mu, kappa, _ = R.random_case(B, 1, 21)
    rng = np.random.default_rng(6)
    mu_gt = (mu[:, 0] + rng.normal(0, 0.2, B)).astype(np.float32)
    kappa_gt = np.where(np.arange(B) % 5 == 0, 0.0, 8.0).astype(np.float32)          # every fifth sample is a symmetric class
    ori = decode.decode(_dev(mu[:, 0]), _dev(kappa[:, 0]))
    ref = R.orient_eval(ori.modes.cpu().numpy(), ori.n_modes.cpu().numpy(), ori.angle.cpu().numpy(), mu_gt=mu_gt, kappa_gt=kappa_gt)
    assert (ref["edge"] >= 1e-3).all()
    m = decode.AngularErrors(capacity=B)
    m.update(ori, mu_gt=_dev(mu_gt), kappa_gt=_dev(kappa_gt))
    _same_counts(m.counts(), ref["acc"], 1, B)
    e = m.sample_errors().cpu().double().numpy()
    assert np.abs(e[:, 0] - ref["top1"]).max() <= 1e-4 and np.array_equal(e[:, 0], e[:, 1])   # one mode, one target: cover = top1
    s = m.summary()["overall"]
    assert s["excluded"] == 8 and s["n"] == 32 and s["count_ok_rate"] == 1.0
    with pytest.raises(ValueError, match="either mu_gt and kappa_gt or vm_gt and K_gt"):
        m.update(ori)


# ---- the layers above -----------------------------------------------------------------------------------------------------------
def _seeded(cls, seed=5):
    torch.manual_seed(seed)
    m = cls()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.startswith("head_"):   # the multi-peak heads start at zero: every component would sit at mu = 0
                p.normal_(0.0, 0.5)
    return m.cuda().eval()


def _clouds(oracle, B=4, N=256, seed=31):
    xyz, mu_gt, kappa_gt, _ = oracle.synthetic_clouds(B, N, seed=seed)
    torch.manual_seed(seed)
    centres = [c.cuda() for c in oracle.replay_centres(B, sizes=((N, 128), (128, 32)))]
    return xyz.cuda(), mu_gt.cuda(), kappa_gt.cuda(), centres


def test_predictor_orientation_is_decode_of_its_outputs(oracle):
    from pnpp_hip import decode
    from pnpp_hip.inference import Predictor
    from models.pointnet_pp_8dir import PointNetPP8Dir
    from models.pointnet_pp_mvM import PointNetPPMvM
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    xyz, _, _, centres = _clouds(oracle)
    for cls in (PointNetPPMvM, PointNetPPVonMises):
        p = Predictor(_seeded(cls))
        out = p(xyz, centres=centres)
        want = decode.decode(*out, density=True)
        got = p.orientation(xyz, centres=centres, density=True)
        assert isinstance(got, decode.Orientation) and got.modes.shape == (4, 4 if cls is PointNetPPMvM else 1)
        for g, w in zip(got, want):
            assert torch.equal(g, w) or (torch.isnan(g) == torch.isnan(w)).all() and torch.equal(g.nan_to_num(9.0), w.nan_to_num(9.0))
        assert int(got.n_modes.min()) >= 1
        assert got.density.shape == (4, 359) and p.orientation(xyz, centres=centres, num=65).density is None
    with pytest.raises(TypeError, match="PointNetPPVonMises or a PointNetPPMvM"):
        Predictor(_seeded(PointNetPP8Dir)).orientation(xyz, centres=centres)


def test_evaluate_with_metrics_equals_the_concatenated_batch(oracle):
    from pnpp_hip import decode, ops, trainer
    from models.pointnet_pp_mvM import PointNetPPMvM
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    B, N = 24, 256
    xyz, mu_gt, kappa_gt, centres = _clouds(oracle, B, N, seed=41)
    labels = torch.arange(B) % 3

    # single peak: batch = (xyz, mu_gt, kappa_gt, labels)
    model = _seeded(PointNetPPVonMises)
    state = {"i": 0}

    def fwd(m, batch):   # the same centres for the same clouds, whichever way they are batched
        i, b = state["i"], batch[0].size(0)
        state["i"] = (i + b) % B
        return m(batch[0], centres=[c[i:i + b] for c in centres])

    loss = (fwd, lambda out, batch: ops.kl_von_mises_single(out[0], out[1], batch[1], batch[2]))
    loader = trainer.SyntheticLoader([xyz, mu_gt, kappa_gt], 8, False, "cuda", labels=labels)
    assert len(loader) == 3
    plain = trainer.evaluate(model, loss, loader, "cuda")
    m3 = decode.AngularErrors(n_labels=3, capacity=B)
    with_metrics = trainer.evaluate(model, loss, loader, "cuda", label_index=3, metrics=m3)
    assert with_metrics == plain
    whole = decode.AngularErrors(n_labels=3, capacity=B)
    with torch.no_grad():   # the concatenated batch: the same per-batch outputs, decoded and added in one go
        outs = [fwd(model, batch) for batch in loader]
        whole.update_outputs([torch.cat(t) for t in zip(*outs)], (xyz, mu_gt, kappa_gt), labels.cuda())
    assert np.array_equal(m3.counts(), whole.counts()) and m3.summary() == whole.summary()
    assert torch.equal(m3.sample_errors(), whole.sample_errors()) and m3.summary()["samples"] == B
    with pytest.raises(ValueError, match="forward, criterion"):
        trainer.evaluate(model, lambda m, b: loss[1](fwd(m, b), b), loader, "cuda", metrics=m3)

    # multi peak: batch = (xyz, vm_gt, K_gt, labels)
    model = _seeded(PointNetPPMvM)
    K_gt = (torch.arange(B) % 3 + 1).to(torch.int32).cuda()
    vm_gt = torch.zeros(B, 4, 3, device="cuda")
    vm_gt[:, :, 0] = mu_gt[:, None] + torch.arange(4, device="cuda") * (math.pi / 2)
    vm_gt[:, :, 1], vm_gt[:, :, 2] = 8.0, 0.25
    state["i"] = 0
    loss = (fwd, lambda out, batch: ops.match_loss(out[0], out[1], out[2], batch[1], batch[2]))
    loader = trainer.SyntheticLoader([xyz, vm_gt, K_gt], 8, False, "cuda", labels=labels)
    plain = trainer.evaluate(model, loss, loader, "cuda")
    m3 = decode.AngularErrors(n_labels=3)
    assert trainer.evaluate(model, loss, loader, "cuda", label_index=3, metrics=m3) == plain
    whole = decode.AngularErrors(n_labels=3)
    with torch.no_grad():
        outs = [fwd(model, batch) for batch in loader]
        whole.update_outputs([torch.cat(t) for t in zip(*outs)], (xyz, vm_gt, K_gt), labels.cuda())
    assert np.array_equal(m3.counts(), whole.counts()) and m3.summary()["overall"]["n"] == B


def test_predictor_decode_update_in_one_captured_graph(oracle):
    from pnpp_hip import decode
    from pnpp_hip.inference import Predictor
    from models.pointnet_pp_mvM import PointNetPPMvM
    B = 4
    xyz, mu_gt, _, centres = _clouds(oracle, B, 256, seed=51)
    vm_gt = torch.zeros(B, 4, 3, device="cuda")
    vm_gt[:, 0, 0], vm_gt[:, :, 1] = mu_gt, 8.0
    K_gt = torch.ones(B, dtype=torch.int32, device="cuda")
    p = Predictor(_seeded(PointNetPPMvM))
    eager, captured = decode.AngularErrors(capacity=16), decode.AngularErrors(capacity=16)

    def run(acc):
        ori = p.orientation(xyz, centres=centres)
        acc.update(ori, vm_gt=vm_gt, K_gt=K_gt)
        return ori

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        want = run(eager)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    once = eager.counts()
    assert once[-1] == B
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = run(captured)
    assert not captured.counts().any()          # capturing launches nothing
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(captured.counts(), 3 * once)
    assert torch.equal(got.n_modes, want.n_modes) and torch.equal(got.heights, want.heights)
    assert torch.equal(captured.sample_errors()[:B], eager.sample_errors()) and captured.sample_errors().shape == (12, 2)


def _run_script(mod, tmp_path, monkeypatch, argv):
    monkeypatch.setattr(mod, "RES", tmp_path)
    monkeypatch.setattr(mod, "FIGS", tmp_path / "figs")
    for name, value in (("EPOCHS", 1), ("BATCH", 16), ("NUM_POINTS", 256)):
        monkeypatch.setattr(mod, name, value)
    return mod.main(["--synthetic", "64", "--sampler", "device"] + argv)


def test_scripts_write_angular_errors_only_when_asked(tmp_path, monkeypatch):
    import json
    import train_multi_peaks_vonMises_KL as multi
    import train_single_peak_vonMises_KL as single
    for mod, n_test in ((single, 16), (multi, 16)):   # max(BATCH, 0.15 * 64) generated test clouds
        off, on = tmp_path / (mod.__name__ + "_off"), tmp_path / (mod.__name__ + "_on")
        off.mkdir(), on.mkdir()
        _run_script(mod, off, monkeypatch, [])
        assert not (off / "angular_errors.json").exists()
        _, test_kl = _run_script(mod, on, monkeypatch, ["--angular-metrics"])
        s = json.loads((on / "angular_errors.json").read_text())
        assert s["samples"] == n_test and s["overall"]["n"] + s["overall"]["excluded"] == n_test
        assert s["overall"]["n"] > 0 and 0.0 <= s["overall"]["top1"]["median"] <= 180.0
        assert sorted(p.name for p in on.iterdir() if p.is_file()) == sorted([p.name for p in off.iterdir() if p.is_file()] + ["angular_errors.json"])
        if mod is multi:
            assert s["label_names"] == ["synthetic"] and f"Test KL: {test_kl:.6f}" in (on / "results.txt").read_text()
