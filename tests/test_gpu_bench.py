"""GPU: the single-GPU bench run as the driver starts it (a fresh child process).  A plain run measures the headline only;
--dump-outputs writes what the last timed step computed, and the same arguments give the same inputs -- so two runs of the
same build write the same arrays (no float atomics anywhere: DESIGN.md section 4)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _run_bench(extra, timeout=300):
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", *extra],
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_plain_bench_measures_the_headline_and_dumps_the_last_step(tmp_path):
    out = _run_bench(["--dump-outputs", str(tmp_path / "a")])
    assert out["metric"].startswith("clouds/sec fwd+bwd") and out["unit"] == "clouds/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f32" and out["steps"] == 4 and out["warmup"] == 2 and out["full"] is False
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(32 * 1e3 / out["ms_per_step"], rel=1e-6)
    # nothing beyond the headline without --full
    assert out["roofline"] is None and out["cpu_baseline"] is None and out["top_kernels"] == []
    assert "f32_mfma_variant" not in out and "bf16_variant" not in out

    a = _load(tmp_path / "a")
    assert {"loss", "adam.exp_avg", "adam.exp_avg_sq", "model.sa1.convs.0.weight", "model.sa1.bns.0.running_mean"} <= set(a)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert float(a["loss"][0]) == pytest.approx(out["final_loss"], rel=1e-6)
    n_params = sum(v.size for k, v in a.items() if k.startswith("model.") and "running_" not in k)
    assert a["adam.exp_avg"].size == n_params == 1_465_922

    _run_bench(["--dump-outputs", str(tmp_path / "b")])
    b = _load(tmp_path / "b")
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
