"""The workspace layouts of a fully connected block (csrc/fc_api.hip: fc_saved_layout / fc_scratch_layout) are pure host arithmetic on
the descriptor: pnpp_fc_saved_bytes and pnpp_fc_scratch_bytes are evaluated here through ctypes, without a GPU, and compared with
tests/golden/fc_layout.json -- the values recorded from the library before the block's kernels moved to csrc/fc_kernels.hip and the
FcBlock context replaced the routing ladder (tools/make_golden_fc_layout.py writes the file).

The table reaches every term of the two layouts: the mean / istd blocks of max(M, N) floats from both sides, a narrow block (no norm,
N = 16: exempt from the multiple-of-4 rule) and its neighbour N = 20, the dW partials with one partial in the gradient's own pitch,
with two partials and with a padded pitch, M on both sides of 4096 (where dw_plan's rows per partial change), the three norms, and a
descriptor the library rejects."""
import ctypes
import json
import os

import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "fc_layout.json")
NONE, BATCH, LAYER = 0, 1, 2

# name -> (M, K, N, norm)
CASES = {
    "M > N": (512, 64, 128, BATCH),
    "N > M": (32, 64, 256, BATCH),
    "narrow block, N = 16": (8, 256, 16, NONE),
    "its neighbour, N = 20": (8, 256, 20, NONE),
    "one dW partial, in place": (33, 2048, 4096, NONE),
    "two dW partials, bn": (33, 64, 64, BATCH),
    "two dW partials, ln": (33, 64, 64, LAYER),
    "two dW partials, none": (33, 64, 64, NONE),
    "padded dW pitch, K = 260": (33, 260, 132, BATCH),
    "M = 4096": (4096, 64, 64, NONE),
    "M = 4097": (4097, 64, 64, NONE),
    "layer norm head": (5, 512, 256, LAYER),
    "rejected: K = 6 with a norm": (8, 6, 16, BATCH),
}


def layout_rows(h, FcDesc):
    """{"<case> | training=<t>": {saved_bytes, scratch_bytes, error}} from a loaded library (error: its message for a rejected one)."""
    rows = {}
    for name, (M, K, N, norm) in CASES.items():
        for training in (1, 0):
            d = FcDesc()
            d.M, d.K, d.N, d.norm, d.relu, d.training, d.eps, d.momentum, d.drop_scale = M, K, N, norm, 1, training, 1e-5, 0.1, 1.0
            sb, scb = h.pnpp_fc_saved_bytes(ctypes.byref(d)), h.pnpp_fc_scratch_bytes(ctypes.byref(d))
            rows[f"{name} | training={training}"] = {"saved_bytes": sb, "scratch_bytes": scb,
                                                     "error": h.pnpp_last_error().decode() if sb == 0 else None}
    return rows


@pytest.fixture(scope="module")
def rows():
    from pnpp_hip import _lib, build
    build.build()
    return layout_rows(_lib.lib(), _lib.FcDesc)


def test_layouts_equal_the_recorded_ones(rows):
    want = json.load(open(GOLDEN))
    assert sorted(rows) == sorted(want) and len(want) == 2 * len(CASES)
    for key in want:
        assert rows[key] == want[key], (key, rows[key], want[key])


def test_the_table_reaches_every_layout_term(rows):
    """The fixture is only worth something if the cases differ where the layout terms differ."""
    r = lambda name, t=1: rows[f"{name} | training={t}"]
    al = lambda nbytes: -(-nbytes // 256) * 256   # every block is 256-byte aligned
    rej = r("rejected: K = 6 with a norm")
    assert rej["saved_bytes"] == 0 and rej["scratch_bytes"] == 0 and "multiples of 4" in rej["error"]
    for name, (M, K, N, norm) in CASES.items():
        if name.startswith("rejected"):
            continue
        assert r(name)["saved_bytes"] > 0 and r(name)["scratch_bytes"] > 0 and r(name)["error"] is None
        assert r(name) == r(name, 0)   # the layouts do not depend on the mode
    # the mean / istd blocks hold max(M, N) floats: what is left of the kept workspace after z, scale and shift
    stat_blocks = lambda name: r(name)["saved_bytes"] - al(4 * CASES[name][0] * CASES[name][2]) - 2 * al(4 * CASES[name][2])
    assert stat_blocks("M > N") == 2 * al(4 * 512) and stat_blocks("N > M") == 2 * al(4 * 256)
    # the dW partials: what is left of the scratch workspace after the statistics slabs, dz and the masked gradient
    dwslab = lambda name: (r(name)["scratch_bytes"] - al(8 * 512 * 2 * CASES[name][2]) - 2 * al(4 * CASES[name][0] * CASES[name][2]))
    assert dwslab("one dW partial, in place") == 4 * 1 * 4096 * 2048          # one partial, pitch K
    assert dwslab("two dW partials, bn") == 4 * 2 * 64 * 64                    # two row ranges
    assert dwslab("padded dW pitch, K = 260") == 4 * 2 * 132 * 320             # pitch 320 > K
    assert dwslab("narrow block, N = 16") == 4 * 1 * 16 * 256 and dwslab("its neighbour, N = 20") == 4 * 1 * 20 * 256
    assert dwslab("M = 4096") == 4 * 128 * 64 * 64 and dwslab("M = 4097") == 4 * 65 * 64 * 64   # 32 -> 64 rows per partial
    # the norm selects kernels, not layouts
    assert r("two dW partials, bn") == r("two dW partials, ln") == r("two dW partials, none")
