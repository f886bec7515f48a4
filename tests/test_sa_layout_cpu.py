"""The workspace layouts of a set-abstraction level (csrc/sa_api.hip: sa_saved_layout / sa_scratch_layout) are pure host arithmetic on
the descriptor: pnpp_sa_saved_bytes, pnpp_sa_scratch_bytes and the offsets behind pnpp_sa_saved_neighbours / pnpp_sa_saved_argmax are
evaluated here through ctypes, without a GPU, and compared with tests/golden/sa_layout.json -- the values recorded from the library
before the level context replaced the per-function routing predicates (tools/make_golden_sa_layout.py writes the file).

The two pointer functions are given a made-up non-null base address, which is subtracted again; nothing is dereferenced.  The table
covers every routing fact the layouts read: a level on raw coordinates (moment partials in both workspaces), M at and above kSmallM
(the dZ buffer), the delayed layer 0 (source rows and its dW partials), whole-cloud pooling with and without the zmax block, and a
descriptor the library rejects.  The library's switches are at their defaults (no PNPP_* variable set)."""
import ctypes
import json
import os

import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "sa_layout.json")
BASE = 1 << 32   # any 256-byte aligned non-null address

# name -> (B, N, S, K, D, C, group_all)
CASES = {
    "coordinate level": (32, 1024, 128, 32, 0, [64, 64, 128], 0),
    "coordinate level, small batch": (4, 1024, 128, 32, 0, [64, 64, 128], 0),
    "features, S*K <= N, not delayed": (32, 128, 32, 32, 128, [128, 128, 256], 0),
    "delayed layer 0": (2, 256, 96, 64, 8, [256, 64, 64], 0),
    "group_all, small M": (32, 32, 1, 32, 256, [256, 512, 1024], 1),
    "group_all, small M, tiny": (2, 32, 1, 32, 4, [32, 32, 64], 1),
    "group_all, pooling split over K": (2, 1024, 1, 1024, 0, [64, 128, 1024], 1),
    "classifier level, D = 3": (8, 1024, 512, 32, 3, [64, 64, 128], 0),
    "wide neighbourhood": (8, 512, 128, 64, 128, [128, 128, 256], 0),
    "rejected: C[1] = 48": (2, 64, 8, 4, 0, [32, 48, 64], 0),
}


def layout_rows(h, SaDesc):
    """{"<case> | training=<t>": {saved_bytes, scratch_bytes, neighbours_offset, argmax_offset}} from a loaded library."""
    rows = {}
    for name, (B, N, S, K, D, C, group_all) in CASES.items():
        for training in (1, 0):
            d = SaDesc()
            d.B, d.N, d.S, d.K, d.D, d.L, d.group_all, d.training, d.eps, d.momentum = B, N, S, K, D, len(C), group_all, training, 1e-5, 0.1
            for l, c in enumerate(C):
                d.C[l] = c
            nb, am = h.pnpp_sa_saved_neighbours(ctypes.byref(d), BASE), h.pnpp_sa_saved_argmax(ctypes.byref(d), BASE)
            rows[f"{name} | training={training}"] = {
                "saved_bytes": h.pnpp_sa_saved_bytes(ctypes.byref(d)), "scratch_bytes": h.pnpp_sa_scratch_bytes(ctypes.byref(d)),
                "neighbours_offset": None if nb is None else nb - BASE, "argmax_offset": None if am is None else am - BASE}
    return rows


@pytest.fixture(scope="module")
def rows():
    from pnpp_hip import _lib, build
    build.build()
    h = _lib.lib()
    assert h.pnpp_get_matmul_precision() == 0 and h.pnpp_stats_exchange_enabled() == 0
    return layout_rows(h, _lib.SaDesc)


def test_layouts_equal_the_recorded_ones(rows):
    want = json.load(open(GOLDEN))
    assert sorted(rows) == sorted(want) and len(want) == 2 * len(CASES)
    for key in want:
        assert rows[key] == want[key], (key, rows[key], want[key])


def test_the_table_reaches_every_layout_branch(rows):
    """The fixture is only worth something if the cases differ where the routing facts differ."""
    r = lambda name, t=1: rows[f"{name} | training={t}"]
    rej = r("rejected: C[1] = 48")
    assert rej == {"saved_bytes": 0, "scratch_bytes": 0, "neighbours_offset": None, "argmax_offset": None}
    for name in CASES:
        if name.startswith("rejected"):
            continue
        group_all = CASES[name][6]
        assert r(name)["saved_bytes"] > 0 and r(name)["scratch_bytes"] > 0 and r(name)["argmax_offset"] > 0
        assert (r(name)["neighbours_offset"] is None) == bool(group_all)
        assert r(name) == r(name, 0)   # the layouts do not depend on the mode
    # zmax block: (G, C_last) floats follow the arg-max block unless pooling is split over K
    tail = lambda name: r(name)["saved_bytes"] - r(name)["argmax_offset"]
    assert tail("group_all, pooling split over K") == 2 * 1024 * 4       # the (G, C_last) arg-max block alone
    assert tail("group_all, small M, tiny") == 2 * (2 * 64 * 4)          # ... and the zmax block of the same size
