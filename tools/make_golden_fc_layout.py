#!/usr/bin/env python3
"""Writes tests/golden/fc_layout.json: the fully connected block's workspace sizes (saved bytes, scratch bytes, the message of a
rejected descriptor) a given build of the library computes for the descriptor table of tests/test_fc_layout_cpu.py.  Needs no GPU.

    python tools/make_golden_fc_layout.py /path/to/libpnpp_hip.so

The file is a record of what the layouts WERE: regenerate it from the build a layout change starts from, never from the change itself."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "3d-pointcloud-orientation-estimation_amd")):
    sys.path.insert(0, p)

from pnpp_hip import _lib  # noqa: E402  (the descriptor struct and the signatures only; the library is the one named on the command line)
import test_fc_layout_cpu as T  # noqa: E402

h = ctypes.CDLL(os.path.abspath(sys.argv[1]))
for name in ("pnpp_fc_saved_bytes", "pnpp_fc_scratch_bytes"):
    getattr(h, name).restype, getattr(h, name).argtypes = _lib.SIGNATURES[name]
h.pnpp_last_error.restype = ctypes.c_char_p
rows = T.layout_rows(h, _lib.FcDesc)
with open(T.GOLDEN, "w") as f:
    json.dump(rows, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"wrote {T.GOLDEN}: {len(rows)} rows")
