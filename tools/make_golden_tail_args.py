#!/usr/bin/env python3
"""Writes tests/golden/tail_args.json: the return code and the message with which a given build of the library refuses each call in
the table of tests/test_tail_args_cpu.py (step tails, flat-buffer optimiser, stand-alone heads and losses).  Needs no GPU.

    python tools/make_golden_tail_args.py /path/to/libpnpp_hip.so

The file is a record of what the answers WERE: regenerate it from the build a change to these entries starts from, never from the
change itself.  A row the library does not refuse before its launch does not belong in the table and stops the tool."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "3d-pointcloud-orientation-estimation_amd")):
    sys.path.insert(0, p)

from pnpp_hip import _lib  # noqa: E402  (the signatures only; the library is the one named on the command line)
import test_tail_args_cpu as T  # noqa: E402

h = ctypes.CDLL(os.path.abspath(sys.argv[1]))
for name in list(T.ENTRIES) + ["pnpp_last_error"]:
    getattr(h, name).restype, getattr(h, name).argtypes = _lib.SIGNATURES[name]
rows = T.refusals(h)
passed = [k for k, v in rows.items() if v["rc"] not in T.REFUSED]
if passed:
    sys.exit(f"not refused before a launch: {passed}")
with open(T.GOLDEN, "w") as f:
    json.dump(rows, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"wrote {T.GOLDEN}: {len(rows)} rows")
