"""Which kernels a call actually ran: the ProfScope tag of every library launch, recorded with pnpp_profile_enable / pnpp_profile_report.

    tags = record(fn)                      # runs fn() with launch recording on, returns the tags in first-launch order
    expect(tags, present=["gemm_wsd3_kernel<256"], absent=["gemm_wsq_kernel"])

A pattern is a kernel-family prefix ("gemm_wsf3_kernel", "gemm_wsd3_kernel<128,32,A4>") optionally followed by whole fields that must
all be in the same tag ("gemm_smallm_kernel M=256", "gemm_wsf3_kernel<128 grid=76x1").  A parity case that asserts its tags proves which
kernel it measured: when a dispatch predicate moves, the case fails instead of quietly testing something else.

Also a pytest plugin for child processes (tests/test_gpu_switch_forms.py): with `-p dispatch` and PNPP_DISPATCH_TAGS_OUT=<file> in
the environment, the tags of every test call are written to that file as {nodeid: [tags]} when the session ends.
"""
import ctypes
import json
import os
import re

import torch


def record(fn):
    """Run fn() with launch recording on; returns the tags (first-launch order, one entry per distinct tag)."""
    from pnpp_hip import _lib
    lib = _lib.lib()
    torch.cuda.synchronize()
    lib.pnpp_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 18)
        n = lib.pnpp_profile_report(buf, len(buf))
        assert n >= 0, "pnpp_profile_report failed"
        return [ln.split("\t")[0] for ln in buf.value.decode().splitlines()]
    finally:
        lib.pnpp_profile_enable(0)


def _matches(tag, pattern):
    head, *fields = pattern.split()
    return tag.startswith(head) and all(f in tag.split()[1:] for f in fields)


def find(tags, pattern):
    return [t for t in tags if _matches(t, pattern)]


def expect(tags, present=(), absent=()):
    """Every pattern in `present` matches some tag, no pattern in `absent` matches any; the message lists all tags."""
    missing = [p for p in present if not find(tags, p)]
    extra = [(p, find(tags, p)) for p in absent if find(tags, p)]
    assert not missing and not extra, ("missing: %s; must not run: %s\nkernels that ran:\n    " % (missing, extra)) + "\n    ".join(tags)


def field(tag, name):
    """Integer value of a `name=` field of a tag (grid=AxB gives A)."""
    m = re.search(r"\b%s=(\d+)" % re.escape(name), tag)
    assert m, (name, tag)
    return int(m.group(1))


def wave_strip_workers(tag, ncol):
    """Persistent workers of a wave-strip kernel (gemm_wsf03 / wsf3 / wsd3 / wsx): its grid is workers x column blocks."""
    g = field(tag, "grid")
    assert g % ncol == 0, (tag, ncol)
    return g // ncol


# ---- pytest plugin for the switch children --------------------------------------------------------------------------------------------
_OUT = os.environ.get("PNPP_DISPATCH_TAGS_OUT")
_seen = {}

if _OUT:
    import pytest

    @pytest.hookimpl(hookwrapper=True)
    def pytest_runtest_call(item):
        from pnpp_hip import _lib
        lib = _lib.lib()
        torch.cuda.synchronize()
        lib.pnpp_profile_enable(1)
        try:
            yield
        finally:
            torch.cuda.synchronize()
            buf = ctypes.create_string_buffer(1 << 18)
            lib.pnpp_profile_report(buf, len(buf))
            lib.pnpp_profile_enable(0)
            _seen[item.nodeid] = [ln.split("\t")[0] for ln in buf.value.decode().splitlines()]

    def pytest_sessionfinish(session, exitstatus):
        with open(_OUT, "w") as f:
            json.dump(_seen, f, indent=1)
