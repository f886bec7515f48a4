"""Every kernel-selection switch the library reads (env_int("PNPP_...") -- csrc/launch.h, the one parser -- or getenv("PNPP_...") in csrc/)
has a GPU test that runs the form it selects: a case of
tests/test_gpu_switch_forms.py, or an exemption below that names the test owning it.  A switch added without a test fails here, on
the CPU."""
import glob
import os
import re

import test_gpu_switch_forms as forms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3d-pointcloud-orientation-estimation_amd", "csrc")

EXEMPT = {
    "PNPP_MATMUL": "the bf16-operand mode: tests/test_gpu_bf16.py switches it in process and checks its kernels' tags",
    "PNPP_SPLIT_PRODUCTS": "tests/test_gpu_split_products.py and tests/test_gpu_dispatch_bands.py run both product forms in process "
                           "(pnpp_set_split_products); the switch cases that need the float32-MFMA form set it in the child",
}


def _switches_read_by_the_library():
    names = set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")):
        with open(path) as f:
            names.update(re.findall(r'(?:getenv|env_int)\(\s*"(PNPP_[A-Z0-9_]+)"', f.read()))
    return names


def test_the_scan_finds_the_switches():
    names = _switches_read_by_the_library()
    assert {"PNPP_NO_WSF", "PNPP_MID3", "PNPP_WSX3", "PNPP_NO_FC_FUSED", "PNPP_MATMUL"} <= names, sorted(names)
    assert names == {"PNPP_NO_WSF", "PNPP_WSF_NT4", "PNPP_NO_WSP", "PNPP_NO_FC_FUSED", "PNPP_NO_POOL_FUSION", "PNPP_NO_POOL_BWD_FUSION",
                     "PNPP_SPLIT_PRODUCTS", "PNPP_WSF3_NT4", "PNPP_WSF03", "PNPP_MID3", "PNPP_NO_WSQ", "PNPP_WSQ_FORM", "PNPP_NO_MID",
                     "PNPP_NO_WSX", "PNPP_WSF0_WORKERS", "PNPP_WSX_WPC", "PNPP_WSX3", "PNPP_MATMUL"}, sorted(names)


def test_every_switch_has_a_gpu_case_or_a_named_owner():
    tested = {case.split("=")[0] for case in forms.SWITCHES}
    untested = sorted(n for n in _switches_read_by_the_library() if n not in tested and n not in EXEMPT)
    assert not untested, f"switches without a case in tests/test_gpu_switch_forms.py (or an exemption here): {untested}"


def test_every_case_selects_something_and_is_read_by_the_library():
    names = _switches_read_by_the_library()
    for case, (env, levels, present, absent) in forms.SWITCHES.items():
        assert case.split("=")[0] in env and env[case.split("=")[0]] == case.split("=")[1], case
        assert set(env) <= names, (case, sorted(set(env) - names))
        assert levels and set(levels) <= set(forms.LEVEL), case
        assert present, f"{case}: no kernel asserted to run"
    assert not set(EXEMPT) & {case.split("=")[0] for case in forms.SWITCHES}
