"""Every kernel-selection switch of the library (a PNPP_* environment variable read once per process into a static) against the float64
parity suite, in a fresh child process per switch value, each child proving that the alternative kernel ran.

A child runs tests/test_gpu_levels_routed.py -- the level / head-block parity at BASELINE configs[1] (32 clouds of 1024 points), every
ReLU and max-pool decision injected, 1e-5 of each tensor's max-abs -- narrowed with -k to what the switch affects, plus that module's
check that the wave-pair kernels' bounded polls never gave up.  tests/dispatch.py, loaded in the child as a pytest plugin, records the
ProfScope tag of every launch of every test; this side asserts the kernels the switch must select and the ones it must replace.
A switch that only acts when split products are off is combined with PNPP_SPLIT_PRODUCTS=0.

  switch                      what it selects (at configs[1])                                  levels   asserted (present / absent)
  PNPP_NO_WSF=1               forward products on gemm_ws_kernel (not gemm_wsf3 / gemm_wsf)     sa1 sa2  gemm_ws<64 / 128, A1,E1> / gemm_wsf3
  PNPP_NO_WSP=1 (+S0)         sa1 layer-2 backward on gemm_ws_kernel<128,..,dW>                 sa1      gemm_ws<128,..,A5,E2,dW> / gemm_wsp
  PNPP_NO_WSQ=1 (+S0)         sa2 layer-2 backward on gemm_ws_kernel<256,..,dW>                 sa2      gemm_ws<256,..,A5,E2,dW> / gemm_wsq
  PNPP_WSQ_FORM=2 (+S0)       gemm_wsq2_kernel (weight panel in registers)                     sa2      gemm_wsq<256,A5,F2>
  PNPP_NO_WSX=1               sa1 on the generic path: layer 0 stored, no coordinate rebuild    sa1      gemm_ws<4,128,64,A2>, gemm_ws<64,..,A4,E2,dW>,
                                                                                                          dw_xyz / gemm_wsx, gemm_wsf03, rel_moments
  PNPP_WSX3=0                 gemm_wsx dA product on the float32 instruction                    sa1      gemm_wsx<64,1> / gemm_wsx<64,1,S3
  PNPP_WSX3=2                 gemm_wsx dW_1 product on the bf16 pipe too                        sa1      gemm_wsx<64,1,S3,D3>
  PNPP_WSX_WPC=2              gemm_wsx with two workgroups per CU                               sa1      gemm_wsx<64,2> grid=512x1
  PNPP_WSF0_WORKERS=256       gemm_wsf03 with 256 workers (and 256 statistics slabs)            sa1      gemm_wsf03 grid=256x1
  PNPP_WSF03=0                layers 0+1 forward on gemm_wsf0_kernel (float32 MFMA)              sa1      gemm_wsf0 / gemm_wsf03
  PNPP_MID3=0                 sa3 layer-2 forward on gemm_mid_kernel                            sa3      gemm_mid M=1024 N=1024 / gemm_mid3
  PNPP_NO_MID=1               sa3 on the 32 x 32 split-K kernels                                sa3      gemm_smallm N=1024, da_dw_kernel, pool_fwd /
                                                                                                          gemm_mid3, gemm_mid, da_dw_mid
  PNPP_WSF3_NT4=1             gemm_wsf3 with four column tiles per wave (K 64, N 128)           sa1      gemm_wsf3<64 N=128 grid=256x1 / grid=512x1
  PNPP_WSF_NT4=1 (+S0)        gemm_wsf with four column tiles per wave                          sa1      gemm_wsf<64,4 / gemm_wsf<64,2
  PNPP_NO_POOL_FUSION=1       max-pool as a launch of its own                                   sa1-3    pool_fwd (3 levels) / bn_finalize_fwd +pool
  PNPP_NO_POOL_BWD_FUSION=1   sa3's pool_bwd launch kept                                        sa3      pool_bwd G=32
  PNPP_NO_FC_FUSED=1          head-block backward as fc_dx_dw (dz written)                      fc1 fc2  fc_dx_dw / fc_bwd_fused

Not here: PNPP_MATMUL (the bf16-operand mode: tests/test_gpu_bf16.py), PNPP_SPLIT_PRODUCTS (tests/test_gpu_split_products.py and
tests/test_gpu_dispatch_bands.py run both product forms in process).  tests/test_switch_coverage.py fails on the CPU when csrc/ reads a
PNPP_* switch that is neither here nor exempted there.

Children run one at a time under a time limit.  A child that ends by a signal, runs out of time or reports a GPU fault ends the file:
every later case fails without starting a process.
"""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
CHILD_TIMEOUT = 120
S0 = {"PNPP_SPLIT_PRODUCTS": "0"}
LEVEL = {"sa1": "test_sa1_level_kernels", "sa2": "test_sa2_level_kernels", "sa3": "test_sa3_level_kernels", "head": "test_head_block_kernels"}
TESTS_PER = {"sa1": 1, "sa2": 1, "sa3": 1, "head": 2}
POOLED = "bn_finalize_fwd_kernel +pool"

# id -> (environment, levels, present, absent)
SWITCHES = {
    "PNPP_NO_WSF=1": ({"PNPP_NO_WSF": "1"}, ["sa1", "sa2"],
                      ["gemm_ws_kernel<64,64,64,A1,E1> N=128", "gemm_ws_kernel<128,64,64,A1,E1> N=128", "gemm_ws_kernel<128,64,64,A1,E1> N=256"],
                      ["gemm_wsf3", "gemm_wsf_"]),
    "PNPP_NO_WSP=1": (dict(S0, PNPP_NO_WSP="1"), ["sa1"], ["gemm_ws_kernel<128,64,64,A5,E2,dW> N=64"], ["gemm_wsp", "gemm_wsd3"]),
    "PNPP_NO_WSQ=1": (dict(S0, PNPP_NO_WSQ="1"), ["sa2"], ["gemm_ws_kernel<256,64,64,A5,E2,dW> N=128"], ["gemm_wsq", "gemm_wsd3"]),
    "PNPP_WSQ_FORM=2": (dict(S0, PNPP_WSQ_FORM="2"), ["sa2"], ["gemm_wsq_kernel<256,A5,F2>"], ["gemm_wsq_kernel<256,A5>", "gemm_wsd3"]),
    "PNPP_NO_WSX=1": ({"PNPP_NO_WSX": "1"}, ["sa1"], ["gemm_ws_kernel<4,128,64,A2", "gemm_wsf3_kernel<64 N=64", "gemm_ws_kernel<64,64,64,A4,E2,dW>",
                                                      "dw_xyz_kernel"],
                      ["gemm_wsx", "xyz0_post", "rel_moments", "gemm_wsf03", "gemm_wsf0_"]),
    "PNPP_WSX3=0": ({"PNPP_WSX3": "0"}, ["sa1"], ["gemm_wsx_kernel<64,1>"], ["gemm_wsx_kernel<64,1,S3"]),
    "PNPP_WSX3=2": ({"PNPP_WSX3": "2"}, ["sa1"], ["gemm_wsx_kernel<64,1,S3,D3>"], ["gemm_wsx_kernel<64,1,S3>", "gemm_wsx_kernel<64,1>"]),
    "PNPP_WSX_WPC=2": ({"PNPP_WSX_WPC": "2"}, ["sa1"], ["gemm_wsx_kernel<64,2> grid=512x1"], ["gemm_wsx_kernel<64,1"]),
    "PNPP_WSF0_WORKERS=256": ({"PNPP_WSF0_WORKERS": "256"}, ["sa1"], ["gemm_wsf03_kernel grid=256x1"], ["gemm_wsf03_kernel grid=512x1"]),
    "PNPP_WSF03=0": ({"PNPP_WSF03": "0"}, ["sa1"], ["gemm_wsf0_kernel"], ["gemm_wsf03"]),
    "PNPP_MID3=0": ({"PNPP_MID3": "0"}, ["sa3"], ["gemm_mid_kernel M=1024 N=1024", POOLED], ["gemm_mid3"]),
    "PNPP_NO_MID=1": ({"PNPP_NO_MID": "1"}, ["sa3"], ["gemm_smallm_kernel M=1024 N=1024", "da_dw_kernel M=1024", "pool_fwd_kernel G=32"],
                      ["gemm_mid3", "gemm_mid_", "da_dw_mid", POOLED]),
    "PNPP_WSF3_NT4=1": ({"PNPP_WSF3_NT4": "1"}, ["sa1"], ["gemm_wsf3_kernel<64 N=128 grid=256x1"], ["gemm_wsf3_kernel<64 N=128 grid=512x1"]),
    "PNPP_WSF_NT4=1": (dict(S0, PNPP_WSF_NT4="1"), ["sa1"], ["gemm_wsf_kernel<64,4"], ["gemm_wsf_kernel<64,2", "gemm_wsf3"]),
    "PNPP_NO_POOL_FUSION=1": ({"PNPP_NO_POOL_FUSION": "1"}, ["sa1", "sa2", "sa3"],
                              ["pool_fwd_kernel G=4096", "pool_fwd_kernel G=1024", "pool_fwd_kernel G=32"], [POOLED]),
    "PNPP_NO_POOL_BWD_FUSION=1": ({"PNPP_NO_POOL_BWD_FUSION": "1"}, ["sa3"], ["pool_bwd_kernel G=32"], []),
    "PNPP_NO_FC_FUSED=1": ({"PNPP_NO_FC_FUSED": "1"}, ["head"], ["fc_dx_dw_kernel M=32"], ["fc_bwd_fused_kernel"]),
}

FAULT = re.compile(r"memory access fault|page not present|HSA_STATUS_ERROR|hipErrorLaunchFailure|hipErrorIllegalAddress|"
                   r"GPU core dump|Segmentation fault|Aborted", re.I)
_stop = []   # set once a child ended by a signal, ran out of time or reported a GPU fault


def _run_child(env_extra, levels, out_file):
    env = dict(os.environ, **env_extra)
    env["PNPP_DISPATCH_TAGS_OUT"] = out_file
    env["PYTHONPATH"] = TESTS + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    sel = " or ".join([LEVEL[l] for l in levels] + ["test_zz_wave_pair_polls_never_timed_out"])
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        "-m", "pytest", os.path.join(TESTS, "test_gpu_levels_routed.py"), "-m", "gpu", "-q", "-s", "-p", "no:cacheprovider",
        "-p", "dispatch", "-k", sel]
    try:
        return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _stop.append("timeout")
        raise


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_switch_form(switch, tmp_path):
    from dispatch import expect
    assert not _stop, f"an earlier child ended by {_stop[0]}: no further GPU process is started"
    env_extra, levels, present, absent = SWITCHES[switch]
    out_file = str(tmp_path / "tags.json")
    r = _run_child(env_extra, levels, out_file)
    log = r.stdout + r.stderr
    if r.returncode < 0 or FAULT.search(log):
        _stop.append(f"signal {-r.returncode}" if r.returncode < 0 else "a GPU fault")
    want = sum(TESTS_PER[l] for l in levels) + 1
    print(f"\n[{switch}] child exit {r.returncode}\n" + "\n".join(ln for ln in r.stdout.splitlines() if ln.startswith(("[", "    ")))[-6000:])
    assert r.returncode == 0 and re.search(rf"\b{want} passed\b", r.stdout) and not re.search(r"skipped|failed|error", r.stdout.splitlines()[-1]), \
        log[-4000:]
    with open(out_file) as f:
        per_test = json.load(f)
    tags = sorted({t for node, ts in per_test.items() if "test_zz" not in node for t in ts})
    print(f"[{switch}] kernels:\n    " + "\n    ".join(tags))
    expect(tags, present, absent)
