"""Which launches a fully connected block takes (csrc/fc_api.hip: the FcBlock routing facts and the steps they select): one
ops.fc_block forward + backward per row of the table below, the smallest shapes on each side of every routing edge -- the narrow
block and its neighbour (N = 16 / 20), one tile of BatchNorm rows (M = 32 / 33), the fused backward's column bands (N = 256 / 512 /
1024, below them 252) and its need of a gradient to pass on, the dW forms (in place, two partials, padded pitch), eval mode,
LayerNorm with a given and with a drawn mask, and the row-chunked backward (M = 4096 / 4097) without and with BatchNorm.  The full
ordered tag list of each row (tests/dispatch.py) is compared with tests/golden/fc_routes.json, recorded by this module from the
library before the block's host code became a route table:

    python tests/test_gpu_fc_routes.py --record        # on an MI355X, from the commit a routing change starts from

Launches without a ProfScope (fc_bwd_cols_kernel, the LayerNorm kernels, fc_apply_cols_kernel after a BatchNorm finalisation) leave
no tag; the matrix products around them do.  Nothing numeric is asserted here beyond pnpp_fc_recompute_output returning the forward
pass's bits: parity is test_gpu_head_loss.py::test_fc_block, test_gpu_pointnet_bands.py, test_gpu_pt_bands.py,
test_gpu_levels_routed.py."""
import ctypes
import json
import os
import sys

import pytest
import torch
import torch.nn as nn

from conftest import ROOT
import dispatch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "fc_routes.json")

# (M, K, N, norm, x.requires_grad, variant); variant: "train" | "eval" (forward only) | "given mask" | "drawn mask"
ROWS = [
    (8, 256, 16, "none", True, "train"),
    (8, 256, 16, "none", False, "train"),
    (8, 256, 20, "none", True, "train"),
    (32, 64, 256, "bn", True, "train"),
    (32, 64, 512, "bn", True, "train"),
    (32, 64, 1024, "bn", True, "train"),
    (32, 64, 252, "bn", True, "train"),
    (32, 64, 256, "bn", False, "train"),
    (33, 64, 256, "bn", True, "train"),
    (33, 64, 64, "bn", False, "train"),
    (33, 2048, 4096, "none", False, "train"),
    (33, 260, 132, "bn", False, "train"),
    (16, 256, 64, "bn", None, "eval"),
    (5, 512, 256, "ln", True, "given mask"),
    (5, 512, 256, "ln", True, "drawn mask"),
    (4096, 64, 64, "none", True, "train"),
    (4097, 64, 64, "none", True, "train"),
    (4096, 64, 64, "bn", True, "train"),
    (4097, 64, 64, "bn", True, "train"),
]


def row_key(row):
    M, K, N, norm, req, variant = row
    return f"M={M} K={K} N={N} {norm} x.requires_grad={req} {variant}"


def run_block(row):
    """One fc_block forward (+ backward unless eval) of a row; returns (y, x)."""
    from pnpp_hip import ops
    M, K, N, norm, req, variant = row
    torch.manual_seed(M + K + N)
    lin = nn.Linear(K, N).cuda()
    mod = {"bn": nn.BatchNorm1d(N), "ln": nn.LayerNorm(N), "none": None}[norm]
    mod = mod.cuda() if mod is not None else None
    x = torch.randn(M, K, device="cuda", requires_grad=bool(req))
    if variant == "eval":
        mod.eval()
        return ops.fc_block(x, lin, mod, relu=True, training=False), x
    mask = (torch.rand(M, N, device="cuda") < 0.6).to(torch.uint8) if variant == "given mask" else None
    dropout = nn.Dropout(0.4) if variant in ("given mask", "drawn mask") else None
    y = ops.fc_block(x, lin, mod, relu=True, dropout=dropout, training=True, mask=mask)
    y.backward(torch.randn(M, N, device="cuda"))
    return y, x


def record_routes():
    """{row key: the row's tags in launch order} from the library the package loads."""
    return {row_key(row): dispatch.record(lambda: run_block(row)) for row in ROWS}


@pytest.fixture(scope="module")
def routes():
    return record_routes()


def test_the_table_is_the_recorded_one(routes):
    want = json.load(open(GOLDEN))
    assert sorted(routes) == sorted(want) and len(want) == len(ROWS)


@pytest.mark.parametrize("row", ROWS, ids=row_key)
def test_launches_equal_the_recorded_ones(routes, row):
    want = json.load(open(GOLDEN))[row_key(row)]
    assert routes[row_key(row)] == want, "\n".join(["ran:"] + routes[row_key(row)] + ["recorded:"] + want)


def test_recompute_output_returns_the_forward_output():
    """pnpp_fc_recompute_output on the kept workspace of a BatchNorm block with more than 32 rows: the forward pass's y, bit for bit."""
    from pnpp_hip import _lib, ops
    M, K, N = 33, 64, 256
    torch.manual_seed(5)
    lin, bn = nn.Linear(K, N).cuda(), nn.BatchNorm1d(N).cuda()
    x = torch.randn(M, K, device="cuda", requires_grad=True)
    y = ops.fc_block(x, lin, bn, relu=True, training=True)
    d = _lib.FcDesc()
    d.M, d.K, d.N, d.norm, d.relu, d.training, d.eps, d.momentum, d.drop_scale = M, K, N, _lib.NORM_BATCH, 1, 1, bn.eps, bn.momentum, 1.0
    saved = y.grad_fn.saved_tensors[-1]   # the block's kept workspace
    assert saved.dtype == torch.uint8 and saved.numel() == _lib.lib().pnpp_fc_saved_bytes(ctypes.byref(d))
    y2 = torch.full_like(y, float("nan"))
    _lib.check(_lib.lib().pnpp_fc_recompute_output(ctypes.byref(d), saved.data_ptr(), None, y2.data_ptr(), ops._stream()))
    assert torch.equal(y2, y.detach())


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    rows = record_routes()
    with open(GOLDEN, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    print(f"wrote {GOLDEN}: {len(rows)} rows")
