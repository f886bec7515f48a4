"""A level's trailing dW reduction rides in the next level's pooling launch (pnpp_sa_backward_ex, pnpp_hip.ops._TailSlot).

The scenarios run in tests/ride_tails_child.py, once per setting of PNPP_RIDE_TAILS (the switch is read once per process): riding
on (the default) and PNPP_RIDE_TAILS=0, which is the launch sequence of pnpp_sa_backward.  The reduction is the same blocks, the
same order of sums and the same stores whichever launch carries it, so every comparison here is torch.equal.

Shapes.  The smallest at which both launches of a pair exist, checked by the tags of the switched-off run:
    lower      grouped    B 2, N 128, S 64, K 16, D 32, mlp [32, 32, 64]
    upper_all  group_all  B 2, N 64,        D 64, mlp [64, 64, 128]
    upper_grp  grouped    B 2, N 64, S 8, K 8, D 64, mlp [64, 64, 128]
The lower level has S = 64 centres per cloud, not 16: with B * S = 32 groups (<= 64) a small level's finalisation launch takes the
pooled gradient itself and there is no pool_bwd launch to ride in; 128 groups is the next size that has one.  The upper levels
then see 64 points per cloud, 128 rows: layer 0's dW is written in 4 partials (one per 32 rows), so its reduction launch exists
(at 32 rows there is one partial).  4 partials is also the form the merged kernel carries (64 outputs per block).
The lower level groups K = 16 neighbours, not 8: the two levels share one scratch buffer, and the lower level's call launches the
reduction on its own where its opening launch would write over the slabs the reduction reads.  At K = 8 (1,024 rows) the lower
level's dm lies at byte 1,310,720 of the buffer, inside the upper level's dW partials (bytes 1,248,768 - 1,379,840 for the
group_all level); at K = 16 (2,048 rows) it lies at 2,097,152 and its statistics slabs end at 524,288: clear of them.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "ride_tails_child.py")
CHILD_TIMEOUT = 120

POOL = "pool_bwd_kernel G=128 K=16 C=64"
REDUCE = "slab_reduce_kernel N=64 K=67"
MERGED = "pool_bwd_kernel G=128 K=16 C=64 + slab_reduce N=64 K=67"


def _child(tmp, name, env_extra):
    out = tmp / name
    out.mkdir()
    env = dict(os.environ, **env_extra)
    if not env_extra:
        env.pop("PNPP_RIDE_TAILS", None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [CHILD, str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0 and "ride_tails_child: done" in r.stdout, (r.stdout + r.stderr)[-4000:]
    with open(out / "tags.json") as f:
        tags = json.load(f)
    return torch.load(out / "result.pt"), tags


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(gradients, tags) of the scenarios with riding on, and with PNPP_RIDE_TAILS=0; the second child starts only if the first ended well"""
    tmp = tmp_path_factory.mktemp("ride_tails")
    on = _child(tmp, "on", {})
    off = _child(tmp, "off", {"PNPP_RIDE_TAILS": "0"})
    return on, off


def _same_grads(a, b, what):
    keys = sorted(k for k in a if isinstance(a[k], torch.Tensor))
    assert keys and keys == sorted(k for k in b if isinstance(b[k], torch.Tensor)), (what, keys)
    for k in keys:
        assert not torch.isnan(a[k]).any() and a[k].abs().sum() > 0, (what, k)
        assert torch.equal(a[k], b[k]), (what, k, (a[k] - b[k]).abs().max())


@pytest.mark.parametrize("case", ["pair_all", "pair_grp"])
def test_riding_on_equals_riding_off(runs, case):
    """Every parameter gradient and the input gradient bit-equal; with riding on the upper level's reduction is in the lower level's
    pooling launch and nowhere else, with it off the two launches of pnpp_sa_backward are there."""
    from dispatch import expect, field, find
    (on, tags_on), (off, tags_off) = runs
    _same_grads(on[case], off[case], case)
    assert "input" in on[case]
    expect(tags_off[case], [POOL, REDUCE], ["pool_bwd_kernel +"])
    assert field(find(tags_off[case], REDUCE)[0], "split") > 1
    expect(tags_on[case], [MERGED], [REDUCE])
    assert not [t for t in find(tags_on[case], POOL) if "+" not in t.split()], tags_on[case]
    # nothing else moved: the lower level's own reduction is launched by the flush, as the launch it always was
    assert set(tags_on[case]) == (set(tags_off[case]) - set(find(tags_off[case], POOL)) - set(find(tags_off[case], REDUCE))) | set(find(tags_on[case], MERGED))
    assert on[case]["pending_after"] == 0 and off[case]["pending_after"] == 0


def test_flush_when_the_lower_level_never_runs(runs):
    """The lower level is frozen and its input wants no gradient: its backward never runs, the end of the pass launches the upper
    level's reduction on its own."""
    from dispatch import expect
    (on, tags_on), (off, tags_off) = runs
    _same_grads(on["frozen_all"], off["frozen_all"], "frozen_all")
    expect(tags_on["frozen_all"], [REDUCE], ["pool_bwd_kernel"])
    assert sorted(tags_on["frozen_all"]) == sorted(tags_off["frozen_all"])
    assert on["frozen_all"]["pending_after"] == 0


def test_passes_in_a_row_and_captured(runs):
    """Two passes in a row, then one pass captured and replayed twice: the same gradients every time, equal to the switched-off
    run's, and nothing pending after any of them (after the capture for the replays)."""
    (on, _), (off, _) = runs
    assert len(on["passes"]) == 4 and on["passes_pending"] == [0, 0, 0, 0]
    for i, g in enumerate(on["passes"]):
        _same_grads(g, on["passes"][0], f"pass {i} vs pass 0")
        _same_grads(g, off["passes"][i], f"pass {i} on vs off")
    _same_grads(on["passes"][0], on["pair_all"], "passes vs pair_all")


@pytest.mark.parametrize("case", ["alone_all", "alone_grp"])
def test_upper_level_alone(runs, case):
    """No lower level at all: deferral followed by the flush is the launch pnpp_sa_backward makes -- the same tags, the same bits."""
    (on, tags_on), (off, tags_off) = runs
    _same_grads(on[case], off[case], case)
    assert "input" in on[case]
    assert sorted(tags_on[case]) == sorted(tags_off[case]) and [t for t in tags_on[case] if t.startswith(REDUCE.split()[0])]
    assert on[case]["pending_after"] == 0
