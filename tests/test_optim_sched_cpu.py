"""The scheduled optimiser without a GPU (csrc/optim_sched_kernels.hip, csrc/lr_schedule.h, pnpp_hip/optim.py): the schedule is host
arithmetic (pnpp_lr_factor evaluates the function the kernel calls), the entry refuses bad descriptors before any launch, and the
group planning, the schedule objects, the state_dict schema and the scripts' flags are plain Python."""
import ctypes
import math

import pytest
import torch

P = 0x1000                      # fake pointer: non-null, 16-byte aligned; no row below gets as far as a launch
ULP64 = 2.0 ** -53
# (warmup, total, every, start_factor, min_factor, gamma)
SETS = [(0, 50, 7, 0.1, 0.0, 0.5), (5, 50, 7, 0.1, 0.01, 0.5), (1, 2, 1, 0.5, 0.25, 0.1), (13, 200, 40, 0.001, 0.05, 0.3)]
KINDS = ("constant", "cosine", "step")


@pytest.fixture(scope="module")
def L():
    from pnpp_hip import _lib, build
    build.build()
    _lib.lib()
    return _lib


def closed_form(kind, s, warmup, total, every, start, mn, gamma):
    """The issue's formulas, in Python floats."""
    if s < warmup:
        return start + (1.0 - start) * s / warmup
    if kind == "cosine":
        if s >= total:
            return mn
        return mn + (1.0 - mn) * 0.5 * (1.0 + math.cos(math.pi * (s - warmup) / (total - warmup)))
    if kind == "step":
        return max(mn, gamma ** ((s - warmup) // every))
    return 1.0


def _sched_desc(L, kind, warmup, total, every, start, mn, gamma):
    d = L.OptimDesc()
    d.sched_kind, d.warmup, d.total, d.every = KINDS.index(kind), warmup, total, every
    d.start_factor, d.min_factor, d.gamma = start, mn, gamma
    return d


def _factor(L, d, s):
    out = ctypes.c_double(-1.0)
    L.check(L.lib().pnpp_lr_factor(ctypes.byref(d), s, ctypes.byref(out)))
    return out.value


@pytest.mark.parametrize("ps", SETS)
@pytest.mark.parametrize("kind", KINDS)
def test_lr_factor_equals_the_closed_form(L, kind, ps):
    """Every intermediate is at most 1 in magnitude and there are fewer than 16 float64 roundings, the two libraries' cos and pow
    included: 16 x 2^-53 absolute, in units of the base rate."""
    d = _sched_desc(L, kind, *ps)
    total = ps[1]
    worst = 0.0
    for s in list(range(total + 6)) + [10 * total, 2 ** 40]:
        worst = max(worst, abs(_factor(L, d, s) - closed_form(kind, s, *ps)))
    print(f"lr_factor {kind} {ps}: worst |d| = {worst / ULP64:.2f} x 2^-53")
    assert worst <= 16 * ULP64
    past = ps[4] if kind == "cosine" else 1.0 if kind == "constant" else max(ps[4], ps[5] ** ((total + 5 - ps[0]) // ps[2]))
    assert abs(_factor(L, d, total + 5) - past) <= 16 * ULP64          # past `total`: cosine stays at min_factor


@pytest.mark.parametrize("ps", SETS)
@pytest.mark.parametrize("kind", KINDS)
def test_lr_factor_equals_torch_schedulers(L, kind, ps):
    """SequentialLR(LinearLR, CosineAnnealingLR | StepLR | constant) on a CPU parameter, 1e-12 of the base rate (torch's cosine is a
    recursion whose error grows with the step count; the closed forms differ from it by ~1e-14 here)."""
    from torch.optim.lr_scheduler import ConstantLR, CosineAnnealingLR, LinearLR, SequentialLR, StepLR
    warmup, total, every, start, mn, gamma = ps
    if kind == "step":
        mn = 0.0                                                     # StepLR has no floor
    base = 1.0
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))], lr=base)
    if kind == "cosine":
        main = CosineAnnealingLR(opt, T_max=total - warmup, eta_min=mn * base)
    elif kind == "step":
        main = StepLR(opt, step_size=every, gamma=gamma)
    else:
        main = ConstantLR(opt, factor=1.0, total_iters=0)
    sched = SequentialLR(opt, [LinearLR(opt, start_factor=max(start, 1e-300), end_factor=1.0, total_iters=warmup), main],
                         milestones=[warmup]) if warmup else main
    d = _sched_desc(L, kind, warmup, total, every, start, mn, gamma)
    worst = 0.0
    for s in range(total):                                           # torch's cosine turns periodic past T_max; ours stays at min
        worst = max(worst, abs(_factor(L, d, s) - opt.param_groups[0]["lr"] / base))
        opt.step()
        sched.step()
    print(f"lr_factor vs torch {kind} {ps}: worst {worst:.2e}")
    assert worst <= 1e-12


# ---- refusals: pnpp_adamw_step and pnpp_lr_factor check everything on the host -------------------------------------------------------
def _good(L, n=1000):
    d = L.OptimDesc()
    d.n_groups, d.decoupled = 2, 1
    d.end[0], d.end[1] = 400, n
    for j in range(2):
        d.lr_mult[j], d.weight_decay[j] = 1.0, 0.01
    d.sched_kind, d.warmup, d.total, d.every = 1, 5, 50, 7
    d.start_factor, d.min_factor, d.gamma = 0.1, 0.0, 0.5
    d.lr, d.beta1, d.beta2, d.eps, d.grad_scale = 1e-3, 0.9, 0.999, 1e-8, 1.0
    d.max_norm, d.ema_decay, d.zero_grad = 0.0, 0.0, 0
    return d


def _set(name, value, index=None):
    def f(d):
        if index is None:
            setattr(d, name, value)
        else:
            getattr(d, name)[index] = value
    return f


# (what is wrong, change to the descriptor, changed call arguments)
ARGS = dict(param=P, grad=P, exp_avg=P, exp_avg_sq=P, ema=None, n=1000, state=P, grad_sumsq=None)
REFUSALS = [
    ("null param", None, dict(param=None)),
    ("null grad", None, dict(grad=None)),
    ("null exp_avg", None, dict(exp_avg=None)),
    ("null exp_avg_sq", None, dict(exp_avg_sq=None)),
    ("null state", None, dict(state=None)),
    ("n = 0", None, dict(n=0)),
    ("n_groups = 0", _set("n_groups", 0), {}),
    ("n_groups = 9", _set("n_groups", 9), {}),
    ("end not increasing", _set("end", 1000, 0), {}),
    ("end[0] = 0", _set("end", 0, 0), {}),
    ("last end != n", _set("end", 999, 1), {}),
    ("negative lr_mult", _set("lr_mult", -1.0, 1), {}),
    ("infinite lr_mult", _set("lr_mult", math.inf, 0), {}),
    ("nan weight_decay", _set("weight_decay", math.nan, 1), {}),
    ("negative weight_decay", _set("weight_decay", -0.5, 0), {}),
    ("ema_decay = 1", _set("ema_decay", 1.0), dict(ema=P)),
    ("ema_decay < 0", _set("ema_decay", -0.1), {}),
    ("ema_decay > 0, null ema", _set("ema_decay", 0.9), {}),
    ("ema_decay = 0, ema given", None, dict(ema=P)),
    ("max_norm < 0", _set("max_norm", -1.0), dict(grad_sumsq=P)),
    ("max_norm > 0, null grad_sumsq", _set("max_norm", 1.0), {}),
    ("unknown sched_kind", _set("sched_kind", 3), {}),
    ("cosine, total = warmup", _set("total", 5), {}),
    ("step, every = 0", lambda d: (_set("sched_kind", 2)(d), _set("every", 0)(d)), {}),
    ("step, gamma = 0", lambda d: (_set("sched_kind", 2)(d), _set("gamma", 0.0)(d)), {}),
    ("step, gamma > 1", lambda d: (_set("sched_kind", 2)(d), _set("gamma", 1.5)(d)), {}),
    ("start_factor > 1", _set("start_factor", 1.5), {}),
    ("start_factor nan", _set("start_factor", math.nan), {}),
    ("min_factor < 0", _set("min_factor", -0.1), {}),
]


@pytest.mark.parametrize("what,change,call", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_adamw_step_refuses_before_any_launch(L, what, change, call):
    d = _good(L)
    if change is not None:
        change(d)
    a = {**ARGS, **call}
    rc = L.lib().pnpp_adamw_step(ctypes.byref(d), a["param"], a["grad"], a["exp_avg"], a["exp_avg_sq"], a["ema"], a["n"], a["state"],
                                 a["grad_sumsq"], None)
    assert rc == L.PNPP_ERR_ARG, what
    assert L.last_error().startswith("adamw_step: "), L.last_error()


def test_adamw_step_refuses_a_null_descriptor_and_lr_factor_names_itself(L):
    assert L.lib().pnpp_adamw_step(None, P, P, P, P, None, 1000, P, None, None) == L.PNPP_ERR_ARG
    assert L.last_error().startswith("adamw_step: ")
    out = ctypes.c_double()
    assert L.lib().pnpp_lr_factor(None, 0, ctypes.byref(out)) == L.PNPP_ERR_ARG and L.last_error().startswith("lr_factor: ")
    d = _good(L)
    assert L.lib().pnpp_lr_factor(ctypes.byref(d), 0, None) == L.PNPP_ERR_ARG and L.last_error().startswith("lr_factor: ")
    for change in (_set("sched_kind", -1), _set("total", 3), _set("min_factor", 2.0)):
        d = _good(L)
        change(d)
        assert L.lib().pnpp_lr_factor(ctypes.byref(d), 0, ctypes.byref(out)) == L.PNPP_ERR_ARG and L.last_error().startswith("lr_factor: ")


def test_descriptor_layout_matches_c(L, tmp_path):
    """The ctypes mirror of pnpp_optim_desc has the size and the field offsets the C compiler gives it."""
    import os
    import subprocess
    from conftest import ROOT
    fields = [f[0] for f in L.OptimDesc._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "pnpp_hip.h"\nint main(void) { printf("%zu", sizeof(pnpp_optim_desc));\n'
    src += "".join(f'printf(" %zu", offsetof(pnpp_optim_desc, {f}));\n' for f in fields) + "return 0; }\n"
    c, exe = tmp_path / "t.c", tmp_path / "t"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(L.OptimDesc)] + [getattr(L.OptimDesc, f).offset for f in fields]


# ---- plan_groups, decay_groups, Schedule, state_dict schema -------------------------------------------------------------------------
def _params(*sizes):
    return [torch.nn.Parameter(torch.zeros(s)) for s in sizes]


def test_plan_groups():
    from pnpp_hip import optim
    a, b, c, d = _params(3, (2, 5), 7, 1)
    frozen = torch.nn.Parameter(torch.zeros(4), requires_grad=False)
    ps, ends, mults, decays = optim.plan_groups(iter([a, frozen, b, c]))
    assert [id(p) for p in ps] == [id(a), id(b), id(c)] and ends == [20] and mults == [1.0] and decays == [0.0]   # today's layout
    ps, ends, mults, decays = optim.plan_groups([{"params": [c, a], "weight_decay": 0.1}, {"params": [d], "lr_mult": 0.5}, {"params": [b]}],
                                                weight_decay=0.02)
    assert [id(p) for p in ps] == [id(c), id(a), id(d), id(b)] and ends == [10, 11, 21]
    assert mults == [1.0, 0.5, 1.0] and decays == [0.1, 0.02, 0.02]
    with pytest.raises(ValueError, match="more than one"):
        optim.plan_groups([{"params": [a, b]}, {"params": [c, a]}])
    with pytest.raises(ValueError, match="empty"):
        optim.plan_groups([{"params": [a]}, {"params": [frozen]}])
    with pytest.raises(ValueError, match="empty"):
        optim.plan_groups([])
    with pytest.raises(ValueError, match="at most 8"):
        optim.plan_groups([{"params": [p]} for p in _params(*range(1, 10))])
    with pytest.raises(ValueError):
        optim.plan_groups([{"params": [a], "weight_decay": -1.0}])


def test_decay_groups_of_the_von_mises_model():
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    from pnpp_hip import optim
    model = PointNetPPVonMises()
    decayed, plain = optim.decay_groups(model, 1e-2)
    assert decayed["weight_decay"] == 1e-2 and plain["weight_decay"] == 0.0
    assert sum(p.numel() for p in decayed["params"]) + sum(p.numel() for p in plain["params"]) == 1_465_922
    in_plain = {id(p) for p in plain["params"]}
    assert all((p.ndim < 2) == (id(p) in in_plain) for p in model.parameters())
    named = dict(model.named_parameters())
    assert id(named["sa1.bns.0.weight"]) in in_plain and id(named["sa1.convs.0.bias"]) in in_plain
    assert id(named["sa1.convs.0.weight"]) not in in_plain
    ps, ends, _, decays = optim.plan_groups([decayed, plain])
    assert ends[-1] == 1_465_922 and len(ps) == len(named) and decays == [1e-2, 0.0]


def test_schedule_objects(L):
    from pnpp_hip.optim import Schedule
    s = Schedule.cosine(total=50, warmup=5, start_factor=0.1, min_factor=0.01)
    assert abs(s.factor(0) - 0.1) < 1e-15 and abs(s.factor(5) - 1.0) < 1e-15 and abs(s.factor(50) - 0.01) < 1e-15
    assert abs(s.factor(27) - closed_form("cosine", 27, 5, 50, 0, 0.1, 0.01, 1.0)) <= 16 * ULP64
    assert Schedule(**s.to_dict()).to_dict() == s.to_dict()
    assert Schedule.step(7, 0.5).factor(15) == 0.25 and Schedule.constant(warmup=4, start_factor=0.5).factor(2) == 0.75
    open_ended = Schedule.cosine(warmup=3)
    assert open_ended.needs_total() and open_ended.with_total(40).total == 40 and not open_ended.with_total(40).needs_total()
    with pytest.raises(ValueError, match="total"):
        open_ended.factor(0)
    for bad in (lambda: Schedule("linear"), lambda: Schedule.cosine(total=5, warmup=5), lambda: Schedule.step(0, 0.5),
                lambda: Schedule.step(3, 0.0), lambda: Schedule.step(3, 1.5), lambda: Schedule.constant(warmup=-1),
                lambda: Schedule.constant(warmup=2, start_factor=1.5), lambda: Schedule.cosine(total=9, min_factor=-0.1)):
        with pytest.raises(ValueError):
            bad()


def _bare(optim, numel=20):
    """A FlatAdam's host-side fields without its device buffers: what load_state_dict checks before it copies anything."""
    opt = optim.FlatAdam.__new__(optim.FlatAdam)
    opt.params = _params(3, (2, 5), 7)
    opt.group_ends, opt.group_lr_mult, opt.group_weight_decay = [numel], [1.0], [0.0]
    opt.flat_p = torch.zeros(numel)
    opt.ema = None
    return opt


def test_load_state_dict_schema():
    from pnpp_hip import optim
    good = {"version": 1, "step_count": 3, "exp_avg": torch.zeros(20), "exp_avg_sq": torch.zeros(20), "ema": None,
            "hyper": {"lr": 1e-3, "betas": [0.9, 0.999], "eps": 1e-8, "decoupled": True, "ema_decay": 0.0},
            "layout": {"numel": 20, "ends": [20], "lr_mult": [1.0], "weight_decay": [0.0], "shapes": [[3], [2, 5], [7]]}, "schedule": None}
    opt = _bare(optim)
    for key in ("exp_avg", "layout", "schedule", "version"):
        with pytest.raises(ValueError, match="missing"):
            opt.load_state_dict({k: v for k, v in good.items() if k != key})
    with pytest.raises(ValueError, match="version"):
        opt.load_state_dict({**good, "version": 2})
    with pytest.raises(ValueError, match="elements"):
        opt.load_state_dict({**good, "layout": {**good["layout"], "numel": 21}})
    with pytest.raises(ValueError, match="elements"):
        opt.load_state_dict({**good, "exp_avg": torch.zeros(19)})
    with pytest.raises(ValueError, match="layout"):
        opt.load_state_dict({**good, "layout": {**good["layout"], "ends": [8, 20]}})
    with pytest.raises(ValueError, match="layout"):
        opt.load_state_dict({**good, "layout": {**good["layout"], "shapes": [[3], [5, 2], [7]]}})
    with pytest.raises(ValueError, match="one side"):
        opt.load_state_dict({**good, "ema": torch.zeros(20)})


def test_training_scripts_parse_the_optimiser_flags(monkeypatch):
    import train_8dir_KL as t3
    import train_multi_peaks_vonMises_KL as t2
    import train_single_peak_vonMises_KL as t1
    from pnpp_hip import trainer
    for mod in (t1, t2, t3):
        off = mod._parser().parse_args([])
        assert (off.weight_decay, off.lr_schedule, off.warmup, off.ema) == (0.0, "constant", 0, 0.0) and trainer.optim_kwargs(off) == {}
        on = mod._parser().parse_args(["--weight-decay", "0.01", "--lr-schedule", "cosine", "--warmup", "100", "--ema", "0.999"])
        kw = trainer.optim_kwargs(on)
        assert kw["weight_decay"] == 0.01 and kw["ema_decay"] == 0.999
        assert kw["schedule"].kind == "cosine" and kw["schedule"].warmup == 100 and kw["schedule"].needs_total()
        with pytest.raises(SystemExit):
            mod._parser().parse_args(["--lr-schedule", "linear"])
    monkeypatch.setenv("PNPP_WEIGHT_DECAY", "0.05")
    monkeypatch.setenv("PNPP_LR_SCHEDULE", "step")
    monkeypatch.setenv("PNPP_WARMUP", "7")
    monkeypatch.setenv("PNPP_EMA", "0.99")
    env = t1._parser().parse_args([])
    kw = trainer.optim_kwargs(env)
    assert kw["weight_decay"] == 0.05 and kw["ema_decay"] == 0.99 and kw["schedule"].kind == "step" and kw["schedule"].warmup == 7
