"""The scheduled optimiser on the GPU (csrc/optim_sched_kernels.hip through the C ABI, pnpp_hip.optim.FlatAdam, pnpp_hip.trainer.fit):
parameter groups, decoupled and L2 weight decay, the learning-rate schedule evaluated on the device, the averaged weights, resuming.

The float64 restatement and the rounding counts below extend _adam_ref / _adam_check of tests/test_gpu_tail_edges.py by what the new
kernel adds; its operation order is the comment above update_one in csrc/optim_sched_kernels.hip."""
import copy
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                                     # one float32 rounding, relative
ULP64 = 2.0 ** -53
F = lambda v: float(np.float32(v))                 # the float32 the C ABI receives, as a float64
LR, B1, B2, EPS = F(1e-3), F(0.9), F(0.999), F(1e-8)
CAP = 2048 * 256                                   # the grid cap of the scalar form: beyond it the grid-stride loop wraps
BIG_N = CAP + 5
KINDS = ("constant", "cosine", "step")
COEFS = [(1.0, 0.01), (0.5, 0.0), (0.0, 0.1), (2.0, 0.05), (1.0, 0.0), (0.25, 1e-3), (0.0, 0.0), (3.0, 0.5)]   # (lr_mult, weight_decay)


def _report(family, **errs):
    print("  worst[" + family + "] " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()))


@pytest.fixture(scope="module")
def L():
    from pnpp_hip import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _buffers(n, seed):
    """tests/test_gpu_tail_edges.py's _adam_buffers: gradients log-uniform over [1e-12, 1e3] with exact zeros, moments carried in, m
    cancelling against g at every 7th element, every 22nd element at rest (zero gradient and moments), p of order 1."""
    r = np.random.default_rng(seed)
    g = (10.0 ** r.uniform(-12, 3, n) * r.choice([-1.0, 1.0], n)).astype(np.float32)
    i = np.arange(n)
    g[i % 11 == 0] = 0.0
    sign = np.where(g != 0, np.sign(g), r.choice([-1.0, 1.0], n)) * np.where(i % 7 == 3, -1.0, 1.0)
    m = (sign * 10.0 ** r.uniform(-8, 1, n)).astype(np.float32)
    v = ((m.astype(np.float64) ** 2) * 10.0 ** r.uniform(0, 2, n)).astype(np.float32)
    still = i % 22 == 0
    m[still], v[still] = 0.0, 0.0
    p = r.normal(0, 1, n).astype(np.float32)
    return p, g, m, v, still


def _dev(a, offset=0):
    """On the device; offset = 1 puts the data 4 bytes past a 16-byte boundary (the kernel then takes its scalar form)."""
    t = torch.empty(a.size + offset, dtype=torch.from_numpy(a).dtype, device="cuda")
    t[offset:].copy_(torch.from_numpy(a.copy()))
    return t[offset:]


def closed_form(kind, s, warmup, total, every, start, mn, gamma):
    if s < warmup:
        return start + (1.0 - start) * s / warmup
    if kind == "cosine":
        return mn if s >= total else mn + (1.0 - mn) * 0.5 * (1.0 + math.cos(math.pi * (s - warmup) / (total - warmup)))
    if kind == "step":
        return max(mn, gamma ** ((s - warmup) // every))
    return 1.0


SCHED_OFF = ("constant", 0, 0, 0, 1.0, 0.0, 1.0)


def _desc(L, n, ends=None, coefs=((1.0, 0.0),), decoupled=1, sched=SCHED_OFF, gscale=1.0, max_norm=0.0, ema=0.0, zero=0):
    ends = [n] if ends is None else list(ends)
    d = L.OptimDesc()
    d.n_groups, d.decoupled = len(ends), decoupled
    for j, e in enumerate(ends):
        d.end[j], d.lr_mult[j], d.weight_decay[j] = e, coefs[j][0], coefs[j][1]
    kind, d.warmup, d.total, d.every, d.start_factor, d.min_factor, d.gamma = sched
    d.sched_kind = KINDS.index(kind)
    d.lr, d.beta1, d.beta2, d.eps, d.grad_scale, d.max_norm, d.ema_decay, d.zero_grad = LR, B1, B2, EPS, gscale, max_norm, ema, zero
    return d


def _step(L, d, p, g, m, v, state, ema=None, ss=None):
    L.check(L.lib().pnpp_adamw_step(ctypes.byref(d), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                    None if ema is None else ema.data_ptr(), p.numel(), state.data_ptr(),
                                    None if ss is None else ss.data_ptr(), _stream()))


def _rate(state):
    return float(state[2:3].view(torch.float64)[0])


# ---- 1. everything off: the existing kernel, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, BIG_N])
def test_additions_off_equals_adam_step_dev(L, n):
    """One group, multiplier 1, no decay, constant schedule, no average: p, m, v, g and both state words equal pnpp_adam_step_dev's
    (pnpp_adam_step_dev_clip's) on the same inputs, in the 16-byte form and -- buffers 4 bytes off a 16-byte boundary -- the scalar
    one."""
    lib = L.lib()
    p0, g0, m0, v0, _ = _buffers(n, n)
    scratch = torch.empty(1024 * 8, dtype=torch.uint8, device="cuda")
    for seeded, zero, (offset, clip) in itertools.product((0, 1, 999), (0, 1), ((0, False), (1, False), (0, True))):
        if n == BIG_N and (offset or clip) and seeded != 999:
            continue
        ss = None
        old = [_dev(a) for a in (p0, g0, m0, v0)]
        new = [_dev(a, offset) for a in (p0, g0, m0, v0)]
        s_old = torch.tensor([seeded, 0], dtype=torch.int64, device="cuda")
        s_new = torch.tensor([seeded, 0, 0, 0], dtype=torch.int64, device="cuda")
        ptrs = [t.data_ptr() for t in old]
        if clip:
            ss = torch.zeros(1, dtype=torch.float64, device="cuda")
            L.check(lib.pnpp_sumsq(ptrs[1], n, ss.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream()))
            max_norm = F(0.37 * math.sqrt(float(ss))) or F(1.0)            # n = 1 holds a zero gradient
            L.check(lib.pnpp_adam_step_dev_clip(*ptrs, n, s_old.data_ptr(), LR, B1, B2, EPS, 0.5, ss.data_ptr(), max_norm, zero, _stream()))
            _step(L, _desc(L, n, gscale=0.5, max_norm=max_norm, zero=zero), *new, s_new, ss=ss)
        else:
            L.check(lib.pnpp_adam_step_dev(*ptrs, n, s_old.data_ptr(), LR, B1, B2, EPS, 1.0, zero, _stream()))
            _step(L, _desc(L, n, zero=zero), *new, s_new)
        for name, a, b in zip("pgmv", old, new):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, n, seeded, zero, offset, clip)
        assert s_new[:2].tolist() == s_old.tolist() == [seeded + 1, 0] and int(s_new[3]) == 0
        assert _rate(s_new) == LR
    # the two entries alternate on one state
    p, g, m, v = (_dev(a) for a in (p0, g0, m0, v0))
    state = torch.zeros(4, dtype=torch.int64, device="cuda")
    _step(L, _desc(L, n), p, g, m, v, state)
    L.check(lib.pnpp_adam_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, state.data_ptr(), LR, B1, B2, EPS, 1.0, 0, _stream()))
    _step(L, _desc(L, n), p, g, m, v, state)
    assert state.tolist()[:2] == [3, 0]


# ---- 2. one step against float64 ---------------------------------------------------------------------------------------------------------
def _ref(p, g, m, v, s, rate, mult, wd, decoupled, gscale, coef=1.0):
    """The update in float64 on the float32 buffers, per-element mult / wd, at the rate the kernel reported."""
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    t = s + 1
    bc1, bc2 = 1.0 - B1 ** t, 1.0 - B2 ** t
    lr_g = rate * mult
    g0 = g * (gscale * coef)
    l2 = np.zeros_like(p) if decoupled else wd * p
    gi = g0 + l2
    t1, t2 = B1 * m, (1.0 - B1) * gi
    m2 = t1 + t2
    v2 = B2 * v + (1.0 - B2) * gi * gi
    gain = (lr_g / bc1) / (np.sqrt(v2) / math.sqrt(bc2) + EPS)
    dp = gain * m2
    pd = p * (1.0 - lr_g * wd) if decoupled else p
    return dict(p=pd - dp, m=m2, v=v2, dp=dp, gain=gain, mscale=np.abs(t1) + np.abs(t2), gi=gi, gabs=np.abs(g0) + np.abs(l2), pd=pd)


def _allow(ref, p0, decoupled, kg=0):
    """Bounds from counted float32 roundings (U = 2^-24 each); kg: roundings in g * grad_scale * clip (0 or 5, as _adam_check).

    tests/test_gpu_tail_edges.py's _adam_check, whose count this keeps: m carries (4 + kg) U of |b1 m| + |(1 - b1) g|, v (4 + 2 kg) U,
    p one ulp for the final subtraction + 1e-6 |dp| (16.8 U: the seven roundings of step / (sqrt(v) / sqrt(bc2) + eps) * m on top of m's
    four and half of v's four) + 2 kg U |dp|, and where m's two terms cancel the excess of m's allowance, carried through step / denom.
    Added here, one rounding each:
      step_g = (float)(lr_g / bc1)      + 1 U |dp|   (the old kernel's (float)(lr / bc1) is one of the seven; lr_g = rate * mult is float64)
      decay_g = (float)(1 - lr_g wd)    + 1 U |p| <= 1 ulp(p)        decoupled mode
      p * decay_g                       + 1 U |p decay_g| <= 1 ulp(p) decoupled mode
      L2 mode, g' = g + (wd * p): the product and the sum, two roundings: at most 2 U (|g| + |wd p|) =: 2 U gabs in g' on top of kg U |g|;
      it enters m as (1 - b1) x that and v as 2 (1 - b2) |g'| x that (+ its square), with no cancellation assumed: both are added to the
      allowances as absolute terms, and p takes m's through step / denom (the excess term) and half of v's relative one times |dp|."""
    kl = 0 if decoupled else 2
    dg = (kg + kl) * U * ref["gabs"] if kl else np.zeros_like(ref["gabs"])       # L2: error of g' beyond what (4 + kg) U of mscale covers
    m_allow = (4 + kg) * U * ref["mscale"] + (1.0 - B1) * dg
    v_extra = (1.0 - B2) * (2.0 * np.abs(ref["gi"]) * dg + dg * dg)
    v_allow = (4 + 2 * kg) * U * ref["v"] + v_extra
    ulp = np.spacing(np.maximum(np.abs(p0), np.abs(ref["p"])).astype(np.float32)).astype(np.float64)
    m_excess = np.maximum(m_allow - (4 + kg) * U * np.abs(ref["m"]), 0.0)
    v_rel = np.divide(v_extra, ref["v"], out=np.zeros_like(v_extra), where=ref["v"] > 0)
    p_allow = (3 if decoupled else 1) * ulp + (1e-6 + U + 2 * kg * U + 0.5 * v_rel) * np.abs(ref["dp"]) + ref["gain"] * m_excess
    return m_allow, v_allow, p_allow


def _check(tag, out, ref, p0, decoupled, kg=0):
    pg, mg, vg = (a.astype(np.float64) for a in out)
    m_allow, v_allow, p_allow = _allow(ref, p0, decoupled, kg)
    rm = np.abs(mg - ref["m"]) / np.maximum(m_allow, 1e-300)
    rv = np.abs(vg - ref["v"]) / np.maximum(v_allow, 1e-300)
    rp = np.abs(pg - ref["p"]) / p_allow
    sub = float(np.finfo(np.float32).tiny)       # results below the normal range carry an absolute 2^-149 instead
    rm[np.abs(ref["m"]) < sub], rv[ref["v"] < sub] = 0.0, 0.0
    w = (float(rm.max()), float(rv.max()), float(rp.max()))
    assert max(w) <= 1.0, (tag, w)
    return w


def _ends_sets(n):
    """Group layouts: 1, 2, 3 and 8 groups with ends on both sides of 1, 256 and 2048 * 256 (where n allows) and at n - 1."""
    cand = sorted({e for e in (1, 2, 255, 256, 257, CAP - 1, CAP, CAP + 1, n - 1) if 0 < e < n})
    out = [[n]]
    out += [[e, n] for e in cand]
    out += [[a, b, n] for a, b in zip(cand, cand[1:])]
    if n >= 8:
        fill = sorted(set(cand) | {int(x) for x in np.linspace(1, n - 1, 7)})
        while len(fill) > 7:                      # keep the candidates, drop filler from the middle
            extra = [e for e in fill if e not in cand]
            fill.remove(extra[len(extra) // 2] if extra else fill[len(fill) // 2])
        if len(fill) == 7:
            out.append(fill + [n])
    return out


def _sched_cases():
    """Per kind, s at 0, warmup - 1, warmup, total - 1, total, total + 5 (warmup 10, total 50, every 7)."""
    for kind in KINDS:
        for s in (0, 9, 10, 49, 50, 55):
            yield s, (kind, 10, 50, 7, 0.1, 0.05, 0.5)


@pytest.mark.parametrize("n", [1, 255, 256, 257, BIG_N])
def test_one_step_against_float64(L, n):
    """Every layout of _ends_sets with group coefficients from COEFS (wd = 0, and mult = 0 where p must come back bit-unchanged while
    m and v move), both decay modes, counts 0, 1, 999 and 99,999, grad_scale 1 and 0.5, the clip on and off, zero_grad on and off, both
    kernel forms, and every schedule kind at the edges of its pieces.  The rate in state[2] is checked first, absolutely, against the
    closed form: 16 x 2^-53 of the base rate (every intermediate is at most 1, fewer than 16 float64 roundings, cos and pow included);
    the float64 update then takes the reported rate.  Bounds: _allow."""
    lib = L.lib()
    p0, g0, m0, v0, still = _buffers(n, 3 * n + 1)
    scratch = torch.empty(1024 * 8, dtype=torch.uint8, device="cuda")
    layouts = _ends_sets(n)
    long_sched = ("cosine", 5, 200_000, 7, 0.25, 0.01, 0.5)
    cases = []
    # (s, schedule): the schedule's edges, then the four counts under a long cosine, a step and no schedule
    seq = list(_sched_cases()) + [(s, sc) for s in (0, 1, 999, 99_999) for sc in (long_sched, ("step", 2, 0, 40_000, 0.5, 0.2, 0.3), SCHED_OFF)]
    if n == BIG_N:                                    # at the large size: all six positions and every kind, then the four counts
        seq = [seq[i] for i in (1, 2, 6, 9, 10, 13, 17, 18, 22, 26, 27)]
    for i, (s, sched) in enumerate(seq):
        ends = layouts[i % len(layouts)]
        cases.append(dict(s=s, sched=sched, ends=ends, decoupled=(i // 2) % 2, gscale=(1.0, 0.5)[i % 2], clip=(i % 3 == 1),
                          zero=(i // 3) % 2, offset=int(i % 5 == 2), rot=i))
    for ends in layouts[len(seq):]:                   # layouts the cycle did not reach (small n has few cases per layout anyway)
        cases.append(dict(s=1, sched=long_sched, ends=ends, decoupled=len(ends) % 2, gscale=1.0, clip=False, zero=0, offset=0, rot=len(ends)))
    worst, worst_rate = np.zeros(3), 0.0
    idx = np.arange(n)
    for c in cases:
        ends = c["ends"]
        coefs = [COEFS[(c["rot"] + j) % len(COEFS)] for j in range(len(ends))]
        grp = np.searchsorted(np.asarray(ends), idx, side="right")       # the number of ends at or below the index
        mult, wd = (np.asarray([F(cf[k]) for cf in coefs])[grp] for k in (0, 1))
        p, g, m, v = (_dev(a, c["offset"]) for a in (p0, g0, m0, v0))
        state = torch.tensor([c["s"], 0, 0, 0], dtype=torch.int64, device="cuda")
        ss, max_norm, coef, kg = None, 0.0, 1.0, 0
        if c["clip"]:
            ss = torch.zeros(1, dtype=torch.float64, device="cuda")
            L.check(lib.pnpp_sumsq(g.data_ptr(), n, ss.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream()))
            norm = math.sqrt(math.fsum((g0.astype(np.float64) ** 2).tolist())) * c["gscale"]
            max_norm = F(norm * 0.37) if norm > 0 else F(1.0)
            coef = min(1.0, max_norm / (norm + 1e-6))
            kg = 5 if coef < 1.0 else 0
        d = _desc(L, n, ends, coefs, c["decoupled"], c["sched"], c["gscale"], max_norm, 0.0, c["zero"])
        _step(L, d, p, g, m, v, state, ss=ss)
        assert state.tolist()[:2] == [c["s"] + 1, 0] and int(state[3]) == 0, c
        rate = _rate(state)
        kind, *ps = c["sched"]
        drate = abs(rate - LR * closed_form(kind, c["s"], *ps)) / LR
        worst_rate = max(worst_rate, drate)
        assert drate <= 16 * ULP64, (c, drate / ULP64)
        ref = _ref(p0, g0, m0, v0, c["s"], rate, mult, wd, c["decoupled"], c["gscale"], coef)
        out = [t.cpu().numpy() for t in (p, m, v)]
        worst = np.maximum(worst, _check((n, c), out, ref, p0, c["decoupled"], kg))
        assert np.array_equal(g.cpu().numpy(), np.zeros_like(g0) if c["zero"] else g0)
        frozen = mult == 0.0
        assert np.array_equal(out[0][frozen].view(np.int32), p0[frozen].view(np.int32))          # lr_g = 0: p comes back bit-unchanged
        moving = frozen & (g0 != 0) & ~still
        assert not moving.any() or not np.array_equal(out[1][moving], m0[moving])                # ... while the moments move
        rest = still & (wd == 0.0)
        assert np.array_equal(out[0][rest], p0[rest])                                            # nothing to apply: p stays
    _report(f"scheduled Adam n={n}, {len(cases)} cases (fraction of the derived bound)", m=worst[0], v=worst[1], p=worst[2],
            rate_in_2pow53=worst_rate / ULP64)


# ---- 3. the averaged weights -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [0.9, 0.999, 0.9999])
def test_ema_recurrence(L, decay):
    """Eight updates; after each, e = fl(fl(d e) + fl((1 - d) p)) from the kernel's own previous e and new p: three roundings, of d e,
    of (1 - d) p and of their sum -- U of each term's magnitude (d and 1 - d are the float32 values the kernel holds)."""
    n = 1031                                                   # 257 quads and 3 odd elements, two workgroups
    p0, g0, m0, v0, _ = _buffers(n, 17)
    dF, omd = F(decay), F(1.0 - F(decay))
    worst = 0.0
    for offset in (0, 1):
        p, g, m, v = (_dev(a, offset) for a in (p0, g0, m0, v0))
        e = _dev(p0 + np.float32(0.25), offset)
        state = torch.zeros(4, dtype=torch.int64, device="cuda")
        d = _desc(L, n, [600, n], [(1.0, 0.01), (2.0, 0.0)], 1, ("cosine", 2, 8, 1, 0.5, 0.1, 1.0), ema=decay)
        for it in range(8):
            e_prev = e.cpu().numpy().astype(np.float64)
            _step(L, d, p, g, m, v, state, ema=e)
            pn = p.cpu().numpy().astype(np.float64)
            a, b = dF * e_prev, omd * pn
            allow = U * (np.abs(a) + np.abs(b) + np.abs(a + b)) + 2.0 ** -149
            worst = max(worst, float((np.abs(e.cpu().numpy().astype(np.float64) - (a + b)) / allow).max()))
        assert state.tolist()[:2] == [8, 0]
    _report(f"EMA decay={decay} (fraction of the three-rounding bound)", e=worst)
    assert worst <= 1.0


def test_no_average_leaves_the_neighbouring_memory_alone(L):
    """ema_decay = 0 takes a null ema (a buffer with it is refused before the launch); what lies behind the four buffers -- here the
    tensor an average would live in -- is untouched bit for bit, in both kernel forms."""
    n = 1031
    p0, g0, m0, v0, _ = _buffers(n, 23)
    S = 1036                                           # pitch of the five regions: a multiple of 4 floats, so offset 0 is 16-byte aligned
    for offset in (0, 1):
        block = torch.full((5 * S,), 7.25, dtype=torch.float32, device="cuda")
        views = [block[k * S + offset:k * S + offset + n] for k in range(4)]
        for t, a in zip(views, (p0, g0, m0, v0)):
            t.copy_(torch.from_numpy(a))
        before = block.clone()
        state = torch.zeros(4, dtype=torch.int64, device="cuda")
        rc = L.lib().pnpp_adamw_step(ctypes.byref(_desc(L, n)), *[t.data_ptr() for t in views], block[4 * S:].data_ptr(), n,
                                     state.data_ptr(), None, _stream())
        assert rc == L.PNPP_ERR_ARG and L.last_error().startswith("adamw_step: ") and torch.equal(block, before)
        _step(L, _desc(L, n), *views, state)
        touched = torch.zeros_like(block, dtype=torch.bool)
        for k in range(4):
            touched[k * S + offset:k * S + offset + n] = True
        assert torch.equal(block[~touched].view(torch.int32), before[~touched].view(torch.int32))
        assert not torch.equal(views[0], before[offset:offset + n]) and state.tolist()[:2] == [1, 0]


# ---- 4. twenty steps against torch.optim.AdamW / Adam --------------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [1, 0])
def test_twenty_steps_against_torch(L, decoupled):
    """Three groups, warm-up then cosine; torch.optim.AdamW (decoupled) or Adam(weight_decay=) (L2) in float64 on the CPU with a
    SequentialLR(LinearLR, CosineAnnealingLR) of the same shape and the same fixed float32 gradients, |g| in [1e-3, 1].  The parameters
    stay within the sum over the steps so far of _allow's per-step bound, evaluated along the float64 trajectory (+ 1e-12 |dp| per
    step for torch's recursive cosine, tests/test_optim_sched_cpu.py)."""
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, SequentialLR
    n, steps, ends = 777, 20, [256, 513, 777]
    coefs = [(1.0, F(0.01)), (F(0.5), 0.0), (2.0, F(0.1))]
    warmup, total, start = 4, 20, 0.25            # min_factor 0: torch's eta_min is one absolute rate for all groups
    r = np.random.default_rng(5)
    p0 = r.normal(0, 1, n).astype(np.float32)
    grads = (10.0 ** r.uniform(-3, 0, (steps, n)) * r.choice([-1.0, 1.0], (steps, n))).astype(np.float32)
    lo = [0] + ends[:-1]
    tp = [torch.nn.Parameter(torch.from_numpy(p0[a:b].astype(np.float64))) for a, b in zip(lo, ends)]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    topt = cls([{"params": [q], "lr": LR * mult, "weight_decay": wd} for q, (mult, wd) in zip(tp, coefs)], lr=LR, betas=(B1, B2), eps=EPS)
    tsched = SequentialLR(topt, [LinearLR(topt, start_factor=start, end_factor=1.0, total_iters=warmup),
                                 CosineAnnealingLR(topt, T_max=total - warmup, eta_min=0.0)], milestones=[warmup])
    grp = np.searchsorted(np.asarray(ends), np.arange(n), side="right")
    mult, wd = (np.asarray([cf[k] for cf in coefs])[grp] for k in (0, 1))
    p, m, v = _dev(p0), _dev(np.zeros(n, np.float32)), _dev(np.zeros(n, np.float32))
    state = torch.zeros(4, dtype=torch.int64, device="cuda")
    d = _desc(L, n, ends, coefs, decoupled, ("cosine", warmup, total, 1, start, 0.0, 1.0))
    budget, worst = np.zeros(n), 0.0
    for it in range(steps):
        before = np.concatenate([q.detach().numpy() for q in tp])
        tm = np.concatenate([topt.state[q]["exp_avg"].numpy() if topt.state[q] else np.zeros(q.numel()) for q in tp])
        tv = np.concatenate([topt.state[q]["exp_avg_sq"].numpy() if topt.state[q] else np.zeros(q.numel()) for q in tp])
        rate = topt.param_groups[0]["lr"]                       # group 0 has multiplier 1: the base rate torch applies at this step
        ref = _ref(before, grads[it], tm, tv, it, rate, mult, wd, decoupled, 1.0)
        budget += _allow(ref, before, decoupled)[2] + 1e-12 * np.abs(ref["dp"])
        for q, (a, b) in zip(tp, zip(lo, ends)):
            q.grad = torch.from_numpy(grads[it, a:b].astype(np.float64))
        topt.step()
        tsched.step()
        after = np.concatenate([q.detach().numpy() for q in tp])
        assert np.abs(after - ref["p"]).max() <= 1e-13           # the restatement IS torch's update (float64 reassociation only)
        _step(L, d, p, _dev(grads[it]), m, v, state)
        assert abs(_rate(state) - rate) <= 1e-12 * LR
        worst = max(worst, float((np.abs(p.cpu().numpy().astype(np.float64) - after) / budget).max()))
    _report(f"20 steps vs torch, decoupled={decoupled} (fraction of the summed per-step bound)", p=worst)
    assert worst <= 1.0


# ---- 5. a captured step follows the schedule -------------------------------------------------------------------------------------------
def _vm_models():
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    torch.manual_seed(7)
    m1 = PointNetPPVonMises(sampler="device").cuda().train()
    m1.drop.p = 0.0
    return m1, copy.deepcopy(m1)


def test_captured_step_follows_the_schedule(oracle):
    """GraphedStep(fused_optimizer=True) over FlatAdam(decay_groups(model, 1e-2), cosine(total=6, warmup=2, min_factor=0.1), ema 0.99):
    six replays against six eager zero_grad / backward / step() iterations on a deep copy -- flat_p, both moments, the average and the
    rate word equal bit for bit after every step; the six rates are distinct, rise over the warm-up and fall after it, and are
    current_lr()'s within the allowance of the rate check."""
    from pnpp_hip import ops, optim, sampling
    from pnpp_hip.graph import GraphedStep
    m1, m2 = _vm_models()
    mk = lambda m: optim.FlatAdam(optim.decay_groups(m, 1e-2), lr=1e-3, schedule=optim.Schedule.cosine(total=6, warmup=2, min_factor=0.1),
                                  ema_decay=0.99)
    o1, o2 = mk(m1), mk(m2)
    assert o1.n_groups == 2 and o1.numel == 1_465_922
    xyz, mu_gt, kappa_gt, _ = oracle.synthetic_clouds(8, 1024, seed=4)
    xyz, mu_gt, kappa_gt = xyz.cuda(), mu_gt.cuda(), kappa_gt.cuda()
    loss_fn = lambda model: (lambda x, m, k: ops.kl_von_mises_single(*model(x), m, k).mean())
    g = GraphedStep(o1, loss_fn(m1), [xyz, mu_gt, kappa_gt], fused_optimizer=True)
    assert o1.step_count == 0 and torch.equal(o1.flat_p, o2.flat_p) and torch.equal(o1.ema, o2.ema)   # capturing is not stepping
    for a, b in zip(m1.buffers(), m2.buffers()):
        a.copy_(b)
    rates = []
    for it in range(6):
        want = o2.current_lr()
        sampling.reset(10 * it)
        l1 = float(g(xyz, mu_gt, kappa_gt).detach())
        sampling.reset(10 * it)
        o2.zero_grad()
        l2 = loss_fn(m2)(xyz, mu_gt, kappa_gt)
        l2.backward()
        o2.step()
        assert l1 == float(l2), it
        for name in ("flat_p", "exp_avg", "exp_avg_sq", "ema"):
            assert torch.equal(getattr(o1, name).view(torch.int32), getattr(o2, name).view(torch.int32)), (it, name)
        assert torch.equal(o1._step_state, o2._step_state) and o1._step_state.tolist()[:2] == [it + 1, 0]
        rates.append(float(o1.last_lr))
        assert abs(rates[-1] - want) <= 16 * ULP64 * o1.lr and o1.current_lr() == o2.current_lr()
    assert len(set(rates)) == 6 and rates[0] < rates[1] < rates[2] and rates[2] > rates[3] > rates[4] > rates[5]
    assert not torch.equal(o1.ema, o1.flat_p) and float(o1.flat_g.abs().max()) == 0.0


# ---- 6. resume ----------------------------------------------------------------------------------------------------------------------------
def _small_opt(seed=3, **kw):
    from pnpp_hip import optim
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g).cuda()) for s in ((64, 3), (64,), (33, 64), (7,))]
    groups = [{"params": [q for q in ps if q.ndim >= 2], "weight_decay": 0.05}, {"params": [q for q in ps if q.ndim < 2], "lr_mult": 0.5}]
    return optim.FlatAdam(groups, lr=1e-3, schedule=optim.Schedule.cosine(total=6, warmup=2), ema_decay=0.9, **kw)


def test_optimiser_state_dict_resumes_bit_for_bit():
    g = torch.Generator().manual_seed(11)
    straight, first = _small_opt(), _small_opt()
    grads = [torch.randn(straight.numel, generator=g).cuda() for _ in range(6)]
    for it in range(6):
        straight.flat_g.copy_(grads[it])
        if it % 2:
            straight.clip_grad_norm_(1.0, return_norm=False)
        straight.step(zero_grad=True)
    for it in range(3):
        first.flat_g.copy_(grads[it])
        if it % 2:
            first.clip_grad_norm_(1.0, return_norm=False)
        first.step(zero_grad=True)
    sd = copy.deepcopy(first.state_dict())
    second = _small_opt(seed=99)                                   # fresh objects: other weights until the saved ones are put back
    second.flat_p.copy_(first.flat_p)
    second.load_state_dict(sd)
    assert second.step_count == 3 and float(second.last_lr) == float(first.last_lr)
    for it in range(3, 6):
        second.flat_g.copy_(grads[it])
        if it % 2:
            second.clip_grad_norm_(1.0, return_norm=False)
        second.step(zero_grad=True)
    for name in ("flat_p", "exp_avg", "exp_avg_sq", "ema", "_step_state"):
        assert torch.equal(getattr(straight, name), getattr(second, name)), name
    from pnpp_hip import optim
    with pytest.raises(ValueError, match="elements"):
        optim.FlatAdam([torch.nn.Parameter(torch.zeros(5).cuda())], weight_decay=0.1).load_state_dict(sd)


def _fit_setup():
    import synthetic
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    from pnpp_hip import ops, sampling, trainer
    torch.manual_seed(42)
    sampling.reset(0)
    for c in ops._dropout_counters.values():                       # the in-kernel dropout's stream restarts too: a run is its seed's
        c.zero_()
    dev = torch.device("cuda", torch.cuda.current_device())
    model = PointNetPPVonMises(sampler="device").to(dev)
    xyz, mu, kap, _ = synthetic.rotated_clouds(64, 256, seed=5)
    data = [xyz, torch.stack([mu, kap], 1)]
    loaders = {"train": trainer.SyntheticLoader(data, 8, True, dev), "val": trainer.SyntheticLoader([t[:16] for t in data], 8, False, dev)}
    loss = lambda m, b: ops.vm_head_kl_loss(m.features(b[0]), b[1][:, 0].contiguous(), b[1][:, 1].contiguous(), reduction="none")
    return trainer, model, loaders, loss, dev


FIT_KW = dict(weight_decay=1e-2, ema_decay=0.99, clip_norm=1.0, log=lambda *_: None)


def test_fit_resumes_bit_for_bit(tmp_path, monkeypatch):
    """64 clouds of 256 points, batch 8, shuffled: four epochs straight against two epochs, a checkpoint, and fit(resume=) for two
    more from fresh objects.  Final weights, average and the train / val / lr histories are equal bit for bit (the captured step is
    bitwise the eager one: tests/test_gpu_e2e.py::test_hipgraph_replays_are_bitwise_reproducible)."""
    from pnpp_hip import optim
    kept = {}
    real = optim.FlatAdam

    def keeping(*a, **kw):
        kept["opt"] = real(*a, **kw)
        return kept["opt"]

    monkeypatch.setattr(optim, "FlatAdam", keeping)
    sched = lambda: optim.Schedule.cosine(total=32, warmup=5, min_factor=0.05)
    trainer, model, loaders, loss, dev = _fit_setup()
    h4, best4, ep4 = trainer.fit(model, loss, loaders, 4, 1e-3, dev, schedule=sched(), **FIT_KW)
    o4 = kept["opt"]
    trainer, model, loaders, loss, dev = _fit_setup()
    ck = tmp_path / "run.ckpt"
    h2, _, _ = trainer.fit(model, loss, loaders, 2, 1e-3, dev, schedule=sched(), checkpoint=ck, **FIT_KW)
    assert h2["train"] == h4["train"][:2] and h2["lr"] == h4["lr"][:2] and ck.exists()
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    torch.manual_seed(1234)                                        # a fresh process would not share the first leg's generator state
    fresh = PointNetPPVonMises(sampler="device").to(dev)
    hr, bestr, epr = trainer.fit(fresh, loss, loaders, 4, 1e-3, dev, schedule=sched(), resume=ck, **FIT_KW)
    orr = kept["opt"]
    for name in ("flat_p", "exp_avg", "exp_avg_sq", "ema", "_step_state"):
        assert torch.equal(getattr(o4, name), getattr(orr, name)), name
    assert hr["train"] == h4["train"] and hr["val"] == h4["val"] and hr["lr"] == h4["lr"] and len(hr["lr"]) == 4
    assert epr == ep4 and all(torch.equal(best4[k], bestr[k]) for k in best4)
    assert orr.step_count == 32 and hr["ema"] is True


# ---- 7. the averaged weights in use -----------------------------------------------------------------------------------------------------
def test_ema_weights_context(oracle):
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    from pnpp_hip import ops, optim
    from pnpp_hip.inference import Predictor
    torch.manual_seed(3)
    model = PointNetPPVonMises(sampler="device").cuda().train()
    opt = optim.FlatAdam(optim.decay_groups(model, 1e-2), lr=1e-3, ema_decay=0.9)
    xyz, mu_gt, kappa_gt, _ = oracle.synthetic_clouds(4, 1024, seed=9)
    xyz, mu_gt, kappa_gt = xyz.cuda(), mu_gt.cuda(), kappa_gt.cuda()
    for _ in range(3):
        opt.zero_grad()
        ops.kl_von_mises_single(*model(xyz), mu_gt, kappa_gt).mean().backward()
        opt.step()
    torch.manual_seed(7)
    centres = [c.cuda() for c in oracle.replay_centres(4)]
    live_p, live_e = opt.flat_p.clone(), opt.ema.clone()
    assert not torch.equal(live_p, live_e)
    sd = opt.ema_state_dict(model)
    assert torch.equal(opt.flat_p, live_p) and torch.equal(opt.ema, live_e)
    other = PointNetPPVonMises(sampler="device").cuda()
    other.load_state_dict(sd)
    model.eval(), other.eval()
    with torch.no_grad():
        want = other(xyz, centres=centres)
        outside = Predictor(model)(xyz, centres=centres)
        with opt.ema_weights():
            got = model(xyz, centres=centres)
            assert torch.equal(opt.flat_p, live_e) and torch.equal(opt.ema, live_p)
            assert all(torch.equal(v, sd[k]) for k, v in model.state_dict().items())
            inside = Predictor(model)(xyz, centres=centres)
            with pytest.raises(RuntimeError, match="ema_weights"):
                opt.step()
    assert torch.equal(opt.flat_p.view(torch.int32), live_p.view(torch.int32)) and torch.equal(opt.ema.view(torch.int32), live_e.view(torch.int32))
    for a, b in zip(got, want):
        assert torch.equal(a, b)                                   # the context IS the model loaded from ema_state_dict
    for i, (a, b, c) in enumerate(zip(inside, got, outside)):      # tests/test_gpu_inference.py's whole-model gate
        gate = 1e-4 * max(1.0, float(b.abs().max()))
        dlt = float((a.double() - b.double()).abs().max())
        print(f"  output {i}: |predictor inside - eval inside| = {dlt:.3e} (gate {gate:.1e}); inside - outside {float((a - c).abs().max()):.3e}")
        assert dlt <= gate
    assert any(not torch.equal(a, c) for a, c in zip(inside, outside))
    with pytest.raises(RuntimeError, match="ema_decay"):
        with optim.FlatAdam([torch.nn.Parameter(torch.zeros(4).cuda())]).ema_weights():
            pass


# ---- 8. fit with everything on -------------------------------------------------------------------------------------------------------------
def test_fit_with_every_option_and_the_split_step_refusal(tmp_path):
    from pnpp_hip import optim
    from pnpp_hip.graph import GraphedSplitStep
    trainer, model, loaders, loss, dev = _fit_setup()
    sched = optim.Schedule.cosine(warmup=3, min_factor=0.1)         # total from fit: 2 epochs x 8 steps
    hist, best, ep = trainer.fit(model, loss, loaders, 2, 1e-3, dev, schedule=sched, checkpoint=tmp_path / "c.ckpt", **FIT_KW)
    want = [LR * sched.with_total(16).factor(s) for s in (7, 15)]            # the rate of each epoch's last update
    assert hist["ema"] is True and len(hist["lr"]) == 2
    assert all(abs(a - b) <= 16 * ULP64 * LR for a, b in zip(hist["lr"], want)), (hist["lr"], want)
    assert hist["lr"][1] < hist["lr"][0] < 1e-3 * 1.0000001 and all(v == v for v in hist["train"] + hist["val"])
    assert hist["steps"]["graph"] >= 12 and ep in (1, 2) and (tmp_path / "c.ckpt").exists()
    # best_state holds the averaged weights, not the live ones
    ck = torch.load(tmp_path / "c.ckpt", map_location="cpu", weights_only=False)
    key = "sa1.convs.0.weight"
    assert torch.equal(best[key].cpu(), ck["best"][1][key]) and not torch.equal(best[key].cpu(), ck["model"][key])
    two = _small_opt()
    with pytest.raises(ValueError, match="one parameter group"):
        GraphedSplitStep(two, lambda *a: a, lambda *a: a[0].sum(), [torch.zeros(1).cuda()], 0)
    # the defaults still go through the entries they always went through
    one = optim.FlatAdam([torch.nn.Parameter(torch.ones(9).cuda())])
    assert one._scheduled is False and one.n_groups == 1 and one._step_state.numel() == 4 and one.ema is None
