"""tests/golden/tail_edges.npz: an independent reference for the von-Mises loss tail at its branch edges.

Plain Python + mpmath (60 significant digits); nothing here comes from the reference tree, from Cephes or from torch.
The float32 inputs are taken as the exact rationals they are; every result is rounded once to float64.

    bessel_kappa (n,)  float32   every kappa of the sweep
    bessel       (n,3) float64   log I0(k), A(k) = I1/I0, A'(k) = 1 - A^2 - A/k   (A'(0) = 1/2)
    inputs       (N,4) float32   mu_p, kappa_p, mu_q, kappa_q: the full grid kappa_p x kappa_q x (mu_p - mu_q), mu_q = 0
    single       (N,3) float64   single-peak KL (train_single_peak_vonMises_KL.py:23-28, with its kappa_p <= 1e-6 -> a1 = 0
                                 branch), d/d mu_p, d/d kappa_p
    multi        (N,3) float64   multi-peak KL (train_multi_peaks_vonMises_KL.py:38-52: kappa clamped to [1e-6, 500], angle
                                 wrapped to [-pi, pi)), d/d mu_p, d/d kappa_p with the clamp's gate (zero outside [1e-6, 500])

The sweep sits ON the series switch of i0e / i1e (8) and one float32 either side of the thresholds 1e-6 and 500 -- never on
float32(1e-6) or float32(500.0) themselves: there a float32 and a float64 comparison legitimately disagree.

usage: python oracle/make_tail_golden.py [out.npz]      (default: tests/golden/tail_edges.npz)
"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = os.path.join(ROOT, "tests", "golden", "tail_edges.npz")
DPS = 60


def _f32(x):
    return np.float32(x)


def _up(x):
    return np.nextafter(np.float32(x), np.float32(np.inf), dtype=np.float32)


def _down(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf), dtype=np.float32)


def sweep():
    """The grid of the issue, as float32: (kappa_p, kappa_q, mu_p - mu_q)."""
    kp = [0.0, 1e-7, _down(1e-6), _up(1e-6), 1e-4, 0.5, 7.999, 8.0, _up(8.0), 8.5, 50.0, 88.0, 89.0, _down(500.0), _up(500.0),
          1e4, 1e6]
    kq = [0.0, 1e-6, 8.0, 30.0, 500.0]
    d = [0.0, 1e-4, 1.0, 3.1, np.float32(np.pi), -np.float32(np.pi), 2.0 * np.pi]
    kp, kq, d = (np.array(v, dtype=np.float32) for v in (kp, kq, d))
    assert _f32(1e-6) not in kp and _f32(500.0) not in kp
    return kp, kq, d


def compute():
    import mpmath as mp
    mp.mp.dps = DPS
    kp, kq, d = sweep()
    one, half = mp.mpf(1), mp.mpf(1) / 2
    lo, hi = mp.mpf("1e-6"), mp.mpf(500)

    def exact(x):
        return mp.mpf(float(x))                      # a float32 is a float64 is an exact mpf

    def log_i0(k):
        return mp.log(mp.besseli(0, k)) if k > 0 else mp.mpf(0)

    def ratio(k):
        return mp.besseli(1, k) / mp.besseli(0, k) if k > 0 else mp.mpf(0)

    def ratio_prime(k):
        if k == 0:
            return half
        a = ratio(k)
        return one - a * a - a / k

    def single(mp_, kp_, mq_, kq_):
        dd = mp_ - mq_
        a = ratio(kp_)
        base = log_i0(kq_) - log_i0(kp_)
        if kp_ <= lo:                                # a1 := 0: only -log I0(kappa_p) depends on the prediction
            return base, mp.mpf(0), -a
        c, s = mp.cos(dd), mp.sin(dd)
        return base + kp_ * a - kq_ * a * c, kq_ * a * s, ratio_prime(kp_) * (kp_ - kq_ * c)

    def multi(mp_, kp_raw, mq_, kq_raw):
        kp_, kq_ = min(max(kp_raw, lo), hi), min(max(kq_raw, lo), hi)
        two_pi = 2 * mp.pi
        dd = mp_ - mq_ + mp.pi
        dd = dd - two_pi * mp.floor(dd / two_pi) - mp.pi    # python's %: the sign of the divisor
        a = ratio(kp_)
        c, s = mp.cos(dd), mp.sin(dd)
        gate = lo <= kp_raw <= hi                    # torch.clamp passes the gradient on the closed interval
        return (log_i0(kq_) - log_i0(kp_) + a * (kp_ - kq_ * c), a * kq_ * s,
                ratio_prime(kp_) * (kp_ - kq_ * c) if gate else mp.mpf(0))

    ks = np.unique(np.concatenate([kp, kq]))
    bessel = np.array([[float(log_i0(exact(k))), float(ratio(exact(k))), float(ratio_prime(exact(k)))] for k in ks], dtype=np.float64)
    rows = [(dv, a, np.float32(0.0), b) for a in kp for b in kq for dv in d]
    inputs = np.array(rows, dtype=np.float32)
    s_out = np.array([[float(v) for v in single(*map(exact, r))] for r in inputs], dtype=np.float64)
    m_out = np.array([[float(v) for v in multi(*map(exact, r))] for r in inputs], dtype=np.float64)
    return {"bessel_kappa": ks.astype(np.float32), "bessel": bessel, "inputs": inputs, "single": s_out, "multi": m_out}


def npz_bytes(arrays) -> bytes:
    """An .npz (np.load reads it) whose bytes depend on the arrays alone: fixed member order, fixed timestamp, stored."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            member = io.BytesIO()
            np.lib.format.write_array(member, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, member.getvalue())
    return buf.getvalue()


def main(argv):
    out = argv[1] if len(argv) > 1 else DEFAULT
    data = npz_bytes(compute())
    with open(out, "wb") as f:
        f.write(data)
    print(f"wrote {out}: {len(data)} bytes")


if __name__ == "__main__":
    main(sys.argv)
