"""Restatements of CW_check.m:6-8 on top of the oracle's raw2iq, and the inputs of tests/test_cw_check_cpu.py and
tests/test_gpu_cw_check.py.

    phase_rotate = angle( mean( s(2:end)./s(1:(end-1)) ) );
    r = angle( s(2:end)./s(1:(end-1)) ) - phase_rotate;

`numpy_form` is the line-by-line fp64 form (NumPy's complex division is the scaled one MATLAB uses); `longdouble_form` the
same quantities without the scaled division -- (a conj b)/|b|^2 by components, arctan2, sums in longdouble.  Both return
(r, phase_rotate).  `summary(r, thr)` is what a summary row of gsmcal_cw_check_batch holds, with the event list NOT cut at
GSMCAL_CW_MAX_EVENTS.  Every case is a seeded synth.make_cw capture; test_cw_check_cpu.py asserts for each of them the margins
that make the GPU tests' comparisons (indices identical, values within 1e-10 rad) independent of the last bits of either side.
"""
import functools

import numpy as np

import gsmcal
from oracle import gsmcal_oracle as o

THR = 0.2
TILE = gsmcal.CW_TILE
N_CAPTURE = 409600                      # 4*num_frame*fread_len/2 of check_CW_samples_loss_tcp.m
_BIG = dict(n=N_CAPTURE, step=0.7, amp=100.0, noise=0.5, dc=(127.4, 127.6))
_SMALL = dict(n=4099, step=-1.1, amp=60.0, noise=0.3, dc=(127.4, 127.6))

# name -> make_cw arguments.  "drops" are (output index, samples removed): the spike is expected at n = index + 1 (1-based)
CASES = {
    "clean": dict(_BIG, drops=(), seed=11),
    "drops": dict(_BIG, drops=((8191, 3), (100000, 1), (300001, 5), (409598, 2)), seed=12),
    "small": dict(_SMALL, drops=((0, 2), (255, 1), (256, 4), (4097, 3)), seed=13),
    "dense": dict(_SMALL, drops=tuple((60 + 61 * i, 1) for i in range(67)), seed=14),
    "tiny": dict(n=3, step=0.7, amp=20.0, noise=2.0, dc=(127.4, 127.6), drops=(), seed=15),
}


def _ends(n):
    """a capture of n samples with a drop behind the first sample (n = 1) and one at the last ratio (n = N-1)"""
    return dict(_SMALL, n=n, drops=((0, 1), (n - 2, 2)))


# the smallest shapes and the tile seams (N - 1 ratios: one tile is N = TILE + 1).  N = 2 is not among the byte captures: raw2iq
# makes s(2) = -s(1) exactly, so its one ratio is -1, ON atan2's branch cut, where no margin exists; the one-ratio case is S_N2,
# a complex pair handed to CW_check
SHAPES = {
    "n3": CASES["tiny"],
    "tile": dict(_ends(TILE + 1), seed=22),
    "tile_minus_1": dict(_ends(TILE), seed=23),
    "tile_plus_1": dict(_ends(TILE + 2), seed=24),
    "two_tiles_plus_1": dict(_ends(2 * TILE + 2), seed=25),
}
ALL = dict(CASES, **{k: v for k, v in SHAPES.items() if k != "n3"})
S_N2 = np.array([3.0 + 4.0j, 1.0 - 2.0j])


@functools.lru_cache(maxsize=None)
def raw(name):
    b = gsmcal.synth.make_cw(**ALL[name])
    b.setflags(write=False)
    return b


def planted(name):
    """1-based n of the spikes the case's drops must produce"""
    return [pos + 1 for pos, _ in ALL[name]["drops"]]


def numpy_form(s):
    q = s[1:] / s[:-1]
    pr = np.angle(np.sum(q) / len(q))
    return np.angle(q) - pr, float(pr)


def longdouble_form(s):
    ar, ai = s[1:].real.astype(np.longdouble), s[1:].imag.astype(np.longdouble)
    br, bi = s[:-1].real.astype(np.longdouble), s[:-1].imag.astype(np.longdouble)
    den = br * br + bi * bi
    qr, qi = (ar * br + ai * bi) / den, (ai * br - ar * bi) / den
    m = np.longdouble(len(qr))
    pr = np.arctan2(np.sum(qi) / m, np.sum(qr) / m)
    return np.arctan2(qi, qr) - pr, pr


@functools.lru_cache(maxsize=None)
def reference(name):
    """(s, r, phase_rotate, q) of a case in the numpy form; computed once and shared (read-only)"""
    s = o.raw2iq(raw(name))
    r, pr = numpy_form(s)
    for a in (s, r):
        a.setflags(write=False)
    return s, r, pr


def summary(r, thr):
    a = np.abs(r)
    idx = np.flatnonzero(a > thr)
    return {"count": int(len(idx)), "max_abs": float(a.max()), "max_n": int(np.argmax(a)) + 1,
            "events": [(int(i) + 1, float(r[i])) for i in idx]}


def margins(name, thr=THR):
    """The figures test_cw_check_cpu.py bounds for a case: how far its restatement is from every decision an ulp could flip."""
    s, r, pr = reference(name)
    q = s[1:] / s[:-1]
    rl, prl = longdouble_form(s)
    a = np.sort(np.abs(r))
    return {"min_abs_s": float(np.abs(s).min()),
            "dist_pi": float(np.min(np.pi - np.abs(np.angle(q)))),
            "thr_margin": float(np.min(np.abs(np.abs(r) - thr))),
            "abs_mean_q": float(abs(np.sum(q) / len(q))),
            "numpy_vs_longdouble": float(max(np.max(np.abs(r - rl)), abs(pr - prl))),
            "events": [n for n, _ in summary(r, thr)["events"]],
            "lead": float(a[-1] - a[-2]) if len(a) > 1 else float("inf")}
