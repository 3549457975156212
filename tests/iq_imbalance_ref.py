"""Restatement of the I/Q imbalance and clipping check (include/gsmcal.h) for tests/test_iq_imbalance_cpu.py and
tests/test_gpu_iq_imbalance.py.

`raw_row(bytes)` is the raw form: the five sums, A_I, A_Q and C as Python ints -- exact whatever N -- then `math` in exactly the
order the header states, each integer converted to a float once.  `complex_row(s)` is the complex form in fp64 numpy, and
`correct(s, gain, sin_phase)` the numpy twin of gsmcal_iq_correct.  A row is a list of IQ_COLS floats in the order of
gsmcal.IQ_FIELDS."""
import math

import numpy as np

import gsmcal

COLS = gsmcal.IQ_COLS
TILE = gsmcal.IQ_TILE
F = {k: i for i, k in enumerate(gsmcal.IQ_FIELDS)}
NAN, INF = float("nan"), float("inf")


def moments(raw):
    """(N, S_I, S_Q, S_II, S_QQ, S_IQ, A_I, A_Q, C) of an interleaved byte capture as Python ints"""
    raw = np.asarray(raw, dtype=np.uint8).ravel()
    a, b = raw[0::2].astype(np.int64), raw[1::2].astype(np.int64)
    n = len(a)
    s_i, s_q = int(a.sum()), int(b.sum())                       # N <= 2^23 bytes: the int64 sums are exact (< 2^39)
    s_ii, s_qq, s_iq = int((a * a).sum()), int((b * b).sum()), int((a * b).sum())
    return n, s_i, s_q, s_ii, s_qq, s_iq, n * s_ii - s_i * s_i, n * s_qq - s_q * s_q, n * s_iq - s_i * s_q


def derive(row, n, s_i, s_q, a_i, a_q, c):
    """columns 12.. of `row` from floats that were each converted once; the order of operations is the header's"""
    nf = float(n)
    row[F["dc_I"]], row[F["dc_Q"]] = s_i / nf, s_q / nf
    for k in ("var_I", "var_Q", "gain", "sin_phase", "phase_deg", "irr_db", "level_dbfs"):
        row[F[k]] = NAN
    if n < 2:
        row[F["status"]] = float(gsmcal.IQ_SHORT)
        return row
    nn = nf * nf
    var_i, var_q = a_i / nn, a_q / nn
    row[F["var_I"]], row[F["var_Q"]] = var_i, var_q
    lvl = (var_i + var_q) / 32512.5
    row[F["level_dbfs"]] = 10.0 * math.log10(lvl) if lvl > 0.0 else -INF
    if not a_i > 0.0 or not a_q > 0.0:
        row[F["status"]] = float(gsmcal.IQ_FLAT)
        return row
    gain = math.sqrt(a_q / a_i)
    s = c / (math.sqrt(a_i) * math.sqrt(a_q))
    s = 1.0 if s > 1.0 else -1.0 if s < -1.0 else s
    cs = math.sqrt(1.0 - s * s)
    k = 2.0 * gain * s * s / (1.0 + cs)
    num, den = (gain + 1.0) * (gain + 1.0) - k, (gain - 1.0) * (gain - 1.0) + k
    row[F["gain"]], row[F["sin_phase"]] = gain, s
    row[F["phase_deg"]] = math.asin(s) * 180.0 / math.pi
    row[F["irr_db"]] = INF if den == 0.0 else 10.0 * math.log10(num / den)
    row[F["status"]] = float(gsmcal.IQ_OK)
    return row


def raw_row(raw):
    raw = np.asarray(raw, dtype=np.uint8).ravel()
    n, s_i, s_q, s_ii, s_qq, s_iq, a_i, a_q, c = moments(raw)
    a, b = raw[0::2], raw[1::2]
    row = [0.0] * COLS
    row[:12] = [float(n), float(s_i), float(s_q), float(s_ii), float(s_qq), float(s_iq), float(a.min()), float(a.max()),
                float(b.min()), float(b.max()), float(np.count_nonzero((a == 0) | (a == 255))),
                float(np.count_nonzero((b == 0) | (b == 255)))]
    return derive(row, n, float(s_i), float(s_q), float(a_i), float(a_q), float(c))


def raw_table(raw2d):
    return np.array([raw_row(r) for r in np.atleast_2d(raw2d)])


def complex_row(s):
    """the complex form: the sums, A_I, A_Q and C in fp64 (numpy's pairwise sums)"""
    s = np.asarray(s, dtype=np.complex128).ravel()
    x, y = s.real, s.imag
    n = len(s)
    s_i, s_q, s_ii, s_qq, s_iq = float(x.sum()), float(y.sum()), float((x * x).sum()), float((y * y).sum()), float((x * y).sum())
    row = [0.0] * COLS
    row[:12] = [float(n), s_i, s_q, s_ii, s_qq, s_iq, float(x.min()), float(x.max()), float(y.min()), float(y.max()), NAN, NAN]
    nf = float(n)
    return derive(row, n, s_i, s_q, nf * s_ii - s_i * s_i, nf * s_qq - s_q * s_q, nf * s_iq - s_i * s_q)


def abs_term_sums(s):
    """sum |terms| of the five sums of the complex form: the scale of their rounding-error bound"""
    s = np.asarray(s, dtype=np.complex128).ravel()
    x, y = np.abs(s.real), np.abs(s.imag)
    return [float(x.sum()), float(y.sum()), float((x * x).sum()), float((y * y).sum()), float((x * y).sum())]


def correct(s, gain, sin_phase):
    """numpy twin of gsmcal_iq_correct on one stream: out_I = I, out_Q = (Q/g - I*s)/c"""
    s = np.asarray(s, dtype=np.complex128)
    c = math.sqrt(1.0 - sin_phase * sin_phase)
    return s.real + 1j * ((s.imag / gain - s.real * sin_phase) / c)


def to_complex(raw):
    """the bytes as a complex stream without the DC removed (the moments do not care)"""
    raw = np.asarray(raw, dtype=np.uint8).ravel()
    return raw[0::2].astype(np.float64) + 1j * raw[1::2].astype(np.float64)


def ulps(a, b):
    """distance of two finite doubles in units in the last place"""
    ia, ib = np.float64(a).view(np.int64), np.float64(b).view(np.int64)
    ia = ia if ia >= 0 else np.int64(-2 ** 63) - ia
    ib = ib if ib >= 0 else np.int64(-2 ** 63) - ib
    return abs(int(ia) - int(ib))
