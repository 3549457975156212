"""fp64 restatement of apply_calibration and apply_params (include/gsmcal.h) in numpy, written from the
definition, not from the kernel: a capture's bytes with DC and I/Q imbalance removed,
    z[m] = (a_m - dc_i) + j ((b_m - dc_q) / gain - (a_m - dc_i) sin_phase) / c,   c = sqrt(1 - sin_phase^2),
resampled at x(n) = (n + delay) + 1e-6 slope_ppm (n - anchor) by pair_align's 16-tap interpolator (pair_align_ref.h / taps /
valid_mask: one interpolator in the library), turned by exp(-j (phase + (2 pi carrier_hz / sample_rate) (n - anchor))) and scaled.
Every operation of x is rounded on its own, in the order written in pair_align_ref.positions, so floor(x), the valid interval and
the statuses are identical to the kernel's; every sample is corrected before the taps are applied, where the kernel applies the
I/Q correction to the two tap sums.

apply_calibration(raw_row, sample_rate, params_row, out_len) -> dict
    out (out_len,) complex, exactly 0 where not valid;  status, first_valid, end_valid, num_valid;  x, valid (out_len,)
    scale (out_len,) = |scale| sum_k |h_k| (|Re z_k| + |Im z_k|) of the valid samples (0 elsewhere): what the rounding bound is taken of
    exact (out_len,) bool: the positions whose x is a sum of multiples of 1/4 in fp64 (the delay and the drift term)
apply_batch(raw, sample_rate, params, out_len) -> dict: out (D, out_len), info (D, 4), scale, x, exact (D, out_len)
apply_params(table_row, tuned_freq, iq_row=None, delay=0, phase=0, scale=1) -> (10,) row

Also the case builders the CPU and GPU tests share, and the bars with their derivation or their measured value.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pair_align_ref as pa  # noqa: E402

APPLY_PARAMS, APPLY_INFO_COLS = 10, 4
S_ALIGN_SKIPPED = 17
E_ARG = -1
PARAM_FIELDS = ("delay", "slope_ppm", "carrier_hz", "phase", "anchor", "scale", "dc_i", "dc_q", "gain", "sin_phase")
P = {k: i for i, k in enumerate(PARAM_FIELDS)}
K = pa.K
# columns of the calibration table and of the I/Q table that apply_params reads (GSMCAL_T_*, GSMCAL_Q_*)
T_TOTAL_SAMPLING_PPM, T_TOTAL_CARRIER_PPM, T_STATUS, TABLE_COLS = 4, 5, 9, 10
Q_DC_I, Q_DC_Q, Q_GAIN, Q_SIN_PHASE, Q_STATUS, IQ_COLS = 12, 13, 16, 17, 21, 22

# each valid sample against this restatement: 1e-11 |scale| sum_k |h_k| (|Re z_k| + |Im z_k|), the bound DESIGN 20 uses -- the
# 16-term tap sum rounds near 16 * 1.1e-16 of that, the taps differ by a few 1e-16 (sin pi mu and angle-addition constants against
# np.sinc and np.cos), the I/Q correction on the sums instead of on the samples by a few 1e-16 / c, and the de-rotation's argument
# reaches ~1e4 rad at these sizes, where one ulp is 2e-12
SAMPLE_TOL = 1e-11
# the identity row (no delay, no drift, no carrier, scale 1, gain 1, sin_phase 0) on the kernel: mu = 0 selects the sample itself
# and exp(-j 0) = 1; what is left is the one subtraction a - dc, which both sides round alike, and Q / (gain c) with gain c = 1.
# (This restatement holds the identity to SAMPLE_TOL only: np.sinc of a non-zero integer is 4e-17, not 0.)
IDENTITY_TOL = 1e-15


def iq_corrected(raw_row, p):
    """z[m] of the definition, every sample of the capture"""
    raw_row = np.asarray(raw_row, dtype=np.uint8).ravel()
    a, b = raw_row[0::2].astype(np.float64), raw_row[1::2].astype(np.float64)
    c = math.sqrt(1.0 - p[P["sin_phase"]] * p[P["sin_phase"]])
    i = a - p[P["dc_i"]]
    return i + 1j * (((b - p[P["dc_q"]]) / p[P["gain"]] - i * p[P["sin_phase"]]) / c)


def positions(p, out_len):
    """x(n), and where it is formed without a rounding that a last bit could change: a delay and a drift term that are both
    multiples of 1/4 -- the drift term is 0 at n = anchor or without drift, and at +-1000 ppm 0.001 * 250 k rounds to k / 4 exactly, so
    the issue's own delays 0, 0.5, -3.25, 11.75, -20 and n put an x on an integer every 1000th sample there.  Such an x is the same
    number on any machine that rounds each operation on its own; a kernel that fused the multiply-add would floor some of them
    the other way and fail the comparison of the info table and of the samples, which leaves none of them out."""
    x = pa.positions(p[:6], out_len)
    n = np.arange(out_len, dtype=np.float64)
    drift = (p[P["slope_ppm"]] * 1e-6) * (n - p[P["anchor"]])
    return x, (4.0 * drift == np.round(4.0 * drift)) & (4.0 * p[P["delay"]] == np.round(4.0 * p[P["delay"]]))


def apply_calibration(raw_row, sample_rate, params_row, out_len):
    assert out_len >= 1 and sample_rate > 0 and math.isfinite(sample_rate)
    p = np.asarray(params_row, dtype=np.float64).ravel()
    assert len(p) == APPLY_PARAMS
    n_samples = len(np.asarray(raw_row).ravel()) // 2
    out = {"out": np.zeros(out_len, dtype=np.complex128), "first_valid": 0, "end_valid": 0, "num_valid": 0, "x": np.full(out_len, np.nan),
           "valid": np.zeros(out_len, bool), "scale": np.zeros(out_len), "exact": np.zeros(out_len, bool)}
    if not np.all(np.isfinite(p)):
        out["status"] = S_ALIGN_SKIPPED
        return out
    assert abs(p[P["slope_ppm"]]) <= 1000.0 and p[P["gain"]] > 0.0 and abs(p[P["sin_phase"]]) < 1.0
    out["status"] = 0
    x, exact = positions(p, out_len)
    ok = pa.valid_mask(x, n_samples)
    out["x"], out["valid"], out["exact"] = x, ok, exact
    if not ok.any():
        return out
    idx = np.nonzero(ok)[0]
    assert np.all(np.diff(idx) == 1)                               # one interval
    out["first_valid"], out["end_valid"], out["num_valid"] = int(idx[0]), int(idx[-1]) + 1, len(idx)
    z = iq_corrected(raw_row, p)
    base = np.floor(x[ok])
    hk = pa.taps(x[ok] - base)
    zk = z[base.astype(np.int64)[:, None] + K[None, :]]
    n = idx.astype(np.float64)
    angle = p[P["phase"]] + (2.0 * np.pi * p[P["carrier_hz"]] / sample_rate) * (n - p[P["anchor"]])
    out["out"][ok] = p[P["scale"]] * (np.exp(-1j * angle) * np.sum(hk * zk, axis=1))
    out["scale"][ok] = abs(p[P["scale"]]) * np.sum(np.abs(hk) * (np.abs(zk.real) + np.abs(zk.imag)), axis=1)
    return out


def apply_batch(raw, sample_rate, params, out_len):
    raw = np.atleast_2d(np.asarray(raw, dtype=np.uint8))
    params = np.asarray(params, dtype=np.float64).reshape(-1, APPLY_PARAMS)
    d = len(raw)
    assert len(params) == d
    res = {"out": np.zeros((d, out_len), dtype=np.complex128), "info": np.zeros((d, APPLY_INFO_COLS)), "scale": np.zeros((d, out_len)),
           "x": np.full((d, out_len), np.nan), "exact": np.zeros((d, out_len), bool)}
    for i in range(d):
        one = apply_calibration(raw[i], sample_rate, params[i], out_len)
        res["out"][i], res["scale"][i], res["x"][i], res["exact"][i] = one["out"], one["scale"], one["x"], one["exact"]
        res["info"][i] = (one["status"], one["first_valid"], one["end_valid"], one["num_valid"])
    return res


def apply_params(table_row, tuned_freq, iq_row=None, delay=0.0, phase=0.0, scale=1.0):
    """one row of the calibration table (and one of the I/Q table) -> the parameter row; all NaN for a failed row"""
    t = np.asarray(table_row, dtype=np.float64)
    out = np.full(APPLY_PARAMS, np.nan)
    if t[T_STATUS] != 0.0 or not math.isfinite(t[T_TOTAL_SAMPLING_PPM]) or not math.isfinite(t[T_TOTAL_CARRIER_PPM]):
        return out
    e = 1e-6 * t[T_TOTAL_SAMPLING_PPM]
    f_off = 1e-6 * t[T_TOTAL_CARRIER_PPM] * float(tuned_freq)
    out[:] = (delay, t[T_TOTAL_SAMPLING_PPM], f_off * (1.0 + e), phase, 0.0, scale, 127.5, 127.5, 1.0, 0.0)
    if iq_row is not None:
        q = np.asarray(iq_row, dtype=np.float64)
        out[P["dc_i"]], out[P["dc_q"]] = q[Q_DC_I], q[Q_DC_Q]
        if q[Q_STATUS] == 0.0:
            out[P["gain"]], out[P["sin_phase"]] = q[Q_GAIN], q[Q_SIN_PHASE]
    return out


def table_row(sampling_ppm, carrier_ppm, status=0.0):
    """a hand-written row of the calibration table: only the columns apply_params reads are filled"""
    t = np.zeros(TABLE_COLS)
    t[T_TOTAL_SAMPLING_PPM], t[T_TOTAL_CARRIER_PPM], t[T_STATUS] = sampling_ppm, carrier_ppm, status
    return t


def identity_row(dc=127.5):
    return np.array([0.0, 0.0, 0.0, 0.0, 0.0, 1.0, dc, dc, 1.0, 0.0])


def x_is_safe(res):
    """no position that is not exact sits within 1e-9 of an integer (pair_align_ref.no_x_near_an_integer): a last-bit difference
    could floor it the other way.  The GPU tests assert this of every case before they compare."""
    return pa.no_x_near_an_integer(res["x"][~res["exact"]])


# ---- the tone cases (CPU test 4, and the closed loop of the GPU test) ---------------------------------------------------------------
FS_TONE = 2.048e6
CW_DC = (127.4, 127.6)                                             # synth.make_cw's default DC
# (sampling ppm e, carrier ppm c, tuned frequency f_t, baseband tone f_b, samples)
TONE_CASES = ((63.0, -21.5, 433.92e6, 100e3, 4096), (-80.0, 40.0, 1090e6, -250e3, 2048), (1000.0, 0.0, 100e6, 50e3, 1500))


def tone_step(e_ppm, c_ppm, f_t, f_b, fs=FS_TONE):
    """phase step per dongle sample of a tone f_b seen through a dongle whose clock runs e fast and whose carrier is c off: the
    dongle samples at ideal time k / (1 + e), and its carrier error turns sample k by 2 pi c 1e-6 f_t k / fs"""
    return 2.0 * math.pi * (f_b / (1.0 + 1e-6 * e_ppm) + c_ppm * 1e-6 * f_t) / fs


def tone_frequency(z, fs=FS_TONE):
    """mean phase step of a tone as a frequency: the angle of sum z[k+1] conj(z[k])"""
    z = np.asarray(z)
    return float(np.angle(np.sum(z[1:] * np.conj(z[:-1]))) * fs / (2.0 * math.pi))


# Residual tone frequency (Hz) the restatement leaves on TONE_CASES with synth.make_cw's default seed, amplitude and noise, the tone
# corrected by apply_params of the planted e and c with the known DC, measured by tone_frequency over the valid interval.  The
# uncorrected offsets are -9 335, +43 580 and -48 Hz.  What is left is estimator noise (byte rounding and the 0.5-LSB noise of the
# capture over 1 500 .. 4 096 samples) and the interpolator's pass-band ripple.
TONE_RESIDUAL_HZ = (0.669, 1.162, 2.241)
# the bar: twice the largest, for seed-to-seed estimator noise (the allowance DESIGN 20 uses)
TONE_BAR_HZ = 2 * 2.241


# ---- the designed cases of the comparison with the kernel (tests/test_gpu_apply_calibration.py) -------------------------------------
PARITY_N = (1, 15, 16, 17, 255, 256, 257, 600, 4099)
PARITY_D = (1, 3, 5)
PARITY_SLOPES = (0.0, 63.0, -63.0, 1000.0, -1000.0)
PARITY_FS = 2.4e6
IMBALANCE = (1.07, math.sin(math.radians(3.0)))                    # gain, sin_phase of the rows "with imbalance"


def parity_out_lens(n):
    return sorted({1, 255, 256, 257, n, n + 300})


def parity_delays(n):
    return (0.0, 0.5, -3.25, 11.75, -20.0, float(n))


def parity_rows(n):
    """every combination of slope, delay, anchor and imbalance for captures of n samples: 120 rows.  They cover no valid sample at
    all (n < 16, delay = n), a window clipped at either end (negative and positive delays), a tile boundary inside the drift
    (+-1000 ppm moves base by 4 samples against n over 4 099), and, with out_len = n + 300, outputs past the end of the capture."""
    rows = []
    for slope in PARITY_SLOPES:
        for delay in parity_delays(n):
            for anchor in (0.0, n / 2.0):
                for imb in (False, True):
                    k = len(rows)
                    rows.append([delay, slope, (-1) ** k * (1234.5 + 7.0 * k), 0.7 - 0.01 * k, anchor, 0.37 if imb else 1.0,
                                 127.4 if imb else 127.5, 127.6 if imb else 127.5, IMBALANCE[0] if imb else 1.0, IMBALANCE[1] if imb else 0.0])
    return np.array(rows)


def parity_batches(n):
    """the 120 rows dealt into batches of 1, 3, 5, 1, 3, 5 ... captures -> [(raw (D, 2n) uint8, params (D, 10))]"""
    rows = parity_rows(n)
    rng = np.random.Generator(np.random.Philox(key=[23, n]))
    out, at, turn = [], 0, 0
    while at < len(rows):
        d = min(PARITY_D[turn % 3], len(rows) - at)
        out.append((rng.integers(0, 256, size=(d, 2 * n), dtype=np.uint8), rows[at:at + d]))
        at, turn = at + d, turn + 1
    return out
