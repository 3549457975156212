"""fp64 restatement of row_coherence and apply_params_refine (include/gsmcal.h) in numpy, written from the
definition, not from the kernels: pair_coherence's estimator (tests/pair_coherence_ref.py) on any rows on one nominal time base, over
a caller's list of windows of one length.  Also the designed rows, the wideband closed loop and the bars the CPU and GPU tests share.

row_coherence(x, a, b, lag0, starts, win_len, fs, max_lag, min_coherence, max_gap, valid) -> dict
    row        (ROW_COLS,) the table row (api.ROW_FIELDS, then start | delay | phase | freq | coherence | edge)
    corr       (W, 2M+1, 4) complex, NaN where a window was not evaluated
    ea, eb     (W, 4), (W, 2M+1, 4): the energies under the same sums
    babs       (W, 2M+1, 4): sum (|Re b| + |Im b|)(|Re a| + |Im a|) under the same sums -- what the rounding bound of corr is taken of
    evaluated, edge, used   (W,) bool;  mstar (W,) int (0 where not evaluated)
  and, per evaluated window, pair_coherence_ref's tie diagnostics: gap, curvature, coh_margin (ties_ok reads them).
apply_params_refine(coh_row, params_in, variant=None) -> (status, (10,) row): Python floats, every operation rounded on its own, in
    the order of csrc/apply_refine.h; variant names one of the four WRONG compositions the closed loop must tell from the right one.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pair_coherence_ref as pcr  # noqa: E402

MAX_ROW_WINDOWS, MAX_ROW_LAG, ROW_CHUNK = 128, 64, 512
ROW_COLS = 20 + 6 * MAX_ROW_WINDOWS
K = 4
S_PAIR_FEW, S_ALIGN_SKIPPED, E_ARG = 16, 17, -1
HEAD = ("status", "num_windows", "num_eval", "num_used", "num_adjacent", "lag0", "delay0", "rel_sampling_ppm", "delay_rms",
        "rel_carrier_hz", "window_carrier_hz", "phase0", "phase_rms", "mean_coherence", "min_coherence_seen", "max_lag",
        "win_len", "sample_rate", "min_coherence", "max_gap")
WINDOW = ("start", "delay", "phase", "freq", "coherence", "edge")
wrap = pcr.wrap
ties_ok = pcr.ties_ok


def col(name):
    """first column of a per-window field, or the column of a head field"""
    return HEAD.index(name) if name in HEAD else 20 + WINDOW.index(name) * MAX_ROW_WINDOWS


def row_coherence(x, a, b, lag0, starts, win_len, fs, max_lag=16, min_coherence=0.5, max_gap=None, valid=None):
    x = np.atleast_2d(np.asarray(x, dtype=np.complex128))
    d, stride = x.shape
    starts = [int(s) for s in np.asarray(starts).ravel()]
    W, M, lag0 = len(starts), int(max_lag), int(lag0)
    max_gap = 8.0 * win_len if max_gap is None else float(max_gap)
    assert 1 <= W <= MAX_ROW_WINDOWS and 16 <= win_len <= 65536 and 1 <= M <= MAX_ROW_LAG and 0 <= a < d and 0 <= b < d
    assert all(s >= 0 for s in starts) and all(s1 > s0 for s0, s1 in zip(starts, starts[1:])) and 0.0 <= min_coherence <= 1.0 and max_gap >= 0
    valid = np.array([[0, stride]] * d) if valid is None else np.asarray(valid, dtype=np.int64).reshape(d, 2)
    Ls, NL = win_len // 4, 2 * M + 1
    row = np.full(ROW_COLS, np.nan)
    out = {"row": row, "corr": np.full((W, NL, K), np.nan + 1j * np.nan), "ea": np.full((W, K), np.nan), "eb": np.full((W, NL, K), np.nan),
           "babs": np.full((W, NL, K), np.nan), "evaluated": np.zeros(W, bool), "edge": np.zeros(W, bool), "used": np.zeros(W, bool),
           "mstar": np.zeros(W, int), "gap": np.full(W, np.nan), "curvature": np.full(W, np.nan), "coh_margin": np.full(W, np.nan),
           "M": M, "Ls": Ls}
    row[col("num_windows")], row[col("lag0")], row[col("max_lag")] = W, lag0, M
    row[col("win_len")], row[col("sample_rate")], row[col("min_coherence")], row[col("max_gap")] = win_len, fs, min_coherence, max_gap
    xa, xb = x[a], x[b]
    (first_a, end_a), (first_b, end_b) = valid[a], valid[b]
    delay, phase, freq, coh = (np.full(W, np.nan) for _ in range(4))
    view = np.lib.stride_tricks.sliding_window_view
    for j, p in enumerate(starts):
        if not (first_a <= p and p + 4 * Ls <= end_a and first_b <= p + lag0 - M and p + lag0 + M + 4 * Ls <= end_b):
            continue
        out["evaluated"][j] = True
        row[col("start") + j] = p
        c, eb, ba = np.empty((NL, K), dtype=np.complex128), np.empty((NL, K)), np.empty((NL, K))
        for k in range(K):
            av = xa[p + k * Ls: p + (k + 1) * Ls]
            lo = p + lag0 - M + k * Ls
            bw = view(xb[lo: lo + Ls + 2 * M], Ls)                 # (NL, Ls): b at the lags -M .. M
            out["ea"][j, k] = np.sum(np.abs(av) ** 2)
            c[:, k] = np.sum(bw * np.conj(av), axis=1)
            eb[:, k] = np.sum(np.abs(bw) ** 2, axis=1)
            ba[:, k] = (np.abs(bw.real) + np.abs(bw.imag)) @ (np.abs(av.real) + np.abs(av.imag))
        out["corr"][j], out["eb"][j], out["babs"][j] = c, eb, ba
        y = np.sum(np.abs(c) ** 2, axis=1)
        ms = int(np.argmax(y))                                     # the first maximum
        out["mstar"][j] = ms - M
        ys = np.sort(y)
        out["gap"][j] = (ys[-1] - ys[-2]) / ys[-1] if ys[-1] > 0 else np.inf      # (y all exact zeros -- a zero row: the first lag, no last bit to differ)
        if ms == 0 or ms == NL - 1:
            out["edge"][j] = True
            row[col("edge") + j] = 1.0
            continue
        row[col("edge") + j] = 0.0
        den = y[ms - 1] - 2 * y[ms] + y[ms + 1]
        out["curvature"][j] = abs(den) / y[ms]
        delay[j] = lag0 + (ms - M) + 0.5 * (y[ms - 1] - y[ms + 1]) / den
        cm = c[ms]
        th = np.angle(np.sum(cm[1:] * np.conj(cm[:-1])))
        freq[j] = th * fs / (2 * np.pi * Ls)
        phase[j] = np.angle(np.sum(cm * np.exp(-1j * th * (np.arange(K) - 1.5))))
        e = math.sqrt(np.sum(out["ea"][j]) * np.sum(eb[ms]))
        coh[j] = np.sum(np.abs(cm)) / e if e > 0 else np.nan
        out["coh_margin"][j] = abs(coh[j] - min_coherence) if e > 0 else np.inf      # (0 / 0: NaN, never used, no tie)
        out["used"][j] = bool(coh[j] >= min_coherence)
    for name, v in (("delay", delay), ("phase", phase), ("freq", freq), ("coherence", coh)):
        row[col(name): col(name) + W] = v
    used = np.nonzero(out["used"])[0]
    row[col("num_eval")], row[col("num_used")], row[col("num_adjacent")] = np.sum(out["evaluated"]), len(used), 0
    if len(used) < 2:
        row[0] = S_PAIR_FEW
        return out
    row[0] = 0.0
    p_all = np.array(starts, dtype=np.float64)
    t = p_all[used] - p_all[used[0]]
    dl, ph = delay[used], phase[used]
    tb, db = np.mean(t), np.mean(dl)
    slope = np.sum((t - tb) * (dl - db)) / np.sum((t - tb) ** 2)
    d0 = db - slope * tb
    row[col("delay0")], row[col("rel_sampling_ppm")] = d0, 1e6 * slope
    row[col("delay_rms")] = math.sqrt(np.mean((dl - (d0 + slope * t)) ** 2))
    fc = np.mean(freq[used])
    row[col("window_carrier_hz")] = fc
    g = np.diff(t)
    adj = g <= max_gap
    row[col("num_adjacent")] = np.sum(adj)
    rel = fc
    if np.any(adj):
        u = np.exp(1j * ph)
        z = np.sum((u[1:] * np.conj(u[:-1]) * np.exp(-2j * np.pi * fc * g / fs))[adj])
        rel = fc + np.angle(z) * fs / (2 * np.pi * np.mean(g[adj]))
    row[col("rel_carrier_hz")] = rel
    w = np.exp(1j * (ph - 2 * np.pi * rel * t / fs))
    p0 = np.angle(np.sum(w))
    row[col("phase0")] = p0
    row[col("phase_rms")] = math.sqrt(np.mean(np.angle(w * np.exp(-1j * p0)) ** 2))
    row[col("mean_coherence")], row[col("min_coherence_seen")] = np.mean(coh[used]), np.min(coh[used])
    return out


# ---- apply_params_refine --------------------------------------------------------------------------------------------------------
VARIANTS = ("delay_sign", "carrier_sign", "phase_sign", "no_cross")
AP = {k: i for i, k in enumerate(("delay", "slope_ppm", "carrier_hz", "phase", "anchor", "scale", "dc_i", "dc_q", "gain", "sin_phase"))}


def apply_params_refine(coh_row, params_in, variant=None):
    r = [float(v) for v in np.asarray(coh_row, dtype=np.float64).ravel()]
    pin = [float(v) for v in np.asarray(params_in, dtype=np.float64).ravel()]
    assert len(r) == ROW_COLS and len(pin) == 10 and variant in (None,) + VARIANTS
    nan_row = np.full(10, np.nan)
    nan_row[AP["scale"]] = pin[AP["scale"]]
    first = next((j for j in range(MAX_ROW_WINDOWS) if r[col("start") + j] == r[col("start") + j] and r[col("edge") + j] == 0.0
                  and r[col("coherence") + j] >= r[col("min_coherence")]), None)
    fs, delay0, ppm, f, phase0 = r[col("sample_rate")], r[col("delay0")], r[col("rel_sampling_ppm")], r[col("rel_carrier_hz")], r[col("phase0")]
    if (not all(math.isfinite(v) for v in pin) or r[0] != 0.0 or first is None or not all(math.isfinite(v) for v in (delay0, ppm, f, phase0, fs))
            or not fs > 0.0):
        return S_ALIGN_SKIPPED, nan_row
    if variant == "delay_sign":
        delay0 = -delay0
    if variant == "carrier_sign":
        f = -f
    if variant == "phase_sign":
        phase0 = -phase0
    two_pi = 2.0 * math.pi
    d1, s1, f1, phi1, A1 = pin[AP["delay"]], 1e-6 * pin[AP["slope_ppm"]], pin[AP["carrier_hz"]], pin[AP["phase"]], pin[AP["anchor"]]
    s = 1e-6 * ppm
    p0 = r[col("start") + first]
    Ls = float(math.floor(r[col("win_len")] / 4.0))
    n_c = p0 + (4.0 * Ls - 1.0) / 2.0
    Du = delay0 + s * (A1 - p0)
    slope_ppm = 1e6 * (s + s1 + s * s1)
    if not abs(slope_ppm) <= 1000.0:
        return E_ARG, nan_row
    out = np.array(pin)
    out[AP["delay"]] = d1 + Du * (1.0 + s1)
    out[AP["slope_ppm"]] = slope_ppm
    out[AP["anchor"]] = A1
    out[AP["carrier_hz"]] = (f1 + f) * (1.0 + s)
    cross = 0.0 if variant == "no_cross" else (two_pi * f1 / fs) * Du
    out[AP["phase"]] = phi1 + cross + phase0 + (two_pi * f * (1.0 + s) / fs) * (A1 - n_c)
    return 0, out


def refine_cases():
    """(coh_row, params_in) pairs for the bit comparison of the library's helper with the restatement: ordinary rows, the first used
    window not the first one, an anchor that is not 0, a status-16 row, no used window, NaN / Inf in either input, |slope'| > 1000"""
    def coh(delay0=-11.328, ppm=0.61, f=520.2, phase0=0.098, status=0.0, starts=(2000.0, 11000.0, 20000.0), cohs=(0.9, 0.91, 0.89), edges=(0.0, 0.0, 0.0),
            win_len=1184.0, fs=2.048e6, minc=0.5):
        r = np.full(ROW_COLS, np.nan)
        r[:16] = (status, len(starts), len(starts), len(starts), len(starts) - 1, -11.0, delay0, ppm, 0.01, f, f + 3.0, phase0, 0.02, 0.9, 0.89, 16.0)
        r[16:20] = (win_len, fs, minc, 8 * win_len)
        for j, (s, c, e) in enumerate(zip(starts, cohs, edges)):
            r[col("start") + j], r[col("coherence") + j], r[col("edge") + j] = s, c, e
        return r
    par = np.array([0.0, 62.5, -9156.4, 0.0, 0.0, 1.0, 127.4, 127.6, 1.0, 0.0])
    par2 = np.array([-3.25, -30.6, 5380.1, 0.7, 30000.0, 0.37, 127.1, 128.2, 1.07, 0.05])
    cases = [(coh(), par), (coh(), par2), (coh(delay0=0.044, ppm=-0.003, f=-0.42, phase0=-3.1), par2),
             (coh(cohs=(0.3, 0.91, 0.89)), par2), (coh(edges=(1.0, 0.0, 0.0), cohs=(np.nan, 0.91, 0.89)), par),
             (coh(starts=(np.nan, 11000.0, 20000.0)), par), (coh(win_len=19.0, starts=(0.0, 40.0, 90.0)), par2),
             (coh(status=16.0), par), (coh(cohs=(0.1, 0.2, 0.3)), par), (coh(delay0=np.nan), par), (coh(f=np.inf), par),
             (coh(), np.where(np.arange(10) == 2, np.nan, par)), (coh(), np.where(np.arange(10) == 5, np.inf, par)),
             (coh(ppm=990.0), par), (coh(ppm=-1100.0), par2), (coh(ppm=937.4414), par)]
    return cases


# ---- the designed rows: pair_coherence_ref's designed pair for any length ---------------------------------------------------------------
# a: a seeded unit-modulus row whose phase is noise, +-pi/2 per symbol of DESIGN_OV samples, smoothed over two symbols;
# b[n] = a(n - D) exp(j (phi + 2 pi f n / fs)) + noise, the shift a linear phase ramp in the FFT domain (circular over the row).
DESIGN_OV = 4
SIGMA = pcr.SIGMA


def designed_rows(n, D, phi, f, fs, seed):
    """-> a, b (complex, n samples), plant {"delay", "freq", "phi", "psi_step"}"""
    ov = DESIGN_OV
    rng = np.random.Generator(np.random.Philox(key=[int(seed), n]))
    sym = rng.integers(0, 2, n // ov + 2) * 2.0 - 1.0
    step = np.repeat(sym, ov)[:n] * (np.pi / 2) / ov
    h = np.hanning(2 * ov + 1)
    step = np.convolve(step, h / h.sum(), mode="same")
    a = np.exp(1j * np.cumsum(step))
    k = np.fft.fftfreq(n)
    shifted = np.fft.ifft(np.fft.fft(a) * np.exp(-2j * np.pi * k * D))
    b = shifted * np.exp(1j * (phi + 2 * np.pi * f * np.arange(n) / fs))
    b = b + SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / math.sqrt(2)
    return a, b, {"delay": D, "freq": f, "phi": phi, "psi_step": step, "fs": fs}


def designed_phase(plant, starts, win_len):
    """the planted phase of b against a at the centre of the 4 Ls samples of each window, in b's index"""
    L = 4 * (win_len // 4)
    return wrap(plant["phi"] + 2 * np.pi * plant["freq"] * (np.asarray(starts, dtype=np.float64) + plant["delay"] + (L - 1) / 2) / plant["fs"])


def designed_bounds(plant, starts, win_len):
    """pair_coherence_ref.designed_bounds, restated for windows of L = 4 Ls samples at `starts` (each term with its origin there):
      d      the residual misalignment |D - round(D)|: the correlation is taken on the sample grid
      delay  2 x the parabola's bias on a raised-cosine lobe of half-width w = DESIGN_OV at the offset d, plus 1.5 x the coupling
             of the planted frequency into the delay, om sum_k S_k / sum_k V_k over the four segments of Ls samples (S_k = sum
             psi'(n)(n - centre of segment k), V_k = sum (psi' - its segment mean)^2; the largest over the windows) -- S_k grows as
             Ls^1.5 and V_k as Ls, so at Ls = 1024 the term is larger than at 296 and it is computed, not scaled --, plus five
             standard deviations of the noise SIGMA / sqrt(2 L) / beta
      phase  1.5 d x the largest mean phase step over a segment, plus 2 pi f d / fs, plus 5 SIGMA / sqrt(2 L)
      freq   (2 * 1.5 d seg + 5 SIGMA / sqrt(Ls)) fs / (2 pi Ls)
      pair   delay0 as delay; phase0 as phase; rel_carrier_hz: the phases of windows `gap` apart (the smallest distance between
             two starts), each within the phase bound: 2 phase fs / (2 pi gap); rel_sampling_ppm: 1e6 * 2 delay / span of the starts."""
    D, f, fs, step = plant["delay"], plant["freq"], plant["fs"], plant["psi_step"]
    Ls = win_len // 4
    L = 4 * Ls
    starts = [int(s) for s in starts]
    d = abs(D - round(D))
    w = float(DESIGN_OV)
    bias = abs(math.tan(math.pi * d / w) / (2 * math.tan(math.pi / (2 * w))) - d)
    beta = math.sqrt(np.mean(step ** 2))
    segs = [[step[p + k * Ls: p + (k + 1) * Ls] for k in range(K)] for p in starts]
    seg = max(abs(np.mean(s)) for sg in segs for s in sg)
    om, ctr = 2 * np.pi * f / fs, np.arange(Ls) - (Ls - 1) / 2
    coupling = max(abs(om * sum(np.sum(s * ctr) for s in sg) / sum(np.sum((s - s.mean()) ** 2) for s in sg)) for sg in segs)
    delay = 2 * bias + 1.5 * coupling + 5 * SIGMA / math.sqrt(2 * L) / beta
    phase = 1.5 * d * seg + 2 * np.pi * f * d / fs + 5 * SIGMA / math.sqrt(2 * L)
    freq = (2 * 1.5 * d * seg + 5 * SIGMA / math.sqrt(Ls)) * fs / (2 * np.pi * Ls)
    gap, span = min(np.diff(starts)), starts[-1] - starts[0]
    return {"delay": delay, "phase": phase, "freq": freq, "rel_carrier_hz": 2 * phase * fs / (2 * np.pi * gap), "rel_sampling_ppm": 1e6 * 2 * delay / span}


# ---- the wideband closed loop: three retuned dongles on one transmission -------------------------------------------------------------
LOOP_FS, LOOP_TUNED, LOOP_N = 2.048e6, 433.92e6, 60000
# (e ppm, c ppm, start, tuner phase) planted; (e, c) as the calibration table holds them: off by 0.4 .. 0.8 ppm
LOOP_PLANTED = ((63.0, -21.5, 0.0, 0.3), (-30.0, 12.0, 11.37, 2.1), (8.0, 33.0, 5.8, -1.2))
LOOP_ESTIMATE = ((62.5, -21.1), (-30.6, 12.8), (8.45, 32.3))
LOOP_STARTS = tuple(2000 + 9000 * j for j in range(7))
LOOP_WIN, LOOP_M = 1184, 16
LOOP_LAG0 = (0, -11, -6)                                           # round(start_0 - start_b)
LOOP_PAIRS = ((0, 0), (0, 1), (0, 2))
# What the restatement itself leaves between dongle 0 and dongles 1, 2 after ONE refinement on this design (the largest of the two
# pairs; tests/test_row_coherence_cpu.py prints them): the parabola's bias on a lobe that is no parabola, the interpolator's
# pass-band ripple and the byte rounding of the captures.  The bars are twice these (the allowance DESIGN 20 and 23 use).
LOOP_RESIDUAL = {"delay0": 0.01559, "rel_carrier_hz": 0.07097, "phase0": 0.005834, "mean_coherence": 0.999253}
LOOP_BARS = {"delay0": 2 * LOOP_RESIDUAL["delay0"], "rel_carrier_hz": 2 * LOOP_RESIDUAL["rel_carrier_hz"], "phase0": 2 * LOOP_RESIDUAL["phase0"],
             "mean_coherence": 1.0 - 2 * (1.0 - LOOP_RESIDUAL["mean_coherence"])}


def loop_captures(synth):
    """-> raw (3, 2 LOOP_N) uint8, first-pass params (3, 10) from apply_ref.apply_params of the table's estimates"""
    import apply_ref as ar
    raw = np.stack([synth.make_wideband(dongle=i, n=LOOP_N, sample_rate=LOOP_FS, tuned_freq=LOOP_TUNED, e_ppm=e, c_ppm=c, start=st, phase=ph,
                                        tx_key=5)[0] for i, (e, c, st, ph) in enumerate(LOOP_PLANTED)])
    params = np.stack([ar.apply_params(ar.table_row(e, c), LOOP_TUNED) for e, c in LOOP_ESTIMATE])
    params[:, AP["dc_i"]], params[:, AP["dc_q"]] = 127.4, 127.6     # make_wideband's DC, known
    return raw, params


def loop_table(coherence, out, info):
    """the three rows (0, 0), (0, 1), (0, 2) of `coherence` on the rows `out` of an apply pass -> (3, ROW_COLS)"""
    valid = np.asarray(info)[:, 1:3].astype(np.int64)
    return np.stack([coherence(out, a, b, LOOP_LAG0[b], valid) for a, b in LOOP_PAIRS])


def ref_coherence(out, a, b, lag0, valid):
    return row_coherence(out, a, b, lag0, LOOP_STARTS, LOOP_WIN, LOOP_FS, LOOP_M, 0.5, None, valid)["row"]


def ref_apply(raw, params):
    import apply_ref as ar
    res = ar.apply_batch(raw, LOOP_FS, params, LOOP_N)
    return res["out"], res["info"]


def closed_loop(raw, params, apply, coherence, refine, passes=1):
    """apply -> coherence -> refine (`passes` times) -> apply -> coherence.  apply(raw, params) -> out, info (D, 4); coherence as
    ref_coherence; refine(coh_row, params_row) -> (status, row).  Dongle 0 keeps its row.  -> dict: tables (one per apply pass),
    params (likewise), out, info of the last pass, statuses of the refinements"""
    tables, plist, statuses = [], [np.array(params, dtype=np.float64)], []
    out, info = apply(raw, plist[-1])
    tables.append(loop_table(coherence, out, info))
    for _ in range(passes):
        nxt = plist[-1].copy()
        for b in (1, 2):
            st, nxt[b] = refine(tables[-1][b], plist[-1][b])
            statuses.append(st)
        plist.append(nxt)
        out, info = apply(raw, nxt)
        tables.append(loop_table(coherence, out, info))
    return {"tables": tables, "params": plist, "out": out, "info": info, "statuses": statuses}


def loop_figures(table):
    """the largest |delay0|, |rel_carrier_hz|, |phase0| and the smallest mean coherence over the pairs (0, 1), (0, 2); status != 0
    anywhere -> None"""
    t = np.asarray(table)[1:]
    if np.any(t[:, 0] != 0.0):
        return None
    return {"delay0": float(np.max(np.abs(t[:, col("delay0")]))), "rel_carrier_hz": float(np.max(np.abs(t[:, col("rel_carrier_hz")]))),
            "phase0": float(np.max(np.abs(t[:, col("phase0")]))), "mean_coherence": float(np.min(t[:, col("mean_coherence")]))}


def within_bars(fig, factor=1.0):
    """every figure under its bar (x factor): the coherence bar is a floor, 1 - factor (1 - bar)"""
    return (fig is not None and fig["delay0"] <= factor * LOOP_BARS["delay0"] and fig["rel_carrier_hz"] <= factor * LOOP_BARS["rel_carrier_hz"]
            and fig["phase0"] <= factor * LOOP_BARS["phase0"] and fig["mean_coherence"] >= 1.0 - factor * (1.0 - LOOP_BARS["mean_coherence"]))


def misses_some_bar(fig, factor=1.5):
    """a wrong variant: nothing correlates (status 16 somewhere), or some figure beyond factor x its bar"""
    return (fig is None or fig["delay0"] >= factor * LOOP_BARS["delay0"] or fig["rel_carrier_hz"] >= factor * LOOP_BARS["rel_carrier_hz"]
            or fig["phase0"] >= factor * LOOP_BARS["phase0"] or 1.0 - fig["mean_coherence"] >= factor * (1.0 - LOOP_BARS["mean_coherence"]))
