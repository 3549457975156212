"""fp64 restatement of pair_coherence (include/gsmcal.h) in numpy, written from the definition, not from the
kernels: delay, phase, frequency and coherence of stream b against stream a on the SCH and BCCH bursts of a's table, and the
per-pair summaries.  Also the designed pair and the calibrated triple the CPU and GPU tests share.

pair_coherence(r, r_len, pos_info, ov, a, b, lag0, max_lag, min_coherence) -> dict
    row        (PAIR_COLS,) the table row (api.PAIR_FIELDS, then pos | delay | phase | freq | coherence | edge)
    corr       (MAX_PAIR_BURSTS, 2M+1, 4) complex, NaN where no burst was evaluated
    ea, eb     (MAX_PAIR_BURSTS, 4), (MAX_PAIR_BURSTS, 2M+1, 4): the energies under the same sums
    evaluated, edge, used   (MAX_PAIR_BURSTS,) bool;  mstar (MAX_PAIR_BURSTS,) int (0 where not evaluated)
  and, per evaluated burst, how far it is from a decision that a value differing in its last bits could take the other way:
    gap        (y_max - y_second) / y_max, the relative gap between the two largest y[m]
    curvature  |y[m*-1] - 2 y[m*] + y[m*+1]| / y[m*] (NaN at an edge)
    coh_margin |coherence - min_coherence| (NaN at an edge)
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MAX_HITS = 24
MAX_POS_ROWS = 6 * MAX_HITS
MAX_PAIR_BURSTS = MAX_HITS + 4 * MAX_HITS
PAIR_COLS = 16 + 6 * MAX_PAIR_BURSTS
K = 4
S_POST_NO_POS, S_PAIR_FEW, E_CAPACITY = 10, 16, -4
HEAD = ("status", "num_bursts", "num_eval", "num_used", "num_adjacent", "lag0", "delay0", "rel_sampling_ppm", "delay_rms",
        "rel_carrier_hz", "burst_carrier_hz", "phase0", "phase_rms", "mean_coherence", "min_coherence_seen", "max_lag")
BURST = ("pos", "delay", "phase", "freq", "coherence", "edge")
FC = 957.4e6


def fs_of(ov):
    return (1625e3 / 6) * ov


def matlab_round(x):
    return math.copysign(math.floor(abs(x) + 0.5), x)


def col(name):
    """first column of a per-burst field, or the column of a head field"""
    return HEAD.index(name) if name in HEAD else 16 + BURST.index(name) * MAX_PAIR_BURSTS


def wrap(x):
    return (np.asarray(x) + np.pi) % (2 * np.pi) - np.pi


def pair_coherence(r, r_len, pos_info, ov, a, b, lag0, max_lag=None, min_coherence=0.5):
    r = np.atleast_2d(np.asarray(r, dtype=np.complex128))
    d, stride = r.shape
    pos_info = np.asarray(pos_info, dtype=np.float64).reshape(d, 2, MAX_POS_ROWS)
    M = 2 * ov if max_lag is None else int(max_lag)
    assert ov in (2, 4, 8) and 1 <= M <= 4 * ov and 0 <= a < d and 0 <= b < d
    L, Ls, NL, fs = 148 * ov, 37 * ov, 2 * M + 1, fs_of(ov)
    nbmax = MAX_PAIR_BURSTS
    row = np.full(PAIR_COLS, np.nan)
    out = {"row": row, "corr": np.full((nbmax, NL, K), np.nan + 1j * np.nan), "ea": np.full((nbmax, K), np.nan),
           "eb": np.full((nbmax, NL, K), np.nan), "evaluated": np.zeros(nbmax, bool), "edge": np.zeros(nbmax, bool),
           "used": np.zeros(nbmax, bool), "mstar": np.zeros(nbmax, int), "gap": np.full(nbmax, np.nan),
           "curvature": np.full(nbmax, np.nan), "coh_margin": np.full(nbmax, np.nan), "M": M}
    row[col("lag0")], row[col("max_lag")] = lag0, M
    row[1:5] = 0.0
    len_a, len_b = min(int(r_len[a]), stride), min(int(r_len[b]), stride)
    pi = pos_info[a]
    if len_a < 1 or len_b < 1 or np.all(pi == -1.0):
        row[0] = S_POST_NO_POS
        return out
    rows = [i for i in range(MAX_POS_ROWS) if pi[1, i] in (1.0, 2.0)]
    row[col("num_bursts")] = len(rows)
    if len(rows) > nbmax:
        row[0] = E_CAPACITY
        return out
    xa, xb = r[a], r[b]
    p_all = np.zeros(nbmax)
    delay, phase, freq, coh = (np.full(nbmax, np.nan) for _ in range(4))
    seg = np.arange(Ls)
    for j, i in enumerate(rows):
        pos = pi[0, i]
        if not (pos == pos) or abs(pos) > 2.0 ** 52:
            continue
        p = int(matlab_round(pos)) - 1
        if not (0 <= p and p + L <= len_a and 0 <= p + lag0 - M and p + lag0 + M + L <= len_b):
            continue
        out["evaluated"][j] = True
        p_all[j] = p
        row[col("pos") + j] = pos
        c = np.empty((NL, K), dtype=np.complex128)
        eb = np.empty((NL, K))
        for k in range(K):
            av = xa[p + k * Ls + seg]
            out["ea"][j, k] = np.sum(np.abs(av) ** 2)
            for mi in range(NL):
                bv = xb[p + lag0 + (mi - M) + k * Ls + seg]
                c[mi, k] = np.sum(bv * np.conj(av))
                eb[mi, k] = np.sum(np.abs(bv) ** 2)
        out["corr"][j], out["eb"][j] = c, eb
        y = np.sum(np.abs(c) ** 2, axis=1)
        ms = int(np.argmax(y))                                    # the first maximum
        out["mstar"][j] = ms - M
        ys = np.sort(y)
        out["gap"][j] = (ys[-1] - ys[-2]) / ys[-1] if ys[-1] > 0 else 0.0
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
        out["coh_margin"][j] = abs(coh[j] - min_coherence)
        out["used"][j] = bool(coh[j] >= min_coherence)
    nb = len(rows)
    for name, v in (("delay", delay), ("phase", phase), ("freq", freq), ("coherence", coh)):
        row[col(name): col(name) + nbmax] = v
    used = np.nonzero(out["used"])[0]
    row[col("num_eval")], row[col("num_used")] = np.sum(out["evaluated"][:nb]), len(used)
    if len(used) < 2:
        row[0] = S_PAIR_FEW
        return out
    row[0] = 0.0
    t = p_all[used] - p_all[used[0]]
    dl, ph = delay[used], phase[used]
    tb, db = np.mean(t), np.mean(dl)
    slope = np.sum((t - tb) * (dl - db)) / np.sum((t - tb) ** 2)
    d0 = db - slope * tb
    row[col("delay0")], row[col("rel_sampling_ppm")] = d0, 1e6 * slope
    row[col("delay_rms")] = math.sqrt(np.mean((dl - (d0 + slope * t)) ** 2))
    fc = np.mean(freq[used])
    row[col("burst_carrier_hz")] = fc
    g = np.diff(t)
    adj = g <= 1875 * ov
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


def ties_ok(want, gap=1e-6, curvature=1e-4, coh=1e-6):
    """the three conditions under which a value that differs in its last bits cannot change a decision"""
    ev = want["evaluated"]
    inner = ev & ~want["edge"]
    return bool(np.all(want["gap"][ev] >= gap) and np.all(want["curvature"][inner] >= curvature) and np.all(want["coh_margin"][inner] >= coh))


def raw_table(pos):
    """[(pos, type), ...] -> the (2, MAX_POS_ROWS) table with -1 padding"""
    t = -np.ones((2, MAX_POS_ROWS))
    if len(pos):
        t[:, :len(pos)] = np.asarray(pos, dtype=np.float64).T
    return t


# ---- the designed pair ---------------------------------------------------------------------------------------------------
# a: three frames of a seeded unit-modulus stream whose phase is noise: +-pi/2 per symbol, one symbol = ov samples, smoothed over two
# symbols (what a GMSK burst looks like to a correlator; |a| = 1 keeps the phase of a segment's correlation at the segment's
# centre).  b[n] = a(n - D) exp(j (phi + 2 pi f n / fs)) + noise: the shift by D = 11.25 samples is a linear phase ramp in the FFT
# domain (circular over the three frames), the noise complex Gaussian with E|w|^2 = SIGMA^2.
DESIGN_D, DESIGN_PHI, DESIGN_F, SIGMA = 11.25, 0.7, 300.0, 0.01
DESIGN_SEED = 20261020


def designed_pair(ov, noise=True):
    """-> a, b (complex, 3 frames), the table [(pos, type)] with an FCCH row and three type-1/2 rows, the planted values"""
    rng = np.random.Generator(np.random.Philox(key=[DESIGN_SEED, ov]))
    n = 3 * 1250 * ov
    sym = rng.integers(0, 2, n // ov + 2) * 2.0 - 1.0
    step = np.repeat(sym, ov)[:n] * (np.pi / 2) / ov
    h = np.hanning(2 * ov + 1)
    step = np.convolve(step, h / h.sum(), mode="same")
    psi = np.cumsum(step)
    a = np.exp(1j * psi)
    k = np.fft.fftfreq(n)
    shifted = np.fft.ifft(np.fft.fft(a) * np.exp(-2j * np.pi * k * DESIGN_D))
    b = shifted * np.exp(1j * (DESIGN_PHI + 2 * np.pi * DESIGN_F * np.arange(n) / fs_of(ov)))
    if noise:
        b = b + SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / math.sqrt(2)
    frame = 1250 * ov
    pos = [(101.0, 0.0), (201.0, 1.0), (201.0 + frame, 2.0), (201.0 + 2 * frame, 2.0)]
    L = 148 * ov
    burst_p = np.array([200.0, 200.0 + frame, 200.0 + 2 * frame])
    plant = {"delay": DESIGN_D, "freq": DESIGN_F, "psi_step": step, "burst_p": burst_p,
             "phase": wrap(DESIGN_PHI + 2 * np.pi * DESIGN_F * (burst_p + DESIGN_D + (L - 1) / 2) / fs_of(ov))}
    return a, b, pos, plant


def designed_bounds(ov, plant):
    """What the planted values come back within, from the design and the noise level (first order, each term with its origin):
      d      the residual misalignment |D - round(D)| = 0.25 sample: the correlation is taken on the sample grid
      delay  the parabola through three samples of a lobe is exact for a parabola only.  For a raised-cosine lobe of half-width w
             it returns tan(pi d / w) / (2 tan(pi / (2 w))) for an offset d; the correlation lobe of a stream with one symbol per
             ov samples is at least w = ov wide on either side, so |bias| <= that expression's distance from d at w = ov; twice
             that is allowed (the lobe is no exact raised cosine); plus the coupling of the planted frequency into the delay:
             with w = 2 pi f / fs, d/dtau of sum_k |c_k|^2 at the true delay is 2 Ls w sum_k S_k, S_k = sum_n psi'(n) (n - centre
             of segment k) -- a stream that happens to run faster late in a segment looks delayed under a positive offset -- and
             the second derivative -2 Ls sum_k V_k, V_k = sum_n (psi'(n) - its segment mean)^2, so the maximum moves by
             w sum S_k / sum V_k, computed here from the design (the largest over the three bursts, times 1.5 for the second
             order); plus five standard deviations of the noise term SIGMA / sqrt(2 L) / beta, beta = the rms phase step of a
             (rad/sample)
      phase  at a misalignment d the product a(n + d) conj(a(n)) has the phase d psi'(n): a segment's correlation turns by d times
             the mean phase step over the segment (computed here from the design, the largest over the twelve segments), the burst's by
             at most as much; 1.5 times that for the second order, plus 2 pi f d / fs (the centre moves with the lag), plus five
             standard deviations of the noise SIGMA / sqrt(2 L)
      freq   theta is a mean of three segment-to-segment steps, each off by at most twice the segment term:
             (2 * 1.5 * seg + 5 SIGMA / sqrt(Ls)) fs / (2 pi Ls)
      pair   delay0 as delay; phase0 as phase; rel_carrier_hz: the phases of bursts a frame apart, each within the phase bound,
             2 * phase / (2 pi frame / fs); rel_sampling_ppm: 1e6 * 2 * delay / (2 frames)."""
    L, Ls, fs, frame = 148 * ov, 37 * ov, fs_of(ov), 1250 * ov
    d = abs(DESIGN_D - round(DESIGN_D))
    w = float(ov)
    bias = abs(math.tan(math.pi * d / w) / (2 * math.tan(math.pi / (2 * w))) - d)
    step = plant["psi_step"]
    beta = math.sqrt(np.mean(step ** 2))
    seg = max(abs(np.mean(step[int(p) + k * Ls: int(p) + (k + 1) * Ls])) for p in plant["burst_p"] for k in range(K))
    om, ctr = 2 * np.pi * DESIGN_F / fs, np.arange(Ls) - (Ls - 1) / 2
    segs = [[step[int(p) + k * Ls: int(p) + (k + 1) * Ls] for k in range(K)] for p in plant["burst_p"]]
    coupling = max(abs(om * sum(np.sum(s * ctr) for s in sg) / sum(np.sum((s - s.mean()) ** 2) for s in sg)) for sg in segs)
    delay = 2 * bias + 1.5 * coupling + 5 * SIGMA / math.sqrt(2 * L) / beta
    phase = 1.5 * d * seg + 2 * np.pi * DESIGN_F * d / fs + 5 * SIGMA / math.sqrt(2 * L)
    freq = (2 * 1.5 * d * seg + 5 * SIGMA / math.sqrt(Ls)) * fs / (2 * np.pi * Ls)
    return {"delay": delay, "phase": phase, "freq": freq, "rel_carrier_hz": 2 * phase * fs / (2 * np.pi * frame),
            "rel_sampling_ppm": 1e6 * 2 * delay / (2 * frame)}


def designed_streams(ov, noise=True):
    """the designed pair as (r, r_len, pos_info) of two streams: a is stream 0 (with the table), b stream 1 (an all -1 table)"""
    a, b, pos, plant = designed_pair(ov, noise)
    r = np.stack([a, b])
    pi = np.stack([raw_table(pos), raw_table([])])
    return r, np.array([len(a), len(b)], dtype=np.int64), pi, plant


def periodic_self_stream(ov):
    """A stream to correlate with itself: one segment of Ls unit-modulus samples repeated, bursts at multiples of Ls.  For a general
    stream the sums at the lags -m and +m cover different samples, and the delay of a stream against itself is zero only to about
    1e-3 sample.  Over a whole period the sum at -m is the conjugate of the sum at +m, so y is even in the lag, the parabola's
    offset is zero up to rounding, and every c[0][k] is real.  -> r (1, n), r_len, pos_info (1, 2, MAX_POS_ROWS)"""
    Ls = 37 * ov
    rng = np.random.Generator(np.random.Philox(key=[DESIGN_SEED, 100 + ov]))
    v = np.exp(1j * np.cumsum(rng.uniform(-0.6, 0.6, Ls)))
    r = np.tile(v, 100)[None, :]
    pos = [(float(q * Ls + 1), t) for q, t in ((2, 1.0), (40, 2.0), (80, 2.0))]
    return r, np.array([r.shape[1]], dtype=np.int64), raw_table(pos)[None]


# ---- the calibrated triple: three dongles on one transmission -----------------------------------------------------------------
TRIPLE = ((0, 7000.0), (5, 7003.5), (4, 897.78))              # (dongle, frac_start)
TRIPLE_PAIRS = ((0, 1), (0, 2), (1, 2))


def triple_stream_args(i):
    dongle, frac = TRIPLE[i]
    return dict(dongle=dongle, tx_key=7, start_frame=4, bsic=52, fn0=51 * 300 + 4, frac_start=frac)


def triple_planted_delay(a, b):
    """content that starts frac_start samples into the transmission sits that much EARLIER in the capture"""
    return TRIPLE[a][1] - TRIPLE[b][1]


def triple_left_by_the_chain(truth, total_sampling_ppm, total_carrier_ppm, a, b):
    """(carrier Hz, sampling ppm) the chain leaves between b and a: (truth - estimate) of b minus that of a"""
    ls = [truth[i]["sampling_ppm"] - total_sampling_ppm[i] for i in range(len(truth))]
    lc = [truth[i]["carrier_ppm"] - total_carrier_ppm[i] for i in range(len(truth))]
    return (lc[b] - lc[a]) * FC * 1e-6, ls[b] - ls[a]
