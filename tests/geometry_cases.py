"""Shared inputs of the geometry tests: the per-function API at other decimation ratios, window lengths, oversampling
ratios and front-end shapes than the drivers' (decimation_ratio 8, fft_len 16, oversampling 8 / 4 / 2, decim 64, 47 taps).

Every .m function the library replaces takes its geometry as an argument, and so does the C ABI; through it most values
run code the drivers never reach: the direct-DFT window SNR (any fft_len but 16), the whole-block hop walk on its own
spectra, the any-geometry fine certificate and burst kernels, the 37 x N2 FFT at other N2, the LDS-staged front end at
other alignments.  This module holds the CASES only -- streams, argument grids, and the exits the reference takes on them
as tests/test_geometry_cpu.py proves with both oracles; tests/test_gpu_geometry.py runs the library on them.

NOT compared with the oracle: fft_len = 3.  All three bins of a 3-point spectrum are "signal" bins
(move_fft_snr_runtime_avg.m:23), so noise_power = sum(P) - sum(P(max_set)) is the difference of the SAME three numbers
added in two orders: exactly 0 in the oracle (SNR = +Inf, a hit on window 1), +-1 ulp of the sum in an equally correct
DFT (a huge finite SNR, or a NaN that never hits).  The result is defined by rounding alone; the tests only ask that a
call with fft_len = 3 returns cleanly with hit_idx = -1 or inside [1, nwin].  (fft_len = 2 IS well defined -- the three
"signal" bins count the other bin twice, noise_power < 0, the SNR is NaN and nothing ever hits -- and is compared.)

Plain module: numpy, scipy, synth and the oracle -- nothing here touches the GPU."""
import math

import numpy as np
from scipy.signal import resample_poly

from gsmcal import synth
from oracle import gsmcal_oracle as oracle

FC = 957.4e6
MARGIN_DB = 1e-6          # the certificate margin of k_coarse_scan (kernels_detect.h): decisions nearer than this are replayed
MAX_DROP_FRACTION = 0.1   # of a grid's cases that may be left out because the oracle's own margin is inside MARGIN_DB


def coef47():
    return synth.fir1(46, 200e3 / synth.FS)


def filtered(raw, coef=None):
    """filter(coef,1,raw2iq(raw)) by the oracle: the 8x stream the drivers hand to the chain (gsm_sync_demod.m:107-110)"""
    return oracle.matlab_filter(coef47() if coef is None else coef, oracle.raw2iq(raw.astype(np.float64)))


# ---- coarse stage ---------------------------------------------------------------------------------------------------------
COARSE_DRS = (2, 3, 4, 5, 6, 7, 10, 12, 16, 20, 32, 37, 40, 64, 74)
COARSE_DONGLES = (0, 3)
COARSE_FRAMES = 64
NO_BCCH_DONGLE = 9
HALF_D0_DRS = (8, 40)     # 12500/dr lands on .5
HALF_D1_DRS = (4, 20)     # 13750/dr lands on .5


def coarse_geometry(dr):
    """FCCH_coarse_position.m:15-25,35-36 in integers (no floating point: the .5 cases are decided exactly):
    fft_len = 2^floor(log2(148/dr)), mv_len, n_first = ceil(28750/dr), d0 = round(12500/dr), d1 = round(13750/dr)"""
    fft_len = 0 if dr > 148 else 1 << ((148 // dr).bit_length() - 1)      # 2^k <= 148/dr  <=>  2^k <= floor(148/dr)
    half_up = lambda a: (2 * a + dr) // (2 * dr)                          # round(a/dr), halves away from zero (a > 0)
    return {"fft_len": fft_len, "mv_len": 10 * fft_len, "n_first": -(-28750 // dr), "d0": half_up(12500), "d1": half_up(13750)}


def coarse_captures():
    """name -> 8x filtered stream of a 64-frame capture: the two dongles, and one carrier without a BCCH"""
    out = {f"dongle{d}": filtered(synth.make_stream(dongle=d, num_frames=COARSE_FRAMES)[0]) for d in COARSE_DONGLES}
    out["no_bcch"] = filtered(synth.make_stream(dongle=NO_BCCH_DONGLE, num_frames=COARSE_FRAMES, bcch=False)[0])
    return out


def coarse_cut(r8, dr):
    """the stream FCCH_coarse_position(., dr) expects: one sample per dr symbols"""
    return np.ascontiguousarray(r8[0::8 * dr])


def window_snrs(s, fft_len):
    """the oracle's SNR of every window of s (move_fft_snr_runtime_avg.m:18-27), empty when none fits"""
    nwin = len(s) - (fft_len - 1)
    if nwin < 1:
        return np.zeros(0)
    return oracle._window_snr(oracle._power_spectra(s, 1, nwin, fft_len))


def _margin(snr, avg, th):
    """distance of one decision `snr - avg > th` from its threshold; a NaN SNR is a definite miss in any arithmetic"""
    m = abs((snr - avg) - th)
    return math.inf if math.isnan(m) else m


def move_margin(snr_all, mv_len, th):
    """Replay of move_fft_snr_runtime_avg.m:30-42 on given window SNRs -> (hit window 1-based or -1, avg the hit saw, smallest
    margin over every window the reference evaluates, up to and including the deciding one)"""
    store = [999.0] * mv_len
    sum_snr = 0.0
    for v in store:
        sum_snr += v
    head, worst = 0, math.inf
    for i, snr in enumerate(snr_all):
        snr = float(snr)
        avg = sum_snr / mv_len
        worst = min(worst, _margin(snr, avg, th))
        if snr - avg > th:
            return i + 1, snr - (snr - avg), worst
        sum_snr = sum_snr - store[head]
        sum_snr = sum_snr + snr
        store[head] = snr
        head = (head + 1) % mv_len
    return -1, math.inf, worst


def specific_margin(snr_all, lo, hi, th, avg):
    """smallest margin over the windows specific_fft_snr_fix_avg.m:10-25 evaluates in [lo, hi] (1-based, those that fit)"""
    worst = math.inf
    for i in range(max(lo, 1), min(hi, len(snr_all)) + 1):
        snr = float(snr_all[i - 1])
        worst = min(worst, _margin(snr, avg, th))
        if snr - avg > th:
            break
    return worst


def coarse_margin(s, dr, th=10.0):
    """smallest decision margin of FCCH_coarse_position(s, dr): the moving search and every hop candidate"""
    geo = coarse_geometry(dr)
    fft_len = geo["fft_len"]
    snr_all = window_snrs(s, fft_len)
    hit, avg, worst = move_margin(snr_all[:geo["n_first"] - (fft_len - 1)], geo["mv_len"], th)
    if hit < 0:
        return worst
    limit = (len(s) - (fft_len - 1)) - 5
    cur = hit
    while True:
        found = False
        for d in (geo["d0"], geo["d1"]):
            nxt = cur + d
            if nxt > limit:
                return worst
            worst = min(worst, specific_margin(snr_all, nxt - 5, nxt + 5, th, avg))
            hits = [i for i in range(nxt - 5, nxt + 6) if snr_all[i - 1] - avg > th]
            if hits:
                cur, found = hits[0], True
                break
        if not found:
            return worst


# ---- detector arguments ---------------------------------------------------------------------------------------------------
DET_FFT_LENS = (2, 3, 4, 5, 12, 16, 17, 32, 63, 64)
DET_THS = (3.0, 10.0)
DET_FRAMES = 20
UNCOMPARED_FFT_LENS = (3,)          # see the module docstring


def det_mv_lens(fft_len):
    return (1, 7, 10 * fft_len, 5000)


def det_stream():
    """one short decimated stream: 20 frames of dongle 0, every 64th filtered sample (3 125 samples)"""
    return np.ascontiguousarray(filtered(synth.make_stream(dongle=0, num_frames=DET_FRAMES)[0])[0::64])


def move_cases():
    """(fft_len, mv_len, th, len or None): the grid on the whole stream, then the three shortest streams per fft_len -- with
    th = 10 (nothing hits against the 999 dB seed) and th = -2000 (the first window does, where one fits)"""
    cases = [(f, mv, th, None) for f in DET_FFT_LENS for mv in det_mv_lens(f) for th in DET_THS]
    cases += [(f, 10 * f, th, n) for f in DET_FFT_LENS for n in (f - 1, f, f + 1) for th in (10.0, -2000.0)]
    return cases


def specific_cases(snr_all, fft_len, th=10.0):
    """Target sets for specific_fft_snr_fix_avg on a stream with window SNRs snr_all (the oracle's), 11 windows each like the
    hop walk's: name -> (target_set, th, avg_snr).  avg_snr is placed half-way between the SNRs it has to separate, so the
    margins are as wide as the stream allows.  Where every SNR is NaN (fft_len = 2) or undefined (3) avg_snr is 0."""
    nwin = len(snr_all)
    fin = np.where(np.isfinite(snr_all), snr_all, -np.inf)
    cases = {}
    if np.all(np.isinf(fin)) or fft_len in UNCOMPARED_FFT_LENS:
        lo = nwin // 2
        cases["miss"] = ((lo, lo + 10), th, 0.0)
        cases["ends_on_last_window"] = ((nwin - 10, nwin), th, 0.0)
        cases["one_past_the_last_window"] = ((nwin - 9, nwin + 1), th, 0.0)
        return cases
    lo = 100
    seg = fin[lo - 1:lo + 10]
    cases["first_window"] = ((lo, lo + 10), th, float(seg[0]) - th - 1.0)
    cases["miss"] = ((lo, lo + 10), th, float(np.max(seg)) - th + 1.0)
    # last window of the set: the set ends on the largest SNR of a stretch, everything before it in the set is smaller
    for hi in range(nwin // 2, nwin - 20):
        seg = fin[hi - 11:hi]
        if seg[-1] > np.max(seg[:-1]) + 0.1:
            cases["last_window"] = ((hi - 10, hi), th, float(0.5 * (seg[-1] + np.max(seg[:-1]))) - th)
            break
    tail = fin[nwin - 11:nwin]
    cases["ends_on_last_window_miss"] = ((nwin - 10, nwin), th, float(np.max(tail)) - th + 1.0)
    cases["ends_on_last_window_hit"] = ((nwin - 10, nwin), th, float(np.min(tail)) - th - 1.0)
    tail = fin[nwin - 10:nwin]
    cases["one_past_the_last_window_miss"] = ((nwin - 9, nwin + 1), th, float(np.max(tail)) - th + 1.0)     # MATLAB: index error
    cases["one_past_the_last_window_hit"] = ((nwin - 9, nwin + 1), th, float(np.min(tail)) - th - 1.0)     # returns before it
    return cases


# ---- oversampled streams --------------------------------------------------------------------------------------------------
OVS = (1, 3, 5, 6, 12, 16)
OV_FRAMES = 61
OV_DONGLE = 3
# a sampling error the fine AND the SCH stage have to resample for: the SCH stage's estimate is quantised (one sample over the
# span of the hits), and at 233 ppm the fine stage leaves a rest of at least one quantum at every ov below (at 300 ppm it
# leaves none at four of the five)
PPM_CAPTURE = {"dongle": 3, "sampling_ppm": 233.0}
# the exit the reference takes along the chain, per capture and ov (include/gsmcal.h GSMCAL_S_*, 0: all three stages complete);
# tests/test_geometry_cpu.py holds both oracles to this table
CHAIN_EXIT = {"plain": {1: oracle.S_SCH_EDGE, 3: 0, 5: 0, 6: 0, 12: 0, 16: 0, 30: 0},
              "ppm": {1: oracle.S_SCH_EDGE, 3: 0, 5: 0, 6: 0, 12: 0, 16: 0}}
DEMOD_OVS = (1, 2, 3, 16)
CHAIN_MAX_OV = 30         # the largest ratio the chain's kernels hold in LDS (tests/test_gpu_geometry.py computes it): plain capture only


def ov_base_streams():
    """name -> 8x filtered stream of the two 61-frame captures"""
    return {"plain": filtered(synth.make_stream(dongle=OV_DONGLE, num_frames=OV_FRAMES)[0]),
            "ppm": filtered(synth.make_stream(num_frames=OV_FRAMES, **PPM_CAPTURE)[0])}


def resample(r8, ov):
    """the 8x stream at ov samples per symbol (polyphase resampling; what the signal means physically does not matter here,
    which exits the reference takes on it does)"""
    return np.ascontiguousarray(resample_poly(r8, ov, 8))


def training_sequence(ov):
    return synth.sch_training_sequence(ov)


def oracle_chain(o, r, ov, ts):
    """gsm_sync_demod.m:117-120 function by function with oracle module `o` -> dict of every output and the exit taken"""
    res = {}
    info = [{}, {}, {}, {}]
    res["coarse_pos"], res["coarse_snr"] = o.FCCH_coarse_position(r[0::8 * ov], 8, info=info[0])
    res["fcch_pos"], res["r1"], res["sp1"], res["cp1"] = o.FCCH_fine_correction(r, res["coarse_pos"], ov, FC, info=info[1])[:4]
    res["pos_info"], res["r2"], res["sp2"] = o.SCH_corr_rate_correction(res["r1"], res["fcch_pos"], ts, ov, info=info[2])
    res["r3"], res["cp2"] = o.carrier_correct_post_SCH(res["r2"], res["pos_info"], ov, FC, info=info[3])
    res["exit"] = next((i["exit"] for i in info if i.get("exit")), 0)
    res["info"] = info
    return res


# ---- front end --------------------------------------------------------------------------------------------------------------
FE_STREAMS = 3
FE_NS = (1, 7, 46, 47, 255, 256, 257, 4099, 65536 + 5)
FE_DECIMS = (1, 2, 3, 7, 63, 64, 65, 100, 255)


def fe_filters():
    """name -> taps: 1, 2, 47 (the drivers'), 48 and 300 taps, the last two NOT mirror-symmetric (general_taps.ramp's recipe:
    a low-pass times a rising exponential, unit DC gain), so a reversed tap order cannot pass"""
    wn = 200e3 / synth.FS

    def ramp(n):
        h = synth.fir1(n - 1, wn) * np.exp(np.linspace(0.0, math.log(4.0), n))
        return h / np.sum(h)
    return {"one": np.array([1.0]), "two": np.array([0.75, 0.25]), "fir47": synth.fir1(46, wn), "ramp48": ramp(48), "ramp300": ramp(300)}


# (n, decim, filter): the cross product thinned by hand.  Every n, every decim and every filter occurs; n < ntaps (1, 7, 46
# against 47 / 48 / 300 taps; 255, 256, 257 against 300), n < decim, nd = ceil(n/decim) in {1, 256, 257}, more than one
# block of 256 outputs (65 541 / 256: 257 of them), ntaps > 256, and 2n % 16 != 0 for every n but 256 (each of the three streams then starts at another
# offset from a 16-byte boundary).
FE_TRIPLES = (
    (1, 1, "one"), (1, 64, "fir47"), (1, 255, "ramp300"),
    (7, 1, "two"), (7, 2, "ramp48"), (7, 3, "fir47"), (7, 63, "ramp300"), (7, 7, "one"),
    (46, 1, "fir47"), (46, 2, "ramp300"), (46, 7, "ramp48"), (46, 65, "two"),
    (47, 1, "ramp48"), (47, 3, "fir47"), (47, 64, "one"), (47, 100, "ramp300"),
    (255, 1, "ramp300"), (255, 2, "one"), (255, 63, "fir47"), (255, 255, "ramp48"),
    (256, 1, "fir47"), (256, 1, "ramp300"), (256, 64, "ramp48"), (256, 255, "two"),
    (257, 1, "ramp48"), (257, 1, "ramp300"), (257, 2, "fir47"), (257, 65, "one"), (257, 100, "two"),
    (4099, 1, "two"), (4099, 3, "ramp300"), (4099, 7, "fir47"), (4099, 2, "ramp48"), (4099, 64, "fir47"), (4099, 100, "one"),
    (65541, 1, "fir47"), (65541, 2, "ramp48"), (65541, 63, "ramp300"), (65541, 64, "fir47"), (65541, 65, "two"),
    (65541, 255, "ramp48"), (65541, 256, "one"), (65541, 255, "ramp300"),
)


def fe_raw(n):
    """(3, 2n) seeded bytes with a DC offset that differs between I and Q and between the streams"""
    rng = np.random.default_rng(7000 + n)
    raw = rng.integers(0, 200, size=(FE_STREAMS, 2 * n)) + np.array([[0, 40] * n, [30, 5] * n, [55, 55] * n])
    return raw.astype(np.uint8)


def fe_bound(coef, x):
    """2 ntaps 2^-53 sum|coef| max|x|: the fp64 dot-product bound (each of ntaps products and sums rounds once, relative
    2^-53, of magnitude <= sum|coef| max|x|), doubled because the oracle's own lfilter carries the same error"""
    return 2.0 * len(coef) * 2.0 ** -53 * float(np.sum(np.abs(coef))) * float(np.max(np.abs(x)))
