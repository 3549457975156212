"""fp64 restatement of BCCH_demod.m, written line by line from the .m file, for the BCCH_demod tests.

The function as the project states it:
    [normal_training_sequence_idx, r, carrier_ppm] = BCCH_demod(s, pos_info, normal_training_sequence, ov, carrier_freq)
`carrier_freq` is the name :71 uses without defining it (every sibling takes it as an argument), `normal_training_sequence`
the name :97 uses for the third parameter.  The FCCH block (:49-68) goes through the oracle's _fcch_tone_estimate: it is the
block of carrier_correct_post_SCH.m:58-72.

`bcch_demod` returns None at the :9 exit, otherwise a dict
    status        0, 11 (:14, fewer than 4 type-2 rows) or 13 (:103, the first four bursts disagree)
    idx, r, carrier_ppm      the three outputs (-1 where the .m file leaves them at their initial value)
    fo, mean_fo              :68 per burst and :70
    num_bcch                 type-2 rows
    corr_val                 (8, num_bcch): :97 for EVERY type-2 row, as the batch form reports it (the .m file: the first four
                             columns); NaN columns where a row beyond the fourth has its window outside the stream
    max_idx, peak, runner_up, phase, ratio      per column: the 1-based first maximum of |corr_val| (:99), its value, the
                             second largest, the angle of the winner, peak / runner_up
    num_agree                columns whose max_idx equals the first column's
    lines                    what :15 / :69 / :72 / :101 / :104 print, as (text, numbers) pairs: `report` formats them
One of the first four windows outside the stream raises the oracle's MatlabIndexError (:95).
Without a type-0 row mean([]) is NaN (:70) and r, corr_val and carrier_ppm are NaN.  MATLAB's max over an all-NaN column answers
index 1, a number without a meaning; here no winner is reported: max_idx NaN, idx -1, status 13.

Also here: the designed streams the CPU and the GPU tests share."""
import math

import numpy as np

from oracle import gsmcal_oracle as o

SYMBOL_RATE = (1625.0 / 6.0) * 1e3                                   # :19
S_POST_FEW_BCCH, S_BCCH_TSC_MIXED = 11, 13
MIN_RATIO = 1.05                                                     # every compared burst: winner / runner-up in the restatement


def bcch_demod(s, pos_info, normal_training_sequence, oversampling_ratio, carrier_freq):
    pos_info = np.atleast_2d(np.asarray(pos_info, dtype=np.float64))
    if np.all(pos_info == -1):                                       # :9
        return None
    out = {"status": 0, "idx": -1, "r": -1.0, "carrier_ppm": -1.0, "lines": []}      # :6-8
    bcch_idx = pos_info[:, 1] == 2                                   # :13
    out["num_bcch"] = int(np.sum(bcch_idx))
    if np.sum(bcch_idx) < 4:                                         # :14
        out["lines"].append(("The number of BCCH bursts is less than 4!", None))     # :15
        out["status"] = S_POST_FEW_BCCH
        return out
    s = np.asarray(s, dtype=np.complex128).ravel()
    nts = np.asarray(normal_training_sequence, dtype=np.complex128)
    sampling_rate = SYMBOL_RATE * oversampling_ratio                 # :20
    target_freq = SYMBOL_RATE / 4                                    # :21
    len_ts_ov = 26 * oversampling_ratio                              # :34-35
    len_pre_ov = 61 * oversampling_ratio                             # :36-37
    assert nts.shape == (len_ts_ov, 8)
    fcch_pos = pos_info[pos_info[:, 1] == 0, 0]                      # :49-50
    fft_len = 148 * oversampling_ratio                               # :53-54
    if len(fcch_pos):
        _, _, _, fo = o._fcch_tone_estimate(s, fcch_pos, fft_len, sampling_rate)     # :56-68
        mean_fo = o._seq_mean(fo)                                    # :70
    else:
        fo, mean_fo = np.zeros(0), math.nan                          # mean([]) = NaN
    out["fo"], out["mean_fo"] = np.asarray(fo, dtype=np.float64), mean_fo
    out["lines"].append(("post SCH freq ", out["fo"]))               # :69
    carrier_ppm = 1e6 * (mean_fo - target_freq) / carrier_freq       # :71
    out["carrier_ppm"] = carrier_ppm
    out["lines"].append(("carrier ppm and mean fo ", np.array([carrier_ppm, mean_fo])))      # :72
    comp_freq = target_freq - mean_fo                                # :74
    comp_phase_rotate = comp_freq * 2 * np.pi / sampling_rate        # :75
    with np.errstate(invalid="ignore"):
        r = s * np.exp(1j * (np.arange(len(s), dtype=np.float64) * comp_phase_rotate))       # :76
    out["r"] = r
    bcch_pos = pos_info[bcch_idx, 0]                                 # :84
    nb = len(bcch_pos)
    corr_mat = np.full((len_ts_ov, nb), np.nan + 0j)
    win_max = np.full(nb, np.nan)
    for i in range(nb):                                              # :92 runs to num_bcch_used = 4; the batch form goes on
        sp = int(bcch_pos[i]) + len_pre_ov                           # :93
        ep = sp + len_ts_ov - 1                                      # :94
        if sp < 1 or ep > len(s):
            if i < 4:
                raise o.MatlabIndexError("BCCH training-sequence window outside the signal")
            continue
        corr_mat[:, i] = r[sp - 1:ep]                                # :95
        win_max[i] = np.max(np.abs(s[sp - 1:ep]))
    with np.errstate(invalid="ignore"):
        corr_val = nts.conj().T @ corr_mat                           # :97
    mag = np.abs(corr_val)
    max_idx, peak, runner, phase = (np.full(nb, np.nan) for _ in range(4))
    for i in range(nb):                                              # :99
        if np.all(np.isnan(mag[:, i])):
            continue
        k = int(np.argmax(mag[:, i]))                                # the first maximum
        max_idx[i], peak[i] = k + 1, mag[k, i]
        runner[i] = np.max(np.delete(mag[:, i], k))
        phase[i] = np.angle(corr_val[k, i])
    out.update(corr_val=corr_val, max_idx=max_idx, peak=peak, runner_up=runner, phase=phase, win_max=win_max)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["ratio"] = peak / runner
    out["num_agree"] = int(np.sum(max_idx == max_idx[0]))
    first = max_idx[:4]
    if not np.any(np.isnan(first)) and np.sum(np.abs(first - np.mean(first))) == 0:  # :100
        out["lines"].append(("Normal training sequence idx (BCCH) ", np.array([first[0]])))  # :101
        out["idx"] = int(first[0])                                   # :102
    else:
        out["lines"].append(("Fail to identity normal training sequence idx (BCCH).", None))  # :104
        out["status"] = S_BCCH_TSC_MIXED
    return out


def report(res, num2str):
    """the console text of one call: the restatement's lines with their numbers through `num2str`"""
    if res is None:
        return ""
    return "".join(t + (num2str(v) if v is not None else "") + "\n" for t, v in res["lines"])


# ---- inputs shared by the CPU and the GPU tests ------------------------------------------------------------------------------
def gap(ov):
    return 8 * ov + ov // 4 if ov >= 4 else 9 * ov


def designed_stream(synth, ov, codes, nf=1, f=137.5, seed=0):
    """nf FCCH bursts (148 zero bits), then one normal burst per entry of `codes` carrying TSC[code] between seeded data bits;
    each burst modulated between 4 guard bits, the bursts gap(ov) zeros apart, the whole mixed with exp(2 pi i f n / fs).
    Returns (s, pos_info): the FCCH rows (type 0) and the normal bursts as BCCH rows (type 2), 1-based starts."""
    rng = np.random.default_rng(100 * ov + seed)
    g = synth.gmsk_frequency_pulse(sps=ov)
    blen, step = 148 * ov, 148 * ov + gap(ov)
    nbur = nf + len(codes)
    s = np.zeros(nbur * step - gap(ov), dtype=np.complex128)
    pos = np.zeros((nbur, 2))
    for i in range(nbur):
        if i < nf:
            bits = np.zeros(148, dtype=np.int8)
        else:
            bits = np.concatenate([np.zeros(3, np.int8), rng.integers(0, 2, 58, dtype=np.int8), synth.TSC[codes[i - nf]],
                                   rng.integers(0, 2, 58, dtype=np.int8), np.zeros(3, np.int8)])
        padded = np.concatenate([np.zeros(4, np.int8), bits, np.zeros(4, np.int8)])
        s[i * step:i * step + blen] = synth.gmsk_modulate(synth.diff_precode(padded), ov, g)[4 * ov:4 * ov + blen]
        pos[i] = i * step + 1, (0 if i < nf else 2)
    fs = SYMBOL_RATE * ov
    return s * np.exp(2j * np.pi * f * np.arange(len(s)) / fs), pos


def decimate_by_2(r, pos_info):
    """the 8x stream and its table at 4x (what test_gpu_fcch_demod.py does)"""
    pi4 = np.array(pos_info, dtype=np.float64)
    pi4[:, 0] = np.floor((pi4[:, 0] - 1) / 2) + 1
    return np.ascontiguousarray(np.asarray(r)[::2]), pi4
