"""fp64 restatement of FCCH_demod.m:5-66, written line by line from the .m file, for the FCCH_demod tests.

Two forms: `fcch_demod` (vectorised over the bursts, the tone estimate through the oracle's _fcch_tone_estimate, which is the
same block of FCCH_fine_correction.m:148-155) and `fcch_demod_loop` (one burst at a time, everything spelled out).  Both
return a dict
    freq, snr, max_idx (the offset max_idx - (fft_len/2+1) the reference prints, :66), mean_freq, carrier_ppm,
    noise_ratio (noise_power / sum(band) per burst: how much of the band sum is left after the signal sum is taken off --
                 the condition of the SNR's subtraction)
or None at the :8 exit.  snr is NaN where noise_power < 0 (MATLAB's log10 of a negative number is complex) and +Inf where it
is 0.  Also here: the designed-spectrum and tone inputs the CPU and the GPU tests share."""
import math

import numpy as np

from oracle import gsmcal_oracle as o

SYMBOL_RATE = (1625.0 / 6.0) * 1e3                                   # :30


def _snr(signal_power, noise_power):
    if noise_power < 0:
        return math.nan                                              # :62 would be complex
    if noise_power == 0:
        return math.inf
    return 10.0 * math.log10(signal_power / noise_power)


def _mean(freq):
    return o._seq_mean(freq) if len(freq) else math.nan              # :44 mean([]) = NaN


def fcch_demod(s, pos_info, oversampling_ratio, carrier_freq):
    pos_info = np.atleast_2d(np.asarray(pos_info, dtype=np.float64))
    if np.all(pos_info == -1):                                       # :8
        return None
    s = np.asarray(s, dtype=np.complex128).ravel()
    fft_len = (2 * 3 + 142) * oversampling_ratio                     # :13-16
    fcch_pos = pos_info[pos_info[:, 1] == 0, 0]                      # :18-19
    num_fcch = len(fcch_pos)                                         # :20
    sampling_rate = SYMBOL_RATE * oversampling_ratio                 # :31
    half = fft_len // 2
    if num_fcch:
        _, ipr, _, freq = o._fcch_tone_estimate(s, fcch_pos, fft_len, sampling_rate)      # :22-42
        max_idx = np.rint(ipr * fft_len / (2.0 * np.pi)).astype(np.int64) + half + 1      # 1-based, as :34 returns it
        mat = np.stack([s[int(p) - 1:int(p) - 1 + fft_len] for p in fcch_pos], axis=1)
        fd = np.abs(np.fft.fft(mat, axis=0)) ** 2                    # :28
        fd = np.concatenate([fd[half:, :], fd[:half, :]], axis=0)   # :33
        assert np.array_equal(np.argmax(fd, axis=0) + 1, max_idx)
    else:
        freq, max_idx, fd = np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros((fft_len, 0))
    mean_freq = _mean(freq)                                          # :44
    carrier_ppm = 1e6 * (mean_freq - SYMBOL_RATE / 4) / carrier_freq  # :47-48
    half_noise_len = int(math.ceil((fft_len * 200e3 / sampling_rate) / 2))       # :53
    sp = (half + 1) - half_noise_len                                 # :55
    ep = (half + 1) + half_noise_len - 1                             # :56
    offs = np.arange(-2, 3)[:, None]
    sig_set = np.mod(max_idx[None, :] + offs - 1, fft_len) + 1       # :58-59
    signal_power = np.array([np.sum(fd[sig_set[:, i] - 1, i]) for i in range(num_fcch)])      # :60
    band_power = np.array([np.sum(fd[sp - 1:ep, i]) for i in range(num_fcch)])
    noise_power = band_power - signal_power                          # :61
    snr = np.array([_snr(a, b) for a, b in zip(signal_power, noise_power)])      # :62
    return {"freq": np.asarray(freq, dtype=np.float64), "snr": snr, "max_idx": max_idx - (half + 1), "mean_freq": mean_freq,
            "carrier_ppm": carrier_ppm, "noise_ratio": noise_power / band_power if num_fcch else np.zeros(0)}


def fcch_demod_loop(s, pos_info, oversampling_ratio, carrier_freq):
    pos_info = np.atleast_2d(np.asarray(pos_info, dtype=np.float64))
    if np.all(pos_info == -1):                                       # :8
        return None
    s = np.asarray(s, dtype=np.complex128).ravel()
    fft_len = 148 * oversampling_ratio
    sampling_rate = SYMBOL_RATE * oversampling_ratio
    half = fft_len // 2
    half_noise_len = int(math.ceil((fft_len * 200e3 / sampling_rate) / 2))
    freq, snr, idx, ratio = [], [], [], []
    for row in pos_info:
        if row[1] != 0:
            continue
        sp = int(row[0])
        ep = sp + fft_len - 1
        if sp < 1 or ep > len(s):
            raise o.MatlabIndexError("FCCH burst window outside the signal")
        x = s[sp - 1:ep]                                             # :26
        fd = np.abs(np.fft.fft(x)) ** 2                              # :28
        fd = np.concatenate([fd[half:], fd[:half]])                 # :33
        max_idx = int(np.argmax(fd)) + 1                             # :34
        ipr = 2.0 * np.pi * (max_idx - (half + 1)) / fft_len         # :36
        y = x * np.exp(-1j * (np.arange(fft_len, dtype=np.float64) * ipr))       # :37
        ang = np.angle(y)
        pr = np.exp(1j * ang[1:]) / np.exp(1j * ang[:-1])            # :39
        tot = np.sum(pr)
        phase = math.atan2(tot.imag / len(pr), tot.real / len(pr))   # :40
        freq.append(sampling_rate * (ipr + phase) / (2.0 * np.pi))   # :42
        lo = (half + 1) - half_noise_len                             # :55
        hi = (half + 1) + half_noise_len - 1                         # :56
        sig = 0.0
        for k in range(max_idx - 2, max_idx + 3):                    # :58
            sig += fd[(k - 1) % fft_len]                             # :59-60
        band = float(np.sum(fd[lo - 1:hi]))
        noise = band - sig                                           # :61
        snr.append(_snr(sig, noise))                                 # :62
        idx.append(max_idx - (half + 1))                             # :66
        ratio.append(noise / band)
    mean_freq = _mean(freq)
    return {"freq": np.array(freq), "snr": np.array(snr), "max_idx": np.array(idx, dtype=np.int64), "mean_freq": mean_freq,
            "carrier_ppm": 1e6 * (mean_freq - SYMBOL_RATE / 4) / carrier_freq, "noise_ratio": np.array(ratio)}


# ---- inputs shared by the CPU and the GPU tests ------------------------------------------------------------------------------
DESIGNED_SNR_DB = 10.0 * math.log10(3.51 / 106.49)                   # five peak bins 0.25+0.49+2.25+0.36+0.16 against 110 - 3.51


def designed_spectrum(ov, p, seed=0):
    """A burst whose spectrum is designed: 110 unit-amplitude band bins with seeded phases, amplitudes 0.5, 0.7, 1.5, 0.6, 0.4
    at the peak index p (0-based, fftshift order) and its wrapped neighbours.  Returns (s, pos_info): the burst between five
    zeros on either side, at position 6.  Expected: max_idx offset p - fft_len/2, snr DESIGNED_SNR_DB for the four wrap
    positions p in {0, 1, fft_len-2, fft_len-1} (their five bins lie outside the band)."""
    fft_len = 148 * ov
    half = fft_len // 2
    rng = np.random.default_rng(1000 * ov + seed)
    sh = np.zeros(fft_len, dtype=np.complex128)                      # fftshift order
    sh[half - 55:half + 55] = np.exp(2j * np.pi * rng.random(110))
    for d, a in zip(range(-2, 3), (0.5, 0.7, 1.5, 0.6, 0.4)):
        sh[(p + d) % fft_len] = a * np.exp(2j * np.pi * rng.random())
    spec = np.concatenate([sh[half:], sh[:half]])                   # back from fftshift order
    x = np.fft.ifft(spec)
    s = np.concatenate([np.zeros(5), x, np.zeros(5)])
    return s, np.array([[6.0, 0.0]])


def tone_windows(ov, k, seed=0):
    """exp(2 pi i (k+0.3) n / fft_len) plus seeded noise of sigma 0.1 over 3*fft_len samples; three windows: the first, one at
    fft_len/2+7 and the last possible one."""
    fft_len = 148 * ov
    rng = np.random.default_rng(seed + 7919 * (k % 1009) + ov)
    n = np.arange(3 * fft_len)
    s = np.exp(2j * np.pi * (k + 0.3) * n / fft_len) + 0.1 * (rng.standard_normal(len(n)) + 1j * rng.standard_normal(len(n)))
    pos = np.array([[1.0, 0.0], [fft_len // 2 + 7.0, 0.0], [2.0 * fft_len + 1.0, 0.0]])
    return s, pos
