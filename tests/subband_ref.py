"""Restatements of the multi-channel diversity scanner's per-capture loop (multi_rtl_sdr_diversity_scanner_another_bak.m:191-203)
and the inputs the sub-band tests share (tests/test_subband_cpu.py, tests/test_gpu_subband.py).

literal   :191-203 line by line in fp64: raw2iq, the mixer exp(1i*(1:N)*w), filter, mean(abs(.)^2)     -- the reference
loop      the same, one sample at a time
exact     the modulated-tap form in longdouble: |sum_k (c_k e^{-jwk}) X[n-k]|^2 with X = N*c - S exact integers.  It
          forms no n*w product, so it is free of the rounding of n*w that `literal` (and MATLAB) carry."""
import numpy as np

from oracle import gsmcal_oracle as o

FS = 2.048e6


def literal(a, coef, w, decim=1):
    """a: 2N bytes of one capture, w: phase_rotate (radians per sample).  :191-203, rows 1:decim:end."""
    r = o.raw2iq(np.asarray(a, dtype=np.float64))                               # :175
    n = len(r)
    tmp = r * np.exp(1j * np.arange(1, n + 1) * w)                              # :196
    r_flt = o.matlab_filter(np.asarray(coef, dtype=np.float64), tmp)            # :199
    return float(np.mean(np.abs(r_flt[::decim]) ** 2))                          # :203


def loop(a, coef, w, decim=1):
    """`literal` one sample at a time: DC of raw2iq.m:8, the mixer at sample index 1..N, causal FIR with zero initial state."""
    import cmath
    a = [float(v) for v in a]
    n = len(a) // 2
    mi = sum(a[0::2]) / n
    mq = sum(a[1::2]) / n
    x = [complex(a[2 * i] - mi, a[2 * i + 1] - mq) * cmath.exp(1j * ((i + 1) * w)) for i in range(n)]
    acc, cnt = 0.0, 0
    for j in range(0, n, decim):
        y = 0j
        for k in range(len(coef)):
            if j - k >= 0:
                y += coef[k] * x[j - k]
        acc += abs(y) ** 2
        cnt += 1
    return acc / cnt


def exact(a, coef, w, decim=1):
    """The modulated-tap form in longdouble (80-bit on x86): no mixer, exact integer DC removal."""
    L = np.longdouble
    a = np.asarray(a).astype(np.int64)
    n = len(a) // 2
    xr = (n * a[0::2] - int(a[0::2].sum())).astype(L)
    xi = (n * a[1::2] - int(a[1::2].sum())).astype(L)
    nd = -(-n // decim)
    yr = np.zeros(nd, dtype=L)
    yi = np.zeros(nd, dtype=L)
    for k, c in enumerate(np.asarray(coef, dtype=np.float64)):
        ph = L(k) * L(w)
        hr, hi = L(c) * np.cos(ph), -L(c) * np.sin(ph)
        j0 = -(-k // decim)                                                     # first kept row with a sample under tap k
        if j0 >= nd:
            break
        ar, ai = xr[j0 * decim - k::decim][:nd - j0], xi[j0 * decim - k::decim][:nd - j0]      # X[j*decim - k], j = j0 .. nd-1
        yr[j0:] += hr * ar - hi * ai
        yi[j0:] += hr * ai + hi * ar
    return float(np.sum(yr * yr + yi * yi) / L(nd) / (L(n) * L(n)))


def table(fn, raw, coef, w, decim, rows=None):
    """fn (literal / exact) over a batch: raw (D, 2N), w (D, J) with NaN slots -> (D, J), NaN where w is NaN or the row is not
    in `rows`."""
    w = np.atleast_2d(np.asarray(w, dtype=np.float64))
    out = np.full(w.shape, np.nan)
    for c in (range(w.shape[0]) if rows is None else rows):
        for j in range(w.shape[1]):
            if not np.isnan(w[c, j]):
                out[c, j] = fn(raw[c], coef, w[c, j], decim)
    return out


def tone_captures(d, n, seed, dc=(127.5, 127.5), amp=40.0, noise=3.0):
    """d captures of n samples: a tone at a random offset plus Gaussian noise around `dc`, rounded and clipped to bytes
    (the generator of tests/test_gpu_spectrum.py)."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    out = np.empty((d, 2 * n), dtype=np.uint8)
    for i in range(d):
        f = rng.uniform(-0.5, 0.5)
        ph = 2 * np.pi * f * k + rng.uniform(0, 2 * np.pi)
        out[i, 0::2] = np.clip(np.rint(dc[0] + amp * np.cos(ph) + noise * rng.standard_normal(n)), 0, 255)
        out[i, 1::2] = np.clip(np.rint(dc[1] + amp * np.sin(ph) + noise * rng.standard_normal(n)), 0, 255)
    return out


def phase(rel_hz):
    """phase_rotate of :195 for a relative frequency, with the sign that moves it to 0 Hz (shift_sign = -1)."""
    return -np.asarray(rel_hz, dtype=np.float64) * 2 * np.pi / FS


# ---- the cases of tests/test_gpu_subband.py::test_cases: name -> (raw (D, 2N), coef, w (D, J), decim, rows to check) -----------
CASES = ("64taps/11", "128taps/16", "nsub1", "asym33", "coef=[1]", "n_lt_ntaps", "odd_n", "n4097", "n8191", "n1", "decim10",
         "decim7", "decim_gt_n", "phases", "ragged")
W7 = phase([-200e3, -100e3, 0, 100e3, 200e3, np.nan, np.nan])                    # the defaults' slots (:71: 7 at 100 kHz)
NAN = np.nan


def case(name, spectrum_filter, fir1=None):
    """spectrum_filter: gsmcal.dist.spectrum_filter (the design of :51-54)."""
    d, n, decim = 4, 30001, 1
    c32 = spectrum_filter(FS, 100e3, 0.2)[1]
    coef, w = c32, np.tile(phase([-200e3, -100e3, 0, 100e3, 200e3]), (d, 1))
    if name == "64taps/11":
        coef = spectrum_filter(FS, 50e3, 0.2)[1]
        w = np.tile(phase(-250e3 + 50e3 * np.arange(11)), (d, 1))
    elif name == "128taps/16":
        coef = spectrum_filter(FS, 10e3, 0.2)[1]
        w = np.tile(phase(np.linspace(-250e3, 250e3, 16)), (d, 1))
    elif name == "nsub1":
        w = np.tile(phase([-100e3]), (d, 1))
    elif name == "asym33":
        coef = np.random.default_rng(33).standard_normal(33)
    elif name == "coef=[1]":
        coef = np.array([1.0])
        w = np.tile(phase([-200e3, 0, 56e3]), (d, 1))
    elif name == "n_lt_ntaps":
        coef, n = spectrum_filter(FS, 10e3, 0.2)[1], 77
    elif name == "odd_n":
        n = 20481
    elif name in ("n4097", "n8191", "n1"):
        n = int(name[1:])
    elif name.startswith("decim"):
        decim = {"decim10": 10, "decim7": 7, "decim_gt_n": 40000}[name]
    elif name == "phases":
        w = np.tile(np.array([0.0, np.pi, -3.0, 40.0]), (d, 1))
    elif name == "ragged":
        v = phase([-244e3, -144e3, -44e3, 56e3, 156e3, 256e3, 6e3])
        w = np.array([v,
                      [NAN, v[1], NAN, v[3], NAN, NAN, NAN],
                      [v[2], NAN, NAN, NAN, NAN, NAN, v[5]],
                      [NAN] * 7])
    assert len(coef) == {"64taps/11": 64, "128taps/16": 128, "asym33": 33, "coef=[1]": 1, "n_lt_ntaps": 128}.get(name, 32)
    return tone_captures(d, n, 7), np.asarray(coef, dtype=np.float64), w, decim


def defaults(spectrum_filter):
    """:40-57 as shipped: 100 kHz, 0.2 s -> 32 taps, 409 600 samples; 3 captures, 5 points and 2 unused slots each."""
    _, coef, _, n = spectrum_filter(FS, 100e3, 0.2)
    return tone_captures(3, n, 7), coef, np.tile(W7, (3, 1)), 1


def large_dc(spectrum_filter):
    """DC at the rails, a tone of a byte or two (tests/test_gpu_spectrum.py::test_large_dc_with_weak_tone)."""
    _, coef, _, _ = spectrum_filter(FS, 100e3, 0.2)
    n = 30001
    raws = [tone_captures(2, n, 5, dc=dc, amp=1.5, noise=0.4) for dc in ((252.0, 3.0), (3.0, 251.0), (250.0, 250.0))]
    return np.concatenate(raws), coef, np.tile(phase([-200e3, 0, 100e3]), (6, 1)), 1


MANY_ROWS = (0, 1, 500, 1001, 1500, 2002, 2003)


def many(spectrum_filter):
    """D = 2004 (four dongles x 501 captures) of 4000 samples, 5 points each; MANY_ROWS are compared."""
    _, coef, _, _ = spectrum_filter(FS, 100e3, 0.2)
    return tone_captures(2004, 4000, 11), coef, np.tile(phase([-200e3, -100e3, 0, 100e3, 200e3]), (2004, 1)), 1


def planted_sweep(plan, num_samples, num_dongle=2, emitters=(935.3e6 + 1e3, 936.4e6 + 1e3, 937.2e6 + 1e3), seed=21):
    """A synthetic multi-channel sweep: r_all_raw (2*num_samples, num_dongle, length(real_freq)) with carriers at `emitters`
    (1 kHz off grid points: a carrier exactly on a tuned frequency is DC, which raw2iq removes) and a little noise.  With
    c = I + jQ a carrier at RF centre + f sits at +f."""
    rng = np.random.default_rng(seed)
    k = np.arange(num_samples)
    ncap = len(plan["real_freq"])
    out = np.empty((2 * num_samples, num_dongle, ncap), dtype=np.uint8)
    for dg in range(num_dongle):
        for c, centre in enumerate(plan["real_freq"]):
            i = np.full(num_samples, 127.5) + 0.3 * rng.standard_normal(num_samples)
            q = np.full(num_samples, 127.5) + 0.3 * rng.standard_normal(num_samples)
            for e in emitters:
                if abs(e - centre) < FS / 2:                                     # inside this capture's Nyquist band
                    ph = 2 * np.pi * (e - centre) / FS * k + rng.uniform(0, 2 * np.pi)
                    i += (30 + 5 * dg) * np.cos(ph)
                    q += (30 + 5 * dg) * np.sin(ph)
            out[0::2, dg, c] = np.clip(np.rint(i), 0, 255)
            out[1::2, dg, c] = np.clip(np.rint(q), 0, 255)
    return out
