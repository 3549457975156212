"""CPU tests of the band power-spectrum scanners (multi_rtl_sdr_split_scanner.m, multi_rtl_sdr_diversity_scanner.m):
filter design, frequency plans, records, the fp64 restatement the GPU tests compare against, and the C ABI / MEX surface
of gsmcal_band_power_batch.  No GPU needed."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import gsmcal_oracle as o

import gsmcal.dist  # noqa: F401  (gsmcal does not import its multi-GPU layer by itself)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gsmcal_band_power_batch", "gsmcal_band_power_batch_dev")


def restate(a, coef, decim):
    """mean(abs(filter(coef,1,raw2iq(a))(1:decim:end)).^2) in fp64 (split_scanner.m:154-156), a: 2N bytes."""
    y = o.matlab_filter(np.asarray(coef, dtype=np.float64), o.raw2iq(np.asarray(a, dtype=np.float64)))
    return float(np.mean(np.abs(y[::decim]) ** 2))


def loop_restate(a, coef, decim):
    """The same, one sample at a time: DC of raw2iq.m:8, causal FIR with zero initial state, rows 1:decim:end."""
    a = [float(v) for v in a]
    n = len(a) // 2
    mi = sum(a[0::2]) / n
    mq = sum(a[1::2]) / n
    x = [complex(a[2 * i] - mi, a[2 * i + 1] - mq) for i in range(n)]
    acc, cnt = 0.0, 0
    for j in range(0, n, decim):
        y = 0j
        for k in range(len(coef)):
            if j - k >= 0:
                y += coef[k] * x[j - k]
        acc += abs(y) ** 2
        cnt += 1
    return acc / cnt


@pytest.mark.parametrize("rbw, order, decim", [(1e3, 127, 1024), (5e3, 127, 204), (10e3, 127, 102), (25e3, 127, 40),
                                               (50e3, 63, 20), (100e3, 31, 10), (200e3, 31, 5), (500e3, 31, 2),
                                               (1e6, 31, 1)])
def test_spectrum_filter_design(gsmcal_mod, rbw, order, decim):
    """split_scanner.m:51-54,57,71: 2^ceil(log2(fs/RBW))-1 clamped to 31..127, fir1 at RBW/fs, floor(fs/(2 RBW))."""
    co, coef, dr, ns = gsmcal_mod.dist.spectrum_filter(2.048e6, rbw, 0.1)
    assert (co, dr, ns) == (order, decim, 204800)
    assert len(coef) == order + 1 and len(coef) in (32, 64, 128)
    assert np.array_equal(coef, coef[::-1])                       # symmetric to the last bit
    assert np.array_equal(coef, gsmcal_mod.synth.fir1(order, rbw / 2.048e6))
    assert abs(np.sum(coef) - 1.0) < 1e-12


def test_spectrum_filter_rejects_fractional_sample_counts(gsmcal_mod):
    with pytest.raises(ValueError):
        gsmcal_mod.dist.spectrum_filter(2.048e6, 50e3, 0.1000001)
    with pytest.raises(ValueError):
        gsmcal_mod.dist.spectrum_filter(2.048e6, 5e6, 0.1)         # decimate_ratio 0
    assert gsmcal_mod.dist.spectrum_filter(1e6, 50e3, 0.5)[3] == 500000


def _vec2mat_literal(start, stop, step, nd):
    """split_scanner.m:62-67 statement by statement."""
    freq_orig = []
    k = 0
    while start + k * step <= stop + 1e-6:
        freq_orig.append(start + k * step)
        k += 1
    per = int(math.ceil(len(freq_orig) / nd))
    num_pad = per * nd - len(freq_orig)
    freq = freq_orig + [freq_orig[-1] + (i + 1) * step for i in range(num_pad)]
    return [[freq[i * per + j] for j in range(per)] for i in range(nd)], num_pad


@pytest.mark.parametrize("nd", [1, 2, 3, 4, 7])
def test_split_plan_matches_literal_vec2mat(gsmcal_mod, nd):
    freq, pad = gsmcal_mod.dist.scan_frequency_plan(935e6, 960e6, 50e3, nd)
    lit, lpad = _vec2mat_literal(935e6, 960e6, 50e3, nd)
    assert pad == lpad and freq.shape == (nd, len(lit[0]))
    assert np.allclose(freq, np.array(lit), rtol=0, atol=1e-3)
    power = np.arange(freq.size, dtype=np.float64) + 1.0
    rec = gsmcal_mod.dist.split_spectrum_record(power, 935e6, 960e6, 50e3, nd, 0, 0.1, 2.048e6)
    assert rec["power_spectrum"].shape == (freq.size,) and np.array_equal(rec["freq"], freq)
    # unit (dongle i, point j) is power_spectrum((i-1)*num_freq_per_sub_band + j) (split_scanner.m:163)
    per = freq.shape[1]
    for i in range(nd):
        assert np.array_equal(rec["power_spectrum"][i * per:(i + 1) * per], power[i * per:(i + 1) * per])


def test_split_record_fields_and_name(gsmcal_mod):
    freq, _ = gsmcal_mod.dist.scan_frequency_plan(935e6, 960e6, 50e3, 4)
    rec = gsmcal_mod.dist.split_spectrum_record(np.ones(freq.size), 935e6, 960e6, 50e3, 4, 0, 0.1, 2.048e6)
    # save(filename, 'power_spectrum', 'start_freq', 'end_freq', 'freq_step', 'observe_time', 'RBW', 'gain', 'sample_rate',
    #      'coef', 'freq')   split_scanner.m:176-177
    assert set(rec) == {"power_spectrum", "start_freq", "end_freq", "freq_step", "observe_time", "RBW", "gain", "sample_rate",
                        "coef", "freq", "filename"}
    assert rec["filename"] == "split_scan_935000000_960000000_gain0_4dongles.mat"
    assert rec["RBW"] == 50e3 and len(rec["coef"]) == 64 and freq.size == 504
    with pytest.raises(ValueError):
        gsmcal_mod.dist.split_spectrum_record(np.ones(501), 935e6, 960e6, 50e3, 4, 0, 0.1, 2.048e6)


def test_diversity_record_combine_fields_and_name(gsmcal_mod):
    rng = np.random.default_rng(3)
    ps = rng.random((3, 501))
    rec = gsmcal_mod.dist.diversity_spectrum_record(ps, 935e6, 960e6, 50e3, 3, 12.5, 0.1, 2.048e6)
    # power_spectrum_combine = mean(power_spectrum, 1)   diversity_scanner.m:176 (linear)
    assert np.array_equal(rec["power_spectrum_combine"], np.mean(ps, axis=0))
    assert rec["power_spectrum"].shape == (3, 501)
    # save(filename, 'power_spectrum', 'power_spectrum_combine', 'start_freq', 'end_freq', 'freq_step', 'observe_time',
    #      'RBW', 'gain', 'sample_rate', 'coef')   diversity_scanner.m:180
    assert set(rec) == {"power_spectrum", "power_spectrum_combine", "start_freq", "end_freq", "freq_step", "observe_time",
                        "RBW", "gain", "sample_rate", "coef", "filename"}
    assert rec["filename"] == "scan_935000000_960000000_gain12.5_3dongles.mat"
    with pytest.raises(ValueError):
        gsmcal_mod.dist.diversity_spectrum_record(rng.random((3, 500)), 935e6, 960e6, 50e3, 3, 0, 0.1, 2.048e6)


@pytest.mark.parametrize("ntaps, decim, n", [(32, 5, 97), (64, 20, 200), (7, 3, 40), (1, 1, 33), (12, 50, 9)])
def test_restatement_matches_per_sample_loop(ntaps, decim, n):
    rng = np.random.default_rng(ntaps * 1000 + n)
    a = rng.integers(0, 256, 2 * n).astype(np.uint8)
    coef = rng.standard_normal(ntaps)
    ref = loop_restate(a, list(coef), decim)
    assert abs(restate(a, coef, decim) - ref) <= 1e-12 * ref
    c = np.full(2 * n, 77, dtype=np.uint8)
    assert restate(c, coef, decim) == 0.0 and loop_restate(c, list(coef), decim) == 0.0


def test_header_exports_and_prototypes(gsmcal_mod):
    txt = open(os.path.join(ROOT, "include", "gsmcal.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in gsmcal_mod.SIGNATURES
        assert hasattr(gsmcal_mod.load(), name)
    src = open(os.path.join(ROOT, "multi-rtl-sdr-calibration_amd", "csrc", "abi_calls.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name


def test_null_context_and_bad_arguments_are_refused(gsmcal_mod):
    """GSMCAL_E_ARG before anything touches a device: a NULL context (any arguments) -- no GPU needed."""
    lib = gsmcal_mod.load()
    raw = np.zeros((2, 64), dtype=np.uint8)
    coef = np.ones(4)
    rp = raw.ctypes.data_as(C.POINTER(C.c_uint8))
    cp = coef.ctypes.data_as(C.POINTER(C.c_double))
    out = np.zeros(2)
    op = out.ctypes.data_as(C.POINTER(C.c_double))
    E_ARG = -1
    assert lib.gsmcal_band_power_batch(None, rp, 2, 32, cp, 4, 2, op) == E_ARG
    assert lib.gsmcal_band_power_batch_dev(None, C.c_void_p(raw.ctypes.data), 2, 32, cp, 4, 2, C.c_void_p(out.ctypes.data)) == E_ARG
    for d, n, nt, dec in ((0, 32, 4, 2), (2, 0, 4, 2), (2, 32, 0, 2), (2, 32, 1025, 2), (2, 32, 4, 0), (-1, 32, 4, 1)):
        assert lib.gsmcal_band_power_batch(None, rp, d, n, cp, nt, dec, op) == E_ARG
        assert lib.gsmcal_band_power_batch_dev(None, C.c_void_p(raw.ctypes.data), d, n, cp, nt, dec,
                                               C.c_void_p(out.ctypes.data)) == E_ARG


@pytest.mark.parametrize("api", ["interleaved", "split"])
def test_mex_band_power_target_compiles_against_the_abi(api):
    """The gsmcal_band_power MEX target through the same gcc -fsyntax-only check as the other targets (test_abi_cpu.py)."""
    r = subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-std=c99", "-DGSMCAL_FN_gsmcal_band_power"] +
                       (["-DGSMCAL_STUB_SPLIT"] if api == "split" else []) +
                       ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mex_stub"),
                        os.path.join(ROOT, "mex", "gsmcal_mex.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "gsmcal_band_power" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
