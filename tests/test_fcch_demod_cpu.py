"""CPU tests of FCCH_demod (FCCH_demod.m:5-66): the restatement the GPU tests compare against (tests/fcch_demod_ref.py) is
checked against itself (two forms) and against spectra designed to have a known answer; the boundary (header, exports, ctypes
prototypes, Python names, MEX target) is checked as tests/test_abi_cpu.py checks the rest."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import fcch_demod_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FC = 957.4e6


def _agree(a, b, tol=1e-12):
    assert np.array_equal(a["max_idx"], b["max_idx"])
    for k in ("freq", "snr", "noise_ratio"):
        assert a[k].shape == b[k].shape
        nan = np.isnan(a[k])
        assert np.array_equal(nan, np.isnan(b[k])), k
        assert np.all(np.abs(a[k][~nan] - b[k][~nan]) <= tol * np.abs(b[k][~nan])), (k, a[k], b[k])
    for k in ("mean_freq", "carrier_ppm"):
        assert (math.isnan(a[k]) and math.isnan(b[k])) or abs(a[k] - b[k]) <= tol * max(abs(b[k]), 1e-300), k


@pytest.mark.parametrize("ov", [8, 4])
def test_loop_and_vectorised_restatement_agree(ov):
    rng = np.random.default_rng(5 + ov)
    fft_len = 148 * ov
    n = np.arange(6 * fft_len)
    s = np.exp(2j * np.pi * 37.2 * n / fft_len) + 0.2 * (rng.standard_normal(len(n)) + 1j * rng.standard_normal(len(n)))
    pos = np.array([[3.0, 0.0], [40.0, 1.0], [fft_len + 11.0, 0.0], [900.0, 2.0], [5.0 * fft_len + 1, 0.0]])
    a, b = ref.fcch_demod(s, pos, ov, FC), ref.fcch_demod_loop(s, pos, ov, FC)
    assert len(a["freq"]) == 3 and np.all(a["max_idx"] == 37) and np.all(np.isfinite(a["snr"]))
    _agree(a, b)
    for k in (-30, 100, -fft_len // 2):                        # a peak off centre, one outside the band, the wrap
        s, pos = ref.tone_windows(ov, k)
        _agree(ref.fcch_demod(s, pos, ov, FC), ref.fcch_demod_loop(s, pos, ov, FC))


def test_restatement_exits():
    assert ref.fcch_demod(-1.0, np.array([[-1.0, -1.0]]), 8, FC) is None
    assert ref.fcch_demod_loop(-1.0, -np.ones((72, 2)), 8, FC) is None
    for f in (ref.fcch_demod, ref.fcch_demod_loop):
        r = f(np.ones(5000, dtype=complex), np.array([[10.0, 1.0], [200.0, 2.0]]), 8, FC)
        assert len(r["freq"]) == len(r["snr"]) == len(r["max_idx"]) == 0
        assert math.isnan(r["mean_freq"]) and math.isnan(r["carrier_ppm"])


@pytest.mark.parametrize("ov", [8, 4])
@pytest.mark.parametrize("wrap", [0, 1, -2, -1])
def test_designed_spectrum_gives_the_designed_answer(ov, wrap):
    """110 unit band bins, five peak bins 0.5/0.7/1.5/0.6/0.4 at the ends of the fftshift-ed spectrum (their wrapped
    neighbours lie at the other end): max_idx = p - fft_len/2 and snr = 10 log10(3.51/106.49) = -14.8200171... dB -- the
    whole signal sum is taken off the band sum although none of its bins lies in the band (:61)."""
    fft_len = 148 * ov
    p = wrap % fft_len
    s, pos = ref.designed_spectrum(ov, p)
    assert abs(ref.DESIGNED_SNR_DB - (-14.8200171)) < 1e-6
    for f in (ref.fcch_demod, ref.fcch_demod_loop):
        r = f(s, pos, ov, FC)
        assert r["max_idx"].tolist() == [p - fft_len // 2]
        assert abs(r["snr"][0] - ref.DESIGNED_SNR_DB) <= 1e-12, r["snr"][0] - ref.DESIGNED_SNR_DB
        assert abs(r["noise_ratio"][0] - 106.49 / 110.0) <= 1e-12


def test_tones_outside_the_band_give_nan():
    for k in (37, 20, -30, 50):
        r = ref.fcch_demod(*ref.tone_windows(8, k), 8, FC)
        assert np.all(np.isfinite(r["snr"])) and np.all(r["max_idx"] == k) and np.all(np.abs(r["noise_ratio"]) >= 1e-3)
    for k in (100, -592, 591):
        r = ref.fcch_demod(*ref.tone_windows(8, k), 8, FC)
        assert np.all(np.isnan(r["snr"])) and np.all(np.abs(r["noise_ratio"]) >= 1e-3)


# ---- the boundary --------------------------------------------------------------------------------------------------------------
NEW = ("gsmcal_FCCH_demod", "gsmcal_fcch_demod_batch", "gsmcal_fcch_demod_batch_dev")


def test_new_symbols_are_declared_exported_and_bound(gsmcal_mod):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsmcal.h")).read(), flags=re.S)
    lib = gsmcal_mod.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared in include/gsmcal.h"
        assert hasattr(lib, name), f"{name} is not exported by libgsmcal.so"
        assert name in gsmcal_mod.SIGNATURES
    assert len(gsmcal_mod.SIGNATURES["gsmcal_FCCH_demod"][1]) == 15
    assert len(gsmcal_mod.SIGNATURES["gsmcal_fcch_demod_batch"][1]) == 9
    assert len(gsmcal_mod.SIGNATURES["gsmcal_fcch_demod_batch_dev"][1]) == 9
    for name in ("FCCH_demod", "fcch_demod_batch", "fcch_demod_batch_dev", "demod_rows"):
        assert callable(getattr(gsmcal_mod, name))


def test_demod_table_constants_match_python(gsmcal_mod):
    txt = open(os.path.join(ROOT, "include", "gsmcal.h")).read()
    m = re.search(r"#define GSMCAL_DEMOD_COLS \(4 \+ 3 \* GSMCAL_MAX_HITS\)", txt)
    assert m and gsmcal_mod.DEMOD_COLS == 4 + 3 * gsmcal_mod.MAX_HITS == 76
    cols = {k: v for k, v in re.findall(r"GSMCAL_D_([A-Z_]+) = ([^,/\n]+)", txt)}
    val = {k: eval(v.replace("GSMCAL_MAX_HITS", str(gsmcal_mod.MAX_HITS))) for k, v in cols.items()}  # noqa: S307 - the header's own integers
    assert val == {"NUM_FCCH": 0, "MEAN_FREQ": 1, "CARRIER_PPM": 2, "STATUS": 3, "FREQ": 4, "SNR": 28, "MAX_IDX": 52}
    assert gsmcal_mod.DEMOD_FIELDS == ("num_fcch", "mean_freq", "carrier_ppm", "status")
    t = np.arange(2 * 76, dtype=np.float64).reshape(2, 76)
    rows = gsmcal_mod.demod_rows(t)
    assert rows["status"].tolist() == [3.0, 79.0] and rows["freq"][1, 0] == 80.0 and rows["snr"][0, 0] == 28.0 and rows["max_idx"][0, 23] == 75.0


@pytest.mark.parametrize("api", ["interleaved", "split"])
def test_mex_target_compiles_against_the_abi(api):
    """the exact compiler line of test_abi_cpu.py::test_mex_gateway_compiles_against_the_abi, for the new target"""
    r = subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-std=c99", "-DGSMCAL_FN_FCCH_demod"] +
                       (["-DGSMCAL_STUB_SPLIT"] if api == "split" else []) +
                       ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mex_stub"),
                        os.path.join(ROOT, "mex", "gsmcal_mex.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "defined(GSMCAL_FN_FCCH_demod)" in open(os.path.join(ROOT, "mex", "gsmcal_mex.c")).read()
