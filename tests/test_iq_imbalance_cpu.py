"""CPU tests of the I/Q imbalance and clipping check (include/gsmcal.h): the restatement of tests/iq_imbalance_ref.py
against rows worked by hand and at the overflow edge N = 2^23, the generator's new arguments, the recovery of a planted imbalance,
the whitening identity of the correction, the MEX target and the header's constants.

Recovery bounds (set before the generator was run, from a numpy trial with the impairment emulated on the bytes, about twice what
it showed): gain within 2e-3 and phase within 0.02 deg on CW captures, 0.02 and 0.5 deg on GSM captures -- a GSM capture at 8x
oversampling holds far fewer independent samples than bytes."""
import hashlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import iq_imbalance_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("gsmcal_IQ_imbalance", "gsmcal_iq_imbalance_batch", "gsmcal_iq_imbalance_batch_dev", "gsmcal_iq_correct")
F = ref.F
N_MAX = 1 << 23
# sha256 of the default captures, taken before make_stream / make_cw had the iq_* arguments
SHA_STREAM_4 = "b6c98a79b5a4fccd8e928c57e4c2b46a1c5f151f021d86f9a58a86c6cee2e1b8"      # make_stream(num_frames=4)
SHA_STREAM = "65ba79d0f248be6943208e75f9ce616b8d98db02f421607cb2d1f77ab36b4fbc"        # make_stream()
SHA_CW = "86946f5196d6f37a5edf160266c9be2f289d63857c48773aa8e4d4b2ecf4349b"            # make_cw(20000)
G, PHI = 1.05, 3.0


def interleave(a, b):
    raw = np.empty(2 * len(a), dtype=np.uint8)
    raw[0::2], raw[1::2] = a, b
    return raw


def test_four_samples_worked_by_hand():
    row = ref.raw_row(interleave([1, 3, 5, 7], [2, 2, 6, 6]))
    # S_I = 16, S_Q = 16, S_II = 84, S_QQ = 80, S_IQ = 2 + 6 + 30 + 42 = 80; A_I = 336 - 256 = 80, A_Q = 320 - 256 = 64, C = 64
    assert row[:12] == [4, 16, 16, 84, 80, 80, 1, 7, 2, 6, 0, 0]
    assert ref.moments(interleave([1, 3, 5, 7], [2, 2, 6, 6]))[6:] == (80, 64, 64)
    gain, s = math.sqrt(0.8), 64.0 / (math.sqrt(80.0) * 8.0)
    c = math.sqrt(1.0 - s * s)
    k = 2.0 * gain * s * s / (1.0 + c)
    assert row[F["dc_I"]] == 4.0 and row[F["dc_Q"]] == 4.0 and row[F["var_I"]] == 5.0 and row[F["var_Q"]] == 4.0
    assert row[F["gain"]] == gain and row[F["sin_phase"]] == s and abs(s - 2.0 / math.sqrt(5.0)) < 1e-15
    assert row[F["phase_deg"]] == math.asin(s) * 180.0 / math.pi and abs(row[F["phase_deg"]] - 63.43494882292201) < 1e-12
    assert row[F["irr_db"]] == 10.0 * math.log10(((gain + 1.0) ** 2 - k) / ((gain - 1.0) ** 2 + k))
    assert row[F["level_dbfs"]] == 10.0 * math.log10(9.0 / 32512.5) and row[F["status"]] == 0
    # |K1|^2/|K2|^2 of the model, formed the plain way
    g, phi = gain, math.asin(s)
    k1, k2 = (1 + g * complex(math.cos(phi), math.sin(phi))) / 2, (1 - g * complex(math.cos(phi), -math.sin(phi))) / 2
    assert abs(row[F["irr_db"]] - 10.0 * math.log10(abs(k1) ** 2 / abs(k2) ** 2)) < 1e-12


def test_constant_rail_is_flat_and_one_sample_is_short():
    row = ref.raw_row(interleave([9, 9, 9, 9, 9], [1, 2, 3, 4, 5]))
    assert row[F["status"]] == 2 and row[:12] == [5, 45, 15, 405, 55, 135, 9, 9, 1, 5, 0, 0]
    assert row[F["var_I"]] == 0.0 and row[F["var_Q"]] == 2.0 and row[F["dc_I"]] == 9.0 and row[F["dc_Q"]] == 3.0
    assert row[F["level_dbfs"]] == 10.0 * math.log10(2.0 / 32512.5)
    assert all(math.isnan(row[F[k]]) for k in ("gain", "sin_phase", "phase_deg", "irr_db"))
    row = ref.raw_row(interleave([0], [255]))
    assert row[F["status"]] == 1 and row[:12] == [1, 0, 255, 0, 65025, 0, 0, 0, 255, 255, 1, 1]
    assert row[F["dc_I"]] == 0.0 and row[F["dc_Q"]] == 255.0
    assert all(math.isnan(row[F[k]]) for k in ("var_I", "var_Q", "gain", "sin_phase", "phase_deg", "irr_db", "level_dbfs"))
    balanced = ref.raw_row(interleave([1, 3, 1, 3], [1, 1, 3, 3]))             # gain 1, phase 0: the denominator is exactly 0
    assert balanced[F["gain"]] == 1.0 and balanced[F["sin_phase"]] == 0.0 and balanced[F["irr_db"]] == math.inf


def test_the_overflow_edge_at_two_to_the_23():
    full = np.full(2 * N_MAX, 255, dtype=np.uint8)
    m = ref.moments(full)
    assert m[:6] == (N_MAX, 255 * N_MAX, 255 * N_MAX, 65025 * N_MAX, 65025 * N_MAX, 65025 * N_MAX) and m[6:] == (0, 0, 0)
    row = ref.raw_row(full)
    assert row[F["status"]] == 2 and row[F["clip_I"]] == N_MAX and row[F["level_dbfs"]] == -math.inf
    assert all(v < 2.0 ** 53 for v in row[:12])
    saw = np.tile(np.array([0, 0, 255, 255], dtype=np.uint8), N_MAX // 2)     # both rails 0, 255, 0, 255, ...: the largest A
    m = ref.moments(saw)
    assert m[6] == m[7] == m[8] == 65025 * 2 ** 44 and m[6] < 2 ** 62
    row = ref.raw_row(saw)
    assert row[F["gain"]] == 1.0 and row[F["sin_phase"]] == 1.0 and row[F["phase_deg"]] == 90.0 and row[F["status"]] == 0
    edge = interleave(np.full(N_MAX, 255), np.tile([0, 255], N_MAX // 2))      # the capture tests/test_gpu_iq_imbalance.py hands to the GPU
    m = ref.moments(edge)
    assert m[6:] == (0, 65025 * 2 ** 44, 0) and ref.raw_row(edge)[F["status"]] == 2


def test_generators_are_byte_identical_without_the_new_arguments(gsmcal_mod):
    s = gsmcal_mod.synth
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()   # noqa: E731
    raw, truth = s.make_stream(num_frames=4)
    assert sha(raw) == SHA_STREAM_4 and truth["iq_gain"] is None and truth["iq_phase_deg"] is None
    assert sha(s.make_stream()[0]) == SHA_STREAM
    assert sha(s.make_cw(20000)) == SHA_CW


def test_with_the_new_arguments_only_the_q_bytes_differ(gsmcal_mod):
    s = gsmcal_mod.synth
    a, b = s.make_cw(20000), s.make_cw(20000, iq_gain=G, iq_phase_deg=PHI)
    assert np.array_equal(a[0::2], b[0::2]) and np.count_nonzero(a[1::2] != b[1::2]) > 10000
    (a, _), (b, t) = s.make_stream(num_frames=4), s.make_stream(num_frames=4, iq_gain=G, iq_phase_deg=PHI)
    assert np.array_equal(a[0::2], b[0::2]) and np.count_nonzero(a[1::2] != b[1::2]) > 10000
    assert t["iq_gain"] == G and t["iq_phase_deg"] == PHI
    only_gain = s.make_cw(2048, iq_gain=G)
    assert abs(ref.raw_row(only_gain)[F["gain"]] - G) < 2e-3 and abs(ref.raw_row(only_gain)[F["phase_deg"]]) < 0.02


@pytest.mark.parametrize("n", [20000, 2048])
def test_recovery_of_a_planted_imbalance_on_cw(gsmcal_mod, n):
    row = ref.raw_row(gsmcal_mod.synth.make_cw(n, iq_gain=G, iq_phase_deg=PHI))
    print("make_cw(%d): gain error %.3g, phase error %.3g deg, irr %.2f dB" % (n, row[F["gain"]] - G, row[F["phase_deg"]] - PHI, row[F["irr_db"]]))
    assert abs(row[F["gain"]] - G) <= 2e-3 and abs(row[F["phase_deg"]] - PHI) <= 0.02


@pytest.mark.parametrize("frames", [16, 102])
def test_recovery_of_a_planted_imbalance_on_gsm(gsmcal_mod, frames):
    for dongle in range(6):
        row = ref.raw_row(gsmcal_mod.synth.make_stream(dongle=dongle, num_frames=frames, iq_gain=G, iq_phase_deg=PHI)[0])
        print("make_stream(dongle=%d, num_frames=%d): gain error %.3g, phase error %.3g deg" % (dongle, frames, row[F["gain"]] - G, row[F["phase_deg"]] - PHI))
        assert abs(row[F["gain"]] - G) <= 0.02 and abs(row[F["phase_deg"]] - PHI) <= 0.5, (dongle, frames)


def test_correction_whitens_the_sample_moments(gsmcal_mod):
    """iq_correct with a capture's own gain and s: exact in real arithmetic, 2e4 fp64 terms cannot lose more than 1e-9"""
    for raw in (gsmcal_mod.synth.make_cw(20000, iq_gain=G, iq_phase_deg=PHI), gsmcal_mod.synth.make_stream(num_frames=2, iq_gain=0.93, iq_phase_deg=-5.0)[0]):
        x = ref.to_complex(raw)
        x = x - x.mean()
        row = ref.complex_row(x)
        after = ref.complex_row(ref.correct(x, row[F["gain"]], row[F["sin_phase"]]))
        print("whitened: gain - 1 = %.3g, s = %.3g" % (after[F["gain"]] - 1.0, after[F["sin_phase"]]))
        assert abs(after[F["gain"]] - 1.0) <= 1e-9 and abs(after[F["sin_phase"]]) <= 1e-9
        assert abs(row[F["gain"]] - ref.raw_row(raw)[F["gain"]]) <= 1e-12      # the complex form agrees with the integer form


def test_header_declares_and_library_exports_the_entry_points(gsmcal_mod):
    txt = open(os.path.join(ROOT, "include", "gsmcal.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = gsmcal_mod.load()
    for s in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % s, code), s + " is not declared in include/gsmcal.h"
        assert hasattr(lib, s) and s in gsmcal_mod.SIGNATURES
    for f in ("IQ_imbalance", "iq_imbalance_batch", "iq_imbalance_batch_dev", "iq_correct", "iq_rows"):
        assert callable(getattr(gsmcal_mod, f))
    assert callable(gsmcal_mod.ingest.check_front_end)


def test_constants_match_the_header(gsmcal_mod):
    txt = open(os.path.join(ROOT, "include", "gsmcal.h")).read()

    def define(name):
        return re.search(r"#define %s (.+?)\s*(?:/\*|$)" % name, txt, flags=re.M).group(1)
    assert int(define("GSMCAL_IQ_COLS")) == gsmcal_mod.IQ_COLS == len(gsmcal_mod.IQ_FIELDS) == 22
    assert int(define("GSMCAL_IQ_TILE")) == gsmcal_mod.IQ_TILE
    assert define("GSMCAL_IQ_MAX_N") == "(1L << 23)" and gsmcal_mod.IQ_MAX_N == N_MAX
    assert (int(define("GSMCAL_IQ_OK")), int(define("GSMCAL_IQ_SHORT")), int(define("GSMCAL_IQ_FLAT"))) == \
        (gsmcal_mod.IQ_OK, gsmcal_mod.IQ_SHORT, gsmcal_mod.IQ_FLAT) == (0, 1, 2)
    for i, k in enumerate(gsmcal_mod.IQ_FIELDS):                                # the named indices follow IQ_FIELDS
        assert int(define("GSMCAL_Q_" + k.upper())) == i, k


def test_iq_rows_names_the_columns(gsmcal_mod):
    t = np.array([ref.raw_row(interleave([1, 3, 5, 7], [2, 2, 6, 6])), ref.complex_row([1 + 2j, 3 + 2j, 5 + 6j, 7 + 6j])])
    rows = gsmcal_mod.iq_rows(t)
    assert rows[0]["n"] == 4 and rows[0]["clip_I"] == 0 and rows[0]["status"] == 0 and rows[0]["var_I"] == 5.0
    assert isinstance(rows[0]["n"], int) and isinstance(rows[0]["status"], int) and list(rows[0]) == list(gsmcal_mod.IQ_FIELDS)
    assert rows[1]["clip_I"] is None and rows[1]["clip_Q"] is None and rows[1]["gain"] == rows[0]["gain"]


@pytest.mark.parametrize("api", ["interleaved", "split"])
def test_mex_iq_imbalance_target_compiles_against_the_abi(api):
    """The IQ_imbalance target of mex/gsmcal_mex.c through `gcc -fsyntax-only` against the declaration-only mex.h (tests/mex_stub),
    once per MEX complex-storage API, as tests/test_abi_cpu.py does for the other targets."""
    src = open(os.path.join(ROOT, "mex", "gsmcal_mex.c")).read()
    assert "defined(GSMCAL_FN_IQ_imbalance)" in src
    r = subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-std=c99", "-DGSMCAL_FN_IQ_imbalance"] +
                       (["-DGSMCAL_STUB_SPLIT"] if api == "split" else []) +
                       ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mex_stub"),
                        os.path.join(ROOT, "mex", "gsmcal_mex.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
