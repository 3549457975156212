"""CPU tests of apply_calibration (include/gsmcal.h): the restatement of tests/apply_ref.py held to the
definition's own consequences -- the identity, agreement with pair_align's restatement, balanced sample moments after the I/Q
correction, the sign and the second-order terms of apply_params on tones -- and the host helper gsmcal_apply_params (pure host
arithmetic in libgsmcal.so; no GPU) held to the restatement.  Nothing here needs a GPU."""
import math
import os
import re

import numpy as np
import pytest

import apply_ref as ar
import iq_imbalance_ref as iq
import pair_align_ref as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = iq.F


def random_bytes(n, key):
    return np.random.Generator(np.random.Philox(key=[23, key])).integers(0, 256, size=2 * n, dtype=np.uint8)


@pytest.mark.parametrize("dc", [127.5, 127.0, 100.25])
def test_identity_reproduces_the_bytes_minus_dc(dc):
    n = 300
    raw = random_bytes(n, 1)
    res = ar.apply_calibration(raw, 2.4e6, ar.identity_row(dc), n)
    assert (res["status"], res["first_valid"], res["end_valid"], res["num_valid"]) == (0, 7, n - 8, n - 15)
    want = (raw[0::2] - dc) + 1j * (raw[1::2] - dc)
    dev = np.abs(res["out"][7:n - 8] - want[7:n - 8])
    print("identity: largest deviation / bound %.3g" % np.max(dev / (ar.SAMPLE_TOL * res["scale"][7:n - 8])))
    assert np.all(dev <= ar.SAMPLE_TOL * res["scale"][7:n - 8])
    assert not res["out"][:7].any() and not res["out"][n - 8:].any() and res["exact"].all()


@pytest.mark.parametrize("ov", [2, 4, 8])
def test_agreement_with_pair_align_on_the_same_bytes(ov):
    """dc = 0, gain = 1, sin_phase = 0, scale = 1 and sample_rate = fs_of(ov): pair_align of the bytes as a complex stream"""
    n = 700
    raw = random_bytes(n, 2 + ov)
    s = raw[0::2].astype(np.float64) + 1j * raw[1::2].astype(np.float64)
    for six in ([11.2503717, 1000.0, 300.0, 0.7, 0.0], [-25.6, 3.7, -40.0, 0.1, 350.0], [0.0, 0.0, 0.0, 0.0, 0.0], [3.4, -1000.0, 3000.0, 1.3, 33.0]):
        row = np.array(six + [1.0, 0.0, 0.0, 1.0, 0.0])
        for out_len in (n, n + 300):
            got = ar.apply_calibration(raw, pa.fs_of(ov), row, out_len)
            want = pa.pair_align(s, n, ov, six + [1.0], out_len)
            assert [got[k] for k in ("status", "first_valid", "end_valid", "num_valid")] == [want[k] for k in ("status", "first_valid", "end_valid", "num_valid")]
            assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["valid"], want["valid"])
            assert np.all(np.abs(got["out"] - want["out"]) <= 1e-14 * want["scale"])       # the same operations but for z's 1 / c = 1 and - i * 0


def test_iq_correction_balances_the_sample_moments(gsmcal_mod):
    """A make_cw capture with a planted imbalance, corrected with the row of the I/Q check taken over the samples the output covers
    ([7, n - 8): an identity row leaves the other fifteen out): the criterion of tests/test_iq_imbalance_cpu.py -- gain - 1 and
    sin_phase of the output below 1e-9."""
    n = 20000
    raw = gsmcal_mod.synth.make_cw(n, iq_gain=1.07, iq_phase_deg=3.0)
    q = np.array(iq.raw_row(raw[2 * 7: 2 * (n - 8)]))
    assert q[F["status"]] == 0 and abs(q[F["gain"]] - 1.07) <= 2e-3
    row = ar.apply_params(ar.table_row(0.0, 0.0), 433.92e6, q)
    assert row[6:].tolist() == [q[F["dc_I"]], q[F["dc_Q"]], q[F["gain"]], q[F["sin_phase"]]] and row[:6].tolist() == [0, 0, 0, 0, 0, 1]
    res = ar.apply_calibration(raw, 2.048e6, row, n)
    assert (res["first_valid"], res["end_valid"]) == (7, n - 8)
    after = iq.complex_row(res["out"][7:n - 8])
    print("after the correction: gain - 1 = %.3g, sin_phase = %.3g, mean %.3g" % (after[F["gain"]] - 1.0, after[F["sin_phase"]], abs(res["out"][7:n - 8].mean())))
    assert abs(after[F["gain"]] - 1.0) <= 1e-9 and abs(after[F["sin_phase"]]) <= 1e-9
    assert abs(res["out"][7:n - 8].mean()) <= 1e-9                 # ... and the DC is gone


@pytest.mark.parametrize("case", range(3))
def test_helper_sign_and_second_order_terms_on_a_tone(gsmcal_mod, case):
    """A tone f_b seen through a dongle e ppm fast and c ppm off at f_t, corrected by apply_params of the planted e and c, has mean
    phase step 2 pi f_b / fs again.  A wrong sign of either term, a missing (1 + e) on the carrier or a missing 1 / (1 + e) on the
    tone leaves between 6 Hz and 87 kHz."""
    e, c, f_t, f_b, n = ar.TONE_CASES[case]
    raw = gsmcal_mod.synth.make_cw(n, step=ar.tone_step(e, c, f_t, f_b))
    row = ar.apply_params(ar.table_row(e, c), f_t)
    row[6:8] = ar.CW_DC                                            # the known DC: a mean over a few tone periods would bias it
    res = ar.apply_calibration(raw, ar.FS_TONE, row, n)
    lo, hi = res["first_valid"], res["end_valid"]
    assert res["status"] == 0 and hi - lo >= n - 20
    before = ar.tone_frequency((raw[0::2] - ar.CW_DC[0]) + 1j * (raw[1::2] - ar.CW_DC[1])) - f_b
    left = ar.tone_frequency(res["out"][lo:hi]) - f_b
    print(f"tone case {case}: {before:+.1f} Hz before, {left:+.3f} Hz after (recorded {ar.TONE_RESIDUAL_HZ[case]}, bar {ar.TONE_BAR_HZ})")
    assert abs(left) <= ar.TONE_BAR_HZ
    assert abs(abs(left) - ar.TONE_RESIDUAL_HZ[case]) <= 0.01      # the recorded value is this construction's


def test_helper_edge_cases_and_the_library_against_the_restatement(gsmcal_mod):
    g = gsmcal_mod
    n = 64
    raw = random_bytes(n, 9)
    # a failed table row -> an all-NaN row -> status 17 and zeros
    for bad in (ar.table_row(63.0, -21.5, status=10.0), ar.table_row(math.inf, math.inf), ar.table_row(5.0, math.nan), ar.table_row(math.nan, 1.0)):
        row = ar.apply_params(bad, 433.92e6)
        assert np.isnan(row).all()
        assert np.isnan(g.apply_params(bad, 433.92e6)).all()
        res = ar.apply_calibration(raw, 2.4e6, row, n)
        assert res["status"] == ar.S_ALIGN_SKIPPED == g.S_ALIGN_SKIPPED and not res["out"].any() and res["num_valid"] == 0
    # an I/Q row with a constant rail keeps its DC and falls back to gain 1, sin_phase 0
    flat = np.array(iq.raw_row(np.array([9, 1, 9, 2, 9, 3, 9, 4, 9, 5], dtype=np.uint8)))
    assert flat[F["status"]] == g.IQ_FLAT and math.isnan(flat[F["gain"]])
    short = np.array(iq.raw_row(np.array([200, 100], dtype=np.uint8)))
    assert short[F["status"]] == g.IQ_SHORT
    for q, dc in ((flat, (9.0, 3.0)), (short, (200.0, 100.0))):
        row = ar.apply_params(ar.table_row(63.0, -21.5), 433.92e6, q)
        assert row[6:].tolist() == [dc[0], dc[1], 1.0, 0.0]
    # the library's helper is the restatement's, bit for bit (the same operations in the same order), scalars or one value per dongle
    table = np.array([ar.table_row(63.0, -21.5), ar.table_row(-80.0, 40.0), ar.table_row(1000.0, 0.0, status=12.0), ar.table_row(0.0, 0.0)])
    iqt = np.array([iq.raw_row(random_bytes(500, 10 + i)) for i in range(3)] + [flat])
    f_t, delay, phase, scale = [433.92e6, 1090e6, 100e6, 868e6], [0.0, 0.5, -3.25, 11.75], [0.1, -0.2, 0.3, 3.0], [1.0, 0.5, 2.0, -1.0]
    got = g.apply_params(table, f_t, iqt, delay, phase, scale)
    want = np.array([ar.apply_params(table[i], f_t[i], iqt[i], delay[i], phase[i], scale[i]) for i in range(4)])
    assert got.shape == (4, g.APPLY_PARAMS) and np.array_equal(got.view(np.uint64)[[0, 1, 3]], want.view(np.uint64)[[0, 1, 3]]) and np.isnan(got[2]).all()
    got = g.apply_params(table, 433.92e6)
    want = np.array([ar.apply_params(t, 433.92e6) for t in table])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[[0, 1, 3]], want[[0, 1, 3]])
    assert got[0].tolist() == [0.0, 63.0, 1e-6 * -21.5 * 433.92e6 * (1.0 + 1e-6 * 63.0), 0.0, 0.0, 1.0, 127.5, 127.5, 1.0, 0.0]
    with pytest.raises(ValueError):
        g.apply_params(table, 433.92e6, iqt[:2])


def test_header_declares_and_library_exports_the_entry_points(gsmcal_mod):
    g = gsmcal_mod
    txt = open(os.path.join(ROOT, "include", "gsmcal.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = g.load()
    for s in ("gsmcal_apply_calibration_batch", "gsmcal_apply_calibration_batch_resident", "gsmcal_apply_params"):
        assert re.search(r"\bint %s\s*\(" % s, code), s + " is not declared in include/gsmcal.h"
        assert hasattr(lib, s) and s in g.SIGNATURES
    assert not re.search(r"gsmcal_apply\w*_dev\s*\(", txt)         # the registry of the _dev entry points is a follow-up's to extend

    def define(name):
        return int(re.search(r"#define %s (\d+)" % name, txt).group(1))
    assert define("GSMCAL_APPLY_PARAMS") == g.APPLY_PARAMS == ar.APPLY_PARAMS == len(g.APPLY_PARAM_FIELDS)
    assert define("GSMCAL_APPLY_INFO_COLS") == g.APPLY_INFO_COLS == ar.APPLY_INFO_COLS
    assert g.APPLY_PARAM_FIELDS == ar.PARAM_FIELDS
    assert [define("GSMCAL_AP_" + k.upper()) for k in ar.PARAM_FIELDS] == list(range(10))
    for f in ("apply_params", "apply_calibration", "apply_calibration_resident", "apply_rows"):
        assert callable(getattr(g, f))
    assert callable(g.ingest.apply_calibration_slot)
    t = g.apply_rows(np.array([[0.0, 7.0, 100.0, 93.0], [17.0, 0.0, 0.0, 0.0]]))
    assert t["status"].tolist() == [0.0, 17.0] and t["num_valid"].tolist() == [93.0, 0.0]
    # the parameter rows are uploaded by every call, not through a cache of the context
    src = open(os.path.join(ROOT, "multi-rtl-sdr-calibration_amd", "csrc", "abi_calls.h")).read()
    body = src[src.index("static int apply_enqueue"):src.index("int gsmcal_apply_params")]
    assert "upload_" not in body and "hipMemcpyAsync(c->ap_rows.p" in body


def test_the_designed_cases_cover_what_they_claim():
    for n in ar.PARITY_N:
        rows = ar.parity_rows(n)
        assert rows.shape == (120, 10) and [len(r) for r, _ in ar.parity_batches(n)][:4] == [1, 3, 5, 1]
    n = 4099
    raw = random_bytes(n, 11)
    seen = set()
    for row in ar.parity_rows(n):
        for out_len in ar.parity_out_lens(n):
            res = ar.apply_calibration(raw, ar.PARITY_FS, row, out_len)
            assert ar.x_is_safe(res)
            if res["num_valid"] == 0:
                seen.add("none")
            else:
                seen.add("clipped at the start" if res["first_valid"] > 0 else "from 0")
                seen.add("clipped at the end" if res["end_valid"] < out_len else "to the end")
                b = np.floor(res["x"][res["valid"]]) - np.nonzero(res["valid"])[0]
                if len(np.unique(b)) > 1 and res["end_valid"] > 256:
                    seen.add("drift across a tile boundary")
    assert seen == {"none", "clipped at the start", "from 0", "clipped at the end", "to the end", "drift across a tile boundary"}, seen
