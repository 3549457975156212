"""GPU parity tests (-m gpu): the HIP path, called through the C ABI, against the CPU oracle on the same
seeded inputs, against the committed golden vectors, and -- at BASELINE.json's full sizes -- through
size-independent properties.  Bars: integer positions bit-exact; ppm within 1e-6 relative (+1e-9 ppm
absolute floor where the oracle value is ~0); reported SNRs within 1e-8 dB; corrected streams
within 2e-8 of their peak magnitude (the derotation exp(1i*k*c) turns a ~1e-14 relative difference in the
estimated tone frequency into k*c*1e-14 ~ 1e-9 rad at k = 1e6, so streams cannot agree tighter than that)."""
import json
import math
import os
import sys

import numpy as np
import pytest

import parity
from oracle import gsmcal_oracle as o

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FC = 957.4e6
STREAM_RTOL = 2e-8


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


@pytest.fixture(scope="module")
def setup(g):
    s = g.synth
    return {"coef": s.fir1(46, 200e3 / s.FS), "coef30": s.fir1(30, 200e3 / s.FS), "ts": s.sch_training_sequence(),
            "num": o.load_num(os.path.join(HERE, "golden", "gsm_chn_filter_8x_num.txt"))}


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(HERE, "golden", "calib_golden.json")) as f:
        return json.load(f)


def stream_close(a, b):
    assert isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape, (np.shape(a), np.shape(b))
    scale = np.max(np.abs(b))
    err = np.max(np.abs(a - b))
    assert err <= STREAM_RTOL * scale, f"stream mismatch: max abs err {err} at scale {scale}"


# ---- a1 / a2: front end ------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(1000, 1), (4099, 3), (20000, 2)])
def test_raw2iq_bit_exact(g, n, d):
    rng = np.random.default_rng(n)
    a = rng.integers(0, 256, size=(2 * n, d), dtype=np.uint8)
    want = o.raw2iq(a.astype(np.float64))
    assert np.array_equal(g.raw2iq(a), want)                       # uint8 as it comes off the wire
    assert np.array_equal(g.raw2iq(a.astype(np.float64)), want)    # doubles holding byte values (fread)
    assert np.array_equal(g.raw2iq(a[:, 0]), want[:, 0])           # vector in, vector out


def test_chn_filter_8x_4x_matches_oracle(g, setup):
    rng = np.random.default_rng(5)
    s = rng.standard_normal((5001, 2)) + 1j * rng.standard_normal((5001, 2))
    want = o.chn_filter_8x_4x(s, setup["num"])
    got = g.chn_filter_8x_4x(s)                    # built-in taps == the .fda numerator
    assert got.shape == want.shape == (2501, 2)
    assert np.max(np.abs(got - want)) < 1e-13
    assert np.max(np.abs(g.chn_filter_8x_4x(s, setup["num"]) - want)) < 1e-13


def test_chn_filter_4x_matches_oracle(g, setup):
    # chn_filter_4x.m:13: filter(Num,1,s) with the 30 taps of gsm_chn_filter_4x.fda, every row kept
    num4 = o.load_num(os.path.join(HERE, "golden", "gsm_chn_filter_4x_num.txt"))
    rng = np.random.default_rng(4)
    s = rng.standard_normal((5001, 2)) + 1j * rng.standard_normal((5001, 2))
    want = o.chn_filter_4x(s, num4)
    assert np.max(np.abs(g.chn_filter_4x(s) - want)) < 1e-13          # built-in taps == the .fda numerator
    assert np.max(np.abs(g.chn_filter_4x(s[:, 0], num4) - want[:, 0])) < 1e-13


def test_driver_front_end_filter_and_decimation(g, setup):
    # gsm_sync_demod.m:107,110,117: r = raw2iq(s); r = filter(coef,1,r); r(1:64:end,i)
    raw = np.stack([g.synth.make_stream(dongle=d, num_frames=8)[0] for d in (0, 1)])
    r = o.matlab_filter(setup["coef"], o.raw2iq(raw.T.astype(np.float64)))
    got = g.frontend_batch(raw, setup["coef"], 64)
    assert got.shape == (2, 1250)
    assert np.max(np.abs(got.T - r[0::64])) < 1e-12
    full = g.frontend_batch(raw, setup["coef"], 1)
    assert np.max(np.abs(full.T - r)) < 1e-12
    assert np.max(np.abs(g.filter(setup["coef"], o.raw2iq(raw.T.astype(np.float64))) - r)) < 1e-12


# ---- a3 / a4 / a5: coarse detector -------------------------------------------------------------
def _coarse_input(g, setup, dongle, frames=102, coef="coef", **kw):
    raw, _ = g.synth.make_stream(dongle=dongle, num_frames=frames, **kw)
    r = o.matlab_filter(setup[coef], o.raw2iq(raw.astype(np.float64)))
    return raw, r


def test_move_fft_snr_runtime_avg(g, setup):
    _, r = _coarse_input(g, setup, 0)
    s = r[0::64][:3594]
    want = o.move_fft_snr_runtime_avg(s, 160, 16, 10)
    got = g.move_fft_snr_runtime_avg(s, 160, 16, 10)
    assert got[0] == want[0] and got[1] == want[1]
    assert abs(got[2] - want[2]) < parity.SNR_ATOL and abs(got[3] - want[3]) < parity.SNR_ATOL
    # other fft lengths go through the generic DFT path
    want8 = o.move_fft_snr_runtime_avg(s, 80, 8, 6)
    got8 = g.move_fft_snr_runtime_avg(s, 80, 8, 6)
    assert got8[:2] == want8[:2] and abs(got8[3] - want8[3]) < parity.SNR_ATOL
    # no hit: sentinel [false, -1, inf, inf]
    noise = np.random.default_rng(0).standard_normal(600) + 1j * np.random.default_rng(1).standard_normal(600)
    assert g.move_fft_snr_runtime_avg(noise, 160, 16, 10) == (False, -1, math.inf, math.inf)


def test_specific_fft_snr_fix_avg(g, setup):
    _, r = _coarse_input(g, setup, 0)
    s = r[0::64]
    pos, _ = o.FCCH_coarse_position(s, 8)
    p = int((pos[1] - 1) / 8 + 1)
    for avg in (-3.0, 50.0):
        want = o.specific_fft_snr_fix_avg(s, (p - 5, p + 5), 16, 10, avg)
        got = g.specific_fft_snr_fix_avg(s, (p - 5, p + 5), 16, 10, avg)
        assert got[:2] == want[:2]
        assert (math.isinf(want[2]) and math.isinf(got[2])) or abs(got[2] - want[2]) < parity.SNR_ATOL
    with pytest.raises(g.GsmcalError):       # MATLAB index error -> GSMCAL_E_INDEX, never an OOB read
        g.specific_fft_snr_fix_avg(s, (0, 5), 16, 10, 0.0)
    # window by window like the reference's loop (:10-11): a hit in a window that fits comes back before a later window would
    # run past the end of s; a miss up to there is the index error
    rng = np.random.default_rng(5)
    t = rng.standard_normal(100) + 1j * rng.standard_normal(100)
    with pytest.raises(g.GsmcalError):
        g.specific_fft_snr_fix_avg(t, (80, 90), 16, 10, 50.0)
    with pytest.raises(g.GsmcalError):
        g.specific_fft_snr_fix_avg(t, (86, 90), 16, 10, 0.0)
    t[82:98] += 40 * np.exp(2j * np.pi * 0.125 * np.arange(16))
    want = o.specific_fft_snr_fix_avg(t, (80, 90), 16, 10, 0.0)
    got = g.specific_fft_snr_fix_avg(t, (80, 90), 16, 10, 0.0)
    assert want[0] and got[:2] == want[:2] and abs(got[2] - want[2]) < parity.SNR_ATOL


@pytest.mark.parametrize("dongle,frames,coef", [(0, 102, "coef"), (3, 102, "coef"), (50, 64, "coef30")])
def test_FCCH_coarse_position(g, setup, dongle, frames, coef):
    _, r = _coarse_input(g, setup, dongle, frames, coef)
    want_p, want_s = o.FCCH_coarse_position(r[0::64], 8)
    got_p, got_s = g.FCCH_coarse_position(r[0::64], 8)
    parity.assert_positions(got_p, want_p, "position")
    assert np.allclose(got_s, want_s, rtol=0, atol=parity.SNR_ATOL)


def test_FCCH_coarse_position_no_fcch_sentinel(g, setup):
    raw, _ = g.synth.make_stream(dongle=9, num_frames=64, bcch=False)
    r = o.matlab_filter(setup["coef30"], o.raw2iq(raw.astype(np.float64)))
    assert o.FCCH_coarse_position(r[0::64], 8) == (-1.0, -1.0)
    assert g.FCCH_coarse_position(r[0::64], 8) == (-1.0, -1.0)


# ---- a6..a9: the chain function by function, as gsm_sync_demod.m:117-124 calls it ---------------------
@pytest.mark.parametrize("dongle", [0, 1, 3, 4])
def test_chain_function_by_function(g, setup, dongle):
    raw, r = _coarse_input(g, setup, dongle)
    ts = setup["ts"]
    # oracle
    o_pos, _ = o.FCCH_coarse_position(r[0::64], 8)
    o_fp, o_r1, o_sp1, o_cp1 = o.FCCH_fine_correction(r, o_pos, 8, FC)
    o_pi, o_r2, o_sp2 = o.SCH_corr_rate_correction(o_r1, o_fp, ts, 8)
    o_r3, o_cp2 = o.carrier_correct_post_SCH(o_r2, o_pi, 8, FC)
    # HIP path, same call sequence
    pos, _ = g.FCCH_coarse_position(r[0::64], 8)
    fp, r1, sp1, cp1 = g.FCCH_fine_correction(r, pos, 8, FC)
    pi, r2, sp2 = g.SCH_corr_rate_correction(r1, fp, ts, 8)
    r3, cp2 = g.carrier_correct_post_SCH(r2, pi, 8, FC)

    parity.assert_positions(fp, o_fp, "FCCH_pos")
    parity.assert_ppm(sp1, o_sp1, "sampling_ppm(1)")
    parity.assert_ppm(cp1, o_cp1, "carrier_ppm(1)")
    parity.assert_positions(pi, o_pi, "pos_info")            # (sentinels included: [-1 -1] or -ones(3K,2), same shape)
    parity.assert_ppm(sp2, o_sp2, "sampling_ppm(2)")
    parity.assert_ppm(cp2, o_cp2, "carrier_ppm(2)")
    for got, want in ((r1, o_r1), (r2, o_r2), (r3, o_r3)):
        if isinstance(want, np.ndarray):
            stream_close(got, want)
        else:
            assert got == -1.0 and want == -1.0
    tot = [g.total_ppm_calculation([sp1, sp2]), g.total_ppm_calculation([cp1, cp2])]
    parity.assert_ppm(tot[0], o.total_ppm_calculation([o_sp1, o_sp2]), "total sampling ppm")
    parity.assert_ppm(tot[1], o.total_ppm_calculation([o_cp1, o_cp2]), "total carrier ppm")


def test_console_diagnostics_are_the_reference_s_lines(g, setup, capsys):
    """SURVEY 5 / VERDICT r5 missing #5: the lines the .m files disp() (FCCH_coarse_position.m:6,92-94, FCCH_fine_correction.m:6,66,
    116,156-161,190, SCH_corr_rate_correction.m:6,80,118, carrier_correct_post_SCH.m:6,73-79, the warnings of the early exits) come
    back from gsmcal_last_call_report after each per-function call -- rebuilt here from the ORACLE's intermediates (first-round
    positions, per-burst tone frequencies and SNRs) with the same num2str: every line must match, value for value as printed."""
    n2s = g.num2str
    raw, r = _coarse_input(g, setup, 0)
    ts = setup["ts"]
    inf1, inf2, inf3 = {}, {}, {}
    o_pos, o_snr = o.FCCH_coarse_position(r[0::64], 8)
    o_fp, o_r1, o_sp1, o_cp1 = o.FCCH_fine_correction(r, o_pos, 8, FC, info=inf1)
    o_pi, o_r2, o_sp2 = o.SCH_corr_rate_correction(o_r1, o_fp, ts, 8, info=inf2)
    o_r3, o_cp2 = o.carrier_correct_post_SCH(o_r2, o_pi, 8, FC, info=inf3)

    def close(got, want):
        """same text, or numbers that agree to the printed precision where the last printed digit sits on a rounding edge"""
        if got == want:
            return True
        ga, wa = got.split(), want.split()
        if len(ga) != len(wa):
            return False
        for a, b in zip(ga, wa):
            if a != b:
                try:
                    if abs(float(a) - float(b)) > 2e-4 * max(1.0, abs(float(b))) * 1e-3 + 1.5e-4:
                        return False
                except ValueError:
                    return False
        return True

    pos, snr = g.FCCH_coarse_position(r[0::64], 8)
    rep = g.last_call_report().split("\n")
    want = [" ", f"FCCH coarse: hit successive {len(o_pos)} FCCH. pos {n2s(o_pos)}", f"FCCH coarse: pos diff {n2s(np.diff(o_pos))}",
            f"FCCH coarse: SNR {n2s(o_snr)}", ""]
    assert len(rep) == len(want) and all(close(a, b) for a, b in zip(rep, want)), rep
    fp, r1, sp1, cp1 = g.FCCH_fine_correction(r, pos, 8, FC)
    rep = g.last_call_report().split("\n")
    fo = inf1["fo_per_burst"]
    want = [" ", f"FCCH fine: first round diff {n2s(np.diff(inf1['first_round_pos']))}", f"FCCH fine: sampling error ppm {n2s(o_sp1)}",
            f"FCCH fine: FCCH freq {n2s(fo)}", f"FCCH fine: mean FCCH freq {n2s(np.mean(fo))}", f"FCCH fine: carrier error ppm {n2s(o_cp1)}",
            f"FCCH fine: SNR {n2s(inf1['fcch_snr'])}", ""]
    assert len(rep) == len(want) and all(close(a, b) for a, b in zip(rep, want)), (rep, want)
    pi, r2, sp2 = g.SCH_corr_rate_correction(r1, fp, ts, 8)
    rep = g.last_call_report().split("\n")
    want = [" ", f"SCH: first round diff {n2s(np.diff(inf2['first_round_sch_pos']))}", f"SCH: sampling error ppm {n2s(o_sp2)}", ""]
    assert len(rep) == len(want) and all(close(a, b) for a, b in zip(rep, want)), (rep, want)
    r3, cp2 = g.carrier_correct_post_SCH(r2, pi, 8, FC)
    rep = g.last_call_report().split("\n")
    fo = inf3["fo_per_burst"]
    want = [" ", f"post SCH: FCCH freq {n2s(fo)}", f"post SCH: mean FCCH freq {n2s(np.mean(fo))}", f"post SCH: carrier error ppm {n2s(o_cp2)}", ""]
    assert len(rep) == len(want) and all(close(a, b) for a, b in zip(rep, want)), (rep, want)
    # the early exits' warnings, and the Python mirror printing them when asked to
    g.set_verbose(True)
    try:
        noise = np.random.default_rng(3).standard_normal(16000) + 1j * np.random.default_rng(4).standard_normal(16000)
        assert g.FCCH_coarse_position(noise, 8) == (-1.0, -1.0)
        g.FCCH_fine_correction(r, pos[:3], 8, FC)
        g.SCH_corr_rate_correction(-1.0, -1.0, ts, 8)
        g.carrier_correct_post_SCH(-1.0, np.array([[-1.0, -1.0]]), 8, FC)
        assert g.total_ppm_calculation([np.inf, np.inf]) == np.inf
    finally:
        g.set_verbose(False)
    out = capsys.readouterr().out
    for line in ("FCCH coarse: No FCCH found!", "FCCH fine: Warning! Length of hits is smaller than 5!", "SCH: Warning! Length of hits is smaller than 5!",
                 "post SCH: Warning! No valid position information!", "total PPM calculation: No valid PPM input!"):
        assert line in out, (line, out)


@pytest.mark.parametrize("ov", [4, 2])
def test_chain_at_other_oversampling_ratios(g, setup, ov):
    """The per-function API takes the oversampling ratio as an argument (every .m file does): 4x and 2x streams
    exercise the general-geometry paths (592- / 296-point spectra, 8 / 4 chunks, other FFT factorisations)."""
    raw, r8 = _coarse_input(g, setup, 3)
    step = 8 // ov
    r = np.ascontiguousarray(r8[0::step])
    ts = np.ascontiguousarray(setup["ts"][0::step])
    o_pos, _ = o.FCCH_coarse_position(r[0::8 * ov], 8)
    pos, _ = g.FCCH_coarse_position(r[0::8 * ov], 8)
    parity.assert_positions(pos, o_pos, "coarse position")
    o_fp, o_r1, o_sp1, o_cp1 = o.FCCH_fine_correction(r, o_pos, ov, FC)
    fp, r1, sp1, cp1 = g.FCCH_fine_correction(r, pos, ov, FC)
    parity.assert_positions(fp, o_fp, "FCCH_pos")
    parity.assert_ppm(sp1, o_sp1, "sampling_ppm(1)")
    parity.assert_ppm(cp1, o_cp1, "carrier_ppm(1)")
    if isinstance(o_r1, np.ndarray):
        stream_close(r1, o_r1)
        o_pi, o_r2, o_sp2 = o.SCH_corr_rate_correction(o_r1, o_fp, ts, ov)
        pi, r2, sp2 = g.SCH_corr_rate_correction(r1, fp, ts, ov)
        parity.assert_positions(pi, o_pi, "pos_info")
        parity.assert_ppm(sp2, o_sp2, "sampling_ppm(2)")
        o_r3, o_cp2 = o.carrier_correct_post_SCH(o_r2, o_pi, ov, FC)
        r3, cp2 = g.carrier_correct_post_SCH(r2, pi, ov, FC)
        parity.assert_ppm(cp2, o_cp2, "carrier_ppm(2)")


def test_fine_correction_sentinels(g, setup):
    _, r = _coarse_input(g, setup, 0)
    # fewer than 5 coarse hits (FCCH_fine_correction.m:12-15)
    fp, rr, sp, cp = g.FCCH_fine_correction(r, [10305.0, 22801.0, 35313.0], 8, FC)
    assert fp == -1.0 and rr == -1.0 and sp == math.inf and cp == math.inf
    # positions that are not FCCH bursts: spacing classification fails or the SNR gate trips -- same as oracle
    bad = np.array([5000.0, 17000.0, 30000.0, 43000.0, 56000.0, 69000.0])
    want = o.FCCH_fine_correction(r, bad, 8, FC)
    got = g.FCCH_fine_correction(r, bad, 8, FC)
    parity.assert_positions(got[0], want[0], "FCCH_pos (bad input)")
    parity.assert_ppm(got[2], want[2], "sampling ppm (bad input)")
    if isinstance(want[1], np.ndarray):
        stream_close(got[1], want[1])
    # a coarse hit in the first 64 symbols would index before the signal: MATLAB errors, the ABI returns E_INDEX
    with pytest.raises(g.GsmcalError):
        g.FCCH_fine_correction(r, [10.0, 12510.0, 25010.0, 37510.0, 50010.0], 8, FC)
    with pytest.raises(o.MatlabIndexError):
        o.FCCH_fine_correction(r, [10.0, 12510.0, 25010.0, 37510.0, 50010.0], 8, FC)


def test_sch_and_post_sentinels(g, setup):
    ts = setup["ts"]
    pi, rr, sp = g.SCH_corr_rate_correction(-1.0, -1.0, ts, 8)          # failed fine stage upstream
    assert pi.shape == (1, 2) and np.all(pi == -1) and rr == -1.0 and sp == math.inf
    rr, cp = g.carrier_correct_post_SCH(-1.0, pi, 8, FC)
    assert rr == -1.0 and cp == math.inf
    # pos_info with fewer than 4 BCCH rows (carrier_correct_post_SCH.m:15-19)
    rr, cp = g.carrier_correct_post_SCH(np.zeros(30000, complex), np.array([[1.0, 0], [10001.0, 1], [20001.0, 2]]), 8, FC)
    assert rr == -1.0 and cp == math.inf
    # SCH peak on the edge of the search window -> pos_info = [-1 -1] (SCH_corr_rate_correction.m:59-63)
    _, r = _coarse_input(g, setup, 0)
    o_pos, _ = o.FCCH_coarse_position(r[0::64], 8)
    o_fp, o_r1, _, _ = o.FCCH_fine_correction(r, o_pos, 8, FC)
    shifted = o_fp + 200.0                                               # pushes the true peak outside the window
    want = o.SCH_corr_rate_correction(o_r1, shifted, ts, 8)
    got = g.SCH_corr_rate_correction(o_r1, shifted, ts, 8)
    assert np.all(want[0] == -1) and np.all(got[0] == -1) and got[0].shape == want[0].shape == (1, 2)
    assert got[1] == -1.0 or isinstance(want[1], np.ndarray)
    parity.assert_ppm(got[2], want[2], "sampling ppm (edge)")
    # spacing failure (SCH_corr_rate_correction.m:106-112): the reference hands back its -ones(3*num_fcch_hit, 2)
    # pre-allocation (:32) and r = s (:87); gsm_sync_demod.m:130 counts those rows
    bent = o_fp.copy()
    bent[2:] += 300.0                                                    # the true peaks leave the search windows: interior maxima
    want = o.SCH_corr_rate_correction(o_r1, bent, ts, 8)
    got = g.SCH_corr_rate_correction(o_r1, bent, ts, 8)
    assert want[0].shape == (3 * len(bent), 2) and np.all(want[0] == -1)
    assert got[0].shape == want[0].shape and np.all(got[0] == -1)
    assert isinstance(want[1], np.ndarray) and isinstance(got[1], np.ndarray) and len(got[1]) == len(want[1])
    assert math.isinf(got[2]) and math.isinf(want[2])
    # fewer than 5 SCH windows inside the stream (:84): same shape, r = -1
    short = o_r1[: int(o_fp[4]) + 9000]                                  # the 5th SCH window runs out of samples
    want = o.SCH_corr_rate_correction(short, o_fp[:5], ts, 8)
    got = g.SCH_corr_rate_correction(short, o_fp[:5], ts, 8)
    assert want[0].shape == (15, 2) and got[0].shape == (15, 2) and np.all(got[0] == -1) and got[1] == -1.0 and want[1] == -1.0


# ---- batched hot path vs golden vectors and vs the oracle ---------------------------------------------
def test_calibrate_batch_against_golden_vectors(g, setup, gold):
    cases = gold["cases"]
    raw = np.stack([g.synth.make_stream(dongle=c["dongle"], arfcn=c["arfcn"], num_frames=c["num_frames"])[0] for c in cases])
    for c, r in zip(cases, raw):
        assert int(np.sum(r.astype(np.uint64))) == c["raw_sum"]
    out = g.calibrate_batch(raw, setup["coef"], setup["ts"], gold["carrier_freq"])
    det = g.last_batch_details(len(cases))

    def num(v):
        return math.inf if v == "inf" else v

    for i, c in enumerate(cases):
        orc = {"coarse_pos": np.asarray(c["coarse_pos"]), "coarse_snr": np.asarray(c["coarse_snr"]),
               "fine_first_round_pos": np.asarray(c["fine_first_round_pos"]), "fcch_pos": np.asarray(c["fcch_pos"]),
               "sch_first_round_pos": np.asarray(c["sch_first_round_pos"]),
               "pos_info": np.asarray(c["pos_info"]).reshape(-1, 2),
               "sampling_ppm": [num(v) for v in c["sampling_ppm"]], "carrier_ppm": [num(v) for v in c["carrier_ppm"]],
               "total_sampling_ppm": num(c["total_sampling_ppm"]), "total_carrier_ppm": num(c["total_carrier_ppm"])}
        parity.compare_stream(orc, out["table"][i], det, i, out["pos_info"][i])
        assert out["r_len"][i] == c["r_len"]


def test_front_end_against_golden_probe_vectors(g, setup, gold):
    """SURVEY 8c front-end vectors from tests/golden/calib_golden.json (the record tests/golden/make_reference_vectors.m
    writes for the reference itself): raw2iq checksums and first / last 16 values, channel-filter output at 32 probe
    indices -- HIP raw2iq and the batch front end at full rate (decimation 1) on the sync and the scanner geometry."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import refvec

    class HipFrontEnd:                                     # the two calls refvec.front_end_record makes, on the GPU
        def __init__(self, raw):
            self.raw = raw

        def raw2iq(self, a):
            return g.raw2iq(self.raw)

        def matlab_filter(self, coef, r):
            return g.frontend_batch(self.raw[None, :], coef, 1)[0]

    for case, coef in [(gold["cases"][0], setup["coef"]), (gold["cases"][3], setup["coef"]), (gold["scans"][0], setup["coef30"])]:
        raw = g.synth.make_stream(dongle=case["dongle"], arfcn=case["arfcn"], num_frames=case["num_frames"], bcch=case.get("bcch", True))[0]
        assert int(np.sum(raw.astype(np.uint64))) == case["raw_sum"]
        fe = refvec.front_end_record(HipFrontEnd(raw), raw, coef)[0]
        assert refvec.compare(case["front_end"], fe, f"dongle {case['dongle']} arfcn {case['arfcn']}", val_rtol=1e-12) == []


def test_calibrate_batch_against_live_oracle_with_stream_output(g, setup):
    dongles = [10, 11, 12, 13, 14, 15]
    raw = np.stack([g.synth.make_stream(dongle=d)[0] for d in dongles])
    out = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC, want_r=True)
    det = g.last_batch_details(len(dongles))
    n_ok = 0
    for i in range(len(dongles)):
        orc = o.calibrate_stream(raw[i], setup["coef"], setup["ts"], FC, keep_r=True)
        parity.compare_stream(orc, out["table"][i], det, i, out["pos_info"][i])
        if isinstance(orc.get("r_correct"), np.ndarray):
            n_ok += 1
            L = int(out["r_len"][i])
            assert L == len(orc["r_correct"])
            stream_close(out["r_correct"][i, :L], orc["r_correct"])
        else:
            assert out["r_len"][i] == -1
    assert n_ok >= 2, "the seeded set should contain streams the reference algorithm calibrates"


def test_scan_batch_against_golden_and_oracle(g, setup, gold):
    scans = gold["scans"]
    raw = np.stack([g.synth.make_stream(dongle=c["dongle"], arfcn=c["arfcn"], num_frames=c["num_frames"], bcch=c["bcch"])[0]
                    for c in scans])
    out = g.fcch_scan_batch(raw, setup["coef30"])
    for i, c in enumerate(scans):
        assert out["num_hit"][i] == c["num_hit"]
        assert abs(out["snr"][i] - c["snr"]) < parity.SNR_ATOL
        n = out["counts"][i]
        if c["coarse_pos"] == [-1.0]:
            assert n == 0 and out["positions"][i, 0] == -1.0
        else:
            parity.assert_positions(out["positions"][i, :n], c["coarse_pos"], "scan positions")
            assert np.allclose(out["pos_snr"][i, :n], c["coarse_snr"], rtol=0, atol=parity.SNR_ATOL)
        live = o.scan_capture(raw[i], setup["coef30"])
        assert live["num_hit"] == out["num_hit"][i] and abs(live["snr"] - out["snr"][i]) < parity.SNR_ATOL


# ---- edge cases --------------------------------------------------------------------------------------
def test_batch_of_one_and_unaligned_lengths(g, setup):
    # 61 frames: 2N = 1 220 000 bytes is not a multiple of 16 per stream -> exercises the unaligned DC-sum path
    raw = np.stack([g.synth.make_stream(dongle=d, num_frames=61)[0][: 2 * 609991] for d in (20, 21, 22)])
    out = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC)
    det = g.last_batch_details(3)
    for i in range(3):
        orc = o.calibrate_stream(raw[i], setup["coef"], setup["ts"], FC)
        parity.compare_stream(orc, out["table"][i], det, i, out["pos_info"][i])
    one = g.calibrate_batch(raw[1:2], setup["coef"], setup["ts"], FC)
    assert np.array_equal(one["table"][0], out["table"][1], equal_nan=True)


def test_noise_only_stream_yields_all_sentinels(g, setup):
    rng = np.random.default_rng(7)
    raw = np.clip(np.round(127.5 + 20 * rng.standard_normal((1, 2 * 1020000))), 0, 255).astype(np.uint8)
    out = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC)
    orc = o.calibrate_stream(raw[0], setup["coef"], setup["ts"], FC)
    assert math.isinf(orc["total_sampling_ppm"]) and math.isinf(orc["total_carrier_ppm"])
    row = out["table"][0]
    assert np.all(np.isinf(row[:6])) and row[6] == 1 and row[7] == 1 and row[8] == -1 and row[9] > 0
    assert out["pos_info"][0].shape == (1, 2) and np.all(out["pos_info"][0] == -1) and out["r_len"][0] == -1


def test_too_short_capture_is_an_error_not_a_crash(g, setup):
    raw = np.stack([g.synth.make_stream(dongle=0, num_frames=20)[0]])    # < 23 frames: s(1:3594) would not exist
    out = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC)
    assert out["table"][0, 9] == -5                                      # GSMCAL_E_INDEX, like MATLAB's index error
    with pytest.raises(o.MatlabIndexError):
        o.calibrate_stream(raw[0], setup["coef"], setup["ts"], FC)


def test_scan_of_too_short_captures_is_an_index_error(g, setup):
    # MATLAB stops at s(1:3594) (FCCH_coarse_position.m:25) when a capture has fewer than 23 frames: E_INDEX, not "no carrier"
    raw = np.stack([g.synth.make_stream(dongle=0, num_frames=20)[0]])
    with pytest.raises(g.GsmcalError, match="-5"):
        g.fcch_scan_batch(raw, setup["coef30"])
    with pytest.raises(o.MatlabIndexError):
        o.scan_capture(raw[0], setup["coef30"])


def test_repeated_batch_calls_on_the_default_stream(g, setup):
    """gsmcal_ctx_create_on_stream(dev, 0): the legacy NULL stream cannot be captured into a hipGraph; repeated identical
    calls must keep working (eager launches) and keep giving the same table."""
    raw = np.stack([g.synth.make_stream(dongle=d, num_frames=102)[0] for d in (0, 3)])
    ref = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC)
    c0 = g.Context(0, stream=0)
    try:
        for _ in range(4):
            out = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC, ctx=c0)
            assert np.array_equal(out["table"], ref["table"], equal_nan=True)
        for _ in range(3):
            sc = g.fcch_scan_batch(raw[:, : 2 * 640000], setup["coef30"], ctx=c0)
        assert sc["num_hit"].shape == (2,)
    finally:
        c0.close()


def test_long_filter_head_rows_are_dc_corrected_per_tap(g, setup):
    """A 129-tap channel filter: the decimated rows 1 and 2 still overlap filter()'s zero initial state (64 j < 128), so
    their DC term is mean * (partial tap sum), not mean * sum(coef).  The scanner path (FIR of the raw bytes + DC
    removal on load) must agree with the oracle, which filters (raw - mean) like the reference."""
    coef = g.synth.fir1(128, 200e3 / g.synth.FS)
    caps = [g.synth.make_stream(dongle=80, arfcn=i, num_frames=64, bcch=True, start_frame=s0, frac_start=100.0)[0]
            for i, s0 in enumerate((49, 0, 9))]                       # FCCH early in the capture: the first windows matter
    raw = np.stack(caps)
    out = g.fcch_scan_batch(raw, coef)
    for i in range(len(caps)):
        live = o.scan_capture(caps[i], coef)
        n = out["counts"][i]
        assert live["num_hit"] == out["num_hit"][i] and abs(live["snr"] - out["snr"][i]) < parity.SNR_ATOL
        if live["coarse_pos"][0] != -1.0:
            parity.assert_positions(out["positions"][i, :n], live["coarse_pos"], "positions (129 taps)")
    # and the detector input itself: the first decimated rows of the front end
    fe = g.frontend_batch(raw, coef, 64)
    want = o.matlab_filter(coef, o.raw2iq(raw.T.astype(np.float64)))[0::64]
    assert np.max(np.abs(fe.T[:8] - want[:8])) < 1e-11


# ---- alternative code paths: every variant must give the oracle's answer ---------------------------------
def test_front_end_variants_agree(g, setup, monkeypatch):
    """Register-row front kernel (symmetric / general taps) vs the generic LDS-tap kernel: same calibration."""
    raw = np.stack([g.synth.make_stream(dongle=d, num_frames=102)[0] for d in (30, 31)])
    sym = setup["coef"]                                        # mirrored taps (synth.fir1, as MATLAB's fir1 returns)
    gen = o.fir1(46, 200e3 / g.synth.FS)                       # scipy's firwin: symmetric only to the last ulp
    assert np.array_equal(sym, sym[::-1]) and not np.array_equal(gen, gen[::-1])
    for coef in (sym, gen):
        fast = g.calibrate_batch(raw, coef, setup["ts"], FC)
        det = g.last_batch_details(2)
        for i in range(2):
            parity.compare_stream(o.calibrate_stream(raw[i], coef, setup["ts"], FC), fast["table"][i], det, i, fast["pos_info"][i])
        monkeypatch.setenv("GSMCAL_FRONT_GENERIC", "1")        # read when a context is created
        other = g.Context(0)
        monkeypatch.delenv("GSMCAL_FRONT_GENERIC")
        try:
            slow = g.calibrate_batch(raw, coef, setup["ts"], FC, ctx=other)
        finally:
            other.close()
        assert np.array_equal(fast["table"][:, 6:], slow["table"][:, 6:])           # counts, status
        np.testing.assert_allclose(fast["table"][:, :6], slow["table"][:, :6], rtol=1e-9, atol=1e-12)
        assert all(np.array_equal(a, b) for a, b in zip(fast["pos_info"], slow["pos_info"]))


@pytest.mark.parametrize("env", [{"GSMCAL_CERT": "0"}, {"GSMCAL_PRESCREEN": "0"}, {"GSMCAL_LANES": "4", "GSMCAL_LANE_MIN": "2"},
                                 {"GSMCAL_FUSE_GATHER": "0"}, {"GSMCAL_SNR_FULL": "0"}, {"GSMCAL_SNR_SCREEN_DB": "-300"},
                                 {"GSMCAL_SNR_SCREEN_DB": "30"}, {"GSMCAL_FUSE_POST": "0"}, {"GSMCAL_POST_SLOTS": "2"},
                                 {"GSMCAL_SNR_FULL": "0", "GSMCAL_SNR_INLINE_MIN": "0"}])
def test_fine_search_modes_and_lanes_agree(g, setup, monkeypatch, env):
    """No certificate (every chunk swept), plain all-bin fp64 search, four concurrent lanes, fine windows through k_gather,
    hop walk on its own spectra / on an unscreened SNR table / falling back because the screening level is above every
    threshold, the four launches behind
    the chunk sweep instead of the fused k_post_chain_r (per-stream exchange inside one launch, decision steps replicated in
    every workgroup): identical tables."""
    raw = np.stack([g.synth.make_stream(dongle=d, num_frames=102)[0] for d in range(40, 48)])
    ref = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC)
    for k, v in env.items():
        monkeypatch.setenv(k, v)                               # read when a context is created
    other = g.Context(0)
    try:
        out = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC, ctx=other)
    finally:
        other.close() if hasattr(other, "close") else None
    assert np.array_equal(ref["table"], out["table"], equal_nan=True)
    assert all(np.array_equal(a, b) for a, b in zip(ref["pos_info"], out["pos_info"]))


@pytest.mark.parametrize("stage", [1, 2, 3, 4])
def test_fused_tail_time_out_is_recovered_with_the_four_launch_tail(g, setup, monkeypatch, stage):
    """a fused tail whose workgroups give up waiting for a peer (in production: another PROCESS's fused tail holding
    the slots; here the test hook GSMCAL_TEST_FUSED_STALL -- workgroup (1, 0) never publishes that stage's result -- with the wait
    cut to 50 ms) no longer costs the call.  Host-buffer entry point: the call itself runs again with the four-launch tail and
    returns the reference table.  Device entry point: a caller that synchronises its stream without the library sees
    GSMCAL_E_HIP in the status column of the stalled stream and no other; gsmcal_sync() runs the call again and every row is
    the reference's."""
    import torch
    raw = np.stack([g.synth.make_stream(dongle=d, num_frames=102)[0] for d in range(40, 48)])
    ref = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC)
    monkeypatch.setenv("GSMCAL_TEST_FUSED_STALL", str(stage))
    monkeypatch.setenv("GSMCAL_FUSED_POLL_S", "0.05")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        cx = g.Context(0, stream=st.cuda_stream)
        monkeypatch.delenv("GSMCAL_TEST_FUSED_STALL")
        monkeypatch.delenv("GSMCAL_FUSED_POLL_S")
        try:
            out = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC, ctx=cx)
            assert cx.fused_tail_reruns() == 1
            assert np.array_equal(out["table"], ref["table"], equal_nan=True)
            assert all(np.array_equal(a, b) for a, b in zip(ref["pos_info"], out["pos_info"]))
            raw_t = torch.from_numpy(raw).to(dev)
            tab = torch.zeros((8, g.TABLE_COLS), dtype=torch.float64, device=dev)
            pos = torch.zeros((8, 2, g.MAX_POS_ROWS), dtype=torch.float64, device=dev)
            g.calibrate_batch_dev(raw_t.data_ptr(), 8, raw.shape[1] // 2, setup["coef"], setup["ts"], FC, tab.data_ptr(), pos.data_ptr(), ctx=cx)
            st.synchronize()                                        # (not gsmcal_sync: the time-out shows)
            t = tab.cpu().numpy()
            assert t[0, 9] == -2.0, t[:, 9]                         # GSMCAL_E_HIP in the stalled stream's row ...
            assert np.array_equal(t[1:], ref["table"][1:], equal_nan=True)   # ... and only there
            cx.sync()                                               # the library's synchronisation runs the call again
            assert cx.fused_tail_reruns() == 2
            assert np.array_equal(tab.cpu().numpy(), ref["table"], equal_nan=True)
            pk = pos.cpu().numpy()
            for i in range(8):
                assert np.array_equal(pk[i, :, :int(ref["table"][i, 7])].T, ref["pos_info"][i]), i
            fused, _ = cx.fused_tail_stats()
            assert fused == 2                                       # (the two re-runs took the four-launch tail)
        finally:
            cx.close()


def test_window_snrs_computed_inside_the_scan_kernel_are_the_table_kernels(g, setup, monkeypatch):
    """Throughput batches build no SNR table in HBM: k_coarse_scan<.., INL> computes the moving search's 3 579 window SNRs into
    its LDS copy itself.  Forced here on a small batch (GSMCAL_SNR_FULL=0) and written out on request
    (GSMCAL_SNR_INLINE_KEEP=1): every value bit for bit what k_coarse_snr stores (GSMCAL_SNR_INLINE_MIN=0), the same tables and
    scanner outputs either way -- and without the request gsmcal_last_batch_snr says that nothing was kept."""
    raw = np.stack([g.synth.make_stream(dongle=d, num_frames=64)[0] for d in (30, 31)] +
                   [g.synth.make_stream(dongle=32, num_frames=64, snr_db=6.0)[0], g.synth.make_stream(dongle=33, num_frames=64, bcch=False)[0]])
    coef31 = g.synth.fir1(30, 200e3 / g.synth.FS)
    made = {}
    for name, env in (("kernel", {"GSMCAL_SNR_INLINE_MIN": "0"}), ("inline_kept", {"GSMCAL_SNR_INLINE_KEEP": "1"}), ("inline", {})):
        monkeypatch.setenv("GSMCAL_SNR_FULL", "0")
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        made[name] = g.Context(0)
        for k in list(env) + ["GSMCAL_SNR_FULL"]:
            monkeypatch.delenv(k)
    try:
        outs, tabs = {}, {}
        for name, cx in made.items():
            cal = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC, ctx=cx)
            if name == "inline":
                with pytest.raises(g.GsmcalError, match="kept no SNR table"):
                    g.last_batch_snr(0, ctx=cx)
            else:
                tabs[name] = [g.last_batch_snr(i, ctx=cx) for i in range(len(raw))]
            outs[name] = (cal["table"], g.fcch_scan_batch(raw, coef31, ctx=cx))
        for i in range(len(raw)):
            (ta, na), (tb, nb) = tabs["kernel"][i], tabs["inline_kept"][i]
            assert na == nb == 3579 and len(ta) == len(tb) == 3579
            assert np.array_equal(ta, tb), f"stream {i}: inline window SNRs differ from k_coarse_snr's"
        for name in ("inline_kept", "inline"):
            assert np.array_equal(outs["kernel"][0], outs[name][0], equal_nan=True)
            for k in outs["kernel"][1]:
                assert np.array_equal(np.asarray(outs["kernel"][1][k]), np.asarray(outs[name][1][k]), equal_nan=True), (name, k)
    finally:
        for cx in made.values():
            cx.close()


def test_stream_mode_kernels_agree_to_rounding_and_with_the_oracle_on_unaligned_captures(g, setup, monkeypatch):
    """r_correct from k_stream_tile_s47 (the drivers' 47 symmetric taps: taps in registers, 1000-sample tiles) against the oracle,
    and from the general k_stream_tile (1016-sample tiles; taken for taps that are symmetric only to the last ulp -- scipy's
    firwin -- which also sends k_fine_cert's window build down its taps-in-LDS loop): the rotators exp(1i*k*c) = S*A*B are
    factored per TILE, so the two tilings differ by the rounding of the three ARGUMENTS (up to 2 ulp(k*c) ~ 1e-11 rad at
    k ~ 6e5) -- on captures whose length is odd (streams after the first start off a 16-byte boundary) and is no multiple of
    either tile."""
    raw = np.stack([g.synth.make_stream(dongle=d, num_frames=61)[0][: 2 * 609991] for d in (20, 21, 22)])
    a = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC, want_r=True)
    checked = 0
    for i in range(3):
        L = int(a["r_len"][i])
        if L < 0:
            continue
        orc = o.calibrate_stream(raw[i], setup["coef"], setup["ts"], FC, keep_r=True)
        assert L == len(orc["r_correct"])
        stream_close(a["r_correct"][i, :L], orc["r_correct"])
        checked += 1
    assert checked >= 1
    gen = o.fir1(46, 200e3 / g.synth.FS)                       # not exactly mirrored: must take the general kernel, same answer within rounding
    c = g.calibrate_batch(raw, gen, setup["ts"], FC, want_r=True)
    for i in range(3):
        L = int(c["r_len"][i])
        if L >= 0 and a["r_len"][i] == L:
            stream_close(c["r_correct"][i, :L], a["r_correct"][i, :L])


def test_pipelined_calls_with_the_corrected_stream(g, setup):
    """Calls in flight (gsmcal_ctx_set_pipeline_depth) that also write r_correct: the next call's table chain runs under this call's
    stream kernel.  Six calls three deep over two different raw batches, each into its own output set: table, r_len and every
    sample of r_correct bit for bit what the one-call-at-a-time path wrote."""
    import torch
    dev = torch.device("cuda", 0)
    raws = [np.stack([g.synth.make_stream(dongle=d, num_frames=61)[0] for d in ds]) for ds in ((20, 21, 22), (23, 24, 25))]
    n = raws[0].shape[1] // 2
    refs = [g.calibrate_batch(r_, setup["coef"], setup["ts"], FC, want_r=True) for r_ in raws]
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        cx = g.Context(0, stream=st.cuda_stream)
        try:
            raw_t = [torch.from_numpy(r_).to(dev) for r_ in raws]
            tabs = [torch.zeros((3, g.TABLE_COLS), dtype=torch.float64, device=dev) for _ in range(6)]
            rls = [torch.zeros((3,), dtype=torch.int64, device=dev) for _ in range(6)]
            rcs = [torch.full((3, n, 2), float("nan"), dtype=torch.float64, device=dev) for _ in range(6)]
            cx.set_pipeline_depth(3)
            for k in range(6):
                g.calibrate_batch_dev(raw_t[k & 1].data_ptr(), 3, n, setup["coef"], setup["ts"], FC, tabs[k].data_ptr(), None,
                                      rcs[k].data_ptr(), rls[k].data_ptr(), ctx=cx)
            cx.sync()
            for k in range(6):
                ref = refs[k & 1]
                assert np.array_equal(tabs[k].cpu().numpy(), ref["table"], equal_nan=True), k
                rl = rls[k].cpu().numpy()
                assert np.array_equal(rl, ref["r_len"]), k
                got = rcs[k].cpu().numpy()
                for i in range(3):
                    L = int(rl[i])
                    if L > 0:
                        assert np.array_equal(got[i, :L, 0] + 1j * got[i, :L, 1], ref["r_correct"][i, :L]), (k, i)
        finally:
            cx.close()


def test_unlike_calls_in_flight(g, setup):
    """Calls in flight need not be alike: batch sizes 5 / 2 / 7 / 3, a different carrier frequency (a changed input: the call joins
    the ones in flight before it uploads), a different filter, the depth changed in mid-sequence, a 130-stream call (two lanes: not
    pipelined, runs joined) and scanner sweeps between them -- every call into its own output set, every output bit for bit what the
    same call gives alone on a fresh context."""
    import torch
    dev = torch.device("cuda", 0)
    s = g.synth
    streams = np.stack([s.make_stream(dongle=40 + d, num_frames=61)[0] for d in range(8)])
    n = streams.shape[1] // 2
    caps = np.stack([s.make_stream(dongle=9300, arfcn=i, num_frames=40, bcch=i % 3 != 2)[0] for i in range(12)])
    coef30 = s.fir1(30, 200e3 / s.FS)
    coef_b = s.fir1(46, 180e3 / s.FS)                          # another 47-tap filter: a changed input
    big = np.stack([streams[i % 8] for i in range(130)])
    # (kind, rows, coef, carrier frequency, depth to set before the call)
    plan = [("cal", slice(0, 5), setup["coef"], FC, 4), ("cal", slice(5, 7), setup["coef"], FC, None), ("scan", slice(0, 12), coef30, None, None),
            ("cal", slice(1, 8), setup["coef"], FC, None), ("cal", slice(0, 3), setup["coef"], 1.8e9, None), ("cal", slice(2, 7), coef_b, FC, None),
            ("cal", slice(0, 5), setup["coef"], FC, 2), ("big", None, setup["coef"], FC, None), ("scan", slice(3, 9), coef30, None, 3),
            ("cal", slice(4, 8), setup["coef"], FC, None), ("cal", slice(0, 5), setup["coef"], FC, None)]
    refs = []
    for kind, rows, coef, fc, _ in plan:                       # every call alone, default context
        if kind == "scan":
            r = g.fcch_scan_batch(caps[rows], coef)
            refs.append(np.stack([r["snr"], r["num_hit"]], axis=1))
        else:
            refs.append(g.calibrate_batch(big if kind == "big" else streams[rows], coef, setup["ts"], fc))
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        cx = g.Context(0, stream=st.cuda_stream)
        try:
            keep, outs = [], []
            scratch = torch.zeros((8, g.TABLE_COLS), dtype=torch.float64, device=dev)
            for k_call, (kind, rows, coef, fc, depth) in enumerate(plan):
                if depth:
                    cx.set_pipeline_depth(depth)
                if k_call in (3, 9):                           # refused calls between the others leave the calls in flight alone
                    for bad_ptr, bad_d, bad_n in ((scratch.data_ptr(), 0, n), (scratch.data_ptr(), 4, 0), (0, 4, n)):
                        with pytest.raises(g.GsmcalError):
                            g.calibrate_batch_dev(bad_ptr, bad_d, bad_n, setup["coef"], setup["ts"], FC, scratch.data_ptr(), ctx=cx)
                if kind == "scan":
                    r_t = torch.from_numpy(np.ascontiguousarray(caps[rows])).to(dev)
                    o_t = torch.zeros((r_t.shape[0], 2), dtype=torch.float64, device=dev)
                    st.synchronize()
                    g.fcch_scan_batch_dev(r_t.data_ptr(), r_t.shape[0], caps.shape[1] // 2, coef, o_t.data_ptr(), ctx=cx)
                    outs.append((o_t,))
                else:
                    raw = big if kind == "big" else np.ascontiguousarray(streams[rows])
                    r_t = torch.from_numpy(raw).to(dev)
                    d = raw.shape[0]
                    tab = torch.zeros((d, g.TABLE_COLS), dtype=torch.float64, device=dev)
                    pos = torch.zeros((d, 2, g.MAX_POS_ROWS), dtype=torch.float64, device=dev)
                    rl = torch.zeros((d,), dtype=torch.int64, device=dev)
                    st.synchronize()
                    g.calibrate_batch_dev(r_t.data_ptr(), d, n, coef, setup["ts"], fc, tab.data_ptr(), pos.data_ptr(), None, rl.data_ptr(), ctx=cx)
                    outs.append((tab, pos, rl))
                keep.append(r_t)
            assert cx.pipeline_depth() == 3
            assert 1 <= cx.pipeline_queues() <= 8               # (four on the pool's boxes: the runtime's hardware queues)
            cx.sync()
            for k, ((kind, rows, coef, fc, _), ref, out) in enumerate(zip(plan, refs, outs)):
                if kind == "scan":
                    assert np.array_equal(out[0].cpu().numpy(), ref, equal_nan=True), k
                    continue
                tab, pos, rl = (o.cpu().numpy() for o in out)
                assert np.array_equal(tab, ref["table"], equal_nan=True), (k, kind)
                assert np.array_equal(rl, ref["r_len"]), k
                for i in range(tab.shape[0]):
                    if tab[i, 8] != -1.0:
                        assert np.array_equal(pos[i, :, :int(tab[i, 7])].T, ref["pos_info"][i]), (k, i)
        finally:
            cx.close()


def test_1024_stream_batch_on_staggered_lanes(g, setup):
    """1 024 streams in one call: four lanes of 256 whose front kernels follow one another (the default from 256 streams per lane
    on) -- every copy of a stream gets the row it gets in a batch of its own."""
    distinct = [g.synth.make_stream(dongle=60 + i, num_frames=61)[0] for i in range(8)]
    ref = g.calibrate_batch(np.stack(distinct), setup["coef"], setup["ts"], FC)
    raw = np.stack([distinct[i % 8] for i in range(1024)])
    for _ in range(3):                                         # eager, graph capture, graph replay
        out = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC)
        for i in range(1024):
            assert np.array_equal(out["table"][i], ref["table"][i % 8], equal_nan=True), i
        assert all(np.array_equal(out["pos_info"][i], ref["pos_info"][i % 8]) for i in range(0, 1024, 37))


def _mixed_draw(i, rng):
    """tests/sweep_parity.py's distribution: low SNR, larger ppm, carriers without a BCCH, nothing pre-selected"""
    kw = {}
    if i % 5 == 1:
        kw["snr_db"] = float(rng.uniform(5, 15))
    if i % 7 == 2:
        kw["sampling_ppm"] = float(rng.uniform(-300, 300))
    if i % 11 == 3:
        kw["bcch"] = False
    if i % 13 == 4:
        kw["carrier_ppm"] = float(rng.uniform(-60, 60))
    return kw


@pytest.mark.parametrize("n_streams", [576, 1024])
def test_wide_batch_of_distinct_streams_every_row_against_the_oracle(g, setup, n_streams):
    """the THROUGHPUT code paths (more than 128 streams per lane: k_coarse_scan<INL>, the four-launch tail with
    stream_tail decisions, staggered lanes, graph replay of the forked plan) on DISTINCT streams -- 576 (two lanes of 288) and
    1 024 (four staggered lanes of 256) seeded 61-frame captures drawn like tests/sweep_parity.py (every 5th at 5-15 dB, large
    ppm, carriers without a BCCH, nothing pre-selected), ONE calibrate call, EVERY row through parity.compare_stream; called
    three times (eager, graph capture, graph replay).  gsm_sync_demod.m:112-124 per stream."""
    rng = np.random.default_rng(n_streams)
    first = 400000 + 2000 * (n_streams % 7)
    jobs = [(first + i, 61, _mixed_draw(i, rng)) for i in range(n_streams)]
    raw = np.stack(parity.pool_map(parity.gen_stream_job, jobs, max_workers=128))
    assert len({r.tobytes()[:2048] for r in raw}) == n_streams
    orcs = parity.pool_map(parity.oracle_job_safe, [(raw[i], setup["coef"], setup["ts"], FC) for i in range(n_streams)], max_workers=128)
    n_cal = 0
    first_table = None
    for rep in range(3):
        out = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC)
        det = g.last_batch_details(n_streams)
        if first_table is None:
            first_table = out["table"].copy()
        else:
            assert np.array_equal(first_table, out["table"], equal_nan=True), f"call {rep} differs from the first"
        for i in range(n_streams):
            orc, err = orcs[i]
            if orc is None:
                assert out["table"][i, 9] < 0, f"stream {i}: the oracle raised '{err}', gpu status {out['table'][i, 9]}"
                continue
            parity.compare_stream(orc, out["table"][i], det, i, out["pos_info"][i])
            n_cal += rep == 0 and out["table"][i, 9] == 0
    assert n_cal > n_streams // 2, "most of the mixed draw should calibrate"


@pytest.mark.parametrize("forced_graphs", [False, True, "pipelined"])
def test_two_contexts_and_a_cu_hog_share_the_gpu(g, setup, monkeypatch, forced_graphs):
    """the fused tail (k_post_chain_r: workgroups exchange results INSIDE one launch) with other tenants on the
    GPU.  Two contexts on two streams, 200 64-stream steps each, enqueued from two host threads, while a third context keeps
    the CUs busy with 1 600-capture scanner batches: every table identical to the single-context reference, no negative
    status, bounded wall time; and the library never had two fused tails in flight at once (the later caller of an overlapping
    pair took the four-launch tail: gsmcal_fused_tail_stats).  forced_graphs: the same with GSMCAL_GRAPH=2 -- every call replayed
    from a captured graph whose fused tail passes the gate at each replay (a busy gate sends that call through eager launches).
    "pipelined" (round 6): both contexts at gsmcal_ctx_set_pipeline_depth(4) -- four calls in flight inside EACH context, on its
    internal streams, into four output sets in turn."""
    pipelined = forced_graphs == "pipelined"
    forced_graphs = forced_graphs is True
    import threading
    import time
    distinct = np.stack([g.synth.make_stream(dongle=8200 + d, num_frames=61)[0] for d in range(8)])
    raw = np.tile(distinct, (8, 1))
    ref = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC)
    assert np.all(ref["table"][:, 9] >= 0)
    n = raw.shape[1] // 2
    caps = np.stack([g.synth.make_stream(dongle=8300, arfcn=i, num_frames=26, bcch=i % 3 != 2)[0] for i in range(8)])
    if forced_graphs:
        monkeypatch.setenv("GSMCAL_GRAPH", "2")              # read when a context is created
    ctxs = [g.Context(0) for _ in range(3)]
    monkeypatch.delenv("GSMCAL_GRAPH", raising=False)
    stop = threading.Event()
    errs, tables = [], {}

    def calib(k):
        try:
            cx = ctxs[k]
            d_raw = cx.alloc(raw.nbytes)
            d_tab = [cx.alloc(64 * g.TABLE_COLS * 8) for _ in range(4)]
            d_pos = [cx.alloc(64 * 2 * g.MAX_POS_ROWS * 8) for _ in range(4)]
            cx.h2d(d_raw, raw)
            cx.sync()
            if pipelined:
                cx.set_pipeline_depth(4)
            got = []
            for step in range(200):
                b = step & 3 if pipelined else 0
                g.calibrate_batch_dev(d_raw, 64, n, setup["coef"], setup["ts"], FC, d_tab[b], d_pos[b], ctx=cx)
                if step % 20 == 19:                                   # twenty steps in flight, then look
                    cx.sync()
                    for bb in ((0, 1, 2, 3) if pipelined else (0,)):
                        t = np.empty((64, g.TABLE_COLS))
                        cx.d2h(t, d_tab[bb])
                        if bb == 0:
                            got.append(t)
                        else:
                            assert np.array_equal(t, got[-1], equal_nan=True)
            tables[k] = got
            for p_ in [d_raw] + d_tab + d_pos:
                cx.free(p_)
        except Exception as e:  # noqa: BLE001
            errs.append((k, repr(e)))

    def hog():
        try:
            cx = ctxs[2]
            big = np.tile(caps, (200, 1))
            while not stop.is_set():
                g.fcch_scan_batch(big, setup["coef30"], ctx=cx)
        except Exception as e:  # noqa: BLE001
            errs.append(("hog", repr(e)))

    th = threading.Thread(target=hog)
    th.start()
    t0 = time.time()
    workers = [threading.Thread(target=calib, args=(k,)) for k in range(2)]
    for w_ in workers:
        w_.start()
    for w_ in workers:
        w_.join(timeout=300)
    wall = time.time() - t0
    stop.set()
    th.join(timeout=120)
    stats = [cx.fused_tail_stats() for cx in ctxs[:2]]
    for cx in ctxs:
        cx.close()
    assert not errs, errs
    assert not any(w_.is_alive() for w_ in workers) and wall < 120.0, f"two contexts beside a CU hog took {wall:.1f} s"
    for k in range(2):
        assert len(tables[k]) == 10
        for t in tables[k]:
            assert np.array_equal(t, ref["table"], equal_nan=True), f"context {k}: table differs from the single-context reference"
            assert np.all(t[:, 9] >= 0)
    fused, fell = sum(s_[0] for s_ in stats), sum(s_[1] for s_ in stats)
    if pipelined:
        assert fused == 0 and fell == 0, stats           # (side-by-side calls take the four-launch tail: the gate is never asked)
    else:
        assert fused + fell == 400 and fused >= 1, stats
    print(f"two contexts + hog: {wall:.2f} s, fused launches {stats[0][0]} + {stats[1][0]}, gate fall-backs {stats[0][1]} + {stats[1][1]}")


def test_large_batches_take_the_throughput_paths(g, setup):
    """More than 512 units: no speculative hop walk, SNR table from its own kernel, four workgroups per CU in the
    coarse scan, two lanes in the calibration chain -- same answers."""
    distinct = [g.synth.make_stream(dongle=60 + i, num_frames=61)[0] for i in range(4)]
    raw = np.stack([distinct[i % 4] for i in range(520)])
    out = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC)
    det = g.last_batch_details(4)
    for i in range(4):
        orc = o.calibrate_stream(distinct[i], setup["coef"], setup["ts"], FC)
        parity.compare_stream(orc, out["table"][i], det, i, out["pos_info"][i])
    for i in range(4, 520):                                  # every copy of a stream gives the same row
        assert np.array_equal(out["table"][i], out["table"][i % 4], equal_nan=True)
    caps = [g.synth.make_stream(dongle=70, arfcn=i, num_frames=40, bcch=(i != 2))[0] for i in range(3)]
    raw = np.stack([caps[i % 3] for i in range(600)])
    sc = g.fcch_scan_batch(raw, setup["coef30"])
    for i in range(3):
        live = o.scan_capture(caps[i], setup["coef30"])
        assert live["num_hit"] == sc["num_hit"][i] and abs(live["snr"] - sc["snr"][i]) < parity.SNR_ATOL
    assert np.array_equal(sc["num_hit"][3:], np.tile(sc["num_hit"][:3], 200)[3:])
    assert np.array_equal(sc["snr"][3:], np.tile(sc["snr"][:3], 200)[3:])


# ---- the BASELINE batch shape itself against the oracle ----------------------------------------------------
def test_baseline_batch_64_distinct_streams_every_row_against_the_oracle(g, setup):
    """BASELINE config 4 on one GPU as bench.py runs it: 64 DISTINCT streams x 1 020 000 samples -- the first
    64 seeds of rank 0's range that the chain calibrates (bench.py's selection, so every stream does the full work) -- in ONE
    calibrate call, and EVERY row against the oracle: positions bit for bit, ppm within 1e-6."""
    ncand = 64 + 64 // 3 + 8
    cands = parity.pool_map(parity.gen_stream_job, [(100000 + i, 102, {}) for i in range(ncand)])
    picked, lo = [], 0
    while len(picked) < 64:
        assert lo < len(cands), "bench.py's candidate range no longer holds 64 calibratable seeds"
        res = g.calibrate_batch(np.stack(cands[lo: lo + 64]), setup["coef"], setup["ts"], FC)
        picked += [cands[lo + i] for i in range(len(res["table"])) if res["table"][i, 9] == 0]
        lo += 64
    raw = np.stack(picked[:64])
    assert len({r.tobytes()[:4096] for r in raw}) == 64
    out = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC)
    det = g.last_batch_details(64)
    assert np.all(out["table"][:, 9] == 0)
    orcs = parity.pool_map(parity.oracle_job, [(raw[i], setup["coef"], setup["ts"], FC) for i in range(64)])
    for i in range(64):
        parity.compare_stream(orcs[i], out["table"][i], det, i, out["pos_info"][i])
    # ... and the same batch through CALLS IN FLIGHT (gsmcal_ctx_set_pipeline_depth): eight consecutive
    # gsmcal_calibrate_batch_dev calls two to eight deep -- whole calls side by side, each with the four-launch tail -- each into its
    # own output set: every table, pos_info and r_len bit for bit what the one-call-at-a-time path (fused tail) returned, and
    # last_batch_details describes the last call
    import torch
    dev = torch.device("cuda", 0)
    raw_t = torch.from_numpy(raw).to(dev)
    n = raw.shape[1] // 2
    for depth in (2, 4, 3, 8, 5):
        st = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(st):
            cx = g.Context(0, stream=st.cuda_stream)
            try:
                cx.set_pipeline_depth(depth)
                assert cx.pipeline_depth() == depth
                tabs = [torch.zeros((64, g.TABLE_COLS), dtype=torch.float64, device=dev) for _ in range(8)]
                poss = [torch.zeros((64, 2, g.MAX_POS_ROWS), dtype=torch.float64, device=dev) for _ in range(8)]
                rls = [torch.zeros((64,), dtype=torch.int64, device=dev) for _ in range(8)]
                for k in range(8):
                    g.calibrate_batch_dev(raw_t.data_ptr(), 64, n, setup["coef"], setup["ts"], FC, tabs[k].data_ptr(), poss[k].data_ptr(),
                                          None, rls[k].data_ptr(), ctx=cx)
                det_p = g.last_batch_details(64, ctx=cx)           # (joins the calls in flight)
                cx.sync()
                for k in range(8):
                    assert np.array_equal(tabs[k].cpu().numpy(), out["table"], equal_nan=True), (depth, k)
                    pk = poss[k].cpu().numpy()
                    for i in range(64):
                        rows = int(out["table"][i, 7])
                        assert np.array_equal(pk[i, :, :rows].T, out["pos_info"][i]), (depth, k, i)
                    assert np.array_equal(rls[k].cpu().numpy(), rls[0].cpu().numpy())
                for key in det:
                    if key == "coarse_snr":
                        # (calls in flight walk the hops on their own spectra instead of the full SNR table: the hits' SNRs -- an
                        # intermediate, compared with the oracle at the same bar elsewhere -- agree to rounding, everything else bit for bit)
                        assert np.allclose(det_p[key], det[key], rtol=0.0, atol=parity.SNR_ATOL, equal_nan=True), key
                    else:
                        assert np.array_equal(np.asarray(det_p[key]), np.asarray(det[key]), equal_nan=True), key
                fused, fell = cx.fused_tail_stats()
                assert fused == 0 and fell == 0                    # (calls in flight never take the fused tail)
                # depth back to 1 mid-way: joins, then behaves as ever (fused tail again)
                cx.set_pipeline_depth(1)
                g.calibrate_batch_dev(raw_t.data_ptr(), 64, n, setup["coef"], setup["ts"], FC, tabs[0].data_ptr(), ctx=cx)
                cx.sync()
                assert np.array_equal(tabs[0].cpu().numpy(), out["table"], equal_nan=True)
                assert cx.fused_tail_stats()[0] == 1
            finally:
                cx.close()


# ---- full BASELINE size: size-independent properties ---------------------------------------------------
def test_full_size_batch_properties(g, setup):
    """64 streams x 1 020 000 samples (BASELINE config 4 on one GPU): (1) every stream's row equals the
    row it gets in a batch of its own (units are independent); (2) two runs are bit-identical;
    (3) ppm-table mode == stream-output mode; (4) 'test on line' (FCCH_fine_correction.m:167-183):
    re-estimating the tone on the corrected stream gives ~zero residual carrier error."""
    distinct = np.stack([g.synth.make_stream(dongle=30 + d)[0] for d in range(8)])
    raw = np.tile(distinct, (8, 1))
    perm = np.random.default_rng(1).permutation(64)
    raw = raw[perm]
    a = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC)
    b = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC)
    assert np.array_equal(a["table"], b["table"], equal_nan=True)
    singles = g.calibrate_batch(distinct, setup["coef"], setup["ts"], FC, want_r=True)
    for i in range(64):
        assert np.array_equal(a["table"][i], singles["table"][perm[i] % 8], equal_nan=True)
    ok = [i for i in range(8) if singles["table"][i, 9] == 0]
    assert ok, "seeded set must contain calibratable streams"
    for i in ok:
        L = int(singles["r_len"][i])
        r = singles["r_correct"][i, :L]
        pi = singles["pos_info"][i]
        r_again, resid = g.carrier_correct_post_SCH(r, pi, 8, FC)
        assert abs(resid) < 1e-6, f"residual carrier ppm after correction: {resid}"
        # and the oracle agrees on one of them (cheap: windows only)
    orc = o.calibrate_stream(distinct[ok[0]], setup["coef"], setup["ts"], FC)
    parity.assert_ppm(singles["table"][ok[0], 4], orc["total_sampling_ppm"], "total sampling ppm")
    parity.assert_ppm(singles["table"][ok[0], 5], orc["total_carrier_ppm"], "total carrier ppm")


def test_randomised_sweep_against_oracle(g, setup):
    """48 seeded streams with a widened distribution (low SNR, large sampling error, non-BCCH carriers): every
    position bit-exact, ppm within 1e-6 (tests/sweep_parity.py runs the same comparison on hundreds of streams)."""
    rng = np.random.default_rng(77)
    n = 48
    kws = []
    for i in range(n):
        kw = {}
        if i % 5 == 1:
            kw["snr_db"] = float(rng.uniform(5, 15))
        if i % 7 == 2:
            kw["sampling_ppm"] = float(rng.uniform(-300, 300))
        if i % 11 == 3:
            kw["bcch"] = False
        kws.append(kw)
    raw = np.stack([g.synth.make_stream(dongle=700 + i, **kws[i])[0] for i in range(n)])
    out = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC)
    det = g.last_batch_details(n)
    calibrated = 0
    for i in range(n):
        orc = o.calibrate_stream(raw[i], setup["coef"], setup["ts"], FC)
        parity.compare_stream(orc, out["table"][i], det, i, out["pos_info"][i])
        calibrated += out["table"][i, 9] == 0
    assert calibrated >= n // 2


def test_native_allgather_of_the_table_single_rank(g, ctx, setup, tmp_path):
    """gsmcal_allgather_table (RCCL through the C ABI, no PyTorch): with one rank the gathered table is the local one;
    both bootstraps (id handed over, id through a file) are exercised.  The multi-rank layout is covered on CPU by
    tests/test_dist_cpu.py (gloo) -- the driver takes the real 8-GPU curve."""
    from gsmcal import dist as gd
    rows, cols = 5, g.TABLE_COLS
    local = np.arange(rows * cols, dtype=np.float64).reshape(rows, cols) + 0.25
    d_loc, d_all = ctx.alloc(local.nbytes), ctx.alloc(local.nbytes)
    try:
        ctx.h2d(d_loc, local)
        for kw in ({"unique_id": gd.NativeComm.unique_id(ctx)}, {"id_file": tmp_path / "gsmcal_id"}):
            comm = gd.NativeComm(ctx, 1, 0, **kw)
            try:
                comm.allgather_table(d_loc, rows, cols, d_all)
                ctx.sync()
                got = np.zeros_like(local)
                ctx.d2h(got, d_all)
                assert np.array_equal(got, local)
            finally:
                comm.close()
    finally:
        ctx.free(d_loc); ctx.free(d_all)


@pytest.mark.parametrize("mode", ["inline", "async"])
def test_native_table_gatherer_single_rank(g, ctx, setup, mode):
    """bench.py's N > 1 exchange step on the C ABI's own collective (gsmcal.dist.NativeTableGatherer): the all-gather in line
    on the context's stream, and on the library's side stream behind an event (gsmcal_allgather_table_async /
    gsmcal_allgather_wait) -- two buffer pairs alternating over several steps of a real calibration, the gathered table equal to
    the local one every time (one rank; the multi-rank layout is covered under gloo on CPU and by tests/multigpu_check.py)."""
    import torch
    from gsmcal import dist as gd
    raw = np.stack([g.synth.make_stream(dongle=d, num_frames=61)[0] for d in (20, 21, 22)])
    ref = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC)["table"]
    dev = torch.device("cuda", 0)
    raw_t = torch.from_numpy(raw).to(dev)
    tabs = [torch.zeros((3, g.TABLE_COLS), dtype=torch.float64, device=dev) for _ in range(2)]
    comm = gd.NativeComm(ctx, 1, 0, unique_id=gd.NativeComm.unique_id(ctx))
    try:
        tg = gd.NativeTableGatherer(ctx, comm, [3], g.TABLE_COLS, dev, mode=mode)
        torch.cuda.synchronize()
        for step in range(5):
            b = step & 1
            tg.wait(b)
            tabs[b].zero_()
            torch.cuda.synchronize()
            g.calibrate_batch_dev(raw_t.data_ptr(), 3, raw.shape[1] // 2, setup["coef"], setup["ts"], np.full(3, FC), tabs[b].data_ptr(), ctx=ctx)
            tg.post(b, tabs[b])
        for b in range(2):
            rows = tg.rows(b)
            ctx.sync()
            if mode == "async":
                ctx.check(ctx.lib.gsmcal_allgather_sync(ctx.h, b), "gsmcal_allgather_sync")
            assert np.array_equal(rows.cpu().numpy(), ref, equal_nan=True)
            assert np.array_equal(tg.own_rows(b).cpu().numpy(), ref, equal_nan=True)
    finally:
        torch.cuda.synchronize()
        comm.close()


def test_SCH_equalise_front_end_of_the_demodulator(g, setup):
    """SURVEY 8f-4, SCH_demod.m:53-59,79-90: equalised SCH bursts (three 1552-point transforms and two spectral divisions per
    burst) from a really calibrated stream, against the oracle; plus the reference's early exit and index error."""
    raw = np.stack([g.synth.make_stream(dongle=d)[0] for d in (0, 3)])
    out = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC, want_r=True)
    done = 0
    for i in range(2):
        if out["table"][i, 9] != 0:
            continue
        L = int(out["r_len"][i])
        r = out["r_correct"][i, :L]
        pi = out["pos_info"][i]
        want = o.SCH_equalise(r, pi, setup["ts"], 8)
        got = g.SCH_equalise(r, pi, setup["ts"], 8)
        assert got.shape == want.shape == (int(np.sum(pi[:, 1] == 1)), 1552)
        assert np.max(np.abs(got - want)) <= 1e-10 * np.max(np.abs(want))
        done += 1
        # index error where MATLAB's s(sp:ep) would run past the stream
        with pytest.raises(g.GsmcalError):
            g.SCH_equalise(r[: int(pi[pi[:, 1] == 1, 0][-1]) + 100], pi, setup["ts"], 8)
    assert done >= 1
    assert g.SCH_equalise(-1.0, np.array([[-1.0, -1.0]]), setup["ts"], 8) is None and \
        o.SCH_equalise(-1.0, np.array([[-1.0, -1.0]]), setup["ts"], 8) is None
    # other oversampling ratio: 776 = 97 x 8 points
    r4 = np.ascontiguousarray(out["r_correct"][0, : int(out["r_len"][0]) : 2]) if out["table"][0, 9] == 0 else None
    if r4 is not None:
        pi4 = out["pos_info"][0].copy()
        pi4[:, 0] = np.floor((pi4[:, 0] - 1) / 2) + 1
        ts4 = np.ascontiguousarray(setup["ts"][0::2])
        want = o.SCH_equalise(r4, pi4, ts4, 4)
        got = g.SCH_equalise(r4, pi4, ts4, 4)
        assert got.shape == want.shape and np.max(np.abs(got - want)) <= 1e-10 * np.max(np.abs(want))


def test_inter_dongle_phase_difference_from_gathered_pos_info(g, setup):
    """SURVEY 8f-2, gsm_sync_demod.m:130-134,151-158: two dongles hear the same transmission through their own clocks;
    the burst map and the sampling-phase difference are computed from the pos_info tables the GPU chain produced, and
    compared with the oracle's restatement evaluated on the oracle's own tables."""
    from gsmcal import dist as gd
    tried = 0
    for key in range(40, 60):
        raw = np.stack([g.synth.make_stream(dongle=900 + key * 2 + j, tx_key=key)[0] for j in range(2)])
        out = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC)
        if np.any(out["table"][:, 9] != 0):
            continue                                               # a stream the reference algorithm rejects: next pair
        tried += 1
        orc = [o.calibrate_stream(raw[j], setup["coef"], setup["ts"], FC) for j in range(2)]
        for j in range(2):
            parity.assert_positions(out["pos_info"][j], orc[j]["pos_info"], f"pos_info dongle {j}")
            assert np.array_equal(gd.burst_map(out["pos_info"][j]), o.burst_map(orc[j]["pos_info"]), equal_nan=True)
        x, dphi = o.sampling_phase_difference(orc[0]["pos_info"], orc[1]["pos_info"])
        assert np.array_equal(gd.sampling_phase_difference(out["pos_info"][0], out["pos_info"][1]), dphi)
        assert np.array_equal(gd.sampling_phase_frames(out["pos_info"][0], out["pos_info"][1]), x)
        # same transmission: every compared burst is the same burst, so the difference is constant to within the
        # +-1 sample of the two independent position estimates
        assert np.max(dphi) - np.min(dphi) <= 2
        if tried == 2:
            break
    assert tried >= 1


def test_fine_search_against_rocfft_spectra(g, setup):
    """A third evaluation of FCCH_fine_correction.m:48-52, test-only: every one of the 1025 x 1184-point spectra of a hit by
    rocFFT (torch.fft on the GPU), max over bins, first max over window starts -- against the first-round positions of
    the HIP path's certificate / sweep / verify scheme (and the oracle's pocketfft).  No library FFT is on the product path."""
    import torch
    raw = np.stack([g.synth.make_stream(dongle=d)[0] for d in (0, 1, 4)])
    g.calibrate_batch(raw, setup["coef"], setup["ts"], FC)
    det = g.last_batch_details(len(raw))
    r_all = g.frontend_batch(raw, setup["coef"], 1)                   # filter(coef,1,raw2iq(s)), every row (GPU, exact order)
    dev = torch.device("cuda", 0)
    for i in range(len(raw)):
        nfine = det["counts"][i, 1]
        assert nfine >= 5
        r = torch.from_numpy(r_all[i]).to(dev)
        for w in range(nfine):
            cp = int(det["coarse_pos"][i, w])
            sp = (cp - 64 - 1) * 8 + 1                               # :40,43 (1-based)
            seg = r[sp - 1: sp - 1 + 1024 + 1184]
            win = seg.unfold(0, 1184, 1)                             # (1025, 1184): window k = s(sp+k : sp+k+1183)
            p = torch.fft.fft(win, dim=1).abs().square().amax(dim=1)
            k = int(torch.argmax(p))                                 # torch.argmax: first maximum is not guaranteed ...
            k = int((p == p[k]).nonzero()[0])                        # ... so take the first index holding it
            assert det["fine_first"][i, w] == sp + k, f"stream {i} hit {w}: rocFFT says {sp + k}, HIP path {det['fine_first'][i, w]}"


def test_params_pod_changes_decisions_and_rejects_geometry(g, setup):
    """gsmcal_params: the thresholds the reference hard-codes.  An impossible SNR gate turns every calibrated stream into
    the :192-196 sentinel and the default brings the first table back; a geometry field is refused.  (Every threshold moved
    against the oracle, the scanner's rule and the rest of set_params' contract: tests/test_gpu_params.py.)"""
    raw = np.stack([g.synth.make_stream(dongle=d)[0] for d in (0, 3)])
    c2 = g.Context(0)
    try:
        ref = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC, ctx=c2)
        assert np.any(ref["table"][:, 9] == 0)
        c2.set_params(fine_gate_snr_db=200.0)
        out = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC, ctx=c2)
        for i in range(2):
            if ref["table"][i, 9] == 0:
                assert out["table"][i, 9] == 6 and out["table"][i, 6] == 1          # GSMCAL_S_FINE_LOW_SNR, FCCH_pos = -1
                parity.assert_ppm(out["table"][i, 0], ref["table"][i, 0], "sampling ppm is set before the gate")
        c2.set_params(fine_gate_snr_db=5.0)
        back = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC, ctx=c2)
        assert np.array_equal(back["table"], ref["table"], equal_nan=True)
        with pytest.raises(g.GsmcalError):
            c2.set_params(fine_max_offset=32)
        assert c2.get_params().fine_max_offset == 64
    finally:
        c2.close()


def test_outputs_in_pinned_host_memory(g, ctx, setup):
    """include/gsmcal.h: the d_* outputs of the *_dev entry points may be pinned host memory -- the kernels that finish
    the batch store the rows there, no copy is queued.  Same table and (snr, num_hit) as through device buffers."""
    import ctypes as C
    import torch
    dp = g._lib.c_double_p
    raw = np.stack([g.synth.make_stream(dongle=d, num_frames=102)[0] for d in (90, 91, 92)])
    D, N = raw.shape[0], raw.shape[1] // 2
    raw_t = torch.from_numpy(raw).cuda()
    coef, ts, cf = setup["coef"], setup["ts"], np.full(D, FC)
    ref = g.calibrate_batch(raw, coef, ts, FC, ctx=ctx)
    for _ in range(3):                       # the repeated call replays a graph: the host pointer is part of it
        host = torch.full((D, g.TABLE_COLS), -7.0, dtype=torch.float64).pin_memory()
        rc = ctx.lib.gsmcal_calibrate_batch_dev(ctx.h, C.c_void_p(raw_t.data_ptr()), D, N, coef.ctypes.data_as(dp), len(coef),
                                                ts.ctypes.data_as(dp), len(ts), cf.ctypes.data_as(dp),
                                                C.c_void_p(host.data_ptr()), None, None, None)
        ctx.check(rc, "gsmcal_calibrate_batch_dev")
        ctx.sync()
        assert np.array_equal(host.numpy(), ref["table"], equal_nan=True)
    caps = np.stack([g.synth.make_stream(dongle=93, arfcn=i, num_frames=40, bcch=(i != 1))[0] for i in range(3)])
    sc = g.fcch_scan_batch(caps, setup["coef30"], ctx=ctx)
    caps_t = torch.from_numpy(caps).cuda()
    out = torch.full((3, 2), -7.0, dtype=torch.float64).pin_memory()
    rc = ctx.lib.gsmcal_fcch_scan_batch_dev(ctx.h, C.c_void_p(caps_t.data_ptr()), 3, caps.shape[1] // 2,
                                            setup["coef30"].ctypes.data_as(dp), len(setup["coef30"]),
                                            C.c_void_p(out.data_ptr()), None, None, None)
    ctx.check(rc, "gsmcal_fcch_scan_batch_dev")
    ctx.sync()
    assert np.array_equal(out.numpy()[:, 0], sc["snr"]) and np.array_equal(out.numpy()[:, 1], sc["num_hit"])


def test_multi_lane_graph_replay_of_a_256_stream_batch(g, ctx, setup):
    """VERDICT r2 (missing 6): 256 streams = four lanes (four HIP streams forked off the context's); the second identical
    gsmcal_calibrate_batch_dev call captures the whole fork/join plan into a hipGraph, the third replays it.  Every call
    must give the oracle's rows (8 distinct streams tiled, unselected: calibrating and rejected ones)."""
    import ctypes as C
    import torch
    dp = g._lib.c_double_p
    distinct = [g.synth.make_stream(dongle=300 + i, num_frames=102)[0] for i in range(8)]
    D = 256
    raw = np.stack([distinct[i % 8] for i in range(D)])
    N = raw.shape[1] // 2
    raw_t = torch.from_numpy(raw).cuda()
    coef, ts, cf = setup["coef"], setup["ts"], np.full(D, FC)
    table_t = torch.zeros((D, g.TABLE_COLS), dtype=torch.float64, device="cuda")
    pos_t = torch.zeros((D, 2, g.MAX_POS_ROWS), dtype=torch.float64, device="cuda")
    orc = [o.calibrate_stream(distinct[i], coef, ts, FC) for i in range(8)]
    for call in range(3):
        table_t.fill_(-7.0)
        pos_t.fill_(-7.0)
        torch.cuda.synchronize()
        rc = ctx.lib.gsmcal_calibrate_batch_dev(ctx.h, C.c_void_p(raw_t.data_ptr()), D, N, coef.ctypes.data_as(dp), len(coef),
                                                ts.ctypes.data_as(dp), len(ts), cf.ctypes.data_as(dp),
                                                C.c_void_p(table_t.data_ptr()), C.c_void_p(pos_t.data_ptr()), None, None)
        ctx.check(rc, "gsmcal_calibrate_batch_dev")
        ctx.sync()
        table, pos = table_t.cpu().numpy(), pos_t.cpu().numpy()
        det = g.last_batch_details(8, ctx=ctx)
        for i in range(8):
            k = int(table[i, 7])
            pi = -np.ones((k, 2)) if table[i, 8] == -1.0 else np.ascontiguousarray(pos[i, :, :k].T)
            parity.compare_stream(orc[i], table[i], det, i, pi)
        for i in range(8, D):                                # every copy of a stream, whichever lane it ran on
            assert np.array_equal(table[i], table[i % 8], equal_nan=True), f"call {call}, stream {i}"
            assert np.array_equal(pos[i], pos[i % 8]), f"call {call}, stream {i}"


def test_gsmcal_before_torch_in_one_process():
    """Two HIP runtimes cannot share a process: libgsmcal.so loaded first used to map the system libamdhip64 and a later
    `import torch` (which bundles its own) then found "No HIP GPUs" -- whether a test passed depended on which module had
    been imported first.  _lib.load() now maps the PyTorch wheel's runtime first when one is installed; checked in a fresh
    process, gsmcal first, then torch on the same GPU."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), "tools", "order_check.py"), "gsmcal_first"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch cuda ok" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("libamdhip64") == 1, r.stdout          # one HIP runtime mapped


def test_snr_values_of_the_decision_path_sit_far_inside_the_certificate_margin(g, setup):
    """VERDICT r2 (weak 2): the batch front end filters the RAW bytes (integer tap-pair sums) and removes the DC term when a
    decimated sample is loaded -- not the reference's operation order -- and these SNR values feed the decisions
    `snr - avg > th`.  Measured here instead of argued: every window SNR the coarse detector built for a batch (the 3 579
    moving-search windows of each stream, and the later windows the hop walk looks up where they were computed) against
    the oracle's value for the reference's order.  The certified scan decides only outside 1e-6 dB of the threshold and
    replays the reference's serial loop inside it, so implementation noise below ~1e-7 dB cannot change a decision that the
    exact replay would not also take."""
    dongles = [0, 3, 41, 42]
    raw = np.stack([g.synth.make_stream(dongle=d)[0] for d in dongles] +
                   [g.synth.make_stream(dongle=43, snr_db=7.0)[0], g.synth.make_stream(dongle=44, bcch=False)[0]])
    g.calibrate_batch(raw, setup["coef"], setup["ts"], FC)
    worst = 0.0
    for i in range(len(raw)):
        tab, n_mov = g.last_batch_snr(i)
        r = o.matlab_filter(setup["coef"], o.raw2iq(raw[i].astype(np.float64)))
        s = r[0::64]
        assert n_mov == 3579 and len(tab) == len(s) - 15        # ceil(23*1250/8) - 15 windows; latency path: the whole stream
        want = o._window_snr(o._power_spectra(s, 1, len(s) - 15, 16))
        got = tab[: len(want)]
        assert np.all(np.isfinite(got[:n_mov]))                  # the moving search's windows are all computed
        computed = np.isfinite(got)
        d = np.abs(got[computed] - want[computed])
        worst = max(worst, float(np.max(d)))
        # windows ruled out without a spectrum (-inf) must indeed lie below the screening level (5 dB)
        assert np.all(want[~computed] < 5.0)
        assert np.mean(~computed[n_mov:]) > 0.5                  # and most later windows are
    assert worst < 1e-10, f"largest SNR difference {worst:.3e} dB"  # measured: <= 1.6e-12 dB (median 1.5e-15), six orders inside the 1e-6 dB margin


def test_per_stream_carrier_frequencies_in_one_batch(g, setup):
    """carrier_freq is an argument of FCCH_fine_correction / carrier_correct_post_SCH (gsm_sync_demod.m:14 passes the tuned
    frequency): dongles of one batch may sit on different ARFCNs.  Each stream's carrier ppm must be computed with ITS
    frequency -- in the fused tail (<= 64 streams on one lane) and in the multi-lane plan (130 streams: two lanes, the second
    one starting in the middle of the frequency array)."""
    fcs = np.array([935.2e6, 947.6e6, 957.4e6, 959.8e6])
    distinct = [g.synth.make_stream(dongle=600 + i, carrier_freq=fcs[i])[0] for i in range(4)]
    orc = [o.calibrate_stream(distinct[i], setup["coef"], setup["ts"], fcs[i]) for i in range(4)]
    assert sum(np.isfinite(x["total_carrier_ppm"]) for x in orc) >= 2
    for D in (4, 130):
        raw = np.stack([distinct[i % 4] for i in range(D)])
        cf = np.array([fcs[i % 4] for i in range(D)])
        out = g.calibrate_batch(raw, setup["coef"], setup["ts"], cf)
        det = g.last_batch_details(min(D, 8))
        for i in range(min(D, 8)):
            parity.compare_stream(orc[i % 4], out["table"][i], det, i, out["pos_info"][i])
        for i in range(D):
            assert np.array_equal(out["table"][i], out["table"][i % 4], equal_nan=True), (D, i)
