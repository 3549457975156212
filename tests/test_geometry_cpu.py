"""CPU tests (no GPU) of the geometry cases (tests/geometry_cases.py): both oracles -- the vectorised restatement and the
literal one, which share no helper -- agree on every case, and the premises tests/test_gpu_geometry.py relies on hold, so
that a mismatch there is a bug of the library and not a tie:
  (a) every coarse case with dr <= 37 has at least two hits on one of the two captures (the hop walk runs), the two ratios
      whose +11-frame distance lands on .5 take a +11-frame hop, and the carrier without a BCCH is the sentinel;
  (b) every decision `snr - avg > th` the reference takes on a coarse or detector case -- every window up to the deciding one,
      every hop candidate -- is further than 1e-6 dB (the certificate margin of k_coarse_scan) from its threshold; a case inside
      it is dropped, and at most one in ten of a grid may be;
  (c) at each oversampling ratio the chain takes the exit geometry_cases.CHAIN_EXIT records, and the capture with the sampling
      error makes both resampling stages work (sampling_ppm != 0 behind each);
  (d) the .5 ratios round half away from zero: d0 = 1563 at dr = 8, d1 = 3438 at dr = 4.
Bars between the oracles: positions, flags and indices exact; SNRs and ppm by tests/parity.py; streams 2e-8 of their peak."""
import math

import numpy as np
import pytest

import geometry_cases as gc
import parity
from oracle import gsmcal_oracle as o
from oracle import gsmcal_oracle_literal as lit

STREAM_RTOL = 2e-8


def snr_close(a, b):
    return (a == b) or (math.isnan(a) and math.isnan(b)) or abs(a - b) <= parity.SNR_ATOL


# ---- coarse stage -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def captures():
    return gc.coarse_captures()


@pytest.fixture(scope="module")
def coarse_results(captures):
    """(capture, dr) -> (position, snr) of the first oracle"""
    return {(name, dr): o.FCCH_coarse_position(gc.coarse_cut(r8, dr), dr) for name, r8 in captures.items() for dr in gc.COARSE_DRS}


def test_d_half_ratios_round_away_from_zero():
    assert gc.coarse_geometry(8)["d0"] == 1563 and gc.coarse_geometry(4)["d1"] == 3438
    assert gc.coarse_geometry(40)["d0"] == 313 and gc.coarse_geometry(20)["d1"] == 688
    for dr in gc.HALF_D0_DRS:
        assert (12500 / dr) % 1 == 0.5
        assert o.matlab_round(12500 / dr) == lit.m_round(12500 / dr) == gc.coarse_geometry(dr)["d0"] == math.floor(12500 / dr) + 1
    for dr in gc.HALF_D1_DRS:
        assert (13750 / dr) % 1 == 0.5
        assert o.matlab_round(13750 / dr) == lit.m_round(13750 / dr) == gc.coarse_geometry(dr)["d1"] == math.floor(13750 / dr) + 1
    # the integer form of the geometry is the reference's floating-point one at every ratio of the set (and the drivers')
    for dr in gc.COARSE_DRS + (8,):
        geo = gc.coarse_geometry(dr)
        assert geo["fft_len"] == 2 ** math.floor(math.log2(148 / dr)) and geo["n_first"] == math.ceil(23 * 1250 / dr)
        assert geo["d0"] == o.matlab_round(12500 / dr) and geo["d1"] == o.matlab_round(13750 / dr)
    assert gc.coarse_geometry(75)["fft_len"] == 1 and gc.coarse_geometry(74)["fft_len"] == 2 and gc.coarse_geometry(1)["fft_len"] == 128
    assert sorted({gc.coarse_geometry(dr)["fft_len"] for dr in gc.COARSE_DRS}) == [2, 4, 8, 16, 32, 64]


@pytest.mark.parametrize("dr", gc.COARSE_DRS)
def test_both_oracles_agree_on_the_coarse_cases(captures, coarse_results, dr):
    for name, r8 in captures.items():
        s = gc.coarse_cut(r8, dr)
        p1, s1 = coarse_results[(name, dr)]
        p2, s2 = lit.FCCH_coarse_position(s, dr)
        assert np.array_equal(np.atleast_1d(p1), np.atleast_1d(p2)), (name, dr, p1, p2)
        assert np.allclose(s1, s2, rtol=0, atol=parity.SNR_ATOL), (name, dr)
        # the index error of s(1:n_first) one sample short
        short = s[: gc.coarse_geometry(dr)["n_first"] - 1]
        with pytest.raises(o.MatlabIndexError):
            o.FCCH_coarse_position(short, dr)
        with pytest.raises(IndexError):
            lit.FCCH_coarse_position(short, dr)


def test_a_the_hop_walk_runs_at_every_ratio(coarse_results):
    hits = {dr: [np.size(coarse_results[(f"dongle{d}", dr)][0]) if np.ndim(coarse_results[(f"dongle{d}", dr)][0]) else 0
                 for d in gc.COARSE_DONGLES] for dr in gc.COARSE_DRS}
    print(hits)
    for dr in gc.COARSE_DRS:
        if dr <= 37:
            assert max(hits[dr]) >= 2, (dr, hits[dr])
        else:
            assert hits[dr] == [0, 0], (dr, hits[dr])          # 2-point windows: the SNR is NaN, nothing hits
    for dr in gc.HALF_D1_DRS:                                  # the +11-frame distance that lands on .5 is walked
        gaps = np.concatenate([np.diff(coarse_results[(f"dongle{d}", dr)][0]) for d in gc.COARSE_DONGLES
                               if np.ndim(coarse_results[(f"dongle{d}", dr)][0])])
        assert np.any(np.abs(gaps - 13750) < 60), (dr, gaps)
    # the carrier without a BCCH: the sentinel wherever the windows are long enough to tell a tone (fft_len >= 16)
    for dr in gc.COARSE_DRS:
        if gc.coarse_geometry(dr)["fft_len"] >= 16:
            assert coarse_results[("no_bcch", dr)] == (-1.0, -1.0), dr


def test_b_coarse_decisions_sit_outside_the_certificate_margin(captures):
    worst, dropped, total = math.inf, [], 0
    for name, r8 in captures.items():
        for dr in gc.COARSE_DRS:
            total += 1
            m = gc.coarse_margin(gc.coarse_cut(r8, dr), dr)
            worst = min(worst, m)
            if not m > gc.MARGIN_DB:
                dropped.append((name, dr, m))
    print(f"smallest coarse margin {worst:.3e} dB; dropped {dropped}")
    assert dropped == [], dropped                               # the GPU test runs every (capture, dr): none may be inside
    assert len(dropped) <= gc.MAX_DROP_FRACTION * total


# ---- detector arguments ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def det():
    s = gc.det_stream()
    return s, {f: gc.window_snrs(s, f) for f in gc.DET_FFT_LENS}


def test_move_fft_grid_both_oracles_and_margins(det):
    s, snrs = det
    assert 3000 < len(s) < 3200
    dropped, total, hits = [], 0, 0
    for fft_len, mv_len, th, n in gc.move_cases():
        if fft_len in gc.UNCOMPARED_FFT_LENS:
            continue
        total += 1
        x = s if n is None else s[:n]
        r1 = o.move_fft_snr_runtime_avg(x, mv_len, fft_len, th)
        r2 = lit.move_fft_snr_runtime_avg(x, mv_len, fft_len, th)
        assert r1[:2] == r2[:2] and snr_close(r1[2], r2[2]) and snr_close(r1[3], r2[3]), (fft_len, mv_len, th, n, r1, r2)
        hit, _, m = gc.move_margin(snrs[fft_len] if n is None else gc.window_snrs(x, fft_len), mv_len, th)
        assert hit == r1[1]
        hits += r1[0]
        if not m > gc.MARGIN_DB:
            dropped.append((fft_len, mv_len, th, n, m))
    print(f"{total} cases, {hits} hit, dropped {dropped}")
    assert dropped == [] and len(dropped) <= gc.MAX_DROP_FRACTION * total
    assert hits >= total // 4 and total - hits >= total // 4    # both outcomes are well represented
    # the len edges: no window fits fft_len - 1 samples; one fits fft_len, and hits under th = -2000 unless its SNR is NaN
    for f in gc.DET_FFT_LENS:
        assert o.move_fft_snr_runtime_avg(s[:f - 1], 10 * f, f, -2000.0) == (False, -1, math.inf, math.inf)
        if f not in gc.UNCOMPARED_FFT_LENS:
            assert o.move_fft_snr_runtime_avg(s[:f], 10 * f, f, -2000.0)[:2] == ((True, 1) if f > 2 else (False, -1))


def test_fft_len_2_never_hits_and_3_is_rounding_defined(det):
    s, snrs = det
    assert np.all(np.isnan(snrs[2]))                            # noise_power < 0 in every window
    # 3-point windows: noise_power is 0 or an ulp of the total either side of it -- +Inf, NaN or some 150 dB, by rounding alone
    v = snrs[3]
    print("fft_len 3: +inf", int(np.sum(np.isposinf(v))), "nan", int(np.sum(np.isnan(v))), "finite", int(np.sum(np.isfinite(v))))
    assert np.all(np.isposinf(v) | np.isnan(v) | (v > 140.0)) and np.any(np.isposinf(v))
    # ... and one ulp of the total away from it in another: the literal oracle's definition DFT need not agree, nor need a kernel
    P = np.abs(np.fft.fft(np.lib.stride_tricks.sliding_window_view(s, 3)[:50], axis=1)) ** 2
    assert np.all(np.abs((P[:, 0] + P[:, 1] + P[:, 2]) - (P[:, 2] + P[:, 0] + P[:, 1])) <= 4 * np.spacing(P.sum(axis=1)))


@pytest.mark.parametrize("fft_len", [f for f in gc.DET_FFT_LENS if f not in gc.UNCOMPARED_FFT_LENS])
def test_specific_fft_cases_both_oracles_and_margins(det, fft_len):
    s, snrs = det
    cases = gc.specific_cases(snrs[fft_len], fft_len)
    nwin = len(snrs[fft_len])
    want_names = {"miss"} if fft_len == 2 else {"first_window", "last_window", "miss", "ends_on_last_window_miss", "ends_on_last_window_hit",
                                                "one_past_the_last_window_miss", "one_past_the_last_window_hit"}
    assert want_names <= set(cases), (fft_len, sorted(cases))
    for name, (tset, th, avg) in cases.items():
        m = gc.specific_margin(snrs[fft_len], tset[0], tset[1], th, avg)
        assert m > gc.MARGIN_DB, (fft_len, name, m)
        past = tset[1] > nwin
        try:
            r1 = o.specific_fft_snr_fix_avg(s, tset, fft_len, th, avg)
        except o.MatlabIndexError:
            r1 = "index"
        try:
            r2 = lit.specific_fft_snr_fix_avg(s, tset, fft_len, th, avg)
        except IndexError:
            r2 = "index"
        if r1 == "index" or r2 == "index":
            assert r1 == r2 == "index" and past and "hit" not in name, (fft_len, name, r1, r2)
            continue
        assert r1[:2] == r2[:2] and snr_close(r1[2], r2[2]), (fft_len, name, r1, r2)
        # the design: which window decides
        if name == "first_window":
            assert r1[:2] == (True, tset[0])
        elif name == "last_window":
            assert r1[:2] == (True, tset[1])
        elif name.endswith("_hit"):
            assert r1[:2] == (True, tset[0])
        else:
            assert r1 == (False, -1, math.inf), (fft_len, name, r1)


# ---- oversampled streams ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bases():
    return gc.ov_base_streams()


def same_stream(a, b):
    if not isinstance(a, np.ndarray) or not isinstance(b, np.ndarray):
        return not isinstance(a, np.ndarray) and not isinstance(b, np.ndarray) and a == b
    return a.shape == b.shape and np.max(np.abs(a - b)) <= STREAM_RTOL * np.max(np.abs(a))


@pytest.mark.parametrize("name,ov", [(n, v) for n in ("plain", "ppm") for v in gc.OVS] + [("plain", gc.CHAIN_MAX_OV)])
def test_c_chain_exits_and_both_oracles(bases, name, ov):
    r = gc.resample(bases[name], ov)
    ts = gc.training_sequence(ov)
    # premise (b) for the chain's own coarse call, FCCH_coarse_position(r(1:8*ov:end), 8)
    assert gc.coarse_margin(np.ascontiguousarray(r[0::8 * ov]), 8) > gc.MARGIN_DB
    assert len(ts) == 64 * ov and len(r) == math.ceil(len(bases[name]) * ov / 8)
    a = gc.oracle_chain(o, r, ov, ts)
    b = gc.oracle_chain(lit, r, ov, ts)
    assert a["exit"] == b["exit"] == gc.CHAIN_EXIT[name][ov], (a["exit"], b["exit"])
    for k in ("coarse_pos", "fcch_pos", "pos_info"):
        assert np.array_equal(np.atleast_1d(a[k]), np.atleast_1d(b[k])), (k, a[k], b[k])
    for k in ("sp1", "cp1", "sp2", "cp2"):
        assert parity.ppm_close(float(b[k]), float(a[k])), (k, a[k], b[k])
    for k in ("r1", "r2", "r3"):
        assert same_stream(a[k], b[k]), k
    if gc.CHAIN_EXIT[name][ov] == 0:
        assert a["pos_info"].shape[0] >= 14 and np.sum(a["pos_info"][:, 1] == 1) >= 4 and isinstance(a["r3"], np.ndarray)
        if name == "ppm":
            assert math.isfinite(a["sp1"]) and abs(a["sp1"]) > 100.0 and math.isfinite(a["sp2"]) and a["sp2"] != 0.0, (a["sp1"], a["sp2"])
    else:
        assert np.ndim(a["fcch_pos"]) == 1 and len(a["fcch_pos"]) >= 5      # the fine stage still completes at 1x
        assert a["pos_info"].shape == (1, 2) and np.all(a["pos_info"] == -1) and a["r3"] == -1.0 and math.isinf(a["cp2"])


# ---- front end --------------------------------------------------------------------------------------------------------------
def test_front_end_triples_cover_the_edges():
    filt = gc.fe_filters()
    assert [len(filt[k]) for k in ("one", "two", "fir47", "ramp48", "ramp300")] == [1, 2, 47, 48, 300]
    for k in ("ramp48", "ramp300"):
        assert not np.allclose(filt[k], filt[k][::-1], rtol=1e-3) and abs(np.sum(filt[k]) - 1.0) < 1e-12
    assert np.array_equal(filt["fir47"], filt["fir47"][::-1])
    t = gc.FE_TRIPLES
    assert len(set(t)) == len(t) and 24 <= len(t) <= 48
    assert {n for n, _, _ in t} == set(gc.FE_NS) and {d for _, d, _ in t} >= set(gc.FE_DECIMS) and {f for _, _, f in t} == set(filt)
    nd = lambda n, d: -(-n // d)
    assert any(n < len(filt[f]) for n, _, f in t) and any(n < d for n, d, _ in t)
    assert {1, 256, 257} <= {nd(n, d) for n, d, _ in t}
    assert any(nd(n, d) > 256 and d > 1 for n, d, _ in t) and any(len(filt[f]) > 256 and nd(n, d) > 256 for n, d, f in t)
    assert sum((2 * n) % 16 != 0 for n in gc.FE_NS) == len(gc.FE_NS) - 1
    for n in (1, 7, 4099):
        raw = gc.fe_raw(n)
        assert raw.shape == (3, 2 * n) and raw.dtype == np.uint8
        assert np.array_equal(o.raw2iq(raw.T.astype(np.float64)), lit.raw2iq(raw.T.astype(np.float64)))


def test_front_end_bound_holds_between_two_orders_of_summation():
    """the derived bound 2 ntaps 2^-53 sum|coef| max|x| covers the difference between lfilter and the literal difference equation
    (another order of the same sums) with room to spare, on the longest filter"""
    filt = gc.fe_filters()
    for n, name in ((4099, "ramp300"), (4099, "fir47"), (257, "ramp48")):
        x = o.raw2iq(gc.fe_raw(n).T.astype(np.float64))
        err = np.max(np.abs(o.matlab_filter(filt[name], x) - lit.filter_fir(filt[name], x)))
        bound = gc.fe_bound(filt[name], x)
        print(name, n, f"err {err:.3e} bound {bound:.3e}")
        assert err <= bound
