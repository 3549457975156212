"""CPU tests of pair_align: properties of the fp64 restatement in tests/pair_align_ref.py, the closed loop
measure -> align -> measure on the designed pair, the interpolator's error on a band-limited signal, the gain of the sum, and the
library's host-side gsmcal_pair_align_params against the restatement's.

Bars, with their origin:
  sum of the taps        |sum_k h(k - mu) - 1| <= 2.5e-4 on a grid of mu: a 16-tap Blackman-windowed sinc is no exact partition of
                         unity; the definition's DC gain is furthest from 1 at mu = 1/2, by 1.25e-4 (printed by the test); twice
                         that is allowed
  continuity             h(k - mu) at mu = 1 - e against h(k + 1 - 0) shifted by one tap, and mu = e against mu = 0: the window is
                         zero at |u| = 8 and |h'| <= pi / 2 + the window's slope < 2, so a step e in mu moves a tap by < 2 e
  closed loop            after alignment by the measured parameters, against zero: |delay0|, |phase0| and |rel_carrier_hz| within
                         twice pair_coherence_ref.designed_bounds' delay, phase and rel_carrier_hz -- the estimate used to align and
                         the estimate taken afterwards each carry the bound once; mean_coherence rises; no decision on a tie.
                         rel_sampling_ppm is not asserted: over three bursts the slope is dominated by the coupling of the carrier
                         into the delay, which vanishes with the de-rotation -- it comes back with the opposite sign
  interpolation error    rms |aligned - a| over the valid range <= 2 x pair_align_ref.INTERP_RMS (what the restatement gave when the
                         definition was fixed: 9.5e-3 / 1.2e-3 / 6.5e-5 at ov 2 / 4 / 8; the designed stream is not band-limited at
                         ov 2)
  combining gain         >= 2.8 dB for two equal members under independent noise of power 0.25 (ideal 3.01 dB; the restatement
                         gives 3.1 to 3.2 dB, the excess being the interpolator's slight low-pass on b's noise)
"""
import math
import os
import subprocess

import numpy as np
import pytest

import pair_align_ref as ref
import pair_coherence_ref as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_taps_sum_to_one_within_the_windows_ripple_and_h0_is_one():
    mu = np.linspace(0.0, 1.0, 257)[:-1]
    t = ref.taps(mu)
    dev = np.abs(t.sum(axis=1) - 1.0)
    print("largest |sum of taps - 1|", dev.max(), "at mu", mu[dev.argmax()])
    assert dev.max() <= 2.5e-4
    assert ref.h(0.0) == 1.0 and np.all(np.abs(ref.taps(0.0) - (ref.K == 0)) <= 1e-16)       # (np.sinc(k) is 4e-17, not 0)
    assert abs(ref.h(8.0)) <= 1e-16 and abs(ref.h(-8.0)) <= 1e-16            # the window closes


def test_taps_are_continuous_across_a_base_flip():
    """x just below an integer (base = x0 - 1, mu = 1 - e) and just above (base = x0, mu = e) must weigh the same samples alike:
    tap k of the first is tap k - 1 of the second, and the tap that falls off either end is zero."""
    for e in (1e-12, 1e-9, 1e-6):
        below, at, above = ref.taps(1.0 - e), ref.taps(0.0), ref.taps(e)
        assert np.all(np.abs(below[1:] - at[:-1]) <= 2 * e) and abs(below[0]) <= 2 * e       # k = -7 at mu -> 1: u -> -8
        assert np.all(np.abs(above - at) <= 2 * e)
    # ... and on a signal: the output at x0 - e and x0 + e differs by no more than the signal's own slope allows
    s = np.exp(1j * 0.3 * np.arange(64))
    outs = [ref.pair_align(s, 64, 2, [20.0 + d, 0.0, 0.0, 0.0, 0.0, 1.0], 8)["out"] for d in (-1e-9, 0.0, 1e-9)]
    assert np.all(np.abs(outs[0] - outs[1]) <= 1e-8) and np.all(np.abs(outs[2] - outs[1]) <= 1e-8)
    assert np.all(np.abs(outs[1] - s[20:28]) <= 1e-15)                                         # on the grid: the samples themselves


def test_valid_interval_exactly_at_and_one_past_each_limit():
    """valid iff 0 <= base - 7 and base + 8 < len"""
    s = np.ones(100, dtype=np.complex128)
    for delay, length, out_len, first, end in (
            (7.0, 100, 100, 0, 85),            # base = n + 7: n = 0 is the first with base - 7 = 0; base + 8 < 100 up to n = 84
            (6.999, 100, 100, 1, 86),          # one past the lower limit: n = 0 has base = 6
            (7.0, 16, 4, 0, 1),                # the shortest stream that holds one sample: base = 7, base + 8 = 15 < 16
            (7.0, 15, 4, 0, 0),                # ... and one sample shorter: none
            (-3.5, 100, 100, 11, 96),          # base = floor(n - 3.5) >= 7 from n = 11 (x = 7.5); base + 8 < 100: x < 92 up to n = 95 (x = 91.5)
            (200.0, 100, 50, 0, 0)):           # beyond the stream
        one = ref.pair_align(s[:length], length, 2, [delay, 0.0, 0.0, 0.0, 0.0, 1.0], out_len)
        assert (one["status"], one["first_valid"], one["end_valid"], one["num_valid"]) == (0, first, end, end - first), (delay, length, one["first_valid"], one["end_valid"])
        assert np.all(one["out"][:first] == 0) and np.all(one["out"][end:] == 0) and np.all(one["out"][first:end] != 0)
    # the drift moves the upper limit: x = n + 10 + 1e-3 n reaches len - 8 = 9992 at n = 9972.03: the last valid n is 9972 (x = 9991.97)
    one = ref.pair_align(np.ones(10000), 10000, 2, [10.0, 1000.0, 0.0, 0.0, 0.0, 1.0], 10000)
    assert (one["first_valid"], one["end_valid"]) == (0, 9973)
    assert ref.pair_align(s, 0, 2, [7.0, 0.0, 0.0, 0.0, 0.0, 1.0], 8)["status"] == ref.S_POST_NO_POS
    assert ref.pair_align(s, 100, 2, [7.0, np.nan, 0.0, 0.0, 0.0, 1.0], 8)["status"] == ref.S_ALIGN_SKIPPED


def test_batch_sum_order_skips_and_combined_interval():
    rng = np.random.Generator(np.random.Philox(key=[3, 3]))
    r = rng.standard_normal((3, 200)) + 1j * rng.standard_normal((3, 200))
    params = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.5], [20.5, 100.0, 50.0, 0.3, 10.0, 0.25], [np.nan] * 5 + [0.25], [3.0, 0.0, 0.0, 0.0, 0.0, 2.0]])
    res = ref.pair_align_batch(r, [200, 150, 200, -1], 2, [0, 1, 2, 0], params, 180)
    info = res["info"]
    assert info[:4, 0].tolist() == [0.0, 0.0, 17.0, 0.0] and info[4].tolist() == [3.0, 7.0, 122.0, 2.75]
    assert np.all(res["aligned"][2] == 0)
    want = 0.5 * res["aligned"][0] + 0.25 * res["aligned"][1] + 2.0 * res["aligned"][3]
    assert np.array_equal(res["combined"], want)                   # (invalid samples are exact zeros: the same sum)
    res = ref.pair_align_batch(r, [200, 150, 200], 2, [1], params[2:3], 50)
    assert res["info"].tolist() == [[17.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]] and np.all(res["combined"] == 0)


@pytest.mark.parametrize("ov", [2, 4, 8])
def test_closed_loop_on_the_designed_pair(ov):
    streams = pc.designed_streams(ov)
    r, r_len, pi, plant = streams
    bound = pc.designed_bounds(ov, plant)
    row, before = ref.measured_row(ov, streams=streams)
    n = r.shape[1]
    al = ref.pair_align(r[1], n, ov, row, n)
    after = pc.pair_coherence(np.stack([r[0], al["out"]]), r_len, pi, ov, 0, 1, 0, 3)
    c = pc.col
    b, a = before["row"], after["row"]
    print(f"ov {ov}: delay0 {b[c('delay0')]:.4f} -> {a[c('delay0')]:+.4f}  phase0 {b[c('phase0')]:.4f} -> {a[c('phase0')]:+.4f}  carrier {b[c('rel_carrier_hz')]:.2f} -> "
          f"{a[c('rel_carrier_hz')]:+.3f} Hz  coherence {b[c('mean_coherence')]:.5f} -> {a[c('mean_coherence')]:.5f}  ppm {b[c('rel_sampling_ppm')]:+.3f} -> {a[c('rel_sampling_ppm')]:+.3f}")
    assert b[0] == 0 and a[0] == 0 and a[c("num_used")] == 3
    assert abs(a[c("delay0")]) <= 2 * bound["delay"]
    assert abs(a[c("phase0")]) <= 2 * bound["phase"]
    assert abs(a[c("rel_carrier_hz")]) <= 2 * bound["rel_carrier_hz"]
    assert a[c("mean_coherence")] > b[c("mean_coherence")]
    assert pc.ties_ok(after)


@pytest.mark.parametrize("ov", [2, 4, 8])
def test_interpolation_error_on_the_noise_free_designed_pair(ov):
    a, b, _, _ = pc.designed_pair(ov, noise=False)
    one = ref.pair_align(b, len(a), ov, ref.planted_row(ov), len(a))
    v = one["valid"]
    rms = math.sqrt(np.mean(np.abs(one["out"][v] - a[v]) ** 2))
    print(f"ov {ov}: rms |aligned - a| = {rms:.3e} over {v.sum()} valid samples (recorded {ref.INTERP_RMS[ov]:.2e})")
    assert v.sum() >= len(a) - 32 and rms <= 2 * ref.INTERP_RMS[ov]


@pytest.mark.parametrize("ov", [2, 4, 8])
def test_combining_gain_of_two_equal_members(ov):
    a, _, _, _ = pc.designed_pair(ov, noise=False)
    an, bn, wa = ref.noisy_designed(ov)
    n = len(a)
    res = ref.pair_align_batch(np.stack([an, bn]), [n, n], ov, [0, 1], np.stack([ref.ref_row(0.5), ref.planted_row(ov, 0.5)]), n)
    lo, hi = int(res["info"][2, 1]), int(res["info"][2, 2])
    assert res["info"][2, 0] == 2 and res["info"][2, 3] == 1.0 and hi - lo >= n - 32
    gain = 10 * math.log10(np.mean(np.abs(wa[lo:hi]) ** 2) / np.mean(np.abs(res["combined"][lo:hi] - a[lo:hi]) ** 2))
    print(f"ov {ov}: noise of the sum {gain:.2f} dB below that of a alone")
    assert gain >= 2.8


def test_api_pair_align_params_against_the_restatement(gsmcal_mod):
    g = gsmcal_mod
    rows, want = [], []
    for ov in (2, 4, 8):
        r, r_len, pi, _ = pc.designed_streams(ov)
        for lag0, M in ((11, 3), (11 + 5, 3)):                     # a measured row, and one with every burst at the edge (status 16)
            row = pc.pair_coherence(r, r_len, pi, ov, 0, 1, lag0, M)["row"]
            got = g.pair_align_params(row, ov, weights=0.25)
            exp = ref.pair_align_params(row, ov, 0.5, 0.25)
            assert got.shape == (1, 6) and np.array_equal(got[0], exp, equal_nan=True), (ov, lag0, got, exp)
            assert np.isnan(exp[:5]).all() == (lag0 != 11)
        # the first USED burst decides the anchor: with the threshold above the first burst's coherence it is the second
        row = pc.pair_coherence(r, r_len, pi, ov, 0, 1, 11, 3)["row"].copy()
        row[pc.col("coherence")] = 0.6
        a, b = g.pair_align_params(row, ov, min_coherence=0.7)[0], ref.pair_align_params(row, ov, 0.7, 0.5)
        assert np.array_equal(a, b) and a[4] == 200.0 + 1250 * ov + (148 * ov - 1) / 2
        assert g.pair_align_params(row, ov)[0][4] == 200.0 + (148 * ov - 1) / 2
    # several rows, default weights: equal gain with the reference stream
    r, r_len, pi, _ = pc.designed_streams(4)
    tab = np.stack([pc.pair_coherence(r, r_len, pi, 4, 0, 1, 11, 3)["row"]] * 3)
    assert np.all(g.pair_align_params(tab, 4)[:, 5] == 0.25)
    assert g.ALIGN_PARAM_FIELDS == ref.PARAM_FIELDS and g.ALIGN_INFO_FIELDS == ("status", "first_valid", "end_valid", "num_valid")


def test_python_constants_equal_the_header_and_the_restatement(gsmcal_mod):
    import re
    g = gsmcal_mod
    txt = open(os.path.join(ROOT, "include", "gsmcal.h")).read()
    val = lambda name: int(re.search(rf"{name}\s*=?\s*(\d+)", txt).group(1))
    assert val("#define GSMCAL_MAX_ALIGN_MEMBERS") == g.MAX_ALIGN_MEMBERS == ref.MAX_ALIGN_MEMBERS == 64
    assert val("#define GSMCAL_ALIGN_PARAMS") == g.ALIGN_PARAMS == ref.ALIGN_PARAMS == 6
    assert val("#define GSMCAL_ALIGN_INFO_COLS") == g.ALIGN_INFO_COLS == ref.ALIGN_INFO_COLS == 4
    assert val("GSMCAL_S_ALIGN_SKIPPED") == g.S_ALIGN_SKIPPED == ref.S_ALIGN_SKIPPED == 17
    for name in ("pair_align", "pair_align_batch", "pair_align_batch_dev", "pair_align_params", "align_rows", "coherent_combine"):
        assert callable(getattr(g, name))
    info = np.array([[0, 3, 90, 87], [17, 0, 0, 0], [1, 3, 90, 0.5]], dtype=float)
    t = g.align_rows(info)
    assert t["status"].tolist() == [0, 17] and t["num_valid"].tolist() == [87, 0] and (t["members_used"], t["combined_first"], t["combined_end"], t["weight_sum"]) == (1, 3, 90, 0.5)


@pytest.mark.parametrize("api", ["interleaved", "split"])
def test_mex_pair_align_target_compiles_against_the_abi(api):
    """the gateway's pair_align target through `gcc -fsyntax-only` against the declaration-only mex.h (as tests/test_abi_cpu.py does
    for the targets of its list)"""
    r = subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-std=c99", "-DGSMCAL_FN_pair_align"] +
                       (["-DGSMCAL_STUB_SPLIT"] if api == "split" else []) +
                       ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mex_stub"),
                        os.path.join(ROOT, "mex", "gsmcal_mex.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "defined(GSMCAL_FN_pair_align)" in open(os.path.join(ROOT, "mex", "gsmcal_mex.c")).read()
