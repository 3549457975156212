"""CPU tests of row_coherence and apply_params_refine (include/gsmcal.h): the header and the Python names, the
restatement of tests/row_coherence_ref.py held to pair_coherence's restatement on the designed GSM streams and to planted values on
designed rows, the host helper gsmcal_apply_params_refine (pure host arithmetic in libgsmcal.so; no GPU) held to its restatement bit
for bit, the closed loop make_wideband -> apply -> coherence -> refine -> apply -> coherence in numpy with the four wrong compositions
told apart, and the LDS layout of k_row_xcorr's reads counted on the host.  Nothing here needs a GPU."""
import os
import re

import numpy as np
import pytest

import pair_coherence_ref as pcr
import row_coherence_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "gsmcal.h")) as f:
        return f.read()


def test_header_declares_the_entry_points_and_names_the_columns(gsmcal_mod):
    txt = header()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for sym in ("gsmcal_row_coherence_batch", "gsmcal_row_coherence_batch_resident", "gsmcal_apply_params_refine"):
        assert re.search(r"\bint %s\s*\(" % sym, code), sym
        assert sym in gsmcal_mod.SIGNATURES
    assert not re.search(r"gsmcal_row_coherence\w*_dev\b", code)
    defs = dict(re.findall(r"#define (GSMCAL_\w+) (\S.*?)\s*(?:/\*|$)", txt, flags=re.M))

    def value(name):
        expr = defs[name]
        for k in sorted(defs, key=len, reverse=True):
            expr = re.sub(r"\b%s\b" % k, lambda m: "(%s)" % value(m.group(0)), expr) if k in expr and k != name else expr
        return int(eval(expr, {"__builtins__": {}}))               # (integer arithmetic on the header's own constants)
    assert (value("GSMCAL_MAX_ROW_WINDOWS"), value("GSMCAL_MAX_ROW_LAG"), value("GSMCAL_ROW_CHUNK")) == (128, 64, 512)
    assert value("GSMCAL_ROW_COLS") == gsmcal_mod.ROW_COLS == rr.ROW_COLS == 20 + 6 * 128
    assert (gsmcal_mod.MAX_ROW_WINDOWS, gsmcal_mod.MAX_ROW_LAG, gsmcal_mod.ROW_CHUNK) == (128, 64, 512)
    head = {"coherence": "COH", "min_coherence": "MIN_COHERENCE"}
    for i, name in enumerate(gsmcal_mod.ROW_FIELDS):
        assert value("GSMCAL_R_" + head.get(name, name.upper())) == i == rr.col(name), name
    for j, name in enumerate(gsmcal_mod.ROW_WINDOW_FIELDS):
        assert value("GSMCAL_R_" + head.get(name, name.upper())) == 20 + 128 * j == rr.col(name), name
    assert gsmcal_mod.ROW_FIELDS == rr.HEAD and gsmcal_mod.ROW_WINDOW_FIELDS == rr.WINDOW
    # columns 0..15 carry the meaning of GSMCAL_P_*
    for i, name in enumerate(gsmcal_mod.PAIR_FIELDS):
        assert gsmcal_mod.ROW_FIELDS[i] == name.replace("num_bursts", "num_windows").replace("burst_carrier_hz", "window_carrier_hz")
    t = gsmcal_mod.row_rows(np.arange(2 * rr.ROW_COLS, dtype=np.float64).reshape(2, -1))
    assert t["max_gap"].tolist() == [19.0, 19.0 + rr.ROW_COLS] and t["edge"].shape == (2, 128) and t["edge"][0, 0] == rr.col("edge")


@pytest.mark.parametrize("ov", [2, 4, 8])
def test_restatement_equals_pair_coherence_on_the_designed_streams(ov):
    """windows at the three bursts, win_len 148 ov, fs_of(ov), max_gap 1875 ov: head columns 2..15 and the per-window columns"""
    r, r_len, pi, _ = pcr.designed_streams(ov)
    frame, M = 1250 * ov, 2 * ov
    starts = [200, 200 + frame, 200 + 2 * frame]
    for lag0 in (11, 10, 11 + M):                                   # (the last: every maximum on the edge)
        want = pcr.pair_coherence(r, r_len, pi, ov, 0, 1, lag0, M)
        got = rr.row_coherence(r, 0, 1, lag0, starts, 148 * ov, pcr.fs_of(ov), M, 0.5, 1875 * ov)
        a, b = got["row"][2:16], want["row"][2:16]
        assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
        m = ~np.isnan(b)
        assert np.all(np.abs(a[m] - b[m]) <= 1e-12 * np.abs(b[m])), (ov, lag0, a, b)
        assert got["row"][0] == want["row"][0] and got["row"][1] == 3
        for name, theirs in (("delay", "delay"), ("phase", "phase"), ("freq", "freq"), ("coherence", "coherence"), ("edge", "edge")):
            x, y = got["row"][rr.col(name): rr.col(name) + 3], want["row"][pcr.col(theirs): pcr.col(theirs) + 3]
            assert np.array_equal(np.isnan(x), np.isnan(y)) and np.all(np.abs(x - y)[~np.isnan(y)] <= 1e-12 * np.abs(y[~np.isnan(y)])), (name, x, y)
        assert np.array_equal(got["row"][rr.col("start"): rr.col("start") + 3], want["row"][pcr.col("pos"): pcr.col("pos") + 3] - 1.0)
        assert np.isnan(got["row"][rr.col("start") + 3: rr.col("delay")]).all()
        assert np.all(np.abs(got["corr"] - want["corr"][:3]) <= 1e-12 * np.abs(want["corr"][:3]))
        assert np.array_equal(got["mstar"], want["mstar"][:3]) and np.array_equal(got["used"], want["used"][:3])


def test_planted_values_come_back_on_designed_rows():
    """win_len 4096 (Ls = 1024, two chunks of the sums per segment): the planted delay, phase and carrier within designed_bounds"""
    fs, win, M = 2.4e6, 4096, 8
    D, phi, f = 11.25, 0.7, 90.0
    a, b, plant = rr.designed_rows(40000, D, phi, f, fs, 20261021)
    starts = [300, 9000, 17800, 26000, 34000]
    bound = rr.designed_bounds(plant, starts, win)
    res = rr.row_coherence(np.stack([a, b]), 0, 1, 11, starts, win, fs, M, 0.5, 9000)
    row, c = res["row"], rr.col
    W = len(starts)
    print("bounds", bound)
    dev = {"delay": np.max(np.abs(row[c("delay"): c("delay") + W] - D)), "phase": np.max(np.abs(rr.wrap(row[c("phase"): c("phase") + W] - rr.designed_phase(plant, starts, win)))),
           "freq": np.max(np.abs(row[c("freq"): c("freq") + W] - f)), "rel_carrier_hz": abs(row[c("rel_carrier_hz")] - f),
           "rel_sampling_ppm": abs(row[c("rel_sampling_ppm")]), "delay0": abs(row[c("delay0")] - D),
           "phase0": abs(rr.wrap(row[c("phase0")] - rr.designed_phase(plant, starts, win)[0]))}
    print("deviations", dev)
    assert rr.ties_ok(res) and row[0] == 0 and row[c("num_used")] == W and row[c("num_adjacent")] == W - 1
    assert np.all(row[c("coherence"): c("coherence") + W] >= 0.9)
    for k in ("delay", "phase", "freq", "rel_carrier_hz", "rel_sampling_ppm"):
        assert dev[k] <= bound[k], (k, dev[k], bound[k])
    assert dev["delay0"] <= bound["delay"] and dev["phase0"] <= bound["phase"]
    # windows 8800 apart with max_gap 8000: no adjacent step, rel_carrier_hz is the mean of freq
    far = rr.row_coherence(np.stack([a, b]), 0, 1, 11, starts[1:3], win, fs, M, 0.5, 8000)["row"]
    assert far[c("num_adjacent")] == 0 and far[c("rel_carrier_hz")] == far[c("window_carrier_hz")]


def test_valid_intervals_and_the_four_inequalities():
    a, b, _ = rr.designed_rows(3000, 3.0, 0.1, 0.0, 1e6, 5)
    x = np.stack([a, b])
    win, M, lag0 = 19, 2, 3                                            # Ls = 4: 16 samples are used, not 19
    for valid, p, ev in (([[0, 3000], [0, 3000]], 0, True), ([[5, 3000], [0, 3000]], 4, False), ([[5, 3000], [0, 3000]], 5, True),
                         ([[0, 116], [0, 3000]], 100, True), ([[0, 115], [0, 3000]], 100, False),
                         ([[0, 3000], [101, 3000]], 100, True), ([[0, 3000], [102, 3000]], 100, False),
                         ([[0, 3000], [0, 121]], 100, True), ([[0, 3000], [0, 120]], 100, False)):
        res = rr.row_coherence(x, 0, 1, lag0, [p], win, 1e6, M, 0.5, None, valid)
        assert res["evaluated"].tolist() == [ev], (valid, p)
        assert np.isnan(res["row"][rr.col("start")]) == (not ev) and np.isnan(res["corr"][0]).all() == (not ev)
    assert rr.row_coherence(x, 0, 1, lag0, [2984], win, 1e6, M)["evaluated"].tolist() == [False]       # p + lag0 + M + 16 = 3005 > 3000
    assert rr.row_coherence(x, 0, 1, lag0, [2979], win, 1e6, M)["evaluated"].tolist() == [True]


def test_library_helper_equals_the_restatement_bit_for_bit(gsmcal_mod):
    lib = gsmcal_mod.load()
    dp = gsmcal_mod._lib.c_double_p
    seen = set()
    for coh, par in rr.refine_cases():
        st, want = rr.apply_params_refine(coh, par)
        got = np.full(10, -7.0)
        coh_c, par_c = np.ascontiguousarray(coh), np.ascontiguousarray(par, dtype=np.float64)
        rc = lib.gsmcal_apply_params_refine(coh_c.ctypes.data_as(dp), par_c.ctypes.data_as(dp), got.ctypes.data_as(dp))
        assert rc == st, (rc, st, coh[:16], par)
        assert np.array_equal(got.view(np.uint64)[~np.isnan(want)], want.view(np.uint64)[~np.isnan(want)]), (got, want)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        seen.add(st)
        if st != 0:
            assert np.isnan(got[np.arange(10) != 5]).all() and (got[5] == par[5] or np.isnan(par[5]))
        else:
            assert np.array_equal(got[4:], par[4:])                 # anchor, scale, dc and imbalance are copied
    assert seen == {0, rr.S_ALIGN_SKIPPED, rr.E_ARG}
    ok = rr.refine_cases()[0]
    out = np.zeros(10)
    args = [np.ascontiguousarray(ok[0]).ctypes.data_as(dp), np.ascontiguousarray(ok[1]).ctypes.data_as(dp), out.ctypes.data_as(dp)]
    for i in range(3):
        assert lib.gsmcal_apply_params_refine(*[None if j == i else a for j, a in enumerate(args)]) == rr.E_ARG
    assert not out.any()
    # the wrapper: row for row
    tab = np.stack([c for c, _ in rr.refine_cases()[:4]])
    par = np.stack([p for _, p in rr.refine_cases()[:4]])
    got = gsmcal_mod.apply_params_refine(tab, par)
    assert all(np.array_equal(got[i], rr.apply_params_refine(tab[i], par[i])[1]) for i in range(4))
    with pytest.raises(gsmcal_mod.GsmcalError, match="failed with -1 "):
        gsmcal_mod.apply_params_refine(rr.refine_cases()[14][0], rr.refine_cases()[14][1])


@pytest.fixture(scope="module")
def loop(gsmcal_mod):
    raw, params = rr.loop_captures(gsmcal_mod.synth)
    return raw, params, rr.closed_loop(raw, params, rr.ref_apply, rr.ref_coherence, rr.apply_params_refine)


def test_make_wideband_is_seeded_and_follows_make_streams_convention(gsmcal_mod):
    s = gsmcal_mod.synth
    kw = dict(dongle=2, n=3000, sample_rate=2.048e6, tuned_freq=433.92e6, e_ppm=63.0, c_ppm=-21.5, start=4.25, phase=0.4, tx_key=9, noise=0.0)
    a, ta = s.make_wideband(**kw)
    b, _ = s.make_wideband(**kw)
    assert a.dtype == np.uint8 and a.shape == (6000,) and np.array_equal(a, b) and ta["f_off"] == 1e-6 * -21.5 * 433.92e6
    assert not np.array_equal(a, s.make_wideband(**dict(kw, tx_key=10))[0])
    # evaluated exactly at the dongle's sample times: sample k is s((start + k) / (1 + e)) turned by 2 pi f_off k / fs + phase
    k = np.arange(3000, dtype=np.float64)
    t = (4.25 + k) / (1.0 + 63e-6)
    want = 30.0 * np.exp(1j * (2 * np.pi * np.outer(t, ta["nu"]) + ta["theta"])).sum(axis=1) / np.sqrt(96)
    want = want * np.exp(1j * (2 * np.pi * ta["f_off"] / 2.048e6 * k + 0.4))
    z = (a[0::2] - 127.4) + 1j * (a[1::2] - 127.6)
    assert np.max(np.abs(z - want)) <= 0.5 * np.sqrt(2) + 1e-9 and a.min() > 0 and a.max() < 255      # rounding to bytes alone
    assert np.all(np.abs(ta["nu"]) <= 0.15) and len(ta["nu"]) == 96
    # two dongles given the same key see the same transmission: without errors and without noise, the same bytes
    c0 = s.make_wideband(dongle=0, n=500, tx_key=9, noise=0.0)[0]
    assert np.array_equal(c0, s.make_wideband(dongle=1, n=500, tx_key=9, noise=0.0)[0])


def test_closed_loop_one_refinement_lands_on_the_reference(loop):
    raw, params, res = loop
    first, second = rr.loop_figures(res["tables"][0]), rr.loop_figures(res["tables"][1])
    print("after pass 1:", first)
    print("after one refinement:", second, "bars:", rr.LOOP_BARS)
    assert res["statuses"] == [0, 0]
    # what the first pass leaves: the planted start offsets, a few hundred Hz, the tuners' phases
    t0 = res["tables"][0]
    assert abs(t0[1, rr.col("delay0")] + 11.37) <= 0.1 and abs(t0[2, rr.col("delay0")] + 5.8) <= 0.1
    assert first["rel_carrier_hz"] >= 150.0 and not rr.within_bars(first)
    assert rr.within_bars(second), (second, rr.LOOP_BARS)
    # the bars are twice the residuals written down in row_coherence_ref (and in DESIGN 24): those are what this run gives
    for k, v in rr.LOOP_RESIDUAL.items():
        assert abs(second[k] - v) <= (2e-3 * abs(v) if k != "mean_coherence" else 1e-6), (k, second[k], v)
    # the pair (0, 0): the reference against itself
    assert abs(res["tables"][1][0, rr.col("delay0")]) <= 1e-3 and res["tables"][1][0, rr.col("mean_coherence")] >= 0.9999


@pytest.mark.parametrize("variant", rr.VARIANTS)
def test_each_wrong_composition_misses_a_bar(loop, variant):
    raw, params, _ = loop
    res = rr.closed_loop(raw, params, rr.ref_apply, rr.ref_coherence, lambda c, p: rr.apply_params_refine(c, p, variant))
    fig = rr.loop_figures(res["tables"][1])
    print(variant, fig)
    assert rr.misses_some_bar(fig, 1.5), (variant, fig, rr.LOOP_BARS)


def test_lds_reads_of_k_row_xcorr_meet_no_bank_conflict():
    """ds_read_b128 serves a wave in four groups of 16 lanes; a 16-byte value occupies one of 16 slots of a 256-byte bank row, slot =
    (byte address / 16) mod 16, and two lanes of a group conflict when they read DIFFERENT addresses of one slot.  Lane (sp, g) =
    (l >> 4, l & 15) of k_row_xcorr reads b at the complex index n + sp + g + 16 j (n the same in all lanes) and a at n + sp."""
    groups = ([0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31])
    groups = groups + tuple([l + 32 for l in grp] for grp in groups)
    assert sorted(l for grp in groups for l in grp) == list(range(64))
    for base in range(16):                                           # any alignment of the tile's running index
        for index in (lambda l: base + (l >> 4) + (l & 15), lambda l: base + (l >> 4)):
            for grp in groups:
                slots = {}
                for l in grp:
                    slots.setdefault(index(l) % 16, set()).add(index(l))
                assert all(len(v) == 1 for v in slots.values()), (base, grp, slots)
