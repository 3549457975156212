"""GPU tests of gsmcal_subband_power_batch[_dev] and the multi-channel scan (-m gpu): several sub-band powers per capture
(multi_rtl_sdr_diversity_scanner_another_bak.m:186-210) against the line-by-line fp64 restatement subband_ref.literal:
relative 1e-10 (the figure of tests/test_gpu_spectrum.py), exactly 0 where the restatement is exactly 0, NaN in unused slots,
bit-identical across runs, slots, neighbours, batch positions and batch sizes.  tests/test_subband_cpu.py shows that on every
input used here `literal` sits within 1e-11 of the longdouble modulated-tap form, so no case needs another reference."""
import ctypes as C

import numpy as np
import pytest

import subband_ref as ref

import gsmcal.dist  # noqa: F401

pytestmark = pytest.mark.gpu

FS = ref.FS
TOL = 1e-10


def compare(got, want, tol=TOL):
    """got against a restatement table: NaN exactly where it is NaN, 0 exactly where it is 0, relative tol elsewhere.
    Returns the largest relative deviation."""
    assert got.shape == want.shape
    worst = 0.0
    for (i, j), r in np.ndenumerate(want):
        if np.isnan(r):
            continue
        if r == 0.0:
            assert got[i, j] == 0.0, (i, j, got[i, j])
        else:
            dev = abs(got[i, j] - r) / r
            assert dev <= tol, (i, j, got[i, j], r, dev)
            worst = max(worst, dev)
    return worst


def check(g, ctx, raw, coef, w, decim, rows=None):
    got = g.subband_power_batch(raw, coef, w, decim=decim, ctx=ctx)
    assert np.array_equal(np.isnan(got), np.isnan(w))                            # unused slots, and only those, are NaN
    worst = compare(got if rows is None else np.where(np.isin(np.arange(len(raw)), rows)[:, None], got, np.nan),
                    ref.table(ref.literal, raw, coef, w, decim, rows))
    print("largest relative deviation from literal: %.3g" % worst)
    return got


def test_reference_defaults(g_mod, ctx):
    """:40-57 as shipped: 100 kHz, 0.2 s -> 32 taps, N = 409 600, decim 1; 3 captures, 5 points and 2 unused slots each."""
    raw, coef, w, decim = ref.defaults(g_mod.dist.spectrum_filter)
    assert (len(coef), raw.shape, decim, w.shape) == (32, (3, 2 * 409600), 1, (3, 7))
    got = check(g_mod, ctx, raw, coef, w, decim)
    again = g_mod.subband_power_batch(raw, coef, w, decim=decim, ctx=ctx)
    assert np.array_equal(got, again, equal_nan=True)                            # bit-identical run to run


@pytest.mark.parametrize("name", ref.CASES)
def test_cases(g_mod, ctx, name):
    raw, coef, w, decim = ref.case(name, g_mod.dist.spectrum_filter)
    got = check(g_mod, ctx, raw, coef, w, decim)
    if name == "phases":                                                         # w = 0 is the plain band power
        bp = g_mod.band_power_batch(raw, coef, decim, ctx=ctx)
        assert np.all(np.abs(got[:, 0] - bp) <= TOL * bp)
    if name == "n1":
        assert np.all(got == 0.0)
    if name == "ragged":
        assert np.all(np.isnan(got[3])) and np.isnan(got[1, 0]) and np.isnan(got[2, 3]) and not np.isnan(got[2, 6])


@pytest.mark.parametrize("val", [(0, 0), (255, 255), (17, 200)])
def test_constant_captures_give_exact_zero(g_mod, ctx, val):
    n = 20480
    raw = np.empty((3, 2 * n), dtype=np.uint8)
    raw[:, 0::2], raw[:, 1::2] = val
    w = np.tile(ref.phase([-200e3, -100e3, 0, 100e3, 256e3]), (3, 1))
    for coef, decim in ((g_mod.dist.spectrum_filter(FS, 100e3, 0.2)[1], 1), (np.array([1.0]), 1),
                        (np.random.default_rng(0).standard_normal(45), 3)):
        got = g_mod.subband_power_batch(raw, coef, w, decim=decim, ctx=ctx)
        assert np.all(got == 0.0), got
        assert all(ref.literal(raw[0], coef, v, decim) == 0.0 for v in w[0])


def test_large_dc_with_weak_tone(g_mod, ctx):
    """DC at the rails, a tone of a byte or two: no cancellation (the DC is removed before the filter, in integers)."""
    check(g_mod, ctx, *ref.large_dc(g_mod.dist.spectrum_filter))


def test_many_captures(g_mod, ctx):
    """D = 2004 in one call; a spread subset against the restatement."""
    raw, coef, w, decim = ref.many(g_mod.dist.spectrum_filter)
    check(g_mod, ctx, raw, coef, w, decim, rows=ref.MANY_ROWS)


def test_reproducible_across_slots_neighbours_positions_and_batch_sizes(g_mod, ctx):
    """One (capture, w) pair gives the same bits alone, in slot 0 or slot 6, beside other w, and at positions 0 / 3 / last of
    batches of 1, 4 and 37."""
    coef = g_mod.dist.spectrum_filter(FS, 100e3, 0.2)[1]
    n = 30001
    pool = ref.tone_captures(5, n, 13)
    cap, w0 = pool[0], float(ref.phase(56e3))
    others = ref.phase([-244e3, -144e3, -44e3, 156e3, 256e3, 6e3])
    alone = g_mod.subband_power_batch(cap[None], coef, [[w0]], ctx=ctx)[0, 0]
    lit = ref.literal(cap, coef, w0)
    assert abs(alone - lit) <= TOL * lit
    nan = np.nan
    rows = {0: [w0, nan, nan, nan, nan, nan, nan], 6: [nan, nan, nan, nan, nan, nan, w0],
            3: [others[0], others[1], others[2], w0, others[3], others[4], others[5]],
            4: [others[0], nan, others[2], nan, w0, nan, nan]}
    for slot, row in rows.items():
        got = g_mod.subband_power_batch(cap[None], coef, [row], ctx=ctx)
        assert got[0, slot] == alone, (slot, got[0, slot], alone)
    for d in (1, 4, 37):
        for pos in sorted({0, min(3, d - 1), d - 1}):
            raw = np.stack([pool[1 + (i % 4)] for i in range(d)])
            raw[pos] = cap
            w = np.tile(np.array(rows[3]), (d, 1))
            w[::2, 1] = nan                                                      # neighbours differ from capture to capture
            got = g_mod.subband_power_batch(raw, coef, w, ctx=ctx)
            assert got[pos, 3] == alone, (d, pos)
    # and for a decimated, longer-filter geometry
    coef64 = g_mod.dist.spectrum_filter(FS, 50e3, 0.2)[1]
    a = g_mod.subband_power_batch(cap[None], coef64, [[w0]], decim=10, ctx=ctx)[0, 0]
    raw = np.stack([pool[1], pool[2], cap, pool[3]])
    b = g_mod.subband_power_batch(raw, coef64, np.tile(np.array(rows[3]), (4, 1)), decim=10, ctx=ctx)
    assert b[2, 3] == a


def test_planted_emitters_in_a_multichannel_sweep(g_mod, ctx):
    """Synthetic 2-dongle sweep, 935-937.6 MHz at 100 kHz (27 points out of 6 captures): carriers planted 1 kHz off 935.3, 936.4
    and 937.2 MHz -- 935.3 MHz lies 212 kHz below its capture's centre.  shift_sign = -1: the peaks stand at those points.
    shift_sign = +1 (the script's literal line): each stands at the point mirrored about its capture's centre."""
    start, stop, step, obs = 935.0e6, 937.6e6, 100e3, 0.01
    _, coef, _, n = g_mod.dist.spectrum_filter(FS, step, obs)
    plan = g_mod.dist.multichannel_frequency_plan(start, stop, step, FS)
    freq = plan["freq"]
    assert len(freq) == 27 and len(plan["real_freq"]) == 6
    emitters = (935.3e6, 936.4e6, 937.2e6)
    r_all = ref.planted_sweep(plan, n, num_dongle=2, emitters=tuple(e + 1e3 for e in emitters))
    assert r_all.shape == (2 * n, 2, 6)
    home = {e: next(c for c, k in enumerate(plan["freq_set"]) if np.any(np.abs(freq[k] - e) < 1.0)) for e in emitters}
    assert abs(935.3e6 - plan["real_freq"][home[935.3e6]]) > 200e3

    def peaks(ps):
        return sorted(freq[np.argsort(ps)[-3:]].tolist())

    for sign in (-1, +1):
        rec = g_mod.multichannel_spectrum_scan(r_all, start, stop, step, gain=0, observe_time=obs, sample_rate=FS,
                                               shift_sign=sign, ctx=ctx)
        ps = rec["power_spectrum"]
        assert ps.shape == (2, 27) and rec["filename"] == "scan_935000000_937600000_gain0_2dongles.mat"
        assert np.array_equal(rec["power_spectrum_combine"], np.mean(ps, axis=0))          # :227, linear mean over dongles
        for dg in range(2):                                                      # every point against the restatement
            for c, (k, rel) in enumerate(zip(plan["freq_set"], plan["relative_sub_freq_set"])):
                for u, f in zip(k, rel):
                    lit = ref.literal(r_all[:, dg, c], coef, sign * f * 2 * np.pi / FS)
                    assert abs(ps[dg, u] - lit) <= TOL * lit, (sign, dg, u)
        if sign == -1:
            want = sorted(emitters)
        else:                                                                    # the grid point nearest the mirror image
            want = []
            for e in emitters:
                centre = plan["real_freq"][home[e]]
                k = plan["freq_set"][home[e]]
                u = k[np.argmin(np.abs(freq[k] - (2 * centre - (e + 1e3))))]
                assert abs(freq[u] - (2 * centre - (e + 1e3))) < 40e3            # inside the 100 kHz filter around that point
                want.append(float(freq[u]))
            want = sorted(want)
            assert want == [935.7e6, 936.7e6, 936.9e6]
        for dg in range(2):
            assert peaks(ps[dg]) == want, (sign, dg, peaks(ps[dg]))
        assert peaks(rec["power_spectrum_combine"]) == want
        db = 10 * np.log10(rec["power_spectrum_combine"])
        for f in want:
            u = int(np.argmin(np.abs(freq - f)))
            assert db[u] > db[u - 1] + 3 and db[u] > db[u + 1] + 3, (sign, f, db[u - 1:u + 2])


def test_dev_call_with_pinned_output(g_mod, ctx):
    import torch
    coef = g_mod.dist.spectrum_filter(FS, 100e3, 0.2)[1]
    n = 30001
    raw = ref.tone_captures(6, n, 9)
    w = np.tile(ref.W7, (6, 1))
    w[4, 1] = np.nan
    host = g_mod.subband_power_batch(raw, coef, w, ctx=ctx)
    d_raw = torch.from_numpy(raw).to("cuda:0")
    torch.cuda.synchronize()
    out = torch.full((6, 7), -1.0, dtype=torch.float64).pin_memory()
    g_mod.subband_power_batch_dev(d_raw.data_ptr(), 6, n, coef, w, out.data_ptr(), ctx=ctx)
    ctx.sync()
    assert np.array_equal(out.numpy(), host, equal_nan=True)
    dev = torch.full((6, 7), -1.0, dtype=torch.float64, device="cuda:0")
    g_mod.subband_power_batch_dev(d_raw.data_ptr(), 6, n, coef, w, dev.data_ptr(), decim=1, ctx=ctx)
    ctx.sync()
    assert np.array_equal(dev.cpu().numpy(), host, equal_nan=True)


def test_bad_arguments_with_a_context(g_mod, ctx):
    lib = ctx.lib
    raw = np.zeros((2, 64), dtype=np.uint8)
    coef = np.ones(4)
    w = np.zeros((2, 3))
    out = np.zeros((2, 3))
    dp = C.POINTER(C.c_double)
    rp, cp, wp, op = raw.ctypes.data_as(C.POINTER(C.c_uint8)), coef.ctypes.data_as(dp), w.ctypes.data_as(dp), out.ctypes.data_as(dp)
    for d, n, nt, dec, ns in ((0, 32, 4, 1, 3), (2, 0, 4, 1, 3), (2, 32, 0, 1, 3), (2, 32, 129, 1, 3), (2, 32, 4, 0, 3),
                              (2, 32, 4, 1, 0), (2, 32, 4, 1, 17)):
        assert lib.gsmcal_subband_power_batch(ctx.h, rp, d, n, cp, nt, dec, wp, ns, op) == -1
        assert lib.gsmcal_subband_power_batch_dev(ctx.h, C.c_void_p(raw.ctypes.data), d, n, cp, nt, dec, wp, ns, None) == -1
    assert lib.gsmcal_subband_power_batch(ctx.h, rp, 2, 32, cp, 4, 1, None, 3, op) == -1
    w[0, 1] = -np.inf
    assert lib.gsmcal_subband_power_batch(ctx.h, rp, 2, 32, cp, 4, 1, wp, 3, op) == -1
    w[0, 1] = np.nan
    # the context still works afterwards
    got = g_mod.subband_power_batch(raw, coef, w, ctx=ctx)
    assert np.isnan(got[0, 1]) and np.all(got[~np.isnan(w)] == 0.0)


@pytest.mark.parametrize("depth", [1, 2])
def test_calibration_answers_unchanged_by_interleaved_subband_power(g_mod, depth):
    """Two contexts of the same pipeline depth run the same calibrate_batch_dev calls; one has sub-band calls between and behind
    them.  Tables, gsmcal_last_batch_details and gsmcal_last_call_report agree bit for bit, and the sub-band powers with a plain
    call's."""
    import torch
    synth = g_mod.synth
    coef = synth.fir1(46, 200e3 / synth.FS)
    ts = synth.sch_training_sequence()
    fc = 957.4e6
    raw = np.stack([synth.make_stream(dongle=d)[0] for d in (0, 3)])
    d, n = raw.shape[0], raw.shape[1] // 2
    bcoef = g_mod.dist.spectrum_filter(FS, 100e3, 0.2)[1]
    bn = 30001
    braw = ref.tone_captures(3, bn, 17)
    w = np.tile(ref.W7, (3, 1))
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_braw = torch.from_numpy(braw).to("cuda:0")
    torch.cuda.synchronize()

    def run(interleave):
        c = g_mod.Context(0)
        c.set_pipeline_depth(depth)
        tables = [torch.zeros((d, g_mod.TABLE_COLS), dtype=torch.float64, device="cuda:0") for _ in range(3)]
        bouts = [torch.zeros((3, 7), dtype=torch.float64, device="cuda:0") for _ in range(3)]
        for i in range(3):
            g_mod.calibrate_batch_dev(d_raw.data_ptr(), d, n, coef, ts, fc, tables[i].data_ptr(), ctx=c)
            if interleave:
                g_mod.subband_power_batch_dev(d_braw.data_ptr(), 3, bn, bcoef, w, bouts[i].data_ptr(), ctx=c)
        host = g_mod.subband_power_batch(braw, bcoef, w, ctx=c) if interleave else None
        c.sync()
        if interleave:
            for b in bouts:
                assert np.array_equal(b.cpu().numpy(), host, equal_nan=True)
        return [t.cpu().numpy() for t in tables], g_mod.last_batch_details(d, ctx=c), g_mod.last_call_report(ctx=c), host

    t0, det0, rep0, _ = run(False)
    t1, det1, rep1, host = run(True)
    compare(host, ref.table(ref.literal, braw, bcoef, w, 1))
    for i in range(3):
        assert np.array_equal(t1[i], t0[i], equal_nan=True), i
    for k in det0:
        assert np.array_equal(det1[k], det0[k], equal_nan=True), k
    assert rep1 == rep0
