"""GPU tests of gsmcal_band_power_batch[_dev] (-m gpu): the band power of multi_rtl_sdr_split_scanner.m:154-156 /
multi_rtl_sdr_diversity_scanner.m:156-158 / scan_band_power_spectrum.m:80-84 against the fp64 restatement
mean(abs(oracle.matlab_filter(coef, oracle.raw2iq(a))[::decim])**2): relative 1e-10, exactly 0 where the restatement is
exactly 0, bit-identical across runs, batch positions and batch sizes."""
import ctypes as C

import numpy as np
import pytest

from oracle import gsmcal_oracle as o

import gsmcal.dist  # noqa: F401

pytestmark = pytest.mark.gpu

FS = 2.048e6


def restate(a, coef, decim):
    y = o.matlab_filter(np.asarray(coef, dtype=np.float64), o.raw2iq(np.asarray(a, dtype=np.float64)))
    return float(np.mean(np.abs(y[::decim]) ** 2))


def tone_captures(d, n, seed, dc=(127.5, 127.5), amp=40.0, noise=3.0):
    """d captures of n samples: a tone at a random offset plus Gaussian noise around `dc`, rounded and clipped to bytes."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    out = np.empty((d, 2 * n), dtype=np.uint8)
    for i in range(d):
        f = rng.uniform(-0.5, 0.5)
        ph = 2 * np.pi * f * k + rng.uniform(0, 2 * np.pi)
        out[i, 0::2] = np.clip(np.rint(dc[0] + amp * np.cos(ph) + noise * rng.standard_normal(n)), 0, 255)
        out[i, 1::2] = np.clip(np.rint(dc[1] + amp * np.sin(ph) + noise * rng.standard_normal(n)), 0, 255)
    return out


def check(g, raw, coef, decim, ctx, idx=None, tol=1e-10):
    got = g.band_power_batch(raw, coef, decim, ctx=ctx)
    assert got.shape == (raw.shape[0],)
    for i in (range(raw.shape[0]) if idx is None else idx):
        ref = restate(raw[i], coef, decim)
        if ref == 0.0:
            assert got[i] == 0.0, (i, got[i])
        else:
            assert abs(got[i] - ref) <= tol * ref, (i, got[i], ref)
    return got


def test_reference_defaults(g_mod, ctx):
    """GSM-900 at 50 kHz: fir1(63) (64 symmetric taps), decimation 20, 204 800 samples per capture."""
    _, coef, decim, n = g_mod.dist.spectrum_filter(FS, 50e3, 0.1)
    assert (len(coef), decim, n) == (64, 20, 204800)
    raw = tone_captures(5, n, 1)
    got = check(g_mod, raw, coef, decim, ctx)
    assert np.array_equal(got, g_mod.band_power_batch(raw, coef, decim, ctx=ctx))      # bit-identical run to run


@pytest.mark.parametrize("case", ["128/102", "32/5", "32/1", "coef=[1]", "asym33/7", "asym200/3", "odd_n", "n_not_mult",
                                  "n_lt_ntaps", "d1", "asym1024/600", "long_decim"])
def test_cases(g_mod, ctx, case):
    rng = np.random.default_rng(sum(map(ord, case)))
    d, n = 4, 30001
    if case == "128/102":
        _, coef, decim, _ = g_mod.dist.spectrum_filter(FS, 10e3, 0.1)
    elif case == "32/5":
        _, coef, decim, _ = g_mod.dist.spectrum_filter(FS, 200e3, 0.1)
    elif case == "32/1":
        _, coef, decim, _ = g_mod.dist.spectrum_filter(FS, 1e6, 0.1)
    elif case == "coef=[1]":
        coef, decim = np.array([1.0]), 1
    elif case.startswith("asym"):
        nt, decim = (int(v) for v in case[4:].split("/"))
        coef = rng.standard_normal(nt)
    elif case == "odd_n":
        _, coef, decim, _ = g_mod.dist.spectrum_filter(FS, 50e3, 0.1)
        n = 20481
    elif case == "n_not_mult":
        _, coef, decim, _ = g_mod.dist.spectrum_filter(FS, 10e3, 0.1)
        n = 102 * 200 + 37
    elif case == "n_lt_ntaps":
        _, coef, decim, _ = g_mod.dist.spectrum_filter(FS, 10e3, 0.1)
        n = 77
    elif case == "d1":
        _, coef, decim, _ = g_mod.dist.spectrum_filter(FS, 50e3, 0.1)
        d = 1
    elif case == "long_decim":
        coef, decim = g_mod.synth.fir1(63, 0.01), 40000
        n = 200001
    if case == "coef=[1]" or case == "32/1":
        assert decim == 1
    raw = tone_captures(d, n, 7)
    check(g_mod, raw, coef, decim, ctx)


def test_many_captures(g_mod, ctx):
    """D = 2004 (four dongles x 501 points) in one call; a spread subset against the restatement."""
    _, coef, decim, _ = g_mod.dist.spectrum_filter(FS, 50e3, 0.1)
    n = 4000
    raw = tone_captures(2004, n, 11)
    check(g_mod, raw, coef, decim, ctx, idx=[0, 1, 500, 1001, 1500, 2002, 2003])


@pytest.mark.parametrize("val", [(0, 0), (255, 255), (17, 200), (128, 3)])
def test_constant_captures_give_exact_zero(g_mod, ctx, val):
    n = 20480
    raw = np.empty((3, 2 * n), dtype=np.uint8)
    raw[:, 0::2], raw[:, 1::2] = val
    for coef, decim in ((g_mod.dist.spectrum_filter(FS, 50e3, 0.1)[1], 20), (np.array([1.0]), 1),
                        (np.random.default_rng(0).standard_normal(45), 3)):
        got = g_mod.band_power_batch(raw, coef, decim, ctx=ctx)
        assert np.all(got == 0.0), got
        assert restate(raw[0], coef, decim) == 0.0


def test_large_dc_with_weak_tone(g_mod, ctx):
    """DC at the rails, a tone of a byte or two: no cancellation (the DC is removed before the filter, in integers)."""
    _, coef, decim, n = g_mod.dist.spectrum_filter(FS, 50e3, 0.1)
    for dc in ((252.0, 3.0), (3.0, 251.0), (250.0, 250.0)):
        raw = tone_captures(2, n, 5, dc=dc, amp=1.5, noise=0.4)
        check(g_mod, raw, coef, decim, ctx)


def test_planted_emitters_in_a_split_sweep(g_mod, ctx):
    """Synthetic split sweep (2 dongles, 935-936.5 MHz at 50 kHz): carriers planted 1 kHz off grid points (a carrier exactly
    on the tuned frequency is DC, which raw2iq removes) show as peaks there; one step away the power is ~14 dB down and two
    steps ~48 dB down (the 64-tap fir1 at 50 kHz)."""
    start, stop, step, nd, obs = 935.0e6, 936.5e6, 50e3, 2, 0.01
    _, coef, decim, n = g_mod.dist.spectrum_filter(FS, step, obs)
    freq, _ = g_mod.dist.scan_frequency_plan(start, stop, step, nd)
    units = freq.ravel()                                           # unit order of s_all
    emitters = [935.3e6, 936.1e6]
    rng = np.random.default_rng(21)
    k = np.arange(n)
    s_all = np.empty((2 * n, units.size), dtype=np.uint8)
    for u, f in enumerate(units):
        i = np.full(n, 127.5) + 0.3 * rng.standard_normal(n)
        q = np.full(n, 127.5) + 0.3 * rng.standard_normal(n)
        for e in emitters:
            ph = 2 * np.pi * (e + 1e3 - f) / FS * k + rng.uniform(0, 2 * np.pi)   # 1 kHz off the point: not DC
            i += 60 * np.cos(ph)
            q += 60 * np.sin(ph)
        s_all[0::2, u] = np.clip(np.rint(i), 0, 255)
        s_all[1::2, u] = np.clip(np.rint(q), 0, 255)
    rec = g_mod.split_spectrum_scan(s_all, start, stop, step, nd, gain=0, observe_time=obs, sample_rate=FS, ctx=ctx)
    ps = rec["power_spectrum"]
    assert rec["filename"] == "split_scan_935000000_936500000_gain0_2dongles.mat"
    for u in range(units.size):
        ref = restate(s_all[:, u], coef, decim)
        assert abs(ps[u] - ref) <= 1e-10 * ref
    db = 10 * np.log10(ps)
    for e in emitters:
        u = int(np.argmin(np.abs(units - e)))
        assert abs(units[u] - e) < 1.0
        for v in (u - 1, u + 1):
            assert 11.0 < db[u] - db[v] < 17.0, (e, db[u] - db[v])
        for v in (u - 2, u + 2):
            assert 42.0 < db[u] - db[v] < 56.0, (e, db[u] - db[v])
    peaks = [u for u in range(1, units.size - 1) if db[u] > db[u - 1] and db[u] > db[u + 1] and db[u] > db.max() - 6]
    assert sorted(units[peaks].tolist()) == emitters


def test_diversity_scan_combines_dongles(g_mod, ctx):
    start, stop, step, obs = 935.0e6, 935.5e6, 50e3, 0.01
    _, coef, decim, n = g_mod.dist.spectrum_filter(FS, step, obs)
    nf, ndg = 11, 3
    s_all = np.stack([tone_captures(nf, n, 30 + i).T for i in range(ndg)], axis=2)      # (2N, length(freq), num_dongle)
    rec = g_mod.diversity_spectrum_scan(s_all, start, stop, step, gain=0, observe_time=obs, sample_rate=FS, ctx=ctx)
    assert rec["power_spectrum"].shape == (ndg, nf)
    for i in range(ndg):
        for j in (0, 5, 10):
            ref = restate(s_all[:, j, i], coef, decim)
            assert abs(rec["power_spectrum"][i, j] - ref) <= 1e-10 * ref
    assert np.array_equal(rec["power_spectrum_combine"], np.mean(rec["power_spectrum"], axis=0))


def test_dev_call_with_pinned_output(g_mod, ctx):
    import torch
    _, coef, decim, n = g_mod.dist.spectrum_filter(FS, 50e3, 0.1)
    raw = tone_captures(6, n, 9)
    host = g_mod.band_power_batch(raw, coef, decim, ctx=ctx)
    d_raw = torch.from_numpy(raw).to("cuda:0")
    torch.cuda.synchronize()
    out = torch.full((6,), -1.0, dtype=torch.float64).pin_memory()
    g_mod.band_power_batch_dev(d_raw.data_ptr(), 6, n, coef, decim, out.data_ptr(), ctx=ctx)
    ctx.sync()
    assert np.array_equal(out.numpy(), host)
    dev = torch.full((6,), -1.0, dtype=torch.float64, device="cuda:0")
    g_mod.band_power_batch_dev(d_raw.data_ptr(), 6, n, coef, decim, dev.data_ptr(), ctx=ctx)
    ctx.sync()
    assert np.array_equal(dev.cpu().numpy(), host)


def test_reproducible_across_positions_and_batch_sizes(g_mod, ctx):
    """A capture gives the same bits alone, at any position, in batches that span several Infinity-Cache chunks."""
    _, coef, decim, n = g_mod.dist.spectrum_filter(FS, 50e3, 0.1)
    base = tone_captures(3, n, 13)
    d = 700                                                         # 287 MB of raw bytes: more than one chunk
    big = np.empty((d, 2 * n), dtype=np.uint8)
    for u in range(d):
        big[u] = np.roll(base[u % 3], 2 * (u // 3))
    p_big = g_mod.band_power_batch(big, coef, decim, ctx=ctx)
    for u in (0, 1, 2, 331, 332, 698, 699):
        alone = g_mod.band_power_batch(big[u:u + 1], coef, decim, ctx=ctx)
        assert alone[0] == p_big[u], u
    p_mid = g_mod.band_power_batch(big[300:350], coef, decim, ctx=ctx)
    assert np.array_equal(p_mid, p_big[300:350])
    ref = restate(big[699], coef, decim)
    assert abs(p_big[699] - ref) <= 1e-10 * ref


def test_bad_arguments_with_a_context(g_mod, ctx):
    lib = ctx.lib
    raw = np.zeros((2, 64), dtype=np.uint8)
    coef = np.ones(4)
    out = np.zeros(2)
    rp, cp, op = raw.ctypes.data_as(C.POINTER(C.c_uint8)), coef.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double))
    for d, n, nt, dec in ((0, 32, 4, 2), (2, 0, 4, 2), (2, 32, 0, 2), (2, 32, 1025, 2), (2, 32, 4, 0)):
        assert lib.gsmcal_band_power_batch(ctx.h, rp, d, n, cp, nt, dec, op) == -1
        assert lib.gsmcal_band_power_batch_dev(ctx.h, C.c_void_p(raw.ctypes.data), d, n, cp, nt, dec, None) == -1
    assert lib.gsmcal_band_power_batch(ctx.h, None, 2, 32, cp, 4, 2, op) == -1
    assert lib.gsmcal_band_power_batch(ctx.h, rp, 2, 32, None, 4, 2, op) == -1
    assert lib.gsmcal_band_power_batch(ctx.h, rp, 2, 32, cp, 4, 2, None) == -1
    # the context still works afterwards
    assert np.all(g_mod.band_power_batch(raw, coef, 2, ctx=ctx) == 0.0)


def test_calibration_answers_unchanged_by_interleaved_band_power(g_mod):
    """Two depth-4 contexts run the same calibrate_batch_dev calls (in flight); one has band-power calls between them.  Tables,
    gsmcal_last_batch_details and gsmcal_last_batch_snr agree bit for bit, and so do the band powers with a plain call's."""
    import torch
    synth = g_mod.synth
    coef = synth.fir1(46, 200e3 / synth.FS)
    ts = synth.sch_training_sequence()
    fc = 957.4e6
    raw = np.stack([synth.make_stream(dongle=d)[0] for d in (0, 1, 3)])
    d, n = raw.shape[0], raw.shape[1] // 2
    _, bcoef, bdecim, _ = g_mod.dist.spectrum_filter(FS, 50e3, 0.1)
    braw = tone_captures(3, 204800, 17)
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_braw = torch.from_numpy(braw).to("cuda:0")
    torch.cuda.synchronize()

    def run(interleave):
        c = g_mod.Context(0)
        c.set_pipeline_depth(4)
        bref = g_mod.band_power_batch(braw, bcoef, bdecim, ctx=c)
        tables = [torch.zeros((d, g_mod.TABLE_COLS), dtype=torch.float64, device="cuda:0") for _ in range(5)]
        bouts = [torch.zeros(3, dtype=torch.float64, device="cuda:0") for _ in range(5)]
        for i in range(5):
            g_mod.calibrate_batch_dev(d_raw.data_ptr(), d, n, coef, ts, fc, tables[i].data_ptr(), ctx=c)
            if interleave and i % 2 == 0:
                g_mod.band_power_batch_dev(d_braw.data_ptr(), 3, 204800, bcoef, bdecim, bouts[i].data_ptr(), ctx=c)
        if interleave:
            assert np.array_equal(g_mod.band_power_batch(braw, bcoef, bdecim, ctx=c), bref)
        c.sync()
        if interleave:
            for i in range(0, 5, 2):
                assert np.array_equal(bouts[i].cpu().numpy(), bref), i
        try:
            snr = g_mod.last_batch_snr(1, ctx=c)
        except g_mod.GsmcalError as e:          # (calls in flight keep no SNR table: the same refusal either way)
            snr = (str(e), None)
        return ([t.cpu().numpy() for t in tables], g_mod.last_batch_details(d, ctx=c), snr, bref)

    t0, det0, snr0, b0 = run(False)
    t1, det1, snr1, b1 = run(True)
    assert np.array_equal(b0, b1)
    for i in range(5):
        assert np.array_equal(t1[i], t0[i]), i
    for k in det0:
        assert np.array_equal(det1[k], det0[k]), k
    assert (snr1[0] == snr0[0]) if isinstance(snr0[0], str) else np.array_equal(snr1[0], snr0[0])
    assert snr1[1] == snr0[1]
