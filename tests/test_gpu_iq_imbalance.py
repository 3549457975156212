"""GPU tests of the I/Q imbalance and clipping check (-m gpu): gsmcal_iq_imbalance_batch[_dev] / gsmcal_IQ_imbalance /
gsmcal_iq_correct (k_iq_moments, k_iq_finish, k_iq_correct) against the restatement in tests/iq_imbalance_ref.py.

Bounds of the raw form (derived, not measured): the integer columns 0-11 and the status are exact integer sums, so they must be
equal bit for bit; dc, var, gain and sin_phase are a few correctly rounded operations on the same integers: 2 ulp; phase_deg, irr_db
and level_dbfs go through the library's asin / log10, which differ by ulps between the host and the device: 1e-12 relative; NaN
and +-Inf in the same places.  Complex form: the five sums within 1e-11 of the sum of |terms| (N*eps at N <= 20 000 is 2e-12; four
times that), the derived columns within 1e-9.  iq_correct: 4 eps (|Q/g| + |I s|)/c per element.

The sizes are where tiling, alignment, chunking and overflow can go wrong: not the workload's sizes."""
import ctypes as C
import math

import numpy as np
import pytest

import iq_imbalance_ref as ref

pytestmark = pytest.mark.gpu

F = ref.F
TILE = ref.TILE
EPS = 2.0 ** -52
SIZES = [1, 2, 3, 7, 8, 9, TILE - 1, TILE, TILE + 1, 2 * TILE + 5]
EXACT = list(range(12)) + [F["status"]]
ULP2 = [F[k] for k in ("dc_I", "dc_Q", "var_I", "var_Q", "gain", "sin_phase")]
REL = [F[k] for k in ("phase_deg", "irr_db", "level_dbfs")]
G, PHI = 1.05, 3.0


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_rows(got, want, what):
    """a table of the raw form against the restatement's rows; returns how many of the 2-ulp columns were NOT bit-equal"""
    got, want = np.atleast_2d(got), np.atleast_2d(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape, what
    assert same_bits(got[:, EXACT], want[:, EXACT]), what
    unequal = 0
    for r in range(len(want)):
        for c in ULP2 + REL:
            a, b = float(got[r, c]), float(want[r, c])
            if math.isnan(b) or math.isinf(b):
                assert same_bits(a, b), (what, r, c, a, b)
            elif c in ULP2:
                u = ref.ulps(a, b)
                unequal += u != 0
                assert u <= 2, (what, r, c, a, b)
            else:
                assert math.isfinite(a) and abs(a - b) <= 1e-12 * abs(b), (what, r, c, a, b)
    return unequal


def captures(g, kind, d, n, seed=0):
    if kind == "random":
        return np.random.default_rng(1000 * n + d + seed).integers(0, 256, size=(d, 2 * n), dtype=np.uint8)
    if kind == "cw":
        return np.stack([g.synth.make_cw(n, iq_gain=G + 0.01 * i, iq_phase_deg=PHI - i, seed=11 + i) for i in range(d)])
    raise ValueError(kind)


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_raw_form_equals_the_restatement(g, ctx, n, d):
    unequal = 0
    for kind in ("random", "cw"):
        raw = captures(g, kind, d, n)
        unequal += check_rows(g.iq_imbalance_batch(raw, ctx=ctx), ref.raw_table(raw), (kind, n, d))
    print("n = %d, d = %d: %d of the 2-ulp columns differ from the restatement in their last bits" % (n, d, unequal))


def test_raw_form_on_a_gsm_capture(g, ctx):
    raw = g.synth.make_stream(num_frames=2, iq_gain=G, iq_phase_deg=PHI)[0][None, :]
    unequal = check_rows(g.iq_imbalance_batch(raw, ctx=ctx), ref.raw_table(raw), "make_stream(num_frames=2)")
    print("make_stream(num_frames=2): %d of the 2-ulp columns differ in their last bits" % unequal)


def dev_table(g, ctx, buf, offset, d, n):
    """iq_imbalance_batch_dev on the bytes `offset` into a device copy of buf"""
    lib, vp = ctx.lib, lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.full((d, g.IQ_COLS), -7.0)
    d_raw, d_out = C.c_void_p(), C.c_void_p()
    ctx.check(lib.gsmcal_dev_alloc(ctx.h, buf.nbytes, C.byref(d_raw)), "gsmcal_dev_alloc")
    ctx.check(lib.gsmcal_dev_alloc(ctx.h, out.nbytes, C.byref(d_out)), "gsmcal_dev_alloc")
    try:
        ctx.check(lib.gsmcal_memcpy_h2d(ctx.h, d_raw, vp(buf), buf.nbytes), "gsmcal_memcpy_h2d")
        g.iq_imbalance_batch_dev(d_raw.value + offset, d, n, d_out.value, ctx=ctx)
        ctx.check(lib.gsmcal_memcpy_d2h(ctx.h, vp(out), d_out, out.nbytes), "gsmcal_memcpy_d2h")
    finally:
        lib.gsmcal_dev_free(ctx.h, d_raw)
        lib.gsmcal_dev_free(ctx.h, d_out)
    return out


@pytest.mark.parametrize("n", [7, 9, TILE + 1, 2 * TILE + 5])
def test_dev_form_two_bytes_into_an_allocation(g, ctx, n):
    raw = captures(g, "random", 3, n, seed=5)
    buf = np.concatenate([np.array([3, 250], dtype=np.uint8), raw.ravel(), np.full(30, 255, dtype=np.uint8)])
    got = dev_table(g, ctx, buf, 2, 3, n)
    assert same_bits(got, g.iq_imbalance_batch(raw, ctx=ctx))                  # the same bits at either alignment
    check_rows(got, ref.raw_table(raw), ("offset 2", n))


def test_flat_rows_in_the_middle_and_any_order(g, ctx):
    n = TILE + 3
    raw = captures(g, "random", 5, n, seed=9)
    raw[1, 0::2] = 77                                                           # a constant I rail
    raw[2] = 0
    raw[3] = 255
    got = g.iq_imbalance_batch(raw, ctx=ctx)
    check_rows(got, ref.raw_table(raw), "flat rows")
    assert list(got[:, F["status"]]) == [0, 2, 2, 2, 0]
    assert got[2, F["clip_I"]] == n and got[3, F["clip_Q"]] == n and got[2, F["level_dbfs"]] == -math.inf
    assert got[1, F["clip_I"]] == 0 and got[1, F["min_I"]] == got[1, F["max_I"]] == 77
    for i in range(5):
        assert same_bits(g.iq_imbalance_batch(raw[i:i + 1], ctx=ctx)[0], got[i]), i
    assert same_bits(g.iq_imbalance_batch(raw[::-1], ctx=ctx)[::-1], got)


def test_overflow_edge_at_two_to_the_23(g, ctx):
    n = g.IQ_MAX_N
    raw = np.empty((1, 2 * n), dtype=np.uint8)
    raw[0, 0::2] = 255
    raw[0, 1::2] = np.tile(np.array([0, 255], dtype=np.uint8), n // 2)
    got = g.iq_imbalance_batch(raw, ctx=ctx)
    check_rows(got, ref.raw_table(raw), "N = 2^23")
    assert got[0, F["S_II"]] == 65025.0 * n and got[0, F["S_QQ"]] == 65025.0 * n / 2 and got[0, F["S_IQ"]] == 65025.0 * n / 2
    assert got[0, F["var_Q"]] == 127.5 ** 2 and got[0, F["var_I"]] == 0.0 and got[0, F["status"]] == g.IQ_FLAT
    assert got[0, F["clip_I"]] == n and got[0, F["clip_Q"]] == n


def test_one_sample_too_many_is_unsupported_and_writes_nothing(g, ctx):
    n = g.IQ_MAX_N + 1
    raw = np.zeros(64, dtype=np.uint8)                                          # (never read: the call is refused on its sizes)
    out = np.full(g.IQ_COLS, -7.0)
    rc = ctx.lib.gsmcal_iq_imbalance_batch(ctx.h, raw.ctypes.data_as(g._lib.c_u8_p), 1, n, out.ctypes.data_as(g._lib.c_double_p))
    assert rc == -6 and np.all(out == -7.0) and "2^23" in ctx.lib.gsmcal_last_error(ctx.h).decode()
    rc = ctx.lib.gsmcal_iq_imbalance_batch_dev(ctx.h, C.c_void_p(raw.ctypes.data), 1, n, C.c_void_p(out.ctypes.data))
    assert rc == -6 and np.all(out == -7.0)
    x = np.zeros(4)
    assert ctx.lib.gsmcal_IQ_imbalance(ctx.h, x.ctypes.data_as(g._lib.c_double_p), n, out.ctypes.data_as(g._lib.c_double_p)) == -6
    assert np.all(out == -7.0)


def test_more_captures_than_one_grid_takes(g, ctx):
    d, n = 65538, 33
    i = np.arange(d, dtype=np.uint64)[:, None]
    j = np.arange(2 * n, dtype=np.uint64)[None, :]
    raw = ((((i + 1) * (j + 3) * np.uint64(2654435761)) >> np.uint64(16)) & np.uint64(255)).astype(np.uint8)
    raw[:, :4] = np.arange(d, dtype=np.uint32).view(np.uint8).reshape(d, 4)   # each capture carries its index
    got = g.iq_imbalance_batch(raw, ctx=ctx)
    a, b = raw[:, 0::2].astype(np.int64), raw[:, 1::2].astype(np.int64)
    clip = lambda x: np.count_nonzero((x == 0) | (x == 255), axis=1)            # noqa: E731
    want = np.stack([np.full(d, n), a.sum(1), b.sum(1), (a * a).sum(1), (b * b).sum(1), (a * b).sum(1), a.min(1), a.max(1),
                     b.min(1), b.max(1), clip(a), clip(b)], axis=1).astype(np.float64)
    assert same_bits(got[:, :12], want)
    assert len(np.unique(got[:, 1:6], axis=0)) > d // 2                         # the captures do have sums of their own
    for r in (0, 1, 65534, 65535, 65536, 65537):                                # the derived columns on both sides of the cut
        check_rows(got[r], [ref.raw_row(raw[r])], ("row", r))
    s_i, s_q = want[:, 1], want[:, 2]
    a_i, a_q = n * want[:, 3] - s_i * s_i, n * want[:, 4] - s_q * s_q           # small integers: exact in fp64
    assert same_bits(got[:, F["var_I"]], a_i / (float(n) * n)) and same_bits(got[:, F["dc_Q"]], s_q / n)
    ok = (a_i > 0) & (a_q > 0)
    assert ok.sum() > d - 10 and same_bits(got[ok, F["gain"]], np.sqrt(a_q[ok] / a_i[ok])) and np.all(got[ok, F["status"]] == 0)


# ---- complex form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 255, 257, TILE + 1, 20000])
def test_complex_form_against_the_numpy_restatement(g, ctx, n):
    raw = g.synth.make_cw(n, iq_gain=G, iq_phase_deg=PHI, seed=3)
    s = np.atleast_1d(g.raw2iq(raw, ctx=ctx)) if n > 1 else np.array([0.25 - 1.5j])
    got, want = g.IQ_imbalance(s, ctx=ctx), ref.complex_row(s)
    scale = ref.abs_term_sums(s)
    assert got[0] == n and got[F["status"]] == want[F["status"]] and np.isnan(got[F["clip_I"]]) and np.isnan(got[F["clip_Q"]])
    for k in range(5):
        assert abs(got[1 + k] - want[1 + k]) <= 1e-11 * scale[k], (k, got[1 + k], want[1 + k])
    assert same_bits(got[6:10], want[6:10])                                    # min / max are selections
    for c in range(12, 21):
        if math.isnan(want[c]):
            assert math.isnan(got[c]), c
        else:
            assert abs(got[c] - want[c]) <= 1e-9 * max(1.0, abs(want[c])), (c, got[c], want[c])
    # bit-identical on a second call and for the same stream at another address
    assert same_bits(g.IQ_imbalance(s, ctx=ctx), got)
    pad = np.concatenate([np.zeros(3, dtype=np.complex128), s])
    assert same_bits(g.IQ_imbalance(pad[3:], ctx=ctx), got)
    if n == 20000:                                                              # ... and it agrees with the exact integer form of the same bytes
        exact = g.iq_imbalance_batch(raw[None, :], ctx=ctx)[0]
        assert abs(got[F["gain"]] - exact[F["gain"]]) <= 1e-9 and abs(got[F["sin_phase"]] - exact[F["sin_phase"]]) <= 1e-9


def test_report_lines(g, ctx):
    s = g.raw2iq(g.synth.make_cw(2048, iq_gain=G, iq_phase_deg=PHI), ctx=ctx)
    row = g.IQ_imbalance(s, ctx=ctx)
    want = "I/Q gain %s phase %s deg image rejection %s dB DC %s\n" % (g.num2str(row[F["gain"]]), g.num2str(row[F["phase_deg"]]),
                                                                     g.num2str(row[F["irr_db"]]), g.num2str(row[F["dc_I"]:F["dc_Q"] + 1]))
    assert g.last_call_report(ctx) == want
    flat = g.IQ_imbalance(np.array([1 + 2j, 1 + 3j, 1 - 1j]), ctx=ctx)
    assert flat[F["status"]] == g.IQ_FLAT and g.last_call_report(ctx) == "I/Q imbalance undefined: constant rail.\n"
    short = g.IQ_imbalance(np.array([1 + 2j]), ctx=ctx)
    assert short[F["status"]] == g.IQ_SHORT and g.last_call_report(ctx) == "I/Q imbalance undefined: fewer than two samples.\n"


# ---- iq_correct --------------------------------------------------------------------------------------------------------------------
def test_iq_correct_against_the_numpy_twin_and_in_place(g, ctx):
    rng = np.random.default_rng(4)
    n, d = 1024 + 37, 3
    s = rng.standard_normal((n, d)) * 50.0 + 1j * rng.standard_normal((n, d)) * 50.0
    gain, sp = np.array([1.05, 0.9, 1.0]), np.array([math.sin(math.radians(3.0)), -0.2, 0.0])
    got = g.iq_correct(s, gain, sp, ctx=ctx)
    assert got.shape == s.shape
    for i in range(d):
        want = ref.correct(s[:, i], gain[i], sp[i])
        c = math.sqrt(1.0 - sp[i] * sp[i])
        bound = 4.0 * EPS * (np.abs(s[:, i].imag / gain[i]) + np.abs(s[:, i].real * sp[i])) / c
        assert same_bits(got[:, i].real, s[:, i].real) and np.all(np.abs(got[:, i].imag - want.imag) <= bound), i
    assert same_bits(got[:, 2].imag, s[:, 2].imag)                             # gain 1, phase 0: nothing changes
    # in place (out == s exactly) gives the bits of out of place
    buf = np.ascontiguousarray(s.T)
    fl = buf.view(np.float64)
    dp = lambda a: a.ctypes.data_as(g._lib.c_double_p)                          # noqa: E731
    ctx.check(ctx.lib.gsmcal_iq_correct(ctx.h, dp(fl), n, d, dp(gain), dp(sp), dp(fl)), "iq_correct")
    assert same_bits(buf.T.real, got.real) and same_bits(buf.T.imag, got.imag)


def test_iq_correct_argument_exits(g, ctx):
    lib, dp = ctx.lib, lambda a: a.ctypes.data_as(g._lib.c_double_p)
    x = np.arange(64, dtype=np.float64)                                         # 32 complex samples
    out = np.full(64, -7.0)
    one, zero = np.array([1.0]), np.array([0.0])
    cases = [(dp(x), 32, 1, dp(np.array([0.0])), dp(zero), dp(out), "gain"), (dp(x), 32, 1, dp(np.array([-1.0])), dp(zero), dp(out), "gain"),
             (dp(x), 32, 1, dp(np.array([math.nan])), dp(zero), dp(out), "gain"), (dp(x), 32, 1, dp(np.array([math.inf])), dp(zero), dp(out), "gain"),
             (dp(x), 32, 1, dp(one), dp(np.array([1.0])), dp(out), "sin_phase"), (dp(x), 32, 1, dp(one), dp(np.array([-1.5])), dp(out), "sin_phase"),
             (dp(x), 32, 1, dp(one), dp(np.array([math.nan])), dp(out), "sin_phase"),
             (dp(x), 0, 1, dp(one), dp(zero), dp(out), "len"), (dp(x), 32, 0, dp(one), dp(zero), dp(out), "d and len"),
             (None, 32, 1, dp(one), dp(zero), dp(out), "NULL"), (dp(x), 32, 1, dp(one), dp(zero), None, "NULL"),
             (dp(x), 32, 1, None, dp(zero), dp(out), "NULL")]
    for s, n, d, gp, sp, o, word in cases:
        assert lib.gsmcal_iq_correct(ctx.h, s, n, d, gp, sp, o) == -1, word
        msg = lib.gsmcal_last_error(ctx.h).decode()
        assert "iq_correct" in msg and word in msg, msg
    assert np.all(out == -7.0)
    # a partial overlap: out starts one sample into s
    both = np.arange(66, dtype=np.float64)
    assert lib.gsmcal_iq_correct(ctx.h, dp(both), 32, 1, dp(one), dp(zero), dp(both[2:])) == -1
    assert "overlap" in lib.gsmcal_last_error(ctx.h).decode() and np.array_equal(both, np.arange(66.0))


def test_round_trip_measure_correct_measure(g, ctx):
    raw = g.synth.make_cw(20000, iq_gain=G, iq_phase_deg=PHI)
    row = g.iq_imbalance_batch(raw[None, :], ctx=ctx)[0]
    assert abs(row[F["gain"]] - G) <= 2e-3 and abs(row[F["phase_deg"]] - PHI) <= 0.02
    fixed = g.iq_correct(g.raw2iq(raw, ctx=ctx), row[F["gain"]], row[F["sin_phase"]], ctx=ctx)
    after = g.IQ_imbalance(fixed, ctx=ctx)
    print("after the correction: gain - 1 = %.3g, sin_phase = %.3g, irr %.1f dB (before: %.1f dB)" %
          (after[F["gain"]] - 1.0, after[F["sin_phase"]], after[F["irr_db"]], row[F["irr_db"]]))
    assert abs(after[F["gain"]] - 1.0) <= 1e-9 and abs(after[F["sin_phase"]]) <= 1e-9


# ---- the boundary ------------------------------------------------------------------------------------------------------------------
def test_batch_forms_reject_bad_arguments_with_a_message(g, ctx):
    lib = ctx.lib
    raw = np.zeros(16, dtype=np.uint8)
    out = np.full(g.IQ_COLS, -7.0)
    u8, dp = raw.ctypes.data_as(g._lib.c_u8_p), out.ctypes.data_as(g._lib.c_double_p)
    for args, word in (((u8, 0, 8, dp), "d must"), ((u8, 1, 0, dp), "n must"), ((None, 1, 8, dp), "NULL"), ((u8, 1, 8, None), "NULL")):
        assert lib.gsmcal_iq_imbalance_batch(ctx.h, *args) == -1, word
        msg = lib.gsmcal_last_error(ctx.h).decode()
        assert "iq_imbalance" in msg and word in msg, msg
    vp = C.c_void_p
    for args, word in (((vp(raw.ctypes.data), 0, 8, vp(out.ctypes.data)), "d must"), ((vp(raw.ctypes.data), 1, -1, vp(out.ctypes.data)), "n must"),
                       ((None, 1, 8, vp(out.ctypes.data)), "NULL"), ((vp(raw.ctypes.data), 1, 8, None), "NULL"),
                       ((vp(raw.ctypes.data + 1), 1, 4, vp(out.ctypes.data)), "aligned")):
        assert lib.gsmcal_iq_imbalance_batch_dev(ctx.h, *args) == -1, word
        assert word in lib.gsmcal_last_error(ctx.h).decode()
    assert lib.gsmcal_IQ_imbalance(ctx.h, out.ctypes.data_as(g._lib.c_double_p), 0, dp) == -1
    assert np.all(out == -7.0)
    with pytest.raises(ValueError):
        g.iq_imbalance_batch(np.zeros((2, 5), dtype=np.uint8), ctx=ctx)


def test_dev_form_behind_calibrate_leaves_its_answers_alone(g, ctx):
    s = g.synth
    coef, ts = s.fir1(46, 200e3 / s.FS), s.sch_training_sequence()
    raw = np.stack([s.make_stream(dongle=d, iq_gain=G, iq_phase_deg=PHI)[0] for d in (0, 3)])
    d, n = raw.shape[0], raw.shape[1] // 2
    lib, vp = ctx.lib, lambda a: a.ctypes.data_as(C.c_void_p)

    def run(with_iq):
        table, iq = np.full((d, g.TABLE_COLS), -7.0), np.full((d, g.IQ_COLS), -7.0)
        ptrs = [C.c_void_p() for _ in range(3)]
        for p, a in zip(ptrs, (raw, table, iq)):
            ctx.check(lib.gsmcal_dev_alloc(ctx.h, a.nbytes, C.byref(p)), "gsmcal_dev_alloc")
            ctx.check(lib.gsmcal_memcpy_h2d(ctx.h, p, vp(a), a.nbytes), "gsmcal_memcpy_h2d")
        try:
            g.calibrate_batch_dev(ptrs[0].value, d, n, coef, ts, 957.4e6, ptrs[1].value, ctx=ctx)
            if with_iq:
                g.iq_imbalance_batch_dev(ptrs[0].value, d, n, ptrs[2].value, ctx=ctx)   # directly behind, no synchronisation in between
            ctx.check(lib.gsmcal_memcpy_d2h(ctx.h, vp(table), ptrs[1], table.nbytes), "gsmcal_memcpy_d2h")
            ctx.check(lib.gsmcal_memcpy_d2h(ctx.h, vp(iq), ptrs[2], iq.nbytes), "gsmcal_memcpy_d2h")
            return table, iq, g.last_batch_details(d, ctx=ctx)
        finally:
            for p in ptrs:
                lib.gsmcal_dev_free(ctx.h, p)
    t0, _, det0 = run(False)
    t1, iq, det1 = run(True)
    assert same_bits(t0, t1) and set(det0) == set(det1)
    for k in det0:
        assert np.array_equal(det0[k], det1[k], equal_nan=True), k
    check_rows(iq, ref.raw_table(raw), "behind calibrate_batch_dev")
    assert np.all(np.abs(iq[:, F["gain"]] - G) <= 0.02) and np.all(np.abs(iq[:, F["phase_deg"]] - PHI) <= 0.5)


def test_ingest_check_front_end_on_a_ring_slot(g, ctx):
    caps = [g.synth.make_cw(5000, iq_gain=G, iq_phase_deg=PHI), g.synth.make_cw(5000, amp=140.0, seed=2)]   # the second one clips
    want = g.iq_rows(g.iq_imbalance_batch(np.stack(caps), ctx=ctx))
    ring = g.ingest.Ring(ctx, 2 * len(caps[0]), slots=2)
    try:
        host = ring.host(1)
        host[:len(caps[0])] = caps[0]                                          # two dongles' worth of bytes, dongle-major
        host[len(caps[0]):] = caps[1]
        ring.submit(1)
        rows = g.ingest.check_front_end(ring, 1, 2, 5000, ctx=ctx)
    finally:
        ring.close()
    assert rows == want and rows[0]["clip_I"] == 0 and rows[1]["clip_I"] > 100 and rows[1]["max_Q"] == 255
    check_rows(g.iq_imbalance_batch(np.stack(caps), ctx=ctx), ref.raw_table(np.stack(caps)), "ring slot")
