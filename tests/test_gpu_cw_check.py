"""GPU tests of the CW sample-loss check (-m gpu): gsmcal_CW_check / gsmcal_cw_check_batch[_dev] (k_cw_ratio_sum,
k_cw_finish_mean, k_cw_residual, k_cw_finish_summary) against the numpy restatement of CW_check.m:6-8 in tests/cw_check_ref.py.

Bound: every r_n, phase_rotate, the maximum and the event values within 1e-10 rad ABSOLUTE; the count, the event indices and
the index of the maximum identical.  1e-10 is derived, not measured: a sum of N-1 <= 409 599 terms of modulus ~1 in any order
errs by at most (N-1)*2^-53 ~ 4.5e-11 relative, with |mean q| >= 0.5 that is < 1e-10 rad on phase_rotate; the division and
atan2 add a few 1e-16.  (tests/test_gpu_spectrum.py and test_gpu_subband.py use the same figure for fp64 restatement parity.)
tests/test_cw_check_cpu.py asserts, for every input used here, the margins that keep the exact comparisons clear of the last
bits: no |r_n| within 1e-3 of thr, no angle within 1e-3 of pi, the maximum 1e-3 ahead of the runner-up.

A byte capture of N = 2 is not among the cases: raw2iq makes s(2) = -s(1) exactly, its one ratio is -1, on atan2's branch
cut.  The one-ratio case is a complex pair handed to CW_check (cw_check_ref.S_N2)."""
import ctypes as C

import numpy as np
import pytest

import cw_check_ref as ref

pytestmark = pytest.mark.gpu

THR = ref.THR
TOL = 1e-10


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_row(g, row, r_got, name, thr=THR):
    """one summary row (and the residuals, when asked for) against the restatement of case `name`; returns the largest deviation"""
    _, r, pr = ref.reference(name)
    want = ref.summary(r, thr)
    got = g.cw_rows(row)[0]
    worst = abs(got["phase_rotate"] - pr)
    if r_got is not None:
        assert r_got.shape == r.shape
        worst = max(worst, float(np.max(np.abs(r_got - r))))
    listed = want["events"][:g.CW_MAX_EVENTS]
    assert got["status"] == g.CW_OK and got["count"] == want["count"] and got["max_n"] == want["max_n"]
    assert [n for n, _ in got["events"]] == [n for n, _ in listed]
    worst = max([worst, abs(got["max_abs"] - want["max_abs"])] + [abs(a[1] - b[1]) for a, b in zip(got["events"], listed)])
    print("%s: largest deviation from the numpy restatement %.3g rad, count %d" % (name, worst, got["count"]))
    assert worst <= TOL
    assert np.all(np.isnan(row[5 + 2 * len(listed):]))                    # unused slots
    return got


@pytest.fixture(scope="module")
def batch_small(g, ctx):
    """the cases of N = 4 099 in one batch, summary and residuals: computed once, shared, read-only"""
    names = ["small", "dense"]
    summ, r = g.cw_check_batch(np.stack([ref.raw(k) for k in names]), THR, want_r=True, ctx=ctx)
    summ.setflags(write=False)
    r.setflags(write=False)
    return names, summ, r


@pytest.mark.parametrize("name", ["clean", "drops"])
def test_parity_full_length_captures(g, ctx, name):
    summ, r = g.cw_check_batch(ref.raw(name)[None, :], THR, want_r=True, ctx=ctx)
    got = check_row(g, summ[0], r[0], name)
    assert [n for n, _ in got["events"]] == sorted(ref.planted(name))


def test_parity_small_and_dense(g, batch_small):
    names, summ, r = batch_small
    small = check_row(g, summ[0], r[0], "small")
    assert [n for n, _ in small["events"]] == [1, 256, 257, 4098] and max(abs(v) for _, v in small["events"]) > np.pi   # not wrapped
    dense = check_row(g, summ[1], r[1], "dense")
    # about 67 events at lane and block positions no power-of-two tiling aligns with: the count goes on past the list, the
    # first 16 are listed in order and none is skipped at a tile seam
    assert dense["count"] == 67 > g.CW_MAX_EVENTS == len(dense["events"])
    assert [n for n, _ in dense["events"]] == sorted(ref.planted("dense"))[:16]
    assert np.flatnonzero(np.abs(r[1]) > THR).tolist() == [n - 1 for n in sorted(ref.planted("dense"))]


def test_one_ratio(g, ctx):
    r = g.CW_check(ref.S_N2, ctx=ctx)
    assert r.shape == (1,) and abs(r[0]) <= TOL
    pr = C.c_double()
    buf = np.ascontiguousarray(ref.S_N2)
    out = np.empty(1)
    ctx.check(ctx.lib.gsmcal_CW_check(ctx.h, buf.view(np.float64).ctypes.data_as(g._lib.c_double_p), 2,
                                      out.ctypes.data_as(g._lib.c_double_p), C.byref(pr)), "CW_check")
    assert abs(pr.value - ref.numpy_form(ref.S_N2)[1]) <= TOL and same_bits(out, r)


def test_too_short_capture_is_status_1(g, ctx):
    both = g.cw_check_batch(np.array([[130, 120]], dtype=np.uint8), THR, ctx=ctx)
    summ, r = g.cw_check_batch(np.array([[130, 120]], dtype=np.uint8), THR, want_r=True, ctx=ctx)
    assert same_bits(both, summ) and r.shape == (1, 0)
    row = summ[0]
    assert row[4] == g.CW_SHORT and row[1] == 0.0 and np.all(np.isnan(np.delete(row, [1, 4])))


@pytest.mark.parametrize("name", sorted(ref.SHAPES))
def test_smallest_shapes_and_tile_seams(g, ctx, name):
    key = "tiny" if name == "n3" else name
    summ, r = g.cw_check_batch(ref.raw(key)[None, :], THR, want_r=True, ctx=ctx)
    got = check_row(g, summ[0], r[0], key)
    n = ref.ALL[key]["n"]
    assert r.shape == (1, n - 1)
    if name != "n3":                                                       # a drop at n = 1 and one at the last ratio, n = N-1
        assert [e[0] for e in got["events"]] == [1, n - 1] and got["max_n"] == n - 1
        assert n - 1 in (ref.TILE - 1, ref.TILE, ref.TILE + 1, 2 * ref.TILE + 1)


def test_summary_only_equals_summary_with_r_and_CW_check_of_raw2iq(g, ctx, batch_small):
    names, summ, r = batch_small
    raw = np.stack([ref.raw(k) for k in names])
    assert same_bits(g.cw_check_batch(raw, THR, ctx=ctx), summ)
    for i, k in enumerate(names):
        s = g.raw2iq(ref.raw(k), ctx=ctx)
        assert same_bits(g.CW_check(s, ctx=ctx), r[i]), k


def nan_row_ok(g, row):
    return row[4] == g.CW_ZERO and row[1] == 0.0 and bool(np.all(np.isnan(np.delete(row, [1, 4]))))


def test_zero_sample_is_status_2_and_leaves_the_neighbour_alone(g, ctx):
    iq = np.empty(8, dtype=np.uint8)
    iq[0::2], iq[1::2] = [10, 30, 20, 20], [4, 8, 6, 6]                    # samples 3 and 4 equal the mean
    normal = ref.raw("tiny")
    pad = np.concatenate([normal, [128, 127]]).astype(np.uint8)            # a 4-sample neighbour with other content
    alone, r_alone = g.cw_check_batch(pad[None, :], THR, want_r=True, ctx=ctx)
    summ, r = g.cw_check_batch(np.stack([iq, pad, np.full(8, 77, dtype=np.uint8)]), THR, want_r=True, ctx=ctx)
    assert nan_row_ok(g, summ[0]) and np.all(np.isnan(r[0]))
    assert nan_row_ok(g, summ[2]) and np.all(np.isnan(r[2]))               # a constant capture
    assert summ[1][4] == g.CW_OK and same_bits(summ[1], alone[0]) and same_bits(r[1], r_alone[0])
    const = g.cw_check_batch(np.full((1, 2 * 5000), 9, dtype=np.uint8), THR, ctx=ctx)   # ... of more than one tile
    assert nan_row_ok(g, const[0])


def test_reproducible_at_any_position_in_batches_of_any_size(g, ctx, batch_small):
    names, summ, r = batch_small
    cap = ref.raw("small")
    n = len(cap) // 2
    rng = np.random.default_rng(7)
    alone_s, alone_r = g.cw_check_batch(cap[None, :], THR, want_r=True, ctx=ctx)
    assert same_bits(alone_s[0], summ[0]) and same_bits(alone_r[0], r[0])
    for d, positions in ((4, (0, 3)), (37, (0, 3, 36))):
        for pos in positions:
            raw = rng.integers(90, 166, size=(d, 2 * n), dtype=np.uint8)   # neighbours with other content, the same N
            raw[pos] = cap
            bs, br = g.cw_check_batch(raw, THR, want_r=True, ctx=ctx)
            assert same_bits(bs[pos], summ[0]) and same_bits(br[pos], r[0]), (d, pos)
    # r_stride > n-1: the same bits, and the padding is not written
    stride = n - 1 + 13
    raw2 = np.stack([cap, ref.raw("dense")])
    hr, hs = np.full((2, stride), -7.0), np.full((2, g.CW_COLS), -7.0)
    lib, vp = ctx.lib, lambda a: a.ctypes.data_as(C.c_void_p)
    d_raw, d_r, d_s = C.c_void_p(), C.c_void_p(), C.c_void_p()
    for ptr, a in ((d_raw, raw2), (d_r, hr), (d_s, hs)):
        ctx.check(lib.gsmcal_dev_alloc(ctx.h, a.nbytes, C.byref(ptr)), "gsmcal_dev_alloc")
        ctx.check(lib.gsmcal_memcpy_h2d(ctx.h, ptr, vp(a), a.nbytes), "gsmcal_memcpy_h2d")
    try:
        g.cw_check_batch_dev(d_raw.value, 2, n, THR, d_s.value, d_r.value, stride, ctx=ctx)
        ctx.check(lib.gsmcal_memcpy_d2h(ctx.h, vp(hr), d_r, hr.nbytes), "gsmcal_memcpy_d2h")
        ctx.check(lib.gsmcal_memcpy_d2h(ctx.h, vp(hs), d_s, hs.nbytes), "gsmcal_memcpy_d2h")
    finally:
        for ptr in (d_raw, d_r, d_s):
            lib.gsmcal_dev_free(ctx.h, ptr)
    assert same_bits(hs, summ) and same_bits(hr[:, :n - 1], r) and np.all(hr[:, n - 1:] == -7.0)


def test_no_side_effects_on_the_calibration_answers(g, ctx):
    s = g.synth
    coef, ts = s.fir1(46, 200e3 / s.FS), s.sch_training_sequence()
    raw = np.stack([s.make_stream(dongle=d)[0] for d in (0, 3)])
    g.calibrate_batch(raw, coef, ts, 957.4e6, ctx=ctx)
    before = g.last_batch_details(2, ctx=ctx)
    g.cw_check_batch(np.stack([ref.raw("small"), ref.raw("dense")]), THR, want_r=True, ctx=ctx)
    after = g.last_batch_details(2, ctx=ctx)
    assert set(before) == set(after)
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k


@pytest.mark.parametrize("thr, d", [(0.0, 1), (-0.2, 1), (float("nan"), 1), (float("inf"), 1), (THR, 0)])
def test_errors_are_rejected_with_a_message(g, ctx, thr, d):
    raw = np.ascontiguousarray(ref.raw("tiny"))
    out = np.full(g.CW_COLS, -7.0)
    rc = ctx.lib.gsmcal_cw_check_batch(ctx.h, raw.ctypes.data_as(g._lib.c_u8_p), d, 3, thr, out.ctypes.data_as(g._lib.c_double_p), None, 0)
    assert rc == -1 and np.all(out == -7.0)
    msg = ctx.lib.gsmcal_last_error(ctx.h).decode()
    assert "cw_check" in msg and ("thr" in msg if d else "d must" in msg), msg
    if d:
        with pytest.raises(g.GsmcalError, match="thr must be finite"):
            g.cw_check_batch(raw[None, :], thr, ctx=ctx)


def test_ingest_check_sample_loss_on_a_ring_slot(g, ctx):
    cap = ref.raw("drops")
    n = len(cap) // 2
    want = g.cw_rows(g.cw_check_batch(np.stack([cap, cap]), THR, ctx=ctx))
    ring = g.ingest.Ring(ctx, 2 * len(cap), slots=2)
    try:
        host = ring.host(1)
        host[:len(cap)] = cap                                              # two dongles' worth of bytes, dongle-major
        host[len(cap):] = cap
        ring.submit(1)
        rows = g.ingest.check_sample_loss(ring, 1, 2, n, THR, ctx=ctx)
    finally:
        ring.close()
    assert rows == want and [e[0] for e in rows[1]["events"]] == sorted(ref.planted("drops"))
