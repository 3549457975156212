"""GPU tests of apply_calibration (-m gpu): gsmcal_apply_calibration_batch[_resident] (k_apply_calibration, k_apply_info) against
the fp64 restatement of the definition in tests/apply_ref.py, the bit equalities include/gsmcal.h promises, the discipline of
DESIGN.md section 22 for this entry (extents, guard bands, call history, refusals), and the closed loop calibrate -> apply_params
-> apply_calibration on the device.

Bounds against the restatement, with their origin (tests/apply_ref.py):
  statuses, first_valid, end_valid, num_valid, which samples are zero      identical (x is formed by the same individually rounded
                       operations on both sides, so floor(x) is the same number)
  each valid sample    SAMPLE_TOL = 1e-11 * |scale| sum_k |h_k| (|Re z_k| + |Im z_k|), the bound DESIGN 20 uses
  identity row         IDENTITY_TOL = 1e-15 * the same sum: mu = 0 selects the sample itself
  residual tone of the closed loop    TONE_BAR_HZ around the residual the table's own error predicts
Before comparing, every case asserts on the restatement that no x sits within 1e-9 of an integer but where x is formed exactly
(apply_ref.positions).  Largest deviation / bound seen on an MI355X: see DESIGN.md section 23."""
import ctypes as C

import numpy as np
import pytest

import apply_ref as ar

pytestmark = pytest.mark.gpu

SENT = -7.25                                                       # the sentinel of every output buffer
worst = {}


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


def same_bits(a, b):
    a, b = (np.ascontiguousarray(v).view(np.float64).view(np.uint64) if np.iscomplexobj(v) else np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
            for v in (a, b))
    return a.shape == b.shape and np.array_equal(a, b)


def compare(out, info, want, what, tol=ar.SAMPLE_TOL):
    assert ar.x_is_safe(want), (what, "an x within 1e-9 of an integer")
    assert np.array_equal(info, want["info"]), (what, info, want["info"])
    sc = want["scale"]
    assert out.shape == want["out"].shape, (what, out.shape)
    assert np.array_equal(out == 0, sc == 0) and np.array_equal(want["out"] == 0, sc == 0), (what, "which samples are exactly zero")
    assert same_bits(out[sc == 0], np.zeros(int((sc == 0).sum()), dtype=np.complex128)), (what, "zeros are +0 + 0j")
    dev = np.abs(out - want["out"])
    m = sc > 0
    ratio = float(np.max(dev[m] / (tol * sc[m]))) if m.any() else 0.0
    worst["sample"] = max(worst.get("sample", 0.0), ratio)
    assert np.all(dev <= tol * sc), (what, ratio)


class Resident:
    """One call of the resident form with every buffer between guard bands: raw with 6 bytes in front (an even number keeps the
    2-byte alignment) and 7 behind, out and info with `pad` sentinel values in front and behind, the tail of every output row at
    the sentinel too."""

    def __init__(self, g, ctx, raw, fs, params, out_len, out_stride=None, pad=9):
        import torch
        self.g, self.ctx, self.fs, self.params, self.out_len = g, ctx, fs, np.asarray(params, dtype=np.float64), int(out_len)
        self.raw = np.ascontiguousarray(np.atleast_2d(raw), dtype=np.uint8)
        self.d, self.n = self.raw.shape[0], self.raw.shape[1] // 2
        self.stride = self.out_len + 5 if out_stride is None else int(out_stride)
        self.pad, self.front = pad, 6
        buf = np.full(self.front + self.raw.size + 7, 0xA5, dtype=np.uint8)
        buf[self.front:self.front + self.raw.size] = self.raw.ravel()
        self.raw_all = buf
        self.d_raw = torch.from_numpy(buf).to("cuda:0")
        self.d_out = torch.full((2 * (2 * pad + self.d * max(self.stride, 1)),), SENT, dtype=torch.float64, device="cuda:0")
        self.d_info = torch.full((2 * pad + self.d * g.APPLY_INFO_COLS,), SENT, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()

    def call(self, **kw):
        a = dict(d_raw=self.d_raw.data_ptr() + self.front, d=self.d, n=self.n, params=self.params, fs=self.fs, out_len=self.out_len,
                 out_stride=self.stride, d_out=self.d_out.data_ptr() + 16 * self.pad, d_info=self.d_info.data_ptr() + 8 * self.pad)
        a.update(kw)
        pr = np.ascontiguousarray(a["params"], dtype=np.float64)
        rc = self.ctx.lib.gsmcal_apply_calibration_batch_resident(
            self.ctx.h, C.c_void_p(a["d_raw"]), int(a["d"]), int(a["n"]), float(a["fs"]),
            pr.ctypes.data_as(self.g._lib.c_double_p) if a["params"] is not None else None, int(a["out_len"]), int(a["out_stride"]),
            C.c_void_p(a["d_out"]), C.c_void_p(a["d_info"]))
        self.ctx.sync()
        return rc

    def read(self):
        """-> (out (d, out_len), info (d, 4)) after asserting that nothing else was written and raw is unchanged"""
        o = self.d_out.cpu().numpy().view(np.complex128)
        i = self.d_info.cpu().numpy()
        p = self.pad
        assert np.all(o[:p] == SENT + 1j * SENT) and np.all(o[p + self.d * self.stride:] == SENT + 1j * SENT), "the bytes around out"
        rows = o[p:p + self.d * self.stride].reshape(self.d, self.stride)
        assert np.all(rows[:, self.out_len:] == SENT + 1j * SENT), "the out_stride - out_len tail of a row"
        assert np.all(i[:p] == SENT) and np.all(i[p + self.d * self.g.APPLY_INFO_COLS:] == SENT), "the bytes around info"
        assert np.array_equal(self.d_raw.cpu().numpy(), self.raw_all), "raw"
        return rows[:, :self.out_len].copy(), i[p:p + self.d * self.g.APPLY_INFO_COLS].reshape(self.d, -1).copy()

    def untouched(self):
        return bool(np.all(self.d_out.cpu().numpy() == SENT) and np.all(self.d_info.cpu().numpy() == SENT))


def resident(g, ctx, raw, fs, params, out_len, **kw):
    r = Resident(g, ctx, raw, fs, params, out_len, **kw)
    assert r.call() == 0, ctx.lib.gsmcal_last_error(ctx.h)
    return r.read()


def host_info(t):
    return np.stack([t[k] for k in ("status", "first_valid", "end_valid", "num_valid")], axis=1)


@pytest.mark.parametrize("n", ar.PARITY_N)
def test_parity_with_the_restatement(g, ctx, n):
    """every slope, delay, anchor, with and without imbalance, in batches of 1, 3 and 5 captures, at every out_len; out_stride =
    out_len + 5, every buffer between guard bands (the resident form), and the host form for the first batch of each size"""
    for out_len in ar.parity_out_lens(n):
        for k, (raw, params) in enumerate(ar.parity_batches(n)):
            want = ar.apply_batch(raw, ar.PARITY_FS, params, out_len)
            out, info = resident(g, ctx, raw, ar.PARITY_FS, params, out_len)
            compare(out, info, want, f"n {n} out_len {out_len} batch {k}")
            if k < 3:
                h_out, h_info = g.apply_calibration(raw, params, ar.PARITY_FS, out_len, ctx=ctx)
                assert same_bits(h_out, out) and same_bits(host_info(h_info), info), (n, out_len, k)
    print("largest deviation / bound so far:", {k: f"{v:.3g}" for k, v in worst.items()})


def test_identity_returns_the_bytes_minus_dc(g, ctx):
    n = 600
    raw = np.random.Generator(np.random.Philox(key=[23, 77])).integers(0, 256, size=(1, 2 * n), dtype=np.uint8)
    for dc in (127.5, 127.0, 100.25):
        out, info = resident(g, ctx, raw, 2.4e6, ar.identity_row(dc)[None], n)
        want = ar.apply_batch(raw, 2.4e6, ar.identity_row(dc)[None], n)
        assert info.tolist() == [[0.0, 7.0, n - 8.0, n - 15.0]]
        z = (raw[0, 0::2] - dc) + 1j * (raw[0, 1::2] - dc)
        assert np.all(np.abs(out[0, 7:n - 8] - z[7:n - 8]) <= ar.IDENTITY_TOL * want["scale"][0, 7:n - 8])
        assert not out[0, :7].any() and not out[0, n - 8:].any()


def five_captures():
    n = 777
    rng = np.random.Generator(np.random.Philox(key=[23, 5]))
    raw = rng.integers(0, 256, size=(5, 2 * n), dtype=np.uint8)
    rows = ar.parity_rows(n)
    params = rows[[7, 38, 61, 90, 115]].copy()                      # five different slopes, delays, anchors, with and without imbalance
    return n, raw, params


def test_bit_equality_alone_at_any_position_and_between_the_forms(g, ctx):
    n, raw, params = five_captures()
    out_len = n + 40
    five, info5 = resident(g, ctx, raw, ar.PARITY_FS, params, out_len)
    compare(five, info5, ar.apply_batch(raw, ar.PARITY_FS, params, out_len), "five captures")
    assert info5[:, 0].tolist() == [0.0] * 5 and np.all(info5[:, 3] > 700)
    again, info_again = resident(g, ctx, raw, ar.PARITY_FS, params, out_len)                    # twice in a row
    assert same_bits(again, five) and same_bits(info_again, info5)
    h_out, h_info = g.apply_calibration(raw, params, ar.PARITY_FS, out_len, ctx=ctx)            # host form against resident form
    assert same_bits(h_out, five) and same_bits(host_info(h_info), info5)
    rng = np.random.Generator(np.random.Philox(key=[23, 6]))
    for q in range(5):
        alone, info1 = resident(g, ctx, raw[q:q + 1], ar.PARITY_FS, params[q:q + 1], out_len)   # alone
        assert same_bits(alone[0], five[q]) and same_bits(info1[0], info5[q]), q
        for pos in range(5):                                                                    # at each position of a 5-capture batch,
            other = rng.integers(0, 256, size=raw.shape, dtype=np.uint8)                        # other bytes and other rows around it
            rows = params[rng.permutation(5)]
            other[pos], rows[pos] = raw[q], params[q]
            o, i = resident(g, ctx, other, ar.PARITY_FS, rows, out_len)
            assert same_bits(o[pos], five[q]) and same_bits(i[pos], info5[q]), (q, pos)
    # another stride and other guard bands: the same bits
    o, i = resident(g, ctx, raw, ar.PARITY_FS, params, out_len, out_stride=out_len, pad=3)
    assert same_bits(o, five) and same_bits(i, info5)


def test_call_history_leaves_no_trace(g, ctx):
    n, raw, params = five_captures()
    a_out, a_info = resident(g, ctx, raw, ar.PARITY_FS, params, n)
    rng = np.random.Generator(np.random.Philox(key=[23, 8]))
    nb = 300
    b_raw = rng.integers(0, 256, size=(3, 2 * nb), dtype=np.uint8)
    b_params = ar.parity_rows(nb)[[3, 50, 110]]
    b_out, b_info = resident(g, ctx, b_raw, 1.0e6, b_params, 257)                                # B: other n, out_len, rows, rate, d
    compare(b_out, b_info, ar.apply_batch(b_raw, 1.0e6, b_params, 257), "B")
    a2_out, a2_info = resident(g, ctx, raw, ar.PARITY_FS, params, n)                              # A again gives A's bits
    assert same_bits(a2_out, a_out) and same_bits(a2_info, a_info)
    # a refused call between two good ones: the outputs of the first stay as they are, the second is correct
    r = Resident(g, ctx, raw, ar.PARITY_FS, params, n)
    assert r.call() == 0
    first = r.read()
    bad = params.copy()
    bad[2, 1] = 1000.5
    assert r.call(params=bad) == ar.E_ARG
    kept = r.read()
    assert same_bits(kept[0], first[0]) and same_bits(kept[1], first[1]) and same_bits(first[0], a_out)
    b2_out, b2_info = resident(g, ctx, b_raw, 1.0e6, b_params, 257)
    assert same_bits(b2_out, b_out) and same_bits(b2_info, b_info)
    # the host form after the resident form and back
    h_out, h_info = g.apply_calibration(b_raw, b_params, 1.0e6, 257, ctx=ctx)
    assert same_bits(h_out, b_out) and same_bits(host_info(h_info), b_info)
    a3_out, _ = resident(g, ctx, raw, ar.PARITY_FS, params, n)
    assert same_bits(a3_out, a_out)


def test_refusals_leave_the_outputs_untouched(g, ctx):
    n, raw, params = five_captures()

    def row(col, value):
        p = params.copy()
        p[3, col] = value
        return p
    nan_and_bad = row(1, 2000.0)
    nan_and_bad[3, 3] = np.nan                                     # not a finite row: skipped, not refused
    cases = [("d_raw NULL", dict(d_raw=0)), ("params NULL", dict(params=None)), ("d_out NULL", dict(d_out=0)), ("d_info NULL", dict(d_info=0)),
             ("d 0", dict(d=0)), ("d -1", dict(d=-1)), ("n 0", dict(n=0)), ("out_len 0", dict(out_len=0)), ("out_len -3", dict(out_len=-3)),
             ("out_stride below out_len", dict(out_stride=n - 1)), ("sample_rate 0", dict(fs=0.0)), ("sample_rate < 0", dict(fs=-2.4e6)),
             ("sample_rate inf", dict(fs=np.inf)), ("sample_rate nan", dict(fs=np.nan)),
             ("slope 1000.5", dict(params=row(1, 1000.5))), ("slope -1001", dict(params=row(1, -1001.0))),
             ("gain 0", dict(params=row(8, 0.0))), ("gain < 0", dict(params=row(8, -1.0))),
             ("sin_phase 1", dict(params=row(9, 1.0))), ("sin_phase -1.5", dict(params=row(9, -1.5)))]
    r = Resident(g, ctx, raw, ar.PARITY_FS, params, n)
    for what, kw in cases:
        assert r.call(**kw) == ar.E_ARG, what
        assert r.untouched(), what
    assert r.call(d_raw=r.d_raw.data_ptr() + r.front + 1) == ar.E_ARG and r.untouched()          # raw not 2-byte aligned
    assert b"2-byte aligned" in ctx.lib.gsmcal_last_error(ctx.h)
    assert r.call(params=nan_and_bad) == 0                                                       # |slope_ppm| > 1000 in a row that is not finite
    out, info = r.read()
    assert info[3].tolist() == [17.0, 0.0, 0.0, 0.0] and not out[3].any() and info[[0, 1, 2, 4], 0].tolist() == [0.0] * 4
    # the edges are inside: |slope_ppm| = 1000, |sin_phase| just below 1, a tiny gain
    edge = params.copy()
    edge[0, 1], edge[1, 9], edge[2, 8] = -1000.0, np.nextafter(1.0, 0.0), 1e-3
    assert Resident(g, ctx, raw, ar.PARITY_FS, edge, n).call() == 0
    # the host form: the same refusals, its outputs untouched
    out = np.full((5, n), SENT + 1j * SENT)
    info = np.full((5, g.APPLY_INFO_COLS), SENT)
    dp = g._lib.c_double_p

    def host(raw_p=raw.ctypes.data_as(g._lib.c_u8_p), d=5, n_=n, fs=ar.PARITY_FS, p=params, out_len=n, stride=n, out_p=out.view(np.float64).ctypes.data_as(dp),
             info_p=info.ctypes.data_as(dp)):
        pr = np.ascontiguousarray(p) if p is not None else None
        return ctx.lib.gsmcal_apply_calibration_batch(ctx.h, raw_p, d, n_, float(fs), pr.ctypes.data_as(dp) if pr is not None else None, out_len,
                                                      stride, out_p, info_p)
    for what, kw in (("raw NULL", dict(raw_p=None)), ("params NULL", dict(p=None)), ("out NULL", dict(out_p=None)), ("info NULL", dict(info_p=None)),
                     ("d 0", dict(d=0)), ("n 0", dict(n_=0)), ("out_len 0", dict(out_len=0)), ("stride", dict(stride=n - 1)), ("fs", dict(fs=0.0)),
                     ("fs nan", dict(fs=np.nan)), ("slope", dict(p=row(1, 1000.5))), ("gain", dict(p=row(8, 0.0))), ("sin_phase", dict(p=row(9, -1.0)))):
        assert host(**kw) == ar.E_ARG, what
        assert np.all(out == SENT + 1j * SENT) and np.all(info == SENT), what
    with pytest.raises(g.GsmcalError, match="failed with -1 "):
        g.apply_calibration(raw, row(1, 1000.5), ar.PARITY_FS, ctx=ctx)
    with pytest.raises(ValueError):
        g.apply_calibration(raw, params[:4], ar.PARITY_FS, ctx=ctx)
    # the host form with out_stride > out_len leaves the tail of every row alone
    assert host(out_len=n - 100) == 0
    assert np.all(out[:, n - 100:] == SENT + 1j * SENT) and same_bits(out[:, :n - 100], resident(g, ctx, raw, ar.PARITY_FS, params, n - 100)[0])


def test_a_nan_row_zeroes_exactly_its_own_row(g, ctx):
    n, raw, params = five_captures()
    clean, info_clean = resident(g, ctx, raw, ar.PARITY_FS, params, n)
    failed = g.apply_params(np.stack([ar.table_row(np.inf, np.inf), ar.table_row(5.0, 1.0, status=12.0)]), 433.92e6)
    assert np.isnan(failed).all()
    for bad_row in (failed[0], failed[1], np.where(np.arange(10) == 6, np.inf, params[2]), np.where(np.arange(10) == 2, -np.inf, params[2])):
        p = params.copy()
        p[2] = bad_row
        out, info = resident(g, ctx, raw, ar.PARITY_FS, p, n)
        compare(out, info, ar.apply_batch(raw, ar.PARITY_FS, p, n), "a row that is not finite")
        assert info[2].tolist() == [17.0, 0.0, 0.0, 0.0] and same_bits(out[2], np.zeros(n, dtype=np.complex128))
        keep = [0, 1, 3, 4]
        assert same_bits(out[keep], clean[keep]) and same_bits(info[keep], info_clean[keep])
        h_out, h_info = g.apply_calibration(raw, p, ar.PARITY_FS, ctx=ctx)
        assert same_bits(h_out, out) and h_info["status"].tolist() == [0.0, 0.0, 17.0, 0.0, 0.0]


def test_closed_loop_on_the_device(g, ctx):
    """calibrate_batch_dev on three GSM captures with planted ppm gives the table; three CW captures made from the same planted e and
    c at another tuned frequency are corrected by apply_params(table) and apply_calibration_resident.  What is left of the tone is
    what the table's own error predicts, ((c - c^) 1e-6 f_t) (1 + e^) + f_b ((1 + e^) / (1 + e) - 1), within TONE_BAR_HZ: this holds
    the helper and the kernel, not the chain's accuracy.  Then array_covariance and array_combine take the three rows as they are."""
    import torch
    s = g.synth
    planted = ((63.0, -21.5), (-30.0, 12.0), (8.0, 33.0))
    coef, ts = s.fir1(46, 200e3 / s.FS), s.sch_training_sequence()
    raw = np.stack([s.make_stream(dongle=i, sampling_ppm=e, carrier_ppm=c)[0] for i, (e, c) in enumerate(planted)])
    D, ns = 3, raw.shape[1] // 2
    d_gsm = torch.from_numpy(raw).to("cuda:0")
    d_table = torch.zeros((D, g.TABLE_COLS), dtype=torch.float64, device="cuda:0")
    f_t, f_b, n, fs = 433.92e6, 100e3, 4096, ar.FS_TONE
    cw = np.stack([s.make_cw(n, step=ar.tone_step(e, c, f_t, f_b), seed=s.DEFAULT_SEED + i) for i, (e, c) in enumerate(planted)])
    d_cw = torch.from_numpy(cw).to("cuda:0")
    d_out = torch.full((D, n), SENT, dtype=torch.complex128, device="cuda:0")
    d_info = torch.full((D, g.APPLY_INFO_COLS), SENT, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    g.calibrate_batch_dev(d_gsm.data_ptr(), D, ns, coef, ts, 957.4e6, d_table.data_ptr(), ctx=ctx)
    ctx.sync()                                                     # the one synchronisation: the parameters pass through the host
    table = d_table.cpu().numpy()
    assert table[:, 9].tolist() == [0.0] * 3
    params = g.apply_params(table, f_t)
    params[:, 6:8] = ar.CW_DC                                      # the known DC of make_cw
    assert same_bits(params, np.array([np.concatenate([ar.apply_params(table[i], f_t)[:6], [ar.CW_DC[0], ar.CW_DC[1], 1.0, 0.0]]) for i in range(3)]))
    g.apply_calibration_resident(d_cw.data_ptr(), D, n, params, fs, n, n, d_out.data_ptr(), d_info.data_ptr(), ctx=ctx)
    ctx.sync()
    out, info = d_out.cpu().numpy(), d_info.cpu().numpy()
    compare(out, info, ar.apply_batch(cw, fs, params, n), "closed loop")
    for i, (e, c) in enumerate(planted):
        e_hat, c_hat = table[i, 4], table[i, 5]
        lo, hi = int(info[i, 1]), int(info[i, 2])
        assert info[i, 0] == 0 and hi - lo >= n - 20
        predicted = ((c - c_hat) * 1e-6 * f_t) * (1.0 + 1e-6 * e_hat) + f_b * ((1.0 + 1e-6 * e_hat) / (1.0 + 1e-6 * e) - 1.0)
        left = ar.tone_frequency(out[i, lo:hi], fs) - f_b
        before = ar.tone_frequency((cw[i, 0::2] - ar.CW_DC[0]) + 1j * (cw[i, 1::2] - ar.CW_DC[1]), fs) - f_b
        print(f"dongle {i}: planted {e:+.2f} {c:+.2f} ppm, table {e_hat:+.4f} {c_hat:+.4f}; tone {before:+.1f} Hz before, {left:+.3f} after, "
              f"{predicted:+.3f} predicted")
        assert abs(left - predicted) <= ar.TONE_BAR_HZ
    # ---- the rows are streams on one time base: array_covariance and array_combine take them as they are ----
    lo, hi = int(info[:, 1].max()), int(info[:, 2].min())
    cov = g.array_covariance(out, [0, 1, 2], [(lo, hi - lo)], ctx=ctx)[0]
    assert np.isfinite(cov.view(np.float64)).all() and np.array_equal(cov, cov.conj().T) and np.all(cov.diagonal().imag == 0) and np.all(cov.diagonal().real > 0)
    w, winfo = g.combine_weights(cov, ref=0)
    assert winfo["status"] == 0
    beam = g.array_combine(out, [0, 1, 2], w, ctx=ctx)
    assert beam.shape == (n,) and np.isfinite(beam.view(np.float64)).all() and np.abs(beam[lo:hi]).mean() > 100.0
    print("largest deviation / bound:", {k: f"{v:.3g}" for k, v in worst.items()})


def test_a_ring_slot_is_corrected_in_place_of_the_host_copy(g, ctx):
    """ingest.apply_calibration_slot: the resident form on a submitted ring slot gives the host form's bits"""
    n, raw, params = five_captures()
    ring = g.ingest.Ring(ctx, raw.size, 2)
    try:
        ring.host(1)[:raw.size] = raw.ravel()
        ring.submit(1, raw.size)
        out, info = g.ingest.apply_calibration_slot(ring, 1, 5, n, params, ar.PARITY_FS, ctx=ctx)
    finally:
        ring.close()
    h_out, h_info = g.apply_calibration(raw, params, ar.PARITY_FS, ctx=ctx)
    assert same_bits(out, h_out) and all(np.array_equal(info[k], h_info[k]) for k in info)
