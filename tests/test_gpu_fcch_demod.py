"""GPU tests of FCCH_demod (-m gpu): gsmcal_FCCH_demod / gsmcal_fcch_demod_batch[_dev] (k_fcch_demod, k_fcch_demod_finish)
against the fp64 restatement of FCCH_demod.m:5-66 in tests/fcch_demod_ref.py.

Bounds: max_idx identical; freq and mean_freq within 1e-6 ppm of the carrier (the project's ppm parity bound in Hz, ~9.6e-4 Hz);
carrier_ppm within 1e-6; snr within 1e-6 dB (the margin the project uses for SNR decisions) -- and every compared burst must
have |noise_power| / band_power >= 1e-3 in the restatement, so that the subtraction of :61 cannot eat that margin.  Batch rows
equal the single-stream call bit for bit."""
import math

import numpy as np
import pytest

import fcch_demod_ref as ref

pytestmark = pytest.mark.gpu

FC = 957.4e6
HZ_TOL = 1e-6 * 1e-6 * FC            # 1e-6 ppm of the carrier, in Hz
S_POST_NO_POS = 10


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


@pytest.fixture(scope="module")
def setup(g):
    s = g.synth
    return {"coef": s.fir1(46, 200e3 / s.FS), "ts": s.sch_training_sequence()}


@pytest.fixture(scope="module")
def cal(g, setup):
    """The two synthetic dongles of test_SCH_equalise_front_end_of_the_demodulator, calibrated once: raw bytes, the batch
    outputs, and per stream (r, pos_info, restatement at 8x)."""
    raw = np.stack([g.synth.make_stream(dongle=d)[0] for d in (0, 3)])
    out = g.calibrate_batch(raw, setup["coef"], setup["ts"], FC, want_r=True)
    streams = []
    for i in range(2):
        if out["table"][i, 9] != 0:
            streams.append(None)
            continue
        r = np.ascontiguousarray(out["r_correct"][i, :int(out["r_len"][i])])
        streams.append((r, out["pos_info"][i], ref.fcch_demod(r, out["pos_info"][i], 8, FC)))
    return {"raw": raw, "out": out, "streams": streams}


def compare(got, want, fs_rel=None):
    print("max_idx", got["max_idx"].tolist(), "snr", got["snr"].tolist(), "carrier_ppm", got["carrier_ppm"], want["carrier_ppm"])
    print("  |dfreq| max", np.max(np.abs(got["freq"] - want["freq"]), initial=0.0), "|dsnr| max",
          np.nanmax(np.abs(got["snr"] - want["snr"]), initial=0.0), "noise_ratio min", np.min(np.abs(want["noise_ratio"]), initial=np.inf))
    assert np.all(np.abs(want["noise_ratio"]) >= 1e-3), want["noise_ratio"]
    assert got["max_idx"].dtype == np.int64 and np.array_equal(got["max_idx"], want["max_idx"])
    tol = HZ_TOL if fs_rel is None else fs_rel
    assert got["freq"].shape == want["freq"].shape and np.all(np.abs(got["freq"] - want["freq"]) <= tol)
    assert abs(got["mean_freq"] - want["mean_freq"]) <= tol
    assert abs(got["carrier_ppm"] - want["carrier_ppm"]) <= (1e-6 if fs_rel is None else 1e6 * fs_rel / FC)
    nan = np.isnan(want["snr"])
    assert np.array_equal(np.isnan(got["snr"]), nan)
    assert np.all(np.abs(got["snr"][~nan] - want["snr"][~nan]) <= 1e-6)


def test_calibrated_streams_against_the_restatement(g, cal):
    done = 0
    for st in cal["streams"]:
        if st is None:
            continue
        r, pi, want = st
        compare(g.FCCH_demod(r, pi, 8, FC), want)
        assert len(want["freq"]) == int(np.sum(pi[:, 1] == 0)) >= 5
        done += 1
    assert done >= 1
    # the other oversampling ratio: the same stream decimated by 2 (592-point windows)
    r, pi, _ = next(st for st in cal["streams"] if st is not None)
    r4 = np.ascontiguousarray(r[::2])
    pi4 = pi.copy()
    pi4[:, 0] = np.floor((pi4[:, 0] - 1) / 2) + 1
    compare(g.FCCH_demod(r4, pi4, 4, FC), ref.fcch_demod(r4, pi4, 4, FC))


@pytest.mark.parametrize("ov", [8, 4])
@pytest.mark.parametrize("wrap", [0, 1, -2, -1])
def test_designed_spectrum_at_the_wrap_positions(g, ov, wrap):
    fft_len = 148 * ov
    p = wrap % fft_len
    s, pos = ref.designed_spectrum(ov, p)
    want = ref.fcch_demod(s, pos, ov, FC)
    got = g.FCCH_demod(s, pos, ov, FC)
    assert want["max_idx"].tolist() == [p - fft_len // 2] and abs(want["snr"][0] - ref.DESIGNED_SNR_DB) <= 1e-12
    compare(got, want, fs_rel=1e-6 * ref.SYMBOL_RATE * ov)


@pytest.mark.parametrize("ov", [8, 4])
def test_tones_inside_and_outside_the_band(g, ov):
    fft_len = 148 * ov
    for k in (37, 20, -30, 50, 100, -fft_len // 2, fft_len // 2 - 1):
        s, pos = ref.tone_windows(ov, k)
        want = ref.fcch_demod(s, pos, ov, FC)
        got = g.FCCH_demod(s, pos, ov, FC)
        inside = abs(k) <= 50
        assert len(want["snr"]) == 3 and np.all(np.isfinite(want["snr"]) == inside), (k, want["snr"])
        assert np.all(np.isnan(got["snr"]) != inside), (k, got["snr"])
        assert np.all(want["max_idx"] == k)
        compare(got, want, fs_rel=1e-6 * ref.SYMBOL_RATE * ov)


def test_exits(g, cal):
    r, pi, want = next(st for st in cal["streams"] if st is not None)
    assert g.FCCH_demod(-1.0, np.array([[-1.0, -1.0]]), 8, FC) is None
    assert g.FCCH_demod(r, -np.ones((72, 2)), 8, FC) is None
    none = g.FCCH_demod(r, pi[pi[:, 1] != 0], 8, FC)                      # no type-0 row: mean([]) = NaN
    assert len(none["freq"]) == len(none["snr"]) == len(none["max_idx"]) == 0
    assert math.isnan(none["mean_freq"]) and math.isnan(none["carrier_ppm"])
    many = np.stack([1.0 + 10.0 * np.arange(25), np.zeros(25)], axis=1)   # 25 type-0 rows: one more than GSMCAL_MAX_HITS
    with pytest.raises(g.GsmcalError, match="GSMCAL_E_CAPACITY"):
        g.FCCH_demod(r, many, 8, FC)
    assert len(g.FCCH_demod(r, many[:24], 8, FC)["freq"]) == 24
    # a window that leaves the stream is an argument error (MATLAB: index exceeds matrix dimensions), decided before any read
    last = int(pi[pi[:, 1] == 0, 0][-1])
    with pytest.raises(g.GsmcalError, match="GSMCAL_E_INDEX"):
        g.FCCH_demod(r[: last - 1 + 1184 - 100], pi, 8, FC)
    assert len(g.FCCH_demod(r[: last - 1 + 1184], pi, 8, FC)["freq"]) == len(want["freq"])      # ... the last sample is still inside
    with pytest.raises(g.GsmcalError, match="GSMCAL_E_INDEX"):
        g.FCCH_demod(r, np.array([[0.0, 0.0], [5000.0, 0.0]]), 8, FC)
    with pytest.raises(g.GsmcalError, match="GSMCAL_E_INDEX"):
        g.FCCH_demod(r, np.array([[5000.0, 0.0], [len(r) - 1184 + 2.0, 0.0]]), 8, FC)


def single_row(g, res):
    """what a batch row must hold for the stream FCCH_demod returned `res` for"""
    row = np.full(g.DEMOD_COLS, np.nan)
    k = len(res["freq"])
    row[:4] = k, res["mean_freq"], res["carrier_ppm"], 0.0
    row[4:4 + k], row[28:28 + k], row[52:52 + k] = res["freq"], res["snr"], res["max_idx"]
    return row


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_sentinel_row(row):
    assert row[0] == 0.0 and row[3] == S_POST_NO_POS and np.all(np.isnan(np.delete(row, [0, 3]))), row


def test_batch_rows_equal_the_single_stream_call_bit_for_bit(g, ctx, setup, cal):
    import torch
    out = cal["out"]
    assert all(st is not None for st in cal["streams"]), "both synthetic dongles calibrate (status 0)"
    singles = [single_row(g, g.FCCH_demod(r, pi, 8, FC)) for r, pi, _ in cal["streams"]]
    n = cal["raw"].shape[1] // 2
    # ---- host twin: the two streams as calibrate_batch returned them plus a sentinel row; then in another order ----
    r3 = np.concatenate([out["r_correct"], np.zeros((1, n), dtype=np.complex128)])
    len3 = np.concatenate([out["r_len"], [-1]]).astype(np.int64)
    pi3 = np.concatenate([out["pos_info_raw"], -np.ones((1, 2, g.MAX_POS_ROWS))])
    tab = g.fcch_demod_batch(r3, len3, pi3, 8, FC)
    assert tab.shape == (3, g.DEMOD_COLS)
    for i in range(2):
        assert same_bits(tab[i], singles[i]), (i, tab[i], singles[i])
    check_sentinel_row(tab[2])
    order = [2, 1, 0]
    tab_r = g.fcch_demod_batch(r3[order], len3[order], pi3[order], 8, FC)
    assert same_bits(tab_r, tab[order])
    assert same_bits(g.fcch_demod_batch(r3[1:2], len3[1:2], pi3[1:2], 8, FC)[0], tab[1])       # alone
    rows = g.demod_rows(tab)
    assert rows["status"].tolist() == [0.0, 0.0, 10.0] and rows["num_fcch"][0] == len(cal["streams"][0][2]["freq"])
    # a row with samples but an all -1 table, and one with a table but r_len = -1, carry the sentinel too
    len_x = np.array([len3[0], -1], dtype=np.int64)
    tab_x = g.fcch_demod_batch(r3[:2], len_x, np.stack([-np.ones((2, g.MAX_POS_ROWS)), pi3[1]]), 8, FC)
    check_sentinel_row(tab_x[0])
    check_sentinel_row(tab_x[1])

    # ---- device form behind calibrate_batch_dev, no synchronisation in between; third stream: noise the chain rejects ----
    noise = np.random.default_rng(3).integers(100, 156, size=(1, 2 * n), dtype=np.uint8)
    raw3 = np.concatenate([cal["raw"], noise])
    d_raw = torch.from_numpy(raw3).to("cuda:0")
    torch.cuda.synchronize()

    def buffers():
        return {"table": torch.zeros((3, g.TABLE_COLS), dtype=torch.float64, device="cuda:0"),
                "pos": torch.zeros((3, 2, g.MAX_POS_ROWS), dtype=torch.float64, device="cuda:0"),
                "r": torch.zeros((3, n), dtype=torch.complex128, device="cuda:0"),
                "len": torch.zeros(3, dtype=torch.int64, device="cuda:0"),
                "demod": torch.full((3, g.DEMOD_COLS), -7.0, dtype=torch.float64, device="cuda:0")}

    def calibrate(c, b):
        g.calibrate_batch_dev(d_raw.data_ptr(), 3, n, setup["coef"], setup["ts"], FC, b["table"].data_ptr(), b["pos"].data_ptr(),
                              b["r"].data_ptr(), b["len"].data_ptr(), ctx=c)

    def demod(c, b):
        g.fcch_demod_batch_dev(b["r"].data_ptr(), n, b["len"].data_ptr(), b["pos"].data_ptr(), 3, 8, FC, b["demod"].data_ptr(), ctx=c)

    torch.cuda.synchronize()
    b0 = buffers()
    torch.cuda.synchronize()
    calibrate(ctx, b0)
    ctx.sync()
    det_before = g.last_batch_details(3, ctx=ctx)
    b1 = buffers()
    torch.cuda.synchronize()
    calibrate(ctx, b1)
    demod(ctx, b1)                                                        # enqueued behind the calibrate call, no sync
    ctx.sync()
    det_after = g.last_batch_details(3, ctx=ctx)                          # still answers for the calibrate call
    for k in det_before:
        assert np.array_equal(det_after[k], det_before[k]), k
    assert np.array_equal(b1["table"].cpu().numpy(), b0["table"].cpu().numpy(), equal_nan=True)
    assert b1["len"].cpu().numpy().tolist()[2] == -1 and b1["table"].cpu().numpy()[2, 9] != 0
    dev = b1["demod"].cpu().numpy()
    for i in range(2):
        assert same_bits(dev[i], singles[i]), i
    check_sentinel_row(dev[2])

    # ---- depth 2: two calibrate calls in flight, the demod call behind them ----
    c2 = g.Context(0)
    try:
        c2.set_pipeline_depth(2)
        ba, bb = buffers(), buffers()
        torch.cuda.synchronize()
        calibrate(c2, ba)
        calibrate(c2, bb)
        demod(c2, bb)
        demod(c2, ba)
        c2.sync()
        for b in (ba, bb):
            assert same_bits(b["demod"].cpu().numpy(), dev)
    finally:
        c2.close()


def test_report_lines(g, cal):
    """gsmcal_last_call_report after FCCH_demod: the blank line of :6 and the five lines of :43,45,49,65,66 (the warning of
    :9 is the whole text at the :8 exit), numbers through num2str."""
    r, pi, _ = next(st for st in cal["streams"] if st is not None)
    res = g.FCCH_demod(r, pi, 8, FC)
    want = (" \n"
            "FCCH demod: FCCH freq " + g.num2str(res["freq"]) + "\n"
            "FCCH demod: mean FCCH freq " + g.num2str(res["mean_freq"]) + "\n"
            "FCCH demod: carrier error ppm " + g.num2str(res["carrier_ppm"]) + "\n"
            "FCCH demod: SNR " + g.num2str(res["snr"]) + "\n"
            "FCCH demod: max idx " + g.num2str(res["max_idx"]) + "\n")
    assert g.last_call_report() == want
    assert g.FCCH_demod(-1.0, np.array([[-1.0, -1.0]]), 8, FC) is None
    assert g.last_call_report() == " \nFCCH demod: Warning! No valid position information!\n"
