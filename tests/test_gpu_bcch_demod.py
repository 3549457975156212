"""GPU tests of BCCH_demod (-m gpu): gsmcal_BCCH_demod / gsmcal_bcch_demod_batch[_dev] (k_fcch_demod, k_bcch_corr,
k_bcch_finish, k_bcch_rotate) against the fp64 restatement of BCCH_demod.m in tests/bcch_demod_ref.py.

Bounds, with their origin:
  idx, tsc_idx, num_agree, status, num_bcch                identical
  mean_fo          1e-6 ppm of the carrier in Hz (HZ_TOL, ~9.6e-4 Hz): the project's ppm parity bound (test_gpu_fcch_demod.py)
  carrier_ppm      1e-6
  peak, runner_up, |corr_val|      1e-11 * 26*ov * max|x| of the window: the fp64 rounding bound of a 26*ov-term sum is about
                   26*ov * 2^-52 of that, so this is 200 times the bound at 8x; the common phase does not enter a magnitude
  phase, angle(corr_val), r        2*pi*HZ_TOL/fs * n + 1e-9 rad at sample index n: what the admitted mean_fo difference can
                   move the :76 phasor by (for r: that angle times |s(n)|, the chord is no longer than the arc)
Every compared burst must have winner / runner-up >= 1.05 in the restatement (the inputs here give >= 1.28), or the test fails.
Batch rows equal the single-stream call bit for bit."""
import math

import numpy as np
import pytest

import bcch_demod_ref as ref

pytestmark = pytest.mark.gpu

FC = 957.4e6
HZ_TOL = 1e-6 * 1e-6 * FC            # 1e-6 ppm of the carrier, in Hz
S_POST_NO_POS, S_POST_FEW_BCCH, S_MIXED = 10, 11, 13
DONGLES = (0, 3, 5)                  # calibrate in the oracle and on the GPU; tsc = dongle


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


@pytest.fixture(scope="module")
def nts(g):
    return {ov: g.synth.normal_training_sequences(ov) for ov in (1, 2, 4, 8)}


@pytest.fixture(scope="module")
def cal(g):
    """Dongles 0, 3, 5 (tsc = dongle) and dongle 1 (the chain leaves it with status 6, r_len = -1), calibrated once."""
    s = g.synth
    coef, ts = s.fir1(46, 200e3 / s.FS), s.sch_training_sequence()
    raw = np.stack([s.make_stream(dongle=d, tsc=d)[0] for d in DONGLES + (1,)])
    out = g.calibrate_batch(raw, coef, ts, FC, want_r=True)
    assert out["table"][:3, 9].tolist() == [0.0, 0.0, 0.0] and out["table"][3, 9] == 6.0 and out["r_len"][3] == -1
    streams = [(np.ascontiguousarray(out["r_correct"][i, :int(out["r_len"][i])]), out["pos_info"][i]) for i in range(3)]
    return {"raw": raw, "out": out, "streams": streams, "coef": coef, "ts": ts}


def ang_diff(a, b):
    return np.abs(np.angle(np.exp(1j * (np.asarray(a) - np.asarray(b)))))


def raw_table(g, pos):
    t = -np.ones((2, g.MAX_POS_ROWS))
    t[:, :len(pos)] = np.asarray(pos, dtype=np.float64).T
    return t


def same_bits(a, b):
    a, b = (np.ascontiguousarray(v).view(np.uint64) for v in (a, b))
    return a.shape == b.shape and np.array_equal(a, b)


def compare(got, want, s, pos, ov):
    """one stream: what BCCH_demod returned against the restatement (status 0 or 13)"""
    fs = ref.SYMBOL_RATE * ov
    print("ov", ov, "status", got["status"], "idx", got["idx"], "max_idx", got["max_idx"].tolist(), "ratio min", np.nanmin(want["ratio"]),
          "carrier_ppm", got["carrier_ppm"], want["carrier_ppm"], "d mean_fo", got["mean_fo"] - want["mean_fo"])
    done = ~np.isnan(want["max_idx"])
    assert np.all(want["ratio"][done] >= ref.MIN_RATIO), want["ratio"]
    assert got["status"] == want["status"] and got["idx"] == want["idx"] and got["num_bcch"] == want["num_bcch"] == len(done)
    assert got["num_agree"] == want["num_agree"]
    assert np.array_equal(got["max_idx"], want["max_idx"], equal_nan=True)
    assert abs(got["mean_fo"] - want["mean_fo"]) <= HZ_TOL
    assert abs(got["carrier_ppm"] - want["carrier_ppm"]) <= 1e-6
    mag_tol = 1e-11 * 26 * ov * want["win_max"]
    bpos = np.asarray(pos)[np.asarray(pos)[:, 1] == 2, 0]
    ang_tol = 2 * np.pi * HZ_TOL / fs * (bpos + 87 * ov) + 1e-9           # the window's last sample index bounds every n in it
    for k in ("peak", "runner_up"):
        assert np.array_equal(np.isnan(got[k]), ~done)
        print("  |d", k, "| / tol max", np.max(np.abs(got[k] - want[k])[done] / mag_tol[done]))
        assert np.all(np.abs(got[k] - want[k])[done] <= mag_tol[done])
    print("  d phase / tol max", np.max(ang_diff(got["phase"], want["phase"])[done] / ang_tol[done]))
    assert np.all(ang_diff(got["phase"], want["phase"])[done] <= ang_tol[done])
    cv, cw = got["corr_val"], want["corr_val"][:, :4]
    assert cv.shape == (8, 4)
    assert np.all(np.abs(np.abs(cv) - np.abs(cw)) <= mag_tol[None, :4])
    assert np.all(ang_diff(np.angle(cv), np.angle(cw)) <= ang_tol[None, :4])
    n = np.arange(len(s), dtype=np.float64)
    err = np.abs(got["r"] - want["r"])
    print("  |d r| / tol max", np.max(err / ((2 * np.pi * HZ_TOL / fs * n + 1e-9) * np.maximum(np.abs(s), 1e-300))))
    assert got["r"].shape == want["r"].shape and np.all(err <= (2 * np.pi * HZ_TOL / fs * n + 1e-9) * np.abs(s))


def test_calibrated_streams_against_the_restatement(g, cal, nts):
    done = 0
    for (r, pi), d in zip(cal["streams"], DONGLES):
        for ov in (8, 4):
            s, pos = (r, pi) if ov == 8 else ref.decimate_by_2(r, pi)
            want = ref.bcch_demod(s, pos, nts[ov], ov, FC)
            got = g.BCCH_demod(s, pos, nts[ov], ov, FC)
            compare(got, want, s, pos, ov)
            assert got["idx"] == d + 1 and got["status"] == 0
            assert got["num_bcch"] == int(np.sum(pos[:, 1] == 2)) >= 4 and got["num_agree"] == got["num_bcch"]      # every type-2 row
            done += 1
    assert done >= 4


def check_no_pos_row(row):
    assert row[0] == 0.0 and row[1] == -1.0 and row[4] == S_POST_NO_POS and np.all(np.isnan(np.delete(row, [0, 1, 4]))), row[:8]


def test_batch_rows_equal_the_single_stream_call_bit_for_bit(g, ctx, cal, nts):
    import torch
    out = cal["out"]
    singles = [g.BCCH_demod(r, pi, nts[8], 8, FC) for r, pi in cal["streams"]]
    n = cal["raw"].shape[1] // 2
    # ---- host form: the three streams and dongle 1 exactly as calibrate_batch returned them ----
    res = g.bcch_demod_batch(out["r_correct"], out["r_len"], out["pos_info_raw"], 8, nts[8], FC, want_corr=True, want_r=True)
    assert res["table"].shape == (4, g.BCCH_COLS)
    for i, one in enumerate(singles):
        L = int(out["r_len"][i])
        assert same_bits(res["table"][i], one["row"]), (i, res["table"][i][:8], one["row"][:8])
        assert same_bits(res["corr"][i, :4].view(np.float64), np.ascontiguousarray(one["corr_val"].T).view(np.float64))
        assert res["r_len"][i] == L and same_bits(res["r"][i, :L].view(np.float64), one["r"].view(np.float64))
    check_no_pos_row(res["table"][3])
    assert res["r_len"][3] == -1 and np.all(np.isnan(res["corr"][3].view(np.float64)))
    rows = g.bcch_rows(res["table"])
    assert rows["tsc_idx"].tolist() == [1.0, 4.0, 6.0, -1.0] and rows["status"].tolist() == [0.0, 0.0, 0.0, 10.0]
    assert g.bcch_demod_batch(out["r_correct"][1:2], out["r_len"][1:2], out["pos_info_raw"][1:2], 8, nts[8], FC).tobytes() == \
        res["table"][1:2].tobytes()                                                              # alone, table only

    # ---- device form directly behind calibrate_batch_dev, no synchronisation in between ----
    d_raw = torch.from_numpy(cal["raw"]).to("cuda:0")
    b = {"table": torch.zeros((4, g.TABLE_COLS), dtype=torch.float64, device="cuda:0"),
         "pos": torch.zeros((4, 2, g.MAX_POS_ROWS), dtype=torch.float64, device="cuda:0"),
         "r": torch.zeros((4, n), dtype=torch.complex128, device="cuda:0"),
         "len": torch.zeros(4, dtype=torch.int64, device="cuda:0"),
         "bcch": torch.full((4, g.BCCH_COLS), -7.0, dtype=torch.float64, device="cuda:0"),
         "corr": torch.full((4, g.MAX_BCCH, 8), -7.0, dtype=torch.complex128, device="cuda:0"),
         "r_out": torch.zeros((4, n), dtype=torch.complex128, device="cuda:0"),
         "len_out": torch.full((4,), -7, dtype=torch.int64, device="cuda:0")}
    torch.cuda.synchronize()
    g.calibrate_batch_dev(d_raw.data_ptr(), 4, n, cal["coef"], cal["ts"], FC, b["table"].data_ptr(), b["pos"].data_ptr(),
                          b["r"].data_ptr(), b["len"].data_ptr(), ctx=ctx)
    g.bcch_demod_batch_dev(b["r"].data_ptr(), n, b["len"].data_ptr(), b["pos"].data_ptr(), 4, 8, nts[8], FC, b["bcch"].data_ptr(),
                           b["corr"].data_ptr(), b["r_out"].data_ptr(), b["len_out"].data_ptr(), ctx=ctx)
    ctx.sync()
    dev = b["bcch"].cpu().numpy()
    assert same_bits(dev, res["table"])
    assert b["len_out"].cpu().numpy().tolist() == res["r_len"].tolist()
    assert same_bits(b["corr"].cpu().numpy().view(np.float64), res["corr"].view(np.float64))
    assert same_bits(b["r_out"][0, :int(out["r_len"][0])].cpu().numpy().view(np.float64), singles[0]["r"].view(np.float64))

    # ---- another template set on the same context (the columns in reverse order), then the first one again ----
    rev = np.ascontiguousarray(nts[8][:, ::-1])
    g.bcch_demod_batch_dev(b["r"].data_ptr(), n, b["len"].data_ptr(), b["pos"].data_ptr(), 4, 8, rev, FC, b["bcch"].data_ptr(), ctx=ctx)
    ctx.sync()
    rows_rev = g.bcch_rows(b["bcch"].cpu().numpy())
    assert rows_rev["tsc_idx"].tolist() == [8.0, 5.0, 3.0, -1.0]
    assert same_bits(rows_rev["peak"], rows["peak"]) and same_bits(rows_rev["runner_up"], rows["runner_up"])
    g.bcch_demod_batch_dev(b["r"].data_ptr(), n, b["len"].data_ptr(), b["pos"].data_ptr(), 4, 8, nts[8], FC, b["bcch"].data_ptr(), ctx=ctx)
    ctx.sync()
    assert same_bits(b["bcch"].cpu().numpy(), res["table"])


@pytest.mark.parametrize("ov", [1, 2, 4, 8])
def test_designed_streams(g, nts, ov):
    s, pos = ref.designed_stream(g.synth, ov, [6, 6, 6, 6])
    got = g.BCCH_demod(s, pos, nts[ov], ov, FC)
    compare(got, ref.bcch_demod(s, pos, nts[ov], ov, FC), s, pos, ov)
    assert got["idx"] == 7 and got["status"] == 0
    s, pos = ref.designed_stream(g.synth, ov, [2, 2, 5, 2])
    got = g.BCCH_demod(s, pos, nts[ov], ov, FC)
    compare(got, ref.bcch_demod(s, pos, nts[ov], ov, FC), s, pos, ov)     # r and carrier_ppm are compared in it
    assert got["idx"] == -1 and got["status"] == S_MIXED and got["max_idx"].tolist() == [3, 3, 6, 3] and got["num_agree"] == 3
    assert isinstance(got["r"], np.ndarray) and abs(got["carrier_ppm"] - 0.14362) < 1e-5


def test_eight_codes_in_one_stream(g, nts):
    s, pos = ref.designed_stream(g.synth, 2, list(range(8)), f=-400.0)
    got = g.BCCH_demod(s, pos, nts[2], 2, FC)
    compare(got, ref.bcch_demod(s, pos, nts[2], 2, FC), s, pos, 2)
    assert got["max_idx"].tolist() == list(range(1, 9)) and got["num_agree"] == 1 and got["status"] == S_MIXED


@pytest.mark.parametrize("code", [2, 3])
def test_first_maximum_rule(g, nts, code):
    """template column code+2 overwritten by column code: two bit-identical sums, the first one wins (:99) and the runner-up
    equals the peak exactly.  (code 2: MATLAB's columns 3 and 5, idx 3; code 3: the same one column on.)"""
    ov = 4
    dup = nts[ov].copy()
    dup[:, code + 2] = dup[:, code]
    s, pos = ref.designed_stream(g.synth, ov, [code] * 4)
    got = g.BCCH_demod(s, pos, dup, ov, FC)
    want = ref.bcch_demod(s, pos, nts[ov], ov, FC)
    assert np.all(want["ratio"] >= ref.MIN_RATIO) and want["idx"] == code + 1
    assert got["idx"] == code + 1 and got["status"] == 0 and got["max_idx"].tolist() == [code + 1] * 4
    assert same_bits(got["peak"], got["runner_up"]) and np.all(got["peak"] > 0)
    assert same_bits(got["corr_val"][code].view(np.float64), got["corr_val"][code + 2].view(np.float64))
    assert np.all(np.abs(got["peak"] - want["peak"]) <= 1e-11 * 26 * ov * want["win_max"])


def test_exits_and_edges(g, ctx, nts):
    import torch
    ov = 2
    t = nts[ov]
    s, pos = ref.designed_stream(g.synth, ov, [1, 1, 1, 1, 1])
    # :9 -- every element -1
    assert g.BCCH_demod(s, -np.ones((6, 2)), t, ov, FC) is None
    assert g.BCCH_demod(-1.0, np.array([[-1.0, -1.0]]), t, ov, FC) is None
    tab = g.bcch_demod_batch(s[None, :], [len(s)], -np.ones((1, 2, g.MAX_POS_ROWS)), ov, t, FC)
    check_no_pos_row(tab[0])
    # :14 -- three type-2 rows
    few = g.BCCH_demod(s, pos[:4], t, ov, FC)
    assert few["status"] == S_POST_FEW_BCCH and few["idx"] == -1 and few["r"] == -1.0 and few["carrier_ppm"] == -1.0
    assert few["num_bcch"] == 3 and math.isnan(few["mean_fo"]) and few["corr_val"] is None
    # no type-0 row: mean([]) = NaN
    none = g.BCCH_demod(s, pos[1:], t, ov, FC)
    assert none["idx"] == -1 and math.isnan(none["carrier_ppm"]) and math.isnan(none["mean_fo"]) and np.all(np.isnan(none["peak"]))
    assert np.all(np.isnan(none["max_idx"])) and np.all(np.isnan(none["r"].view(np.float64))) and none["num_bcch"] == 5
    # the fourth BCCH window ends on the stream's last sample; the fifth row's window is outside: NaN slots, status 0
    end4 = int(pos[4, 0]) + 61 * ov + 26 * ov - 1
    got = g.BCCH_demod(s[:end4], pos, t, ov, FC)
    want = ref.bcch_demod(s[:end4], pos, t, ov, FC)
    compare(got, want, s[:end4], pos, ov)
    assert got["status"] == 0 and got["idx"] == 2 and got["num_bcch"] == 5 and got["num_agree"] == 4
    assert math.isnan(got["max_idx"][4]) and math.isnan(got["peak"][4]) and math.isnan(got["phase"][4])
    assert g.BCCH_demod(s[:end4], pos[:5], t, ov, FC)["idx"] == 2
    with pytest.raises(g.GsmcalError, match="GSMCAL_E_INDEX"):
        g.BCCH_demod(s[:end4 - 1], pos[:5], t, ov, FC)
    with pytest.raises(g.GsmcalError, match="GSMCAL_E_INDEX"):            # an FCCH window that leaves the stream
        g.BCCH_demod(s, np.concatenate([pos, [[len(s) - 148 * ov + 2.0, 0.0]]]), t, ov, FC)
    with pytest.raises(g.GsmcalError, match="GSMCAL_E_INDEX"):            # a position below 1
        g.BCCH_demod(s, np.concatenate([[[-61.0 * ov, 2.0]], pos]), t, ov, FC)
    # len_ts = 26*ov - 1: MATLAB's inner dimensions would disagree
    with pytest.raises(g.GsmcalError, match="GSMCAL_E_ARG"):
        g.BCCH_demod(s, pos, t[:-1], ov, FC)
    # r_out aliasing r
    d_r = torch.from_numpy(s[None, :].copy()).to("cuda:0")
    d_len = torch.tensor([len(s)], dtype=torch.int64, device="cuda:0")
    d_pos = torch.from_numpy(raw_table(g, pos)[None]).to("cuda:0")
    d_out = torch.zeros((1, g.BCCH_COLS), dtype=torch.float64, device="cuda:0")
    d_lo = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(g.GsmcalError, match="GSMCAL_E_ARG"):
        g.bcch_demod_batch_dev(d_r.data_ptr(), len(s), d_len.data_ptr(), d_pos.data_ptr(), 1, ov, t, FC, d_out.data_ptr(),
                               d_r_out=d_r.data_ptr(), d_r_len_out=d_lo.data_ptr(), ctx=ctx)
    g.bcch_demod_batch_dev(d_r.data_ptr(), len(s), d_len.data_ptr(), d_pos.data_ptr(), 1, ov, t, FC, d_out.data_ptr(), ctx=ctx)
    ctx.sync()
    assert same_bits(d_out.cpu().numpy()[0], g.BCCH_demod(s, pos, t, ov, FC)["row"])


def test_more_streams_than_one_grid(g, ctx, nts):
    """D = 65 538 designed streams at ov 2 (about 1.7 GB), tiled on the device from four distinct ones: the rows on either
    side of the 65 535-stream launch boundary equal their single-stream calls."""
    import torch
    ov, D = 2, 65538
    sets = [ref.designed_stream(g.synth, ov, codes, f=f, seed=i) for i, (codes, f) in
            enumerate([([0] * 4, 137.5), ([3] * 4, -250.0), ([5, 5, 5, 5], 60.0), ([2, 2, 5, 2], 137.5)])]
    n = len(sets[0][0])
    singles = [g.BCCH_demod(s, pos, nts[ov], ov, FC, want_r=False)["row"] for s, pos in sets]
    assert [int(r[1]) for r in singles] == [1, 4, 6, -1]
    base = torch.from_numpy(np.stack([s for s, _ in sets])).to("cuda:0")
    tabs = torch.from_numpy(np.stack([raw_table(g, pos) for _, pos in sets])).to("cuda:0")
    rep = (D + 3) // 4
    d_r = base.repeat(rep, 1)[:D].contiguous()
    d_pos = tabs.repeat(rep, 1, 1)[:D].contiguous()
    d_len = torch.full((D,), n, dtype=torch.int64, device="cuda:0")
    d_out = torch.zeros((D, g.BCCH_COLS), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    g.bcch_demod_batch_dev(d_r.data_ptr(), n, d_len.data_ptr(), d_pos.data_ptr(), D, ov, nts[ov], FC, d_out.data_ptr(), ctx=ctx)
    ctx.sync()
    for i in (0, 65534, 65535, 65536, 65537):
        assert same_bits(d_out[i].cpu().numpy(), singles[i % 4]), i
    assert torch.equal(d_out[:, 4], torch.tensor([0.0, 0.0, 0.0, 13.0], dtype=torch.float64, device="cuda:0").repeat(rep)[:D])


def test_report_lines(g, cal, nts):
    """gsmcal_last_call_report after BCCH_demod: the restatement's lines (:15, :69, :72, :101 or :104) with their numbers
    through the library's num2str.  The calibrated stream is taken at 4x: at 8x carrier_correct_post_SCH has already removed this
    very estimate, and what :72 prints there is rounding residue (1e-14 ppm) whose digits no two implementations share."""
    r, pi = ref.decimate_by_2(*cal["streams"][0])
    assert g.BCCH_demod(r, pi, nts[4], 4, FC, want_r=False)["status"] == 0
    text = g.last_call_report()
    assert text == ref.report(ref.bcch_demod(r, pi, nts[4], 4, FC), g.num2str)
    assert text.count("\n") == 3 and text.endswith("Normal training sequence idx (BCCH) 1\n")
    s, pos = ref.designed_stream(g.synth, 8, [2, 2, 5, 2])
    assert g.BCCH_demod(s, pos, nts[8], 8, FC, want_r=False)["status"] == S_MIXED
    assert g.last_call_report() == ref.report(ref.bcch_demod(s, pos, nts[8], 8, FC), g.num2str)
    assert g.last_call_report().endswith("Fail to identity normal training sequence idx (BCCH).\n")
    assert g.BCCH_demod(s, pos[:4], nts[8], 8, FC)["status"] == S_POST_FEW_BCCH
    assert g.last_call_report() == ref.report(ref.bcch_demod(s, pos[:4], nts[8], 8, FC), g.num2str) == \
        "The number of BCCH bursts is less than 4!\n"
    assert g.BCCH_demod(s, -np.ones((3, 2)), nts[8], 8, FC) is None and g.last_call_report() == ""
