"""GPU tests of SCH_decode (-m gpu): gsmcal_SCH_decode / gsmcal_sch_decode_batch[_dev] (k_sch_decode, k_sch_finish) against the
fp64 restatement of the definition in tests/sch_decode_ref.py, and against the planted BSIC and frame numbers.

Bounds, with their origin:
  ok, bsic, fn, ts_err, corrected, the counts, the anchor, the status, u       identical
  soft      1e-11 * max|x| of the burst's 142 samples: the margin of the BCCH_demod tests, three orders over the rounding bound
            of a 64-term sum
  slope     1e-11 rad/symbol
  amp, mean_slope     1e-11 relative (mean_slope: 1e-11 rad/symbol)
Every compared burst must have min_merge_margin >= 1e-6 * amp in the restatement (tests/test_sch_decode_cpu.py asserts the same
on the oracle's streams; the bursts here give >= 7 * amp, the windows of the
capacity test that hold no burst >= 0.03 * amp): a decision of the trellis that close to a tie could fall the other
way under a soft value that differs in its last bits, and the test fails rather than leave the burst out.
Batch rows equal the single-stream call bit for bit."""
import numpy as np
import pytest

import sch_decode_ref as ref

pytestmark = pytest.mark.gpu

FC = ref.FC
S_POST_NO_POS, S_NO_DECODE = 10, 14
PER_BURST = ("ok", "bsic_b", "fn", "ts_err", "corrected")


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


@pytest.fixture(scope="module")
def ts(g):
    return {ov: g.synth.sch_training_sequence(ov) if ov == 8 else
            g.synth.gmsk_modulate(g.synth.diff_precode(g.synth.SCH_TRAINING_BITS), ov, g.synth.gmsk_frequency_pulse(sps=ov)) for ov in (1, 2, 4, 8)}


@pytest.fixture(scope="module")
def cal(g, ts):
    """The four chain cases, the two dongles that share a transmission, and dongle 1 (the chain leaves it with status 6 and
    r_len = -1), calibrated in one batch."""
    s = g.synth
    coef = s.fir1(46, 200e3 / s.FS)
    made = [s.make_stream(**ref.chain_stream_args(name)) for name, *_ in ref.CHAIN_CASES]
    made += [s.make_stream(dongle=d, **ref.TX_PAIR) for d in (0, 3)]
    made += [s.make_stream(dongle=1)]
    raw = np.stack([m[0] for m in made])
    out = g.calibrate_batch(raw, coef, ts[8], FC, want_r=True)
    assert out["table"][:6, 9].tolist() == [0.0] * 6 and out["table"][6, 9] == 6.0 and out["r_len"][6] == -1
    streams = [(np.ascontiguousarray(out["r_correct"][i, :int(out["r_len"][i])]), out["pos_info"][i]) for i in range(6)]
    return {"raw": raw, "out": out, "streams": streams, "truth": [m[1] for m in made], "coef": coef}


def raw_table(g, pos):
    t = -np.ones((2, g.MAX_POS_ROWS))
    t[:, :len(pos)] = np.asarray(pos, dtype=np.float64).T
    return t


def same_bits(a, b):
    a, b = (np.ascontiguousarray(v, dtype=np.float64).view(np.uint64) for v in (a, b))
    return a.shape == b.shape and np.array_equal(a, b)


def compare(got, want, s, pos, ov):
    """one stream: what SCH_decode returned against the restatement (status 0 or 14)"""
    ev = ~np.isnan(want["ok"])
    ratio = want["min_merge_margin"][ev] / want["amp"][ev]
    print("ov", ov, "status", got["status"], "bsic", got["bsic"], "fn_anchor", got["fn_anchor"], "ok", got["ok"].tolist(),
          "margin/amp min", np.min(ratio) if len(ratio) else None)
    assert np.all(ratio >= ref.MARGIN), ratio
    for k in ("status", "num_sch", "num_ok", "num_consistent", "bsic", "fn_anchor", "pos_anchor"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in PER_BURST:
        assert np.array_equal(got[k], want[k], equal_nan=True), (k, got[k], want[k])
    assert np.array_equal(got["u"], want["u"])
    assert np.array_equal(np.isnan(got["slope"]), ~ev) and np.array_equal(np.isnan(got["amp"]), ~ev)
    assert np.array_equal(np.isnan(got["soft"]), np.isnan(want["soft"]))
    sp = np.asarray(pos)[np.asarray(pos)[:, 1] == 1, 0]
    for i in np.nonzero(ev)[0]:
        k = np.arange(3, 145)
        win = np.max(np.abs(s[int(sp[i]) + k * ov + ref.delta(ov) - 1]))
        err = np.max(np.abs(got["soft"][i, 3:145] - want["soft"][i, 3:145]))
        assert err <= 1e-11 * win, (i, err, win)
    if np.any(ev):
        print("  |d slope| max", np.max(np.abs(got["slope"] - want["slope"])[ev]), "|d amp| rel max",
              np.max(np.abs(got["amp"] / want["amp"] - 1)[ev]))
        assert np.all(np.abs(got["slope"] - want["slope"])[ev] <= 1e-11)
        assert np.all(np.abs(got["amp"] - want["amp"])[ev] <= 1e-11 * want["amp"][ev])
    if want["num_ok"]:
        assert abs(got["mean_slope"] - want["mean_slope"]) <= 1e-11
    else:
        assert np.isnan(got["mean_slope"])


def test_calibrated_streams_against_the_restatement_and_the_planted_payload(g, cal, ts):
    for (r, pi), truth in zip(cal["streams"][:4], cal["truth"][:4]):
        for ov in (8, 4):
            s, pos = (r, pi) if ov == 8 else ref.decimate_by_2(r, pi)
            got = g.SCH_decode(s, pos, ts[ov], ov, want_soft=True)
            compare(got, ref.sch_decode(s, pos, ov), s, pos, ov)
            # ... and, independently of the restatement, what was planted
            sp = pos[pos[:, 1] == 1, 0]
            ev = ~np.isnan(got["ok"])
            assert got["num_sch"] == len(sp) >= 8 and np.sum(ev) >= len(sp) - 1
            assert got["status"] == 0 and got["bsic"] == truth["bsic"] and np.all(got["ok"][ev] == 1.0)
            assert np.all(got["bsic_b"][ev] == truth["bsic"]) and np.array_equal(got["fn"][ev], ref.expected_fn(truth, sp, ov)[ev])
            assert got["num_consistent"] == got["num_ok"] == int(np.sum(ev))
            assert got["fn_anchor"] == ref.expected_fn(truth, sp, ov)[ev][0] and got["pos_anchor"] == sp[ev][0]
            assert np.all(got["ts_err"][ev] == 0) and np.all(got["corrected"][ev] == 0)
            assert got["bsic"] & 7 == 5                                    # the colour code: the low three bits


@pytest.mark.parametrize("ov", [2, 4, 8])
def test_designed_streams(g, ts, ov):
    for kind in ref.DESIGNED_KINDS:
        s, pos, want = ref.designed_case(ov, kind)
        got = g.SCH_decode(s, pos, ts[ov], ov, want_soft=True)
        compare(got, ref.sch_decode(s, pos, ov), s, pos, ov)
        assert got["status"] == 0 and got["ok"].tolist() == [float(v) for v in want["ok"]]
        assert got["num_consistent"] == want["num_consistent"] and got["bsic"] == ref.DESIGNED_BSIC and got["fn_anchor"] == want["fn0"]
        fns = [(want["fn0"] + f) % ref.HYPER for f in ref.DESIGNED_FRAMES]
        if kind in ("clean", "wrap"):
            assert got["fn"].tolist() == fns
        if kind == "wrong_fn":
            assert got["fn"][3] == fns[3] + 51
        if kind == "other_bsic":
            assert got["bsic_b"].tolist() == [ref.DESIGNED_BSIC] * 4 + [ref.DESIGNED_BSIC ^ 9]
    s, pos = ref.single_burst_stream(ov)
    got = g.SCH_decode(s, pos, ts[ov], ov, want_soft=True)
    compare(got, ref.sch_decode(s, pos, ov), s, pos, ov)
    assert got["status"] == S_NO_DECODE and got["ok"].tolist() == [1.0] and got["fn"][0] == ref.DESIGNED_FN0
    assert (got["bsic"], got["fn_anchor"], got["pos_anchor"], got["num_consistent"]) == (-1, -1, -1, 1)


def check_no_pos_row(row):
    assert row[:8].tolist()[:7] == [0.0, 0.0, 0.0, -1.0, -1.0, -1.0, float(S_POST_NO_POS)] and np.all(np.isnan(row[7:])), row[:9]


def test_batch_rows_equal_the_single_stream_call_bit_for_bit(g, ctx, cal, ts):
    import torch
    out = cal["out"]
    singles = [g.SCH_decode(r, pi, ts[8], 8, want_soft=True) for r, pi in cal["streams"]]
    n = cal["raw"].shape[1] // 2
    D = len(cal["raw"])
    # ---- host form: the streams exactly as calibrate_batch returned them ----
    res = g.sch_decode_batch(out["r_correct"], out["r_len"], out["pos_info_raw"], 8, ts[8], want_soft=True, want_u=True)
    assert res["table"].shape == (D, g.SCH_COLS)
    for i, one in enumerate(singles):
        k = one["num_sch"]
        assert same_bits(res["table"][i], one["row"]), (i, res["table"][i][:8], one["row"][:8])
        assert same_bits(res["soft"][i, :k], one["soft"]) and np.all(np.isnan(res["soft"][i, k:]))
        assert np.array_equal(res["u"][i, :k], one["u"]) and np.all(res["u"][i, k:] == 255)
    check_no_pos_row(res["table"][6])
    assert np.all(np.isnan(res["soft"][6])) and np.all(res["u"][6] == 255)
    rows = g.sch_rows(res["table"])
    assert rows["status"].tolist() == [0.0] * 6 + [10.0]
    assert rows["bsic"].tolist() == [5.0, 29.0, 45.0, 29.0, 52.0, 52.0, -1.0]
    for i in (1, 5):                                                                       # alone, table only
        assert g.sch_decode_batch(out["r_correct"][i:i + 1], out["r_len"][i:i + 1], out["pos_info_raw"][i:i + 1], 8, ts[8]).tobytes() == \
            res["table"][i:i + 1].tobytes()
    # ---- in another order: a row does not depend on its place in the batch ----
    perm = [6, 2, 0, 5, 1, 4, 3]
    again = g.sch_decode_batch(out["r_correct"][perm], out["r_len"][perm], out["pos_info_raw"][perm], 8, ts[8])
    assert same_bits(again, res["table"][perm])

    # ---- device form directly behind calibrate_batch_dev, no synchronisation in between ----
    d_raw = torch.from_numpy(cal["raw"]).to("cuda:0")
    b = {"table": torch.zeros((D, g.TABLE_COLS), dtype=torch.float64, device="cuda:0"),
         "pos": torch.zeros((D, 2, g.MAX_POS_ROWS), dtype=torch.float64, device="cuda:0"),
         "r": torch.zeros((D, n), dtype=torch.complex128, device="cuda:0"),
         "len": torch.zeros(D, dtype=torch.int64, device="cuda:0"),
         "sch": torch.full((D, g.SCH_COLS), -7.0, dtype=torch.float64, device="cuda:0"),
         "soft": torch.full((D, g.MAX_HITS, 148), -7.0, dtype=torch.float64, device="cuda:0"),
         "u": torch.full((D, g.MAX_HITS, 39), 7, dtype=torch.uint8, device="cuda:0")}
    torch.cuda.synchronize()
    g.calibrate_batch_dev(d_raw.data_ptr(), D, n, cal["coef"], ts[8], FC, b["table"].data_ptr(), b["pos"].data_ptr(),
                          b["r"].data_ptr(), b["len"].data_ptr(), ctx=ctx)
    g.sch_decode_batch_dev(b["r"].data_ptr(), n, b["len"].data_ptr(), b["pos"].data_ptr(), D, 8, ts[8], b["sch"].data_ptr(),
                           b["soft"].data_ptr(), b["u"].data_ptr(), ctx=ctx)
    ctx.sync()
    assert same_bits(b["sch"].cpu().numpy(), res["table"])
    assert same_bits(b["soft"].cpu().numpy(), res["soft"]) and np.array_equal(b["u"].cpu().numpy(), res["u"])
    # the calibration's own outputs and answers are untouched by a further call behind it
    before = [b[k].clone() for k in ("table", "pos", "len")] + [torch.view_as_real(b["r"]).clone()]
    det = g.last_batch_details(D, ctx=ctx)
    g.sch_decode_batch_dev(b["r"].data_ptr(), n, b["len"].data_ptr(), b["pos"].data_ptr(), D, 8, ts[8], b["sch"].data_ptr(), ctx=ctx)
    ctx.sync()
    after = [b[k] for k in ("table", "pos", "len")] + [torch.view_as_real(b["r"])]
    assert all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(before, after))
    det2 = g.last_batch_details(D, ctx=ctx)
    assert all(np.array_equal(np.asarray(det[k]), np.asarray(det2[k]), equal_nan=True) for k in det)
    assert same_bits(b["sch"].cpu().numpy(), res["table"])


def test_two_dongles_on_one_transmission(g, cal, ts):
    """dongles 0 and 3 with one tx_key: the same bursts through two clocks.  Bursts less than half a frame apart carry the same
    frame number, and the alignment of the two frame clocks is under half a frame."""
    out = cal["out"]
    tab = g.sch_decode_batch(out["r_correct"][4:6], out["r_len"][4:6], out["pos_info_raw"][4:6], 8, ts[8])
    rows = g.sch_rows(tab)
    assert rows["status"].tolist() == [0.0, 0.0] and rows["bsic"].tolist() == [52.0, 52.0]
    pa, pb = (cal["streams"][i][1] for i in (4, 5))
    pa, pb = pa[pa[:, 1] == 1, 0], pb[pb[:, 1] == 1, 0]
    pairs = 0
    for i, p in enumerate(pa):
        for j, q in enumerate(pb):
            if abs(p - q) < 625 * 8 and rows["ok"][0, i] == 1.0 and rows["ok"][1, j] == 1.0:
                assert rows["fn"][0, i] == rows["fn"][1, j]
                pairs += 1
    assert pairs >= 8
    for k in (0, 1):                                                     # ... and they are the planted frame numbers
        sp = (pa, pb)[k]
        ev = rows["ok"][k, :len(sp)] == 1.0
        assert np.array_equal(rows["fn"][k, :len(sp)][ev], ref.expected_fn(cal["truth"][4 + k], sp, 8)[ev])
    al = g.sch_alignment(tab, 8)
    print("alignment", al.tolist())
    assert al[0] == 0.0 and abs(al[1]) < 625 * 8
    assert g.sch_alignment(tab, 8, ref=1)[0] == -al[1]
    full = g.sch_alignment(g.sch_decode_batch(out["r_correct"][4:], out["r_len"][4:], out["pos_info_raw"][4:], 8, ts[8]), 8)
    assert full[:2].tolist() == al.tolist() and np.isnan(full[2])        # dongle 1: no status 0, NaN
    # the restatement of the same rule
    want = ref.sch_alignment([ref.sch_decode(*cal["streams"][i], 8) for i in (4, 5)], 8)
    assert want.tolist() == al.tolist()


def test_exits_and_edges(g, ctx, ts):
    import torch
    ov = 2
    t = ts[ov]
    s, pos, _ = ref.designed_case(ov, "clean")
    # every element -1, r_len = -1
    assert g.SCH_decode(s, -np.ones((6, 2)), t, ov) is None
    assert g.SCH_decode(-1.0, np.array([[-1.0, -1.0]]), t, ov) is None
    tab = g.sch_decode_batch(s[None, :], [len(s)], -np.ones((1, 2, g.MAX_POS_ROWS)), ov, t)
    check_no_pos_row(tab[0])
    tab = g.sch_decode_batch(s[None, :], [-1], raw_table(g, pos)[None], ov, t)
    check_no_pos_row(tab[0])
    # no type-1 row
    none_pos = np.array([[1.0, 0.0], [500.0, 2.0]])
    got = g.SCH_decode(s, none_pos, t, ov, want_soft=True)
    compare(got, ref.sch_decode(s, none_pos, ov), s, none_pos, ov)
    assert got["status"] == S_NO_DECODE and got["num_sch"] == 0 and got["bsic"] == -1
    # 24 type-1 rows fit, 25 do not
    many = np.stack([pos[0, 0] + 37.0 * np.arange(25), np.ones(25)], axis=1)    # the first one is a burst
    got = g.SCH_decode(s, many[:24], t, ov, want_soft=True)
    compare(got, ref.sch_decode(s, many[:24], ov), s, many[:24], ov)
    assert got["num_sch"] == 24 and got["ok"][0] == 1.0 and not np.any(np.isnan(got["ok"]))
    with pytest.raises(g.GsmcalError, match="GSMCAL_E_CAPACITY"):
        g.SCH_decode(s, many, t, ov)
    tab = g.sch_decode_batch(np.stack([s, s]), [len(s)] * 2, np.stack([raw_table(g, many), raw_table(g, pos)]), ov, t)
    rows = g.sch_rows(tab)
    assert rows["status"].tolist() == [float(ref.E_CAPACITY), 0.0] and rows["num_sch"].tolist() == [25.0, 5.0] and np.all(np.isnan(tab[0, 7:]))
    assert tab[0, 1:6].tolist() == [0.0, 0.0, -1.0, -1.0, -1.0]
    # oversampling ratios and the template's length
    for bad in (1, 3, 16):
        with pytest.raises(g.GsmcalError, match="GSMCAL_E_UNSUPPORTED"):
            g.SCH_decode(s, pos, ts[1] if bad == 1 else np.zeros(64 * bad, complex), bad)
    with pytest.raises(g.GsmcalError, match="GSMCAL_E_ARG"):
        g.SCH_decode(s, pos, t[:-1], ov)
    with pytest.raises(g.GsmcalError, match="GSMCAL_E_ARG"):
        g.sch_decode_batch(s[None, :], [len(s)], raw_table(g, pos)[None], ov, ts[4])
    # symbol 144 of the last burst is the stream's last sample; then one sample short
    end = ref.last_read(pos[4, 0], ov)
    got = g.SCH_decode(s[:end], pos, t, ov, want_soft=True)
    compare(got, ref.sch_decode(s[:end], pos, ov), s[:end], pos, ov)
    assert got["ok"].tolist() == [1.0] * 5 and got["num_consistent"] == 5
    got = g.SCH_decode(s[:end - 1], pos, t, ov, want_soft=True)
    compare(got, ref.sch_decode(s[:end - 1], pos, ov), s[:end - 1], pos, ov)
    assert np.isnan(got["ok"][4]) and got["num_ok"] == 4 and got["status"] == 0 and np.all(got["u"][4] == 255)
    # ... the same through r_len in a wider buffer: the samples behind r_len are not read
    wide = np.full((1, len(s) + 7), np.nan + 0j)
    wide[0, :end - 1] = s[:end - 1]
    tab = g.sch_decode_batch(wide, [end - 1], raw_table(g, pos)[None], ov, t)
    assert same_bits(tab[0], got["row"])
    # NaN, negative, zero and huge positions: not evaluated, no error
    odd = np.concatenate([[[np.nan, 1.0], [-5.0, 1.0], [0.0, 1.0]], pos, [[1e300, 1.0], [float(len(s)), 1.0], [np.inf, 1.0]]])
    got = g.SCH_decode(s, odd, t, ov, want_soft=True)
    compare(got, ref.sch_decode(s, odd, ov), s, odd, ov)
    assert np.all(np.isnan(got["ok"][[0, 1, 2, 8, 9, 10]])) and got["ok"][3:8].tolist() == [1.0] * 5 and got["pos_anchor"] == pos[0, 0]
    # device form on a pinned table
    d_r = torch.from_numpy(s[None, :].copy()).to("cuda:0")
    d_len = torch.tensor([len(s)], dtype=torch.int64, device="cuda:0")
    d_pos = torch.from_numpy(raw_table(g, pos)[None]).to("cuda:0")
    d_out = torch.zeros((1, g.SCH_COLS), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    g.sch_decode_batch_dev(d_r.data_ptr(), len(s), d_len.data_ptr(), d_pos.data_ptr(), 1, ov, t, d_out.data_ptr(), ctx=ctx)
    ctx.sync()
    assert same_bits(d_out.cpu().numpy()[0], g.SCH_decode(s, pos, t, ov)["row"])


def test_more_streams_than_one_grid(g, ctx, ts):
    """D = 65 538 one-burst streams of 160*ov samples at ov 2, each with its own frame number: every per-burst fn exact, and
    status 14 by the rule (one burst is not evidence).  The rows around the 65 535-stream launch boundary equal their
    single-stream calls."""
    import torch
    ov, D = 2, 65538
    s, bsic, fn = ref.many_streams(D, ov)
    n = s.shape[1]
    pos = np.array([[ref.MANY_LEAD + 1.0, 1.0]])
    d_r = torch.from_numpy(s).to("cuda:0")
    d_pos = torch.from_numpy(raw_table(g, pos)).to("cuda:0").repeat(D, 1, 1).contiguous()
    d_len = torch.full((D,), n, dtype=torch.int64, device="cuda:0")
    d_out = torch.zeros((D, g.SCH_COLS), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    g.sch_decode_batch_dev(d_r.data_ptr(), n, d_len.data_ptr(), d_pos.data_ptr(), D, ov, ts[ov], d_out.data_ptr(), ctx=ctx)
    ctx.sync()
    rows = g.sch_rows(d_out.cpu().numpy())
    assert np.array_equal(rows["fn"][:, 0], fn.astype(np.float64)) and np.array_equal(rows["bsic_b"][:, 0], bsic.astype(np.float64))
    assert np.all(rows["ok"][:, 0] == 1.0) and np.all(np.isnan(rows["ok"][:, 1:]))
    assert np.all(rows["status"] == S_NO_DECODE) and np.all(rows["num_ok"] == 1) and np.all(rows["num_consistent"] == 1)
    assert np.all(rows["bsic"] == -1) and np.all(rows["fn_anchor"] == -1) and np.all(rows["ts_err"][:, 0] == 0)
    for i in (0, 65534, 65535, 65536, 65537):
        one = g.SCH_decode(s[i], pos, ts[ov], ov, want_soft=True)
        assert same_bits(d_out[i].cpu().numpy(), one["row"]), i
        if i in (0, 65537):
            compare(one, ref.sch_decode(s[i], pos, ov), s[i], pos, ov)


def test_report_lines(g, cal, ts):
    r, pi = cal["streams"][1]
    got = g.SCH_decode(r, pi, ts[8], 8)
    text = g.last_call_report()
    assert got["status"] == 0 and text == ref.report(ref.sch_decode(r, pi, 8))
    assert text.count("\n") == 2 and text.endswith("BSIC 29 frame number %d at sample %d\n" % (got["fn_anchor"], got["pos_anchor"]))
    s, pos = ref.single_burst_stream(4)
    assert g.SCH_decode(s, pos, ts[4], 4)["status"] == S_NO_DECODE
    assert g.last_call_report() == ref.report(ref.sch_decode(s, pos, 4)) == "SCH bursts 1 decoded 1 consistent 1\nFail to decode the SCH bursts.\n"
    assert g.SCH_decode(s, -np.ones((3, 2)), ts[4], 4) is None and g.last_call_report() == ""
