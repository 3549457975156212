"""GPU tests of BCCH_decode (-m gpu): gsmcal_BCCH_decode / gsmcal_bcch_decode_batch[_dev] (k_bcch_decode, k_bcch_decode_finish)
against the fp64 restatement of the definition in tests/bcch_decode_ref.py, and against the planted system information.

Bounds, with their origin (DESIGN.md section 16's):
  ok, octets, corrected, ts_err, steal, the counts, first_ok, the status      identical
  soft      1e-11 * max|x| of the 142 samples of the burst the value comes from: three orders over the rounding bound of a
            142-term sum
  mean_slope     1e-11 rad/symbol
  amp       1e-11 relative
Every compared block must meet both margins in the restatement (tests/test_bcch_decode_cpu.py asserts the same for every designed
input used here): each |soft| of each of the three passes >= 1e-6 * amp of its burst -- a sign that close to zero could fall the
other way under a value that differs in its last bits and change the decision-directed sums -- and min_merge_margin >= 1e-6 * amp.
The test fails rather than leave a block out.  Batch rows equal the single-stream call bit for bit."""
import numpy as np
import pytest

import bcch_decode_ref as ref

pytestmark = pytest.mark.gpu

FC = ref.FC
S_POST_NO_POS, S_NO_DECODE = 10, 15
IDENTICAL = ("ok", "corrected", "ts_err", "steal")
_MAP = ref.synth.bcch_interleave_map()
_SYMBOL = ref.synth.bcch_data_symbol(_MAP[:, 1])


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


@pytest.fixture(scope="module")
def cal(g):
    """The four chain cases and dongle 1 (the chain leaves it with status 6 and r_len = -1), calibrated in one batch."""
    s = g.synth
    coef, ts = s.fir1(46, 200e3 / s.FS), s.sch_training_sequence()
    made = [s.make_stream(**ref.chain_stream_args(name)) for name, *_ in ref.CHAIN_CASES]
    made += [s.make_stream(dongle=1)]
    raw = np.stack([m[0] for m in made])
    own = g.Context(0)                      # a context of its own: the shared one's staging buffers keep what the other test files left there
    out = g.calibrate_batch(raw, coef, ts, FC, want_r=True, ctx=own)
    own.close()
    assert out["table"][:4, 9].tolist() == [0.0] * 4 and out["table"][4, 9] == 6.0 and out["r_len"][4] == -1
    streams = [(np.ascontiguousarray(out["r_correct"][i, :int(out["r_len"][i])]), out["pos_info"][i]) for i in range(4)]
    return {"raw": raw, "out": out, "streams": streams, "truth": [m[1] for m in made], "coef": coef, "ts": ts}


def raw_table(g, pos):
    t = -np.ones((2, g.MAX_POS_ROWS))
    t[:, :len(pos)] = np.asarray(pos, dtype=np.float64).T
    return t


def same_bits(a, b):
    a, b = (np.ascontiguousarray(v, dtype=np.float64).view(np.uint64) for v in (a, b))
    return a.shape == b.shape and np.array_equal(a, b)


def compare(got, want, s, pos, ov):
    """one stream: what BCCH_decode returned against the restatement (status 0 or 15)"""
    ev = ~np.isnan(want["ok"])
    print("ov", ov, "status", got["status"], "ok", got["ok"].tolist(), "first_ok", got["first_ok"], "min |soft|/amp",
          np.min(want["min_soft"][ev]) if np.any(ev) else None, "margin/amp min", np.min(want["min_merge_margin"][ev]) if np.any(ev) else None)
    assert ref.margins_ok(want), (want["min_soft"], want["min_merge_margin"])
    for k in ("status", "num_blocks", "num_ok", "first_ok"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in IDENTICAL:
        assert np.array_equal(got[k], want[k], equal_nan=True), (k, got[k], want[k])
    assert np.array_equal(got["pos"], want["pos"], equal_nan=True)
    assert got["octets"].shape == want["octets"].shape and np.array_equal(got["octets"], want["octets"])
    assert np.array_equal(np.isnan(got["mean_slope"]), ~ev) and np.array_equal(np.isnan(got["amp"]), ~ev)
    assert np.array_equal(np.isnan(got["soft"]), np.isnan(want["soft"]))
    rows = ref.block_rows(pos)
    k = np.arange(3, 145)
    for i in np.nonzero(ev)[0]:
        win = np.array([np.max(np.abs(s[int(p) + k * ov + ref.delta(ov) - 1])) for p in np.asarray(pos)[rows[i] + 1:rows[i] + 5, 0]])
        err = np.abs(got["soft"][i] - want["soft"][i])
        assert np.all(err <= 1e-11 * win[_MAP[:, 0]]), (i, err.max(), win)
    if np.any(ev):
        print("  |d mean_slope| max", np.max(np.abs(got["mean_slope"] - want["mean_slope"])[ev]), "|d amp| rel max",
              np.max(np.abs(got["amp"] / want["amp"] - 1)[ev]))
        assert np.all(np.abs(got["mean_slope"] - want["mean_slope"])[ev] <= 1e-11)
        assert np.all(np.abs(got["amp"] - want["amp"])[ev] <= 1e-11 * want["amp"][ev])


def test_calibrated_streams_against_the_restatement_and_the_planted_system_information(g, cal):
    blocks = 0
    for (name, dongle, _), (r, pi), truth in zip(ref.CHAIN_CASES, cal["streams"], cal["truth"]):
        for ov in (8, 4):
            s, pos = (r, pi) if ov == 8 else ref.decimate_by_2(r, pi)
            got = g.BCCH_decode(s, pos, ref.CHAIN_TSC, ov, want_soft=True)
            compare(got, ref.bcch_decode(s, pos, ref.CHAIN_TSC, ov), s, pos, ov)
            # ... and, independently of the restatement, what was planted: the cell identity and the LAI through the C parser
            ev = ~np.isnan(got["ok"])
            assert got["status"] == 0 and got["num_blocks"] >= 1 and np.sum(ev) >= 1 and np.all(got["ok"][ev] == 1.0)
            assert np.all(got["corrected"][ev] == 0) and np.all(got["ts_err"][ev] == 0) and np.all(got["steal"][ev] == 8)
            types = set()
            for i in np.nonzero(ev)[0]:
                assert ref.planted_octets(truth, got["octets"][i])
                f = g.si_fields(got["octets"][i])
                assert f["valid"] == 1 and (f["mcc"], f["mnc"], f["mnc_digits"], f["lac"]) == (262, 2 + dongle, 2, 0x1200 + dongle)
                assert f["cell_id"] == (1000 * dongle + 17 if f["si_type"] == 3 else -1) and f["si_type"] in (3, 4)
                types.add(f["si_type"])
            assert got["si"] == g.si_fields(got["octets"][got["first_ok"] - 1])
            blocks += int(np.sum(ev))
            if np.sum(ev) >= 2:
                assert types == {3, 4}                                    # consecutive multiframes alternate
    assert blocks >= 12
    # the wrong training sequence code on a calibrated stream: nothing passes the Fire code
    r, pi = cal["streams"][1]
    got = g.BCCH_decode(r, pi, (ref.CHAIN_TSC + 3) % 8, 8, want_soft=True)
    compare(got, ref.bcch_decode(r, pi, (ref.CHAIN_TSC + 3) % 8, 8), r, pi, 8)
    assert got["status"] == S_NO_DECODE and got["num_ok"] == 0 and np.all(got["octets"] == 0) and got["si"]["valid"] == 0


@pytest.mark.parametrize("ov", ref.SUPPORTED_OV)
def test_designed_blocks(g, ov):
    for kind in ref.DESIGNED_KINDS:
        s, pos, tsc, want = ref.designed_case(ov, kind)
        got = g.BCCH_decode(s, pos, tsc, ov, want_soft=True)
        compare(got, ref.bcch_decode(s, pos, tsc, ov), s, pos, ov)
        assert got["status"] == want["status"] and got["ok"].tolist() == [float(v) for v in want["ok"]]
        assert got["first_ok"] == want["first_ok"]
        for i, good in enumerate(want["ok"]):
            assert np.array_equal(got["octets"][i], ref.DESIGNED_SI if good else np.zeros(23, np.uint8))
        if want["status"] == 0:
            assert (got["si"]["si_type"], got["si"]["cell_id"], got["si"]["mcc"], got["si"]["mnc"], got["si"]["lac"]) == (3, 0xBEEF, 901, 70, 0x0102)
        else:
            assert got["si"]["valid"] == 0
    s, pos, tsc, _ = ref.designed_case(ov, "clean")
    got = g.BCCH_decode(s, pos, (tsc + 1) % 8, ov, want_soft=True)
    compare(got, ref.bcch_decode(s, pos, (tsc + 1) % 8, ov), s, pos, ov)
    assert got["status"] == S_NO_DECODE and got["ts_err"][0] >= 26


def check_no_pos(res, i):
    row = res["table"][i]
    assert row[:4].tolist() == [0.0, 0.0, float(S_POST_NO_POS), -1.0] and np.all(np.isnan(row[4:])), row[:6]
    assert np.all(res["octets"][i] == 0)


def test_batch_rows_equal_the_single_stream_call_bit_for_bit(g, ctx, cal):
    import torch
    out = cal["out"]
    tsc = ref.CHAIN_TSC
    singles = [g.BCCH_decode(r, pi, tsc, 8, want_soft=True) for r, pi in cal["streams"]]
    n = cal["raw"].shape[1] // 2
    D = len(cal["raw"])
    # ---- host form: the streams exactly as calibrate_batch returned them ----
    res = g.bcch_decode_batch(out["r_correct"], out["r_len"], out["pos_info_raw"], 8, tsc, want_soft=True)
    assert res["table"].shape == (D, g.SI_COLS) and res["octets"].shape == (D, g.MAX_HITS, 23)
    for i, one in enumerate(singles):
        k = one["num_blocks"]
        assert same_bits(res["table"][i], one["row"]), (i, res["table"][i][:6], one["row"][:6])
        assert same_bits(res["soft"][i, :k], one["soft"]) and np.all(np.isnan(res["soft"][i, k:]))
        assert np.array_equal(res["octets"][i, :k], one["octets"]) and np.all(res["octets"][i, k:] == 0)
    check_no_pos(res, 4)
    assert np.all(np.isnan(res["soft"][4]))
    rows = g.si_rows(res["table"])
    assert rows["status"].tolist() == [0.0] * 4 + [10.0]
    for i in (1, 3):                                                                       # alone, table and octets
        one = g.bcch_decode_batch(out["r_correct"][i:i + 1], out["r_len"][i:i + 1], out["pos_info_raw"][i:i + 1], 8, tsc)
        assert one["table"].tobytes() == res["table"][i:i + 1].tobytes() and one["octets"].tobytes() == res["octets"][i:i + 1].tobytes()
    # ---- in another order, with one code per stream: a row does not depend on its place in the batch ----
    perm = [4, 2, 0, 1, 3]
    again = g.bcch_decode_batch(out["r_correct"][perm], out["r_len"][perm], out["pos_info_raw"][perm], 8, [tsc] * D)
    assert same_bits(again["table"], res["table"][perm]) and np.array_equal(again["octets"], res["octets"][perm])
    # ... and a code of its own per stream is that stream's: the wrong one for stream 2 only
    codes = [tsc, tsc, (tsc + 1) % 8, tsc, tsc]
    mixed = g.bcch_decode_batch(out["r_correct"], out["r_len"], out["pos_info_raw"], 8, codes)
    assert g.si_rows(mixed["table"])["status"].tolist() == [0.0, 0.0, float(S_NO_DECODE), 0.0, 10.0]
    assert same_bits(mixed["table"][[0, 1, 3, 4]], res["table"][[0, 1, 3, 4]])

    # ---- device form directly behind calibrate_batch_dev, no synchronisation in between ----
    d_raw = torch.from_numpy(cal["raw"]).to("cuda:0")
    b = {"table": torch.zeros((D, g.TABLE_COLS), dtype=torch.float64, device="cuda:0"),
         "pos": torch.zeros((D, 2, g.MAX_POS_ROWS), dtype=torch.float64, device="cuda:0"),
         "r": torch.zeros((D, n), dtype=torch.complex128, device="cuda:0"),
         "len": torch.zeros(D, dtype=torch.int64, device="cuda:0"),
         "si": torch.full((D, g.SI_COLS), -7.0, dtype=torch.float64, device="cuda:0"),
         "soft": torch.full((D, g.MAX_HITS, 456), -7.0, dtype=torch.float64, device="cuda:0"),
         "oct": torch.full((D, g.MAX_HITS, 23), 7, dtype=torch.uint8, device="cuda:0")}
    torch.cuda.synchronize()
    g.calibrate_batch_dev(d_raw.data_ptr(), D, n, cal["coef"], cal["ts"], FC, b["table"].data_ptr(), b["pos"].data_ptr(),
                          b["r"].data_ptr(), b["len"].data_ptr(), ctx=ctx)
    g.bcch_decode_batch_dev(b["r"].data_ptr(), n, b["len"].data_ptr(), b["pos"].data_ptr(), D, 8, tsc, b["si"].data_ptr(),
                            b["oct"].data_ptr(), b["soft"].data_ptr(), ctx=ctx)
    ctx.sync()
    assert same_bits(b["si"].cpu().numpy(), res["table"])
    assert same_bits(b["soft"].cpu().numpy(), res["soft"]) and np.array_equal(b["oct"].cpu().numpy(), res["octets"])
    # the calibration's own outputs and answers are untouched by a further call behind it
    before = [b[k].clone() for k in ("table", "pos", "len")] + [torch.view_as_real(b["r"]).clone()]
    det = g.last_batch_details(D, ctx=ctx)
    g.bcch_decode_batch_dev(b["r"].data_ptr(), n, b["len"].data_ptr(), b["pos"].data_ptr(), D, 8, tsc, b["si"].data_ptr(),
                            b["oct"].data_ptr(), ctx=ctx)
    ctx.sync()
    after = [b[k] for k in ("table", "pos", "len")] + [torch.view_as_real(b["r"])]
    assert all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(before, after))
    det2 = g.last_batch_details(D, ctx=ctx)
    assert all(np.array_equal(np.asarray(det[k]), np.asarray(det2[k]), equal_nan=True) for k in det)
    assert same_bits(b["si"].cpu().numpy(), res["table"])


def test_exits_and_edges(g, ctx):
    import torch
    ov = 2
    cases = ref.edge_cases(ov)
    got = {}
    for name, (s, pos, tsc) in cases.items():
        got[name] = g.BCCH_decode(s, pos, tsc, ov, want_soft=True)
        compare(got[name], ref.bcch_decode(s, pos, tsc, ov), s, pos, ov)
    s, pos, tsc = cases["wrong_tsc"]
    tsc = ref.DESIGNED_TSC
    # every element -1, r_len = -1
    assert g.BCCH_decode(s, -np.ones((6, 2)), tsc, ov) is None
    assert g.BCCH_decode(-1.0, np.array([[-1.0, -1.0]]), tsc, ov) is None
    check_no_pos(g.bcch_decode_batch(s[None, :], [len(s)], -np.ones((1, 2, g.MAX_POS_ROWS)), ov, tsc), 0)
    check_no_pos(g.bcch_decode_batch(s[None, :], [-1], raw_table(g, pos)[None], ov, tsc), 0)
    # no type-2 row; a run of three type-2 rows is no block
    for name in ("no_type2", "run_of_three"):
        assert (got[name]["status"], got[name]["num_blocks"], got[name]["first_ok"]) == (S_NO_DECODE, 0, -1)
        assert got[name]["octets"].shape == (0, 23)
    assert (got["run_of_three_then_other"]["status"], got["run_of_three_then_other"]["num_blocks"]) == (0, 1)
    # 24 blocks fit, 25 do not
    assert (got["blocks24"]["num_blocks"], got["blocks24"]["num_ok"], got["blocks24"]["first_ok"]) == (24, 24, 1)
    assert np.all(got["blocks24"]["octets"] == ref.DESIGNED_SI[None, :])
    many = ref.repeat_blocks(pos, 25)
    with pytest.raises(g.GsmcalError, match="GSMCAL_E_CAPACITY"):
        g.BCCH_decode(s, many, tsc, ov)
    res = g.bcch_decode_batch(np.stack([s, s]), [len(s)] * 2, np.stack([raw_table(g, many), raw_table(g, pos)]), ov, tsc, want_soft=True)
    rows = g.si_rows(res["table"])
    assert rows["status"].tolist() == [float(ref.E_CAPACITY), 0.0] and rows["num_blocks"].tolist() == [25.0, 1.0]
    assert res["table"][0, 1:4].tolist() == [0.0, float(ref.E_CAPACITY), -1.0] and np.all(np.isnan(res["table"][0, 4:]))
    assert np.all(res["octets"][0] == 0) and np.all(np.isnan(res["soft"][0]))
    # oversampling ratios and the training sequence code
    for bad in (1, 3, 16):
        with pytest.raises(g.GsmcalError, match="GSMCAL_E_UNSUPPORTED"):
            g.BCCH_decode(s, pos, tsc, bad)
        with pytest.raises(g.GsmcalError, match="GSMCAL_E_UNSUPPORTED"):
            g.bcch_decode_batch(s[None, :], [len(s)], raw_table(g, pos)[None], bad, tsc)
    for bad in (-1, 8):
        with pytest.raises(g.GsmcalError, match="GSMCAL_E_ARG"):
            g.BCCH_decode(s, pos, bad, ov)
        with pytest.raises(g.GsmcalError, match="GSMCAL_E_ARG"):
            g.bcch_decode_batch(np.stack([s, s]), [len(s)] * 2, np.stack([raw_table(g, pos)] * 2), ov, [tsc, bad])
    # symbol 144 of the last burst is the stream's last sample (the designed stream ends there); then one sample short
    assert len(s) == ref.last_read(pos[4, 0], ov)
    full = g.BCCH_decode(s, pos, tsc, ov)
    assert full["status"] == 0 and full["ok"].tolist() == [1.0]
    short = got["one_short"]
    assert short["status"] == S_NO_DECODE and short["num_blocks"] == 1 and np.isnan(short["ok"][0]) and np.all(short["octets"] == 0)
    # ... the same through r_len in a wider buffer: the samples behind r_len are not read
    wide = np.full((1, len(s) + 7), np.nan + 0j)
    wide[0, :len(s) - 1] = s[:-1]
    res = g.bcch_decode_batch(wide, [len(s) - 1], raw_table(g, pos)[None], ov, tsc)
    assert same_bits(res["table"][0], short["row"])
    wide[0, :len(s)] = s
    res = g.bcch_decode_batch(wide, [len(s)], raw_table(g, pos)[None], ov, tsc)
    assert same_bits(res["table"][0], full["row"]) and np.array_equal(res["octets"][0, 0], ref.DESIGNED_SI)
    # NaN, negative, zero and huge positions: the block is not evaluated, no error
    odd = got["odd_positions"]
    assert odd["num_blocks"] == 7 and np.all(np.isnan(odd["ok"][:6])) and odd["ok"][6] == 1.0 and odd["first_ok"] == 7
    assert np.all(odd["octets"][:6] == 0) and np.array_equal(odd["octets"][6], ref.DESIGNED_SI)
    # device form on its own buffers
    d_r = torch.from_numpy(s[None, :].copy()).to("cuda:0")
    d_len = torch.tensor([len(s)], dtype=torch.int64, device="cuda:0")
    d_pos = torch.from_numpy(raw_table(g, pos)[None]).to("cuda:0")
    d_out = torch.zeros((1, g.SI_COLS), dtype=torch.float64, device="cuda:0")
    d_oct = torch.full((1, g.MAX_HITS, 23), 9, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    g.bcch_decode_batch_dev(d_r.data_ptr(), len(s), d_len.data_ptr(), d_pos.data_ptr(), 1, ov, tsc, d_out.data_ptr(), d_oct.data_ptr(), ctx=ctx)
    ctx.sync()
    assert same_bits(d_out.cpu().numpy()[0], full["row"])
    assert np.array_equal(d_oct.cpu().numpy()[0, 0], ref.DESIGNED_SI) and np.all(d_oct.cpu().numpy()[0, 1:] == 0)


def test_more_streams_than_one_grid(g, ctx):
    """D = 65 538 one-block streams of the smallest length at the smallest supported ov, each with its own cell identity (and the
    MCC one up behind the 16-bit wrap): every identity exact.  The rows around the 65 535-stream launch boundary equal their
    single-stream calls."""
    import torch
    ov, D = min(ref.SUPPORTED_OV), 65538
    s, octets, pos = ref.many_streams(D, ov)
    n = s.shape[1]
    d_r = torch.from_numpy(s).to("cuda:0")
    d_pos = torch.from_numpy(raw_table(g, pos)).to("cuda:0").repeat(D, 1, 1).contiguous()
    d_len = torch.full((D,), n, dtype=torch.int64, device="cuda:0")
    d_out = torch.zeros((D, g.SI_COLS), dtype=torch.float64, device="cuda:0")
    d_oct = torch.full((D, g.MAX_HITS, 23), 5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    g.bcch_decode_batch_dev(d_r.data_ptr(), n, d_len.data_ptr(), d_pos.data_ptr(), D, ov, ref.MANY_TSC, d_out.data_ptr(), d_oct.data_ptr(), ctx=ctx)
    ctx.sync()
    rows = g.si_rows(d_out.cpu().numpy())
    got = d_oct.cpu().numpy()
    assert np.all(rows["status"] == 0) and np.all(rows["num_blocks"] == 1) and np.all(rows["num_ok"] == 1) and np.all(rows["first_ok"] == 1)
    assert np.all(rows["ok"][:, 0] == 1.0) and np.all(np.isnan(rows["ok"][:, 1:])) and np.all(rows["corrected"][:, 0] == 0)
    assert np.array_equal(got[:, 0], octets) and np.all(got[:, 1:] == 0)
    cid = (got[:, 0, 3].astype(np.int64) << 8) | got[:, 0, 4]
    assert np.array_equal(cid, np.arange(D) % 65536)                     # every identity, from the octets themselves
    for i in (0, 1, 65534, 65535, 65536, 65537):
        f = g.si_fields(got[i, 0])
        assert (f["valid"], f["si_type"], f["cell_id"], f["mcc"], f["mnc"], f["lac"]) == (1, 3, i % 65536, 100 + i // 65536, 1, i % 1000)
    for i in (0, 65534, 65535, 65536, 65537):
        one = g.BCCH_decode(s[i], pos, ref.MANY_TSC, ov, want_soft=True)
        assert same_bits(d_out[i].cpu().numpy(), one["row"]), i
        if i in (0, 65537):
            compare(one, ref.bcch_decode(s[i], pos, ref.MANY_TSC, ov), s[i], pos, ov)


def test_report_lines(g, cal):
    r, pi = cal["streams"][1]
    got = g.BCCH_decode(r, pi, ref.CHAIN_TSC, 8)
    text = g.last_call_report()
    f = got["si"]
    assert got["status"] == 0 and text == ref.report(ref.bcch_decode(r, pi, ref.CHAIN_TSC, 8))
    assert text.count("\n") == 2 and text.startswith("BCCH blocks %d decoded %d\n" % (got["num_blocks"], got["num_ok"]))
    assert text.endswith("System information type %d cell identity %d LAI 262-5-%d\n" % (f["si_type"], f["cell_id"], 0x1203))
    s, pos, tsc, _ = ref.designed_case(4, "flipped")
    assert g.BCCH_decode(s, pos, tsc, 4)["status"] == S_NO_DECODE
    assert g.last_call_report() == ref.report(ref.bcch_decode(s, pos, tsc, 4)) == "BCCH blocks 1 decoded 0\nFail to decode the BCCH blocks.\n"
    s, pos, tsc, _ = ref.designed_case(4, "clean")
    assert g.BCCH_decode(s, pos, tsc, 4)["status"] == 0
    assert g.last_call_report() == "BCCH blocks 1 decoded 1\nSystem information type 3 cell identity 48879 LAI 901-70-258\n"
    assert g.BCCH_decode(s, -np.ones((3, 2)), tsc, 4) is None and g.last_call_report() == ""
