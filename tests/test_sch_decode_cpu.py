"""CPU tests of the SCH_decode feature (-m "not gpu"): the synthetic side (synth.sch_encode, sch_info_bits, sch_fields, the bsic= /
fn0= arguments), the fp64 restatement tests/sch_decode_ref.py on the oracle chain and on the designed streams, the margin
condition of every burst the GPU tests compare, and the MEX target."""
import os
import subprocess

import numpy as np
import pytest

import sch_decode_ref as ref
from oracle import gsmcal_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
synth = ref.synth
LAST_SCH_FRAME = ref.HYPER - 10                                   # 2 715 638: T3 = 41 of the last multiframe


@pytest.mark.parametrize("fn", [1, 11, 1326 * 2047 + 41, LAST_SCH_FRAME])
def test_encoder_and_field_map_round_trip(fn):
    assert fn % 51 in (1, 11, 21, 31, 41) and fn < ref.HYPER and (fn != LAST_SCH_FRAME or fn + 10 >= ref.HYPER)
    for bsic in range(64):
        d = synth.sch_info_bits(bsic, fn)
        f = synth.sch_fields(d)
        assert d.shape == (25,) and f["bsic"] == bsic and f["fn"] == fn
        assert (f["t1"], f["t2"], 10 * f["t3p"] + 1) == (fn // 1326, fn % 26, fn % 51)
        assert [int(x) for x in d[2:8]] == [(bsic >> i) & 1 for i in range(6)]          # d(2+i) = BSIC bit i
        c = synth.sch_encode(bsic, fn)
        assert c.shape == (78,) and np.array_equal(c, ref.encode_many([bsic], [fn])[0])
        u, margin = ref.viterbi(1.0 - 2.0 * c)                                           # noiseless soft values
        assert np.array_equal(u[:25], d) and not np.any(u[35:]) and margin >= 2.0
        assert np.array_equal(synth.sch_conv_encode(u), c)
    with pytest.raises(ValueError):
        synth.sch_info_bits(0, fn + 1)                                                   # not an SCH frame
    with pytest.raises(ValueError):
        synth.sch_info_bits(64, fn)


def test_crc_passes_on_an_encoded_word_and_fails_on_a_flipped_bit():
    d = synth.sch_info_bits(37, 51 * 777 + 21)
    u, _ = ref.viterbi(1.0 - 2.0 * synth.sch_encode(37, 51 * 777 + 21))
    assert synth.sch_crc_remainder(u[:35]) == 0x3FF and np.array_equal(u[:25], d)
    assert synth.SCH_CRC_POLY == sum(1 << k for k in (10, 8, 6, 5, 4, 2, 0))
    for k in range(35):
        v = u[:35].copy()
        v[k] ^= 1
        assert synth.sch_crc_remainder(v) != 0x3FF, k
    assert synth.sch_crc_remainder(np.zeros(35, np.int8)) == 0                            # all zeros is no valid word


def test_default_streams_unchanged_and_only_the_sch_payload_differs():
    base, truth = synth.make_stream(dongle=3, num_frames=24)
    assert truth["bsic"] is None and truth["fn0"] is None
    assert synth.make_stream(dongle=3, num_frames=24, bsic=None, fn0=None)[0].tobytes() == base.tobytes()
    sf = truth["start_frame"]
    fn0 = 51 * 9 + sf
    raw, t2 = synth.make_stream(dongle=3, num_frames=24, bsic=29, fn0=fn0)
    assert t2["bsic"] == 29 and t2["fn0"] == fn0 and {k: t2[k] for k in truth if k not in ("bsic", "fn0")} == \
        {k: truth[k] for k in truth if k not in ("bsic", "fn0")}
    assert synth.make_stream(dongle=3, num_frames=24, bsic=29)[1]["fn0"] == sf            # fn0 defaults to the start frame
    with pytest.raises(ValueError):
        synth.make_stream(dongle=3, num_frames=24, bsic=29, fn0=fn0 + 1)                  # fn0 mod 51 != start_frame
    # the waveform: identical outside the two payload fields of the SCH bursts
    rng_a, rng_b = (np.random.Generator(np.random.Philox(key=[5, 7])) for _ in range(2))
    a, b = synth.ideal_waveform(24, 8, rng_a), synth.ideal_waveform(24, 8, rng_b, bsic=29, fn0=51 * 2 + 8)
    diff = np.nonzero(a != b)[0]
    sch_frames = [fr for fr in range(24) if (8 + fr) % 51 % 10 == 1 and (8 + fr) % 51 != 50]
    assert len(sch_frames) >= 2 and len(diff) > 0
    inside = np.zeros(len(a), dtype=bool)
    for fr in sch_frames:                                          # bits 3..41 and 106..144 (the pulse of a bit spans 4 symbols)
        inside[fr * 10000 + 3 * 8: fr * 10000 + 148 * 8] = True
    assert np.all(inside[diff])
    for fr in sch_frames:                                          # ... and the training sequence in the middle keeps its shape:
        mid = slice(fr * 10000 + 46 * 8, fr * 10000 + 106 * 8)     # the other payload in front of it turns it by a multiple of pi/2
        q = a[mid] * np.conj(b[mid])
        assert np.max(np.abs(q - q[0])) < 1e-12 and min(abs(q[0] - v) for v in (1, 1j, -1, -1j)) < 1e-12
    # the capture: bytes differ only inside SCH bursts (frac_start, the FIR-free raw samples and the clock error are known)
    d8 = np.nonzero(base.reshape(-1, 2) != raw.reshape(-1, 2))[0]
    t_ideal = truth["frac_start"] + d8 / (1.0 + truth["sampling_ppm"] * 1e-6) + 1.0
    fr, off = np.divmod(t_ideal, 10000.0)
    assert len(d8) > 100 and np.all(((sf + fr) % 51 % 10 == 1) & (off < 148 * 8 + 2))


@pytest.fixture(scope="module")
def chain():
    """the four chain cases through the oracle chain, once: (r_correct, pos_info, truth)"""
    coef, ts = synth.fir1(46, 200e3 / synth.FS), synth.sch_training_sequence()
    out = {}
    for name, *_ in ref.CHAIN_CASES:
        raw, truth = synth.make_stream(**ref.chain_stream_args(name))
        res = o.calibrate_stream(raw, coef, ts, ref.FC, keep_r=True)
        assert res["status"] == 0
        out[name] = (res["r_correct"], res["pos_info"], truth)
    return out


def check_margin(res):
    ev = ~np.isnan(res["ok"])
    ratio = res["min_merge_margin"][ev] / res["amp"][ev]
    print("   min_merge_margin / amp: min", np.min(ratio) if len(ratio) else None)
    assert np.all(ratio >= ref.MARGIN), ratio


@pytest.mark.parametrize("ov", [8, 4])
@pytest.mark.parametrize("name", [c[0] for c in ref.CHAIN_CASES])
def test_restatement_decodes_the_planted_payload_on_the_oracle_chain(chain, name, ov):
    r, pi, truth = chain[name]
    if ov == 4:
        r, pi = ref.decimate_by_2(r, pi)
    res = ref.sch_decode(r, pi, ov)
    pos = pi[pi[:, 1] == 1, 0]
    ev = ~np.isnan(res["ok"])
    print(name, ov, "num_sch", res["num_sch"], "evaluated", int(np.sum(ev)), "fn", res["fn"][:3], "ts_err max", np.nanmax(res["ts_err"]),
          "corrected max", np.nanmax(res["corrected"]), "slope", res["mean_slope"], "min |soft|/amp",
          np.nanmin(np.abs(res["soft"][ev][:, 3:145]) / res["amp"][ev][:, None]))
    assert truth["bsic"] == 8 * ref.chain_stream_args(name)["dongle"] + 5
    assert res["num_sch"] == len(pos) >= 8 and np.sum(ev) >= res["num_sch"] - 1
    assert np.all(res["ok"][ev] == 1.0) and np.all(res["bsic_b"][ev] == truth["bsic"])
    assert np.array_equal(res["fn"][ev], ref.expected_fn(truth, pos, ov)[ev])
    assert res["status"] == 0 and res["num_consistent"] == res["num_ok"] == int(np.sum(ev)) and res["bsic"] == truth["bsic"]
    assert res["fn_anchor"] == res["fn"][ev][0] and res["pos_anchor"] == pos[ev][0]
    assert np.all(res["ts_err"][ev] == 0) and np.all(res["corrected"][ev] == 0)
    check_margin(res)
    if name == "d3wrap":
        assert truth["fn0"] == ref.HYPER - 153 + truth["start_frame"]


@pytest.mark.parametrize("ov", [2, 4, 8])
def test_restatement_on_the_designed_streams(ov):
    for kind in ref.DESIGNED_KINDS:
        s, pos, want = ref.designed_case(ov, kind)
        res = ref.sch_decode(s, pos, ov)
        print(ov, kind, res["status"], res["ok"].tolist(), res["fn"].tolist(), res["num_consistent"])
        check_margin(res)
        assert res["num_sch"] == 5 and res["ok"].tolist() == [float(v) for v in want["ok"]]
        assert res["status"] == 0 and res["num_ok"] == want["num_ok"] and res["num_consistent"] == want["num_consistent"]
        assert res["bsic"] == ref.DESIGNED_BSIC and res["fn_anchor"] == want["fn0"] and res["pos_anchor"] == pos[0, 0]
        assert 0.0 < res["mean_slope"] < 0.02                      # 300 Hz: 2 pi 300 / 270 833 = 0.00696 rad/symbol, plus the sampling instant
    # the altered bursts, one by one
    s, pos, _ = ref.designed_case(ov, "flipped")
    b = ref.decode_burst(s, pos[2, 0], ov)
    assert not b["ok"] and b["crc"] != 0x3FF                       # the run of flipped bits: the CRC fails
    s, pos, _ = ref.designed_case(ov, "t3p6")
    b = ref.decode_burst(s, pos[1, 0], ov)
    assert not b["ok"] and b["crc"] == 0x3FF and b["fields"]["t3p"] == 6 and b["fields"]["t2"] <= 25
    s, pos, want = ref.designed_case(ov, "wrong_fn")
    res = ref.sch_decode(s, pos, ov)
    assert res["ok"][3] == 1.0 and res["fn"][3] == want["fn0"] + 40 + 51
    s, pos, want = ref.designed_case(ov, "other_bsic")
    res = ref.sch_decode(s, pos, ov)
    assert res["ok"][4] == 1.0 and res["bsic_b"][4] == ref.DESIGNED_BSIC ^ 9 and res["fn"][4] == want["fn0"] + 51
    s, pos, want = ref.designed_case(ov, "wrap")
    res = ref.sch_decode(s, pos, ov)
    assert res["fn"].tolist() == [ref.HYPER - 50, ref.HYPER - 40, ref.HYPER - 30, ref.HYPER - 10, 1.0]
    # a single good burst: one pass of the CRC is not evidence
    s, pos = ref.single_burst_stream(ov)
    res = ref.sch_decode(s, pos, ov)
    check_margin(res)
    assert res["ok"].tolist() == [1.0] and res["fn"][0] == ref.DESIGNED_FN0 and res["num_consistent"] == 1
    assert res["status"] == ref.S_SCH_NO_DECODE and (res["bsic"], res["fn_anchor"], res["pos_anchor"]) == (-1, -1, -1)


def test_restatement_exits_edges_and_alignment():
    ov = 2
    s, pos, want = ref.designed_case(ov, "clean")
    end =ref.last_read(pos[4, 0], ov)                             # symbol 144 of the last burst is the last sample
    res = ref.sch_decode(s[:end], pos, ov)
    check_margin(res)
    assert res["ok"].tolist() == [1.0] * 5 and res["num_consistent"] == 5
    short = ref.sch_decode(s[:end - 1], pos, ov)                   # one sample short: not evaluated, no error
    assert np.isnan(short["ok"][4]) and short["ok"][:4].tolist() == [1.0] * 4 and short["num_sch"] == 5 and short["num_ok"] == 4
    assert np.all(np.isnan(short["soft"][4])) and np.all(short["u"][4] == 255) and short["status"] == 0
    odd = np.concatenate([[[np.nan, 1.0], [-5.0, 1.0], [0.0, 1.0]], pos, [[1e300, 1.0]]])
    res = ref.sch_decode(s, odd, ov)
    assert np.all(np.isnan(res["ok"][[0, 1, 2, 8]])) and res["ok"][3:8].tolist() == [1.0] * 5 and res["num_sch"] == 9
    assert res["status"] == 0 and res["pos_anchor"] == pos[0, 0]
    assert ref.sch_decode(s, -np.ones((4, 2)), ov)["status"] == ref.S_POST_NO_POS
    assert ref.sch_decode(s, pos, ov, r_len=-1)["status"] == ref.S_POST_NO_POS
    none = ref.sch_decode(s, np.array([[1.0, 0.0], [500.0, 2.0]]), ov)
    assert none["status"] == ref.S_SCH_NO_DECODE and none["num_sch"] == 0
    many = np.stack([np.arange(25) * 10.0 + 1, np.ones(25)], axis=1)
    assert ref.sch_decode(s, many, ov)["status"] == ref.E_CAPACITY
    assert ref.sch_decode(s, pos, 1)["status"] == ref.E_UNSUPPORTED
    # sch_alignment: two streams whose anchors are different bursts of the same clock line up at offset 0
    a = ref.sch_decode(s, pos, ov)
    b = ref.sch_decode(s, pos[2:], ov)
    assert a["pos_anchor"] != b["pos_anchor"] and ref.sch_alignment([a, b, none], ov).tolist()[:2] == [0.0, 0.0]
    assert np.isnan(ref.sch_alignment([a, b, none], ov)[2]) and np.all(np.isnan(ref.sch_alignment([none, a], ov)))


def test_margin_of_the_many_stream_inputs():
    """a sample of the 65 538 one-burst streams of the GPU test, through the restatement"""
    s, bsic, fn = ref.many_streams(330, 2)
    pos = np.array([[ref.MANY_LEAD + 1.0, 1.0]])
    assert s.shape == (330, 320) and len(set(fn.tolist())) == 330
    for i in list(range(0, 330, 7)) + [329]:
        res = ref.sch_decode(s[i], pos, 2)
        assert res["ok"].tolist() == [1.0] and res["fn"][0] == fn[i] and res["bsic_b"][0] == bsic[i] and res["status"] == ref.S_SCH_NO_DECODE
        assert res["min_merge_margin"][0] >= ref.MARGIN * res["amp"][0]


@pytest.mark.parametrize("api", ["interleaved", "split"])
def test_sch_decode_mex_target_compiles_against_the_abi(api):
    """the command of test_mex_gateway_compiles_against_the_abi for the SCH_decode target"""
    r = subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-std=c99", "-DGSMCAL_FN_SCH_decode"] +
                       (["-DGSMCAL_STUB_SPLIT"] if api == "split" else []) +
                       ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mex_stub"),
                        os.path.join(ROOT, "mex", "gsmcal_mex.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
