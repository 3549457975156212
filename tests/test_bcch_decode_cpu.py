"""CPU tests of the BCCH_decode feature (-m "not gpu"): the synthetic side (synth.fire_remainder, bcch_block_encode, si3_octets /
si4_octets / si_fields, the si= argument), the C parser include/gsmcal_si.h (through ctypes, and in a stand-alone program under
the address and undefined-behaviour sanitizers), the fp64 restatement tests/bcch_decode_ref.py on the oracle chain and on the
designed blocks, the margin condition of every input the GPU tests compare, and the MEX target."""
import os
import subprocess

import numpy as np
import pytest

import bcch_decode_ref as ref
from oracle import gsmcal_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
synth = ref.synth


def encoded_word(octets):
    """u(0..227) of a block, from the encoder's own steps"""
    d = synth.bcch_bit_order(octets)
    rem = synth.fire_remainder(np.concatenate([d, np.zeros(40, np.int8)])) ^ synth.FIRE_ONES
    par = np.array([(rem >> (39 - i)) & 1 for i in range(40)], dtype=np.int8)
    return np.concatenate([d, par, np.zeros(4, np.int8)])


def test_fire_remainder_is_all_ones_on_an_encoded_word_and_fails_on_every_flipped_bit():
    prod = 0                                                       # (D^23 + 1)(D^17 + D^3 + 1) over GF(2)
    for k in (17, 3, 0):
        prod ^= ((1 << 23) | 1) << k
    assert prod == synth.FIRE_POLY == sum(1 << k for k in (40, 26, 23, 17, 3, 0))
    u = encoded_word(ref.DESIGNED_SI)
    assert u.shape == (228,) and synth.fire_remainder(u[:224]) == synth.FIRE_ONES
    for k in range(224):
        v = u[:224].copy()
        v[k] ^= 1
        assert synth.fire_remainder(v) != synth.FIRE_ONES, k
    assert synth.fire_remainder(np.zeros(224, np.int8)) == 0       # all zeros is no valid word
    # the decoder's trellis takes the noiseless coded word back to u
    e = synth.bcch_block_encode(ref.DESIGNED_SI)
    m = synth.bcch_interleave_map()
    c = e[m[:, 0], np.where(m[:, 1] < 57, m[:, 1], m[:, 1] + 2)]
    assert np.array_equal(c, synth.sch_conv_encode(u))
    got, margin = ref.viterbi(1.0 - 2.0 * c)
    assert np.array_equal(got, u) and margin >= 2.0
    assert np.array_equal(synth.bcch_octets(got[:184]), ref.DESIGNED_SI)
    assert np.array_equal(ref.encode_many(ref.DESIGNED_SI[None, :])[0], e)


def test_interleaver_is_a_bijection_onto_four_bursts_of_114_bits():
    m = synth.bcch_interleave_map()
    assert m.shape == (456, 2) and len({(int(b), int(j)) for b, j in m}) == 456
    assert m[:, 0].min() == 0 and m[:, 0].max() == 3 and m[:, 1].min() == 0 and m[:, 1].max() == 113
    sym = synth.bcch_data_symbol(np.arange(114))
    assert sym[0] == 3 and sym[56] == 59 and sym[57] == 88 and sym[113] == 144 and len(set(sym.tolist())) == 114
    assert not set(sym.tolist()) & (set(range(61, 87)) | set(synth.BCCH_STEAL_SYMBOLS))
    e = synth.bcch_block_encode(ref.DESIGNED_SI)
    assert e.shape == (4, 116) and np.all(e[:, 57:59] == 1)        # the stealing flags
    bits = ref.burst_bits(e[2], 5)
    assert bits.shape == (148,) and np.array_equal(bits[61:87], synth.TSC[5]) and bits[60] == 1 and bits[87] == 1


@pytest.mark.parametrize("cell_id", [0, 65535])
@pytest.mark.parametrize("mnc,digits", [("012", 3), (345, 3), (7, 2), ("99", 2)])
@pytest.mark.parametrize("lac", [0, 0xFFFE])
def test_si_octets_round_trip_through_both_parsers(gsmcal_mod, cell_id, mnc, digits, lac):
    for octets, si_type, cid in ((synth.si3_octets(cell_id, 262, mnc, lac), 3, cell_id), (synth.si4_octets(262, mnc, lac), 4, -1)):
        assert octets.shape == (23,) and octets.dtype == np.uint8 and octets[1] == 0x06 and octets[0] & 3 == 1
        assert octets[2] == (0x1B if si_type == 3 else 0x1C) and np.all(octets[(10 if si_type == 3 else 8):] == 0x2B)
        want = {"valid": 1, "msg_type": int(octets[2]), "si_type": si_type, "cell_id": cid, "mcc": 262, "mnc": int(mnc),
                "mnc_digits": digits, "lac": lac}
        assert synth.si_fields(octets) == want
        assert gsmcal_mod.si_fields(octets) == want                # the C parser, through ctypes
        assert np.array_equal(synth.bcch_octets(synth.bcch_bit_order(octets)), octets)


def test_parsers_refuse_what_they_do_not_recognise(gsmcal_mod):
    good = synth.si3_octets(4660, 1, 1, 2)
    rng = np.random.default_rng(5)
    cases = [good.copy() for _ in range(7)]
    cases[0][1] = 0x05                                             # another protocol discriminator
    cases[1][2] = 0x1D                                             # another message type
    cases[2][5] = 0xA2                                             # MCC digit 2 = 10
    cases[3][6] = 0xFB                                             # MCC digit 3 = 11
    cases[4][7] = 0x1C                                             # MNC digit 1 = 12
    cases[5][6] = 0xA1                                             # MNC digit 3 = 10: neither a digit nor the filler
    cases[6][0] = 0x4A                                             # not a pseudo-length octet
    cases += [np.zeros(23, np.uint8), np.full(23, 255, np.uint8)] + [rng.integers(0, 256, 23).astype(np.uint8) for _ in range(200)]
    for t in range(256):
        c = good.copy()
        c[2] = t
        cases.append(c)
    valid = 0
    for c in cases:
        a, b = synth.si_fields(c), gsmcal_mod.si_fields(c)
        assert a == b, (c, a, b)
        valid += a["valid"]
        if not a["valid"]:
            assert (a["cell_id"], a["mcc"], a["mnc"], a["lac"]) == (-1, -1, -1, -1)
    assert valid == 4 and all(synth.si_fields(c)["valid"] == 0 for c in cases[:9])     # the four SI types of the last loop
    for t, n in ((0x19, 1), (0x1A, 2)):
        c = good.copy()
        c[2] = t
        assert synth.si_fields(c) == {"valid": 1, "msg_type": t, "si_type": n, "cell_id": -1, "mcc": -1, "mnc": -1, "mnc_digits": -1, "lac": -1}
    with pytest.raises(ValueError):
        synth.si3_octets(65536, 262, 1, 1)
    with pytest.raises(ValueError):
        synth.si4_octets(262, "1234", 1)
    with pytest.raises(ValueError):
        synth.bcch_block_encode(np.zeros(22, np.uint8))


def test_default_streams_unchanged_and_only_the_bcch_payload_differs():
    kw = dict(dongle=3, num_frames=40, start_frame=49)
    base, truth = synth.make_stream(**kw)
    assert truth["si"] is None
    assert synth.make_stream(si=None, **kw)[0].tobytes() == base.tobytes()
    si = ref.chain_si(3)
    raw, t2 = synth.make_stream(si=si, **kw)
    assert np.array_equal(t2["si"], si) and {k: t2[k] for k in truth if k != "si"} == {k: truth[k] for k in truth if k != "si"}
    assert np.array_equal(synth.make_stream(si=si[0], **kw)[1]["si"], si[:1])
    with pytest.raises(ValueError):
        synth.make_stream(si=np.zeros(22, np.uint8), **kw)
    # the waveform: identical outside the payload bits of the slot-0 bursts of frames 2..5
    rng_a, rng_b = (np.random.Generator(np.random.Philox(key=[5, 7])) for _ in range(2))
    a, b = synth.ideal_waveform(60, 49, rng_a, tsc=4), synth.ideal_waveform(60, 49, rng_b, tsc=4, si=si)
    diff = np.nonzero(a != b)[0]
    frames = [fr for fr in range(60) if (49 + fr) % 51 in synth.BCCH_FRAMES]
    assert frames == [4, 5, 6, 7, 55, 56, 57, 58] and len(diff) > 0
    inside = np.zeros(len(a), dtype=bool)
    for fr in frames:                                              # bits 3..60 and 87..144 (the pulse of a bit spans 4 symbols)
        inside[fr * 10000 + 3 * 8: fr * 10000 + 148 * 8] = True
    assert np.all(inside[diff]) and all(np.any((diff >= fr * 10000) & (diff < fr * 10000 + 1184)) for fr in frames)
    for fr in frames:                                              # the mid-amble keeps its shape: the other payload in front of
        mid = slice(fr * 10000 + 65 * 8, fr * 10000 + 87 * 8)      # it turns it by a multiple of pi/2
        q = a[mid] * np.conj(b[mid])
        assert np.max(np.abs(q - q[0])) < 1e-12 and min(abs(q[0] - v) for v in (1, 1j, -1, -1j)) < 1e-12
    # the two multiframes carry si[0] and si[1]: frame numbers 49 + 4 = 53 (multiframe 1) and 49 + 55 = 104 (multiframe 2)
    rng_c = np.random.Generator(np.random.Philox(key=[5, 7]))
    c = synth.ideal_waveform(60, 49, rng_c, tsc=4, si=si[::-1])
    assert not np.array_equal(b[4 * 10000:8 * 10000], c[4 * 10000:8 * 10000])
    # the capture: bytes differ only inside BCCH bursts (frac_start and the clock error are known)
    d8 = np.nonzero(base.reshape(-1, 2) != raw.reshape(-1, 2))[0]
    t_ideal = truth["frac_start"] + d8 / (1.0 + truth["sampling_ppm"] * 1e-6) + 1.0
    fr, off = np.divmod(t_ideal, 10000.0)
    assert len(d8) > 100 and np.all(np.isin((49 + fr) % 51, synth.BCCH_FRAMES) & (off < 148 * 8 + 2))


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


def describe(tag, res):
    ev = ~np.isnan(res["ok"])
    print(tag, "status", res["status"], "blocks", res["num_blocks"], "ok", res["ok"].tolist(), "corrected", res["corrected"].tolist(),
          "ts_err", res["ts_err"].tolist(), "steal", res["steal"].tolist(), "mean_slope", res["mean_slope"].tolist(),
          "min |soft|/amp", res["min_soft"][ev].min() if np.any(ev) else None,
          "min_merge_margin/amp", res["min_merge_margin"][ev].min() if np.any(ev) else None)


BLOCKS_SEEN = {}


@pytest.mark.parametrize("ov", [8, 4])
@pytest.mark.parametrize("name", [c[0] for c in ref.CHAIN_CASES])
def test_restatement_decodes_the_planted_blocks_on_the_oracle_chain(chain, name, ov):
    """The prototype of the issue, redone: dongles 0, 3, 5 at their default SNR and dongle 4 at 8 dB, at 8x and decimated to 4x,
    tsc = 5: every block ok, the payload exact, no hard channel error at 8x (nor, as it turns out, at 4x)."""
    r, pi, truth = chain[name]
    if ov == 4:
        r, pi = ref.decimate_by_2(r, pi)
    res = ref.bcch_decode(r, pi, ref.CHAIN_TSC, ov)
    describe("%s ov %d" % (name, ov), res)
    ev = ~np.isnan(res["ok"])
    assert res["num_blocks"] == len(ref.block_rows(pi)) >= 1 and np.sum(ev) >= 1
    assert res["status"] == 0 and np.all(res["ok"][ev] == 1.0) and res["num_ok"] == int(np.sum(ev))
    assert res["first_ok"] == int(np.nonzero(ev)[0][0]) + 1
    for i in np.nonzero(ev)[0]:
        assert ref.planted_octets(truth, res["octets"][i]), (i, res["octets"][i])
        f = synth.si_fields(res["octets"][i])
        dongle = ref.chain_stream_args(name)["dongle"]
        assert f["valid"] == 1 and (f["mcc"], f["mnc"], f["lac"]) == (262, 2 + dongle, 0x1200 + dongle)
        assert f["cell_id"] == (1000 * dongle + 17 if f["si_type"] == 3 else -1)
    assert np.all(res["corrected"][ev] == 0) and np.all(res["ts_err"][ev] == 0) and np.all(res["steal"][ev] == 8)
    assert np.all(res["octets"][~ev] == 0)
    assert ref.margins_ok(res)
    BLOCKS_SEEN[(name, ov)] = int(np.sum(ev))
    if len(BLOCKS_SEEN) == 2 * len(ref.CHAIN_CASES):
        print("blocks in all:", sum(BLOCKS_SEEN.values()))
        assert sum(BLOCKS_SEEN.values()) >= 12


@pytest.mark.parametrize("ov", ref.SUPPORTED_OV)
def test_restatement_on_the_designed_blocks(ov):
    """every supported ov, ov 2 among them (the issue's prototype left it out): the designed noiseless block decodes there too"""
    e = synth.bcch_block_encode(ref.DESIGNED_SI)
    s, pos = ref.designed_stream(ov, [e], noise=0.0)
    res = ref.bcch_decode(s, pos, ref.DESIGNED_TSC, ov)
    describe("noiseless ov %d" % ov, res)
    assert res["status"] == 0 and res["corrected"][0] == 0 and np.array_equal(res["octets"][0], ref.DESIGNED_SI) and ref.margins_ok(res)
    assert len(s) == ref.last_read(pos[4, 0], ov)                  # the stream ends at the last burst's symbol 144
    for kind in ref.DESIGNED_KINDS:
        s, pos, tsc, want = ref.designed_case(ov, kind)
        res = ref.bcch_decode(s, pos, tsc, ov)
        describe("%s ov %d" % (kind, ov), res)
        assert ref.margins_ok(res)
        assert res["num_blocks"] == len(want["ok"]) and res["ok"].tolist() == [float(v) for v in want["ok"]]
        assert res["status"] == want["status"] and res["first_ok"] == want["first_ok"] and res["num_ok"] == sum(want["ok"])
        assert np.all(res["ts_err"] == 0) and np.all(res["steal"] == 8) and np.all(res["pos"] == pos[1::5, 0])
        assert np.all((0.0 < res["mean_slope"]) & (res["mean_slope"] < 0.02))      # 300 Hz: 2 pi 300 / 270 833 = 0.00696 rad/symbol
        for i, good in enumerate(want["ok"]):
            assert np.array_equal(res["octets"][i], ref.DESIGNED_SI if good else np.zeros(23, np.uint8))
            assert (res["corrected"][i] == 0) == bool(good)
        if want["status"] == 0:
            f = synth.si_fields(res["octets"][want["first_ok"] - 1])
            assert (f["si_type"], f["cell_id"], f["mcc"], f["mnc"], f["mnc_digits"], f["lac"]) == (3, 0xBEEF, 901, 70, 2, 0x0102)
    assert ref.designed_case(ov, "good_bad")[3]["first_ok"] == 1 and ref.designed_case(ov, "bad_good")[3]["first_ok"] == 2


def test_restatement_exits_and_edges_and_the_margins_of_every_gpu_input():
    ov = 2
    cases = ref.edge_cases(ov)
    res = {name: ref.bcch_decode(s, pos, tsc, ov) for name, (s, pos, tsc) in cases.items()}
    for name, r in res.items():
        describe(name, r)
        assert ref.margins_ok(r), name
    r = res["wrong_tsc"]                                           # the wrong training sequence: the Fire code fails
    assert r["status"] == ref.S_BCCH_NO_DECODE and r["ok"].tolist() == [0.0] and r["ts_err"][0] >= 26 and np.all(r["octets"] == 0)
    for name in ("no_type2", "run_of_three"):
        assert (res[name]["status"], res[name]["num_blocks"], res[name]["first_ok"]) == (ref.S_BCCH_NO_DECODE, 0, -1)
    r = res["run_of_three_then_other"]
    assert (r["status"], r["num_blocks"], r["ok"].tolist()) == (0, 1, [1.0])
    r = res["blocks24"]
    assert (r["status"], r["num_blocks"], r["num_ok"], r["first_ok"]) == (0, 24, 24, 1)
    s, pos, tsc = cases["blocks24"]
    assert ref.bcch_decode(s, ref.repeat_blocks(pos[:5], 25), tsc, ov)["status"] == ref.E_CAPACITY
    r = res["one_short"]                                           # symbol 144 of the last burst is one sample behind the end
    assert r["status"] == ref.S_BCCH_NO_DECODE and r["num_blocks"] == 1 and np.isnan(r["ok"][0]) and np.isnan(r["pos"][0])
    assert np.all(np.isnan(r["soft"])) and np.all(r["octets"] == 0)
    r = res["odd_positions"]
    assert r["num_blocks"] == 7 and np.all(np.isnan(r["ok"][:6])) and r["ok"][6] == 1.0 and (r["status"], r["first_ok"]) == (0, 7)
    s, pos, tsc = cases["wrong_tsc"]
    assert ref.bcch_decode(s, -np.ones((4, 2)), tsc, ov)["status"] == ref.S_POST_NO_POS
    assert ref.bcch_decode(s, pos, tsc, ov, r_len=-1)["status"] == ref.S_POST_NO_POS
    for bad in (1, 3, 16):
        assert ref.bcch_decode(s, pos, tsc, bad)["status"] == ref.E_UNSUPPORTED
    for bad in (-1, 8):
        assert ref.bcch_decode(s, pos, bad, ov)["status"] == ref.E_ARG
    # the report lines
    good = ref.bcch_decode(*ref.designed_case(ov, "clean")[:2], ref.DESIGNED_TSC, ov)
    assert ref.report(good) == "BCCH blocks 1 decoded 1\nSystem information type 3 cell identity 48879 LAI 901-70-258\n"
    assert ref.report(res["wrong_tsc"]) == "BCCH blocks 1 decoded 0\nFail to decode the BCCH blocks.\n"


def test_margin_of_the_many_stream_inputs():
    """a sample of the 65 538 one-block streams of the GPU test, through the restatement"""
    ov = min(ref.SUPPORTED_OV)
    s, octets, pos = ref.many_streams(120, ov, first=65470)        # across the 16-bit wrap of the cell identity
    n, starts = ref.many_geometry(ov)
    assert s.shape == (120, n) and n == ref.last_read(starts[3], ov) and len({o.tobytes() for o in octets}) == 120
    # the table-driven modulator of many_streams against synth.gmsk_modulate, burst by burst
    assert np.max(np.abs(s[60:72] - ref.many_streams_direct(12, ov, first=65530))) < 1e-12
    for i in list(range(0, 120, 9)) + [65, 66, 119]:
        res = ref.bcch_decode(s[i], pos, ref.MANY_TSC, ov)
        f = synth.si_fields(res["octets"][0])
        assert res["status"] == 0 and np.array_equal(res["octets"][0], octets[i]) and ref.margins_ok(res)
        assert f["cell_id"] == (65470 + i) % 65536 and f["mcc"] == 100 + (65470 + i) // 65536 and f["lac"] == (65470 + i) % 1000
        assert np.array_equal(ref.encode_many(octets[i:i + 1])[0], synth.bcch_block_encode(octets[i]))


@pytest.mark.parametrize("api", ["interleaved", "split"])
def test_bcch_decode_mex_target_compiles_against_the_abi(api):
    """the command of test_mex_gateway_compiles_against_the_abi for the BCCH_decode target"""
    r = subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-std=c99", "-DGSMCAL_FN_BCCH_decode"] +
                       (["-DGSMCAL_STUB_SPLIT"] if api == "split" else []) +
                       ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mex_stub"),
                        os.path.join(ROOT, "mex", "gsmcal_mex.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


SI_DRIVER = r'''
/* a stand-alone program around include/gsmcal_si.h: nothing of the library, nothing of HIP */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gsmcal_si.h"

static unsigned long long state = 88172645463325252ull;
static unsigned char next_byte(void) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (unsigned char)(state >> 24); }

static void show(const unsigned char* o) {
    gsmcal_si_info f;
    const int v = gsmcal_si_fields(o, &f);
    printf("%d %d %d %d %d %d %d %d\n", v, f.msg_type, f.si_type, f.cell_id, f.mcc, f.mnc, f.mnc_digits, f.lac);
}

int main(void) {
    /* heap blocks of exactly 23 octets, so that a read behind the end is caught */
    unsigned char* o = malloc(GSMCAL_SI_OCTETS);
    const unsigned char si3[GSMCAL_SI_OCTETS] = {0x49, 0x06, 0x1B, 0xBE, 0xEF, 0x09, 0xF1, 0x07, 0x01, 0x02, 0x2B, 0x2B, 0x2B,
                                                 0x2B, 0x2B, 0x2B, 0x2B, 0x2B, 0x2B, 0x2B, 0x2B, 0x2B, 0x2B};
    gsmcal_si_info f;
    int t, i, valid = 0;
    if (!o) return 2;
    memset(o, 0, GSMCAL_SI_OCTETS);
    show(o);
    memset(o, 255, GSMCAL_SI_OCTETS);
    show(o);
    memcpy(o, si3, GSMCAL_SI_OCTETS);
    show(o);
    o[3] = 0x21;                                      /* octets 3-5 that are BCD digits too: a type 4 reads its LAI there */
    o[4] = 0xF3;
    for (t = 0; t < 256; ++t) {                       /* every message type byte */
        o[2] = (unsigned char)t;
        valid += gsmcal_si_fields(o, &f);
        if (f.valid != (t >= 0x19 && t <= 0x1C) || f.msg_type != t) return 3;
    }
    for (i = 0; i < 20000; ++i) {                     /* random octets */
        for (t = 0; t < GSMCAL_SI_OCTETS; ++t) o[t] = next_byte();
        if (i % 4 == 0) { o[0] = 0x49; o[1] = 0x06; o[2] = (unsigned char)(0x18 + i % 6); }
        gsmcal_si_fields(o, &f);
        if (f.valid && (f.si_type < 1 || f.si_type > 4 || f.mcc > 999 || f.mnc > 999 || f.lac > 65535 || f.cell_id > 65535)) return 4;
        if (!f.valid && (f.cell_id != -1 || f.mcc != -1 || f.mnc != -1 || f.lac != -1)) return 5;
    }
    if (gsmcal_si_fields(NULL, &f) != 0 || f.valid != 0 || gsmcal_si_fields(o, NULL) != 0) return 6;
    printf("valid types %d\n", valid);
    free(o);
    return 0;
}
'''


def test_si_parser_in_a_stand_alone_program_under_the_sanitizers(tmp_path):
    """include/gsmcal_si.h compiled with the host compiler and -fsanitize=address,undefined into an ordinary executable with its
    own main (the sanitizers' runtimes linked in statically), run directly: all-zero, all-ones, a SYSTEM INFORMATION TYPE 3, every message type byte and random octets."""
    src, exe = tmp_path / "si_driver.c", tmp_path / "si_driver"
    src.write_text(SI_DRIVER)
    r = subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-2000:])
    lines = p.stdout.splitlines()
    assert lines[0] == "0 0 0 -1 -1 -1 -1 -1" and lines[1] == "0 255 0 -1 -1 -1 -1 -1"
    assert lines[2] == "1 27 3 48879 901 70 2 258" and lines[3] == "valid types 4"
    f = synth.si_fields(ref.DESIGNED_SI)
    assert lines[2] == "%d %d %d %d %d %d %d %d" % tuple(f[k] for k in ("valid", "msg_type", "si_type", "cell_id", "mcc", "mnc", "mnc_digits", "lac"))
