"""fp64 restatement of BCCH_decode, written line by line from its definition, for the BCCH_decode tests.

This is the project's own function, not a port: BCCH_demod.m stops at the training sequence index.  The definition:
a block is four type-2 rows of pos_info directly behind a type-1 row (rows i+1..i+4; a shorter run is no block).  Per burst of a
block with 1-based start p, tsc in 0..7 and ov in {2, 4, 8}, delta = (5*ov - 1) div 2:
    1  y_k = s(p + k*ov + delta) * (-j)^k for k = 3..144; if any of the block's four bursts would read outside the stream, or has
       p NaN or < 1, the block is not evaluated: NaN / empty record, no error
    2  pass 0: a_i = 1 - 2*TSC[tsc][i], h = sum_{i<26} y_{61+i} a_i, amp = |h|/26, soft_k = Re(y_k conj(h)/|h|)
    3  two decision-directed refinements: b_k = sign(soft_k) (+1 at zero), b_k = a_{k-61} inside the mid-amble;
       g1 = sum_{k=3..73} y_k b_k, g2 = sum_{k=74..144} y_k b_k, g = g1 + g2, slope = angle(g2 conj(g1))/71,
       soft_k = Re(y_k conj(g)/|g| exp(-j slope (k - 73.5))); positive = bit 0
    4  the 4 x 114 data soft values go to c(0..455) by the inverse of synth.bcch_interleave_map; the stealing positions (burst
       symbols 60 and 87) are counted as hard ones, 0..8, and not used
    5  the 16-state soft Viterbi of section 16 over 228 steps, state 0 to state 0, the same branch metric and strict >
    6  ok: the Fire remainder of u(0..223) is all ones and u(224..227) = 0 (detection only); corrected: Hamming distance between
       the hard c and the re-encoded word; ts_err: hard errors in the 4 x 26 mid-amble bits
Per stream: status 0 iff at least one block is ok, else 15; r_len = -1 or an all -1 pos_info: 10; more than MAX_HITS blocks: -4.

`bcch_decode` returns a dict: status, num_blocks, num_ok, first_ok (1-based, -1 without one) and per block (NaN where it was not
evaluated) ok, pos, corrected, ts_err, steal, mean_slope (the mean of the four bursts' last slope), amp (the mean of the four
bursts' amp), octets (num_blocks, 23) uint8 -- zeros unless ok --, soft (num_blocks, 456); restatement only: min_soft
(num_blocks, 4), the smallest |soft| / amp of the burst over all three passes, and min_merge_margin / amp per block.  The GPU
tests compare only blocks with both at least MARGIN.

Also here: the inputs the CPU and the GPU tests share."""
import importlib
import math

import numpy as np

synth = importlib.import_module("multi-rtl-sdr-calibration_amd.synth")

MAX_HITS = 24
S_POST_NO_POS, S_BCCH_NO_DECODE, E_CAPACITY, E_UNSUPPORTED, E_ARG = 10, 15, -4, -6, -1
MARGIN = 1e-6
FC = 957.4e6
SUPPORTED_OV = (2, 4, 8)


def delta(ov):
    return (5 * ov - 1) // 2


def viterbi(soft):
    """-> (u (n,) int8, min_merge_margin) over n = len(soft)/2 steps.  State = u(k-1)<<3 | u(k-2)<<2 | u(k-3)<<1 | u(k-4); the
    decisions are kept per step and traced back from state 0 (a 228-bit survivor)."""
    n = len(soft) // 2
    pm = [-math.inf] * 16
    pm[0] = 0.0
    dec = []
    marg = []
    for k in range(n):
        s0, s1 = float(soft[2 * k]), float(soft[2 * k + 1])
        npm, dk, mk = [0.0] * 16, [0] * 16, [math.inf] * 16
        for ns in range(16):
            b = ns >> 3
            cand = []
            for old in (0, 1):                                       # the predecessor whose oldest bit u(k-4) is `old`
                p = ((ns & 7) << 1) | old
                c0 = b ^ ((p >> 1) & 1) ^ (p & 1)                    # u(k) + u(k-3) + u(k-4)
                c1 = c0 ^ ((p >> 3) & 1)                             # ... + u(k-1)
                cand.append(pm[p] + ((-s0 if c0 else s0) + (-s1 if c1 else s1)))
            take = 1 if cand[1] > cand[0] else 0                     # strict: the first candidate stays
            npm[ns], dk[ns] = cand[take], take
            if cand[0] > -math.inf and cand[1] > -math.inf:
                mk[ns] = abs(cand[0] - cand[1])
        pm = npm
        dec.append(dk)
        marg.append(mk)
    u = np.zeros(n, dtype=np.int8)
    state, margin = 0, math.inf
    for k in range(n - 1, -1, -1):
        u[k] = state >> 3
        margin = min(margin, marg[k][state])
        state = ((state & 7) << 1) | dec[k][state]
    return u, margin


def detect_burst(s, p, ov, tsc):
    """steps 1-3 for one burst whose reads are inside the stream -> dict(soft (148,), amp, slope, min_soft)"""
    k = np.arange(3, 145)
    y = np.full(148, np.nan + 0j)
    y[3:145] = s[int(p) + k * ov + delta(ov) - 1] * (-1j) ** (k % 4)             # 1
    a = 1.0 - 2.0 * synth.TSC[tsc].astype(np.float64)
    h = np.sum(y[61:87] * a)                                                      # 2
    amp = abs(h) / 26.0
    soft = np.real(y * (np.conj(h) / abs(h)))
    lo = np.min(np.abs(soft[3:145]))
    kk = np.arange(148, dtype=np.float64)
    slope = 0.0
    for _ in (1, 2):                                                              # 3
        b = np.where(soft >= 0.0, 1.0, -1.0)
        b[61:87] = a
        g1, g2 = np.sum(y[3:74] * b[3:74]), np.sum(y[74:145] * b[74:145])
        g = g1 + g2
        slope = np.angle(g2 * np.conj(g1)) / 71.0
        soft = np.real(y * (np.conj(g) / abs(g)) * np.exp(-1j * slope * (kk - 73.5)))
        lo = min(lo, np.min(np.abs(soft[3:145])))
    return {"soft": soft, "amp": float(amp), "slope": float(slope), "min_soft": float(lo / amp)}


_MAP = synth.bcch_interleave_map()
_SYMBOL = synth.bcch_data_symbol(_MAP[:, 1])                                      # c(k) sits at symbol _SYMBOL[k] of burst _MAP[k, 0]


def decode_block(s, ps, ov, tsc):
    """four starts -> None when the block is not evaluated, else a dict of the per-block results"""
    n = len(s)
    for p in ps:
        if not (p >= 1) or not (p + 144 * ov + delta(ov) <= n):
            return None
    bursts = [detect_burst(s, p, ov, tsc) for p in ps]
    soft4 = np.stack([b["soft"] for b in bursts])
    c_soft = soft4[_MAP[:, 0], _SYMBOL]                                           # 4
    steal = int(np.sum(soft4[:, list(synth.BCCH_STEAL_SYMBOLS)] < 0))
    u, margin = viterbi(c_soft)                                                   # 5
    ok = synth.fire_remainder(u[:224]) == synth.FIRE_ONES and not np.any(u[224:])  # 6
    hard = (c_soft < 0).astype(np.int8)
    ts_err = int(np.sum((soft4[:, 61:87] < 0).astype(np.int8) != synth.TSC[tsc][None, :]))
    amps = [b["amp"] for b in bursts]
    slopes = [b["slope"] for b in bursts]
    amp = (((amps[0] + amps[1]) + amps[2]) + amps[3]) / 4.0
    return {"ok": bool(ok), "octets": synth.bcch_octets(u[:184]) if ok else np.zeros(23, np.uint8), "u": u,
            "corrected": int(np.sum(hard != synth.sch_conv_encode(u))), "ts_err": ts_err, "steal": steal,
            "mean_slope": (((slopes[0] + slopes[1]) + slopes[2]) + slopes[3]) / 4.0, "amp": amp, "soft": c_soft,
            "min_soft": np.array([b["min_soft"] for b in bursts]), "margin": margin / amp,
            "burst_amp": np.array(amps)}


def block_rows(pos_info):
    """indices i of the type-1 rows that four type-2 rows follow directly"""
    t = np.asarray(pos_info)[:, 1]
    return [i for i in range(len(t) - 4) if t[i] == 1 and np.all(t[i + 1:i + 5] == 2)]


PER_BLOCK = ("ok", "pos", "corrected", "ts_err", "steal", "mean_slope", "amp")


def bcch_decode(s, pos_info, tsc, ov, r_len=None):
    pos_info = np.atleast_2d(np.asarray(pos_info, dtype=np.float64))
    if ov not in SUPPORTED_OV:
        return {"status": E_UNSUPPORTED}
    if not 0 <= tsc <= 7:
        return {"status": E_ARG}
    s = np.asarray(s, dtype=np.complex128).ravel()
    if r_len is not None:
        s = s[:max(int(r_len), 0)]
    out = {"status": 0, "num_blocks": 0, "num_ok": 0, "first_ok": -1}
    if len(s) < 1 or np.all(pos_info == -1):
        out["status"] = S_POST_NO_POS
        return _pad(out, 0)
    rows = block_rows(pos_info)
    nb = len(rows)
    out["num_blocks"] = nb
    if nb > MAX_HITS:
        out["status"] = E_CAPACITY
        return _pad(out, 0)
    _pad(out, nb)
    for i, row in enumerate(rows):
        b = decode_block(s, pos_info[row + 1:row + 5, 0], ov, tsc)
        if b is None:
            continue
        out["ok"][i], out["pos"][i] = float(b["ok"]), pos_info[row + 1, 0]
        for name in ("corrected", "ts_err", "steal", "mean_slope", "amp"):
            out[name][i] = b[name]
        out["octets"][i], out["soft"][i], out["min_soft"][i], out["min_merge_margin"][i] = b["octets"], b["soft"], b["min_soft"], b["margin"]
    oks = [i for i in range(nb) if out["ok"][i] == 1.0]
    out["num_ok"] = len(oks)
    if oks:
        out["first_ok"] = oks[0] + 1
    else:
        out["status"] = S_BCCH_NO_DECODE
    return out


def _pad(out, nb):
    for name in PER_BLOCK + ("min_merge_margin",):
        out[name] = np.full(nb, np.nan)
    out["soft"] = np.full((nb, 456), np.nan)
    out["min_soft"] = np.full((nb, 4), np.nan)
    out["octets"] = np.zeros((nb, 23), dtype=np.uint8)
    return out


def margins_ok(res):
    """the condition every compared block must meet in the restatement (evaluated blocks only)"""
    ev = ~np.isnan(res["ok"])
    return bool(np.all(res["min_soft"][ev] >= MARGIN) and np.all(res["min_merge_margin"][ev] >= MARGIN))


def report(res):
    """the lines gsmcal_BCCH_decode leaves in the call report"""
    if res["status"] == S_POST_NO_POS:
        return ""
    head = "BCCH blocks %d decoded %d\n" % (res["num_blocks"], res["num_ok"])
    if res["status"] != 0:
        return head + "Fail to decode the BCCH blocks.\n"
    f = synth.si_fields(res["octets"][res["first_ok"] - 1])
    return head + "System information type %d cell identity %d LAI %d-%d-%d\n" % (f["si_type"], f["cell_id"], f["mcc"], f["mnc"], f["lac"])


# ---- inputs shared by the CPU and the GPU tests ------------------------------------------------------------------------------
def decimate_by_2(r, pos_info):
    """the 8x stream and its table at 4x (tests/sch_decode_ref.py has the same)"""
    pi4 = np.array(pos_info, dtype=np.float64)
    pi4[:, 0] = np.floor((pi4[:, 0] - 1) / 2) + 1
    return np.ascontiguousarray(np.asarray(r)[::2]), pi4


CHAIN_TSC = 5
# (name, dongle, snr_db): dongles 0, 3, 5 at their default SNR and dongle 4 at 8 dB
CHAIN_CASES = (("d0", 0, None), ("d3", 3, None), ("d5", 5, None), ("d4_8dB", 4, 8.0))


def chain_si(dongle):
    """what the chain case of `dongle` broadcasts: SI3 and SI4 in alternating multiframes"""
    return np.stack([synth.si3_octets(1000 * dongle + 17, 262, 2 + dongle, 0x1200 + dongle),
                     synth.si4_octets(262, 2 + dongle, 0x1200 + dongle)])


def chain_stream_args(name):
    _, dongle, snr = next(c for c in CHAIN_CASES if c[0] == name)
    return dict(dongle=dongle, snr_db=snr, tsc=CHAIN_TSC, si=chain_si(dongle))


def planted_octets(truth, octets):
    """does a decoded block equal one of the stream's planted blocks?"""
    return any(np.array_equal(octets, b) for b in truth["si"])


def burst_bits(e, tsc):
    """the 148 bits of a normal burst around e(0..115)"""
    e = np.asarray(e, dtype=np.int8)
    return np.concatenate([np.zeros(3, np.int8), e[:58], synth.TSC[tsc], e[58:], np.zeros(3, np.int8)])


DESIGNED_LEAD = 40
DESIGNED_TSC = 3
DESIGNED_SI = synth.si3_octets(0xBEEF, 901, "70", 0x0102)


def designed_stream(ov, blocks, tsc=DESIGNED_TSC, f=300.0, noise=0.02, seed=0, lead=DESIGNED_LEAD):
    """One designed stream: per entry e4 of `blocks` ((4, 116) bits) an SCH-typed row one frame ahead and four normal bursts at frame
    offsets 0..3, block b starting 51 frames behind block b-1's, from sample `lead`; mixed with exp(2 pi i f n / fs), with complex
    white noise of standard deviation `noise` per component.  Returns (s, pos_info): the type-1 row (whose samples nothing reads)
    and the four type-2 rows per block, 1-based starts.  The stream ends at the last burst's symbol 144."""
    rng = np.random.default_rng(7000 * ov + seed)
    g = synth.gmsk_frequency_pulse(sps=ov)
    blen, fl = 148 * ov, 1250 * ov
    starts = [lead + (51 * b + fr) * fl for b in range(len(blocks)) for fr in range(4)]
    n = starts[-1] + 144 * ov + delta(ov) + 1
    s = np.zeros(n + 4 * ov, dtype=np.complex128)
    pos = []
    for i, st in enumerate(starts):
        b, fr = divmod(i, 4)
        if fr == 0:
            pos.append((max(st + 1 - fl, 1), 1))
        padded = np.concatenate([np.zeros(4, np.int8), burst_bits(blocks[b][fr], tsc), np.zeros(4, np.int8)])
        s[st:st + blen] = synth.gmsk_modulate(synth.diff_precode(padded), ov, g)[4 * ov:4 * ov + blen] * np.exp(1j * rng.uniform(0, 6.28))
        pos.append((st + 1, 2))
    s = s[:n]
    s = s * np.exp(2j * np.pi * f * np.arange(n) / (synth.SYMBOL_RATE * ov))
    s = s + noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return s, np.array(pos, dtype=np.float64)


def flipped(e4):
    """a block with a run of 30 coded bits flipped (c(100..129), through the interleaver): more than the code corrects"""
    e4 = np.array(e4)
    for k in range(100, 130):
        B, j = _MAP[k]
        e4[B, j if j < 57 else j + 2] ^= 1
    return e4


DESIGNED_KINDS = ("clean", "flipped", "good_bad", "bad_good")


def designed_case(ov, kind):
    """-> (s, pos_info, tsc, expectation dict(ok, status, first_ok))"""
    e = synth.bcch_block_encode(DESIGNED_SI)
    blocks = {"clean": [e], "flipped": [flipped(e)], "good_bad": [e, flipped(e)], "bad_good": [flipped(e), e]}[kind]
    s, pos = designed_stream(ov, blocks, seed=DESIGNED_KINDS.index(kind))
    ok = {"clean": [1], "flipped": [0], "good_bad": [1, 0], "bad_good": [0, 1]}[kind]
    return s, pos, DESIGNED_TSC, {"ok": ok, "status": 0 if any(ok) else S_BCCH_NO_DECODE, "first_ok": ok.index(1) + 1 if any(ok) else -1}


def last_read(pos, ov):
    """1-based index of the last sample the burst at `pos` reads: symbol 144"""
    return int(pos) + 144 * ov + delta(ov)


# ---- many one-block streams, encoded and modulated in one vectorised pass ----------------------------------------------------
MANY_LEAD = 10
MANY_TSC = 6


def encode_many(octets):
    """bcch_block_encode for (count, 23) octets, written independently of it: the Fire parity as the XOR of the remainders of the
    set bits -> (count, 4, 116) int8"""
    o = np.asarray(octets, dtype=np.uint8)
    count = len(o)
    d = np.unpackbits(o, axis=1, bitorder="little")                   # d(8n + k) = bit k of octet n
    unit = np.array([synth.fire_remainder(np.eye(224, dtype=np.int8)[i]) for i in range(184)], dtype=np.int64)
    rem = np.full(count, synth.FIRE_ONES, dtype=np.int64)
    for k in range(184):
        rem ^= d[:, k] * unit[k]
    par = ((rem[:, None] >> (39 - np.arange(40))[None, :]) & 1).astype(np.uint8)
    z = np.concatenate([np.zeros((count, 4), np.uint8), d, par, np.zeros((count, 4), np.uint8)], axis=1)
    c = np.empty((count, 456), dtype=np.int8)
    c[:, 0::2] = z[:, 4:] ^ z[:, 1:-3] ^ z[:, :-4]
    c[:, 1::2] = z[:, 4:] ^ z[:, 3:-1] ^ z[:, 1:-3] ^ z[:, :-4]
    e = np.ones((count, 4, 116), dtype=np.int8)
    j = _MAP[:, 1]
    e[:, _MAP[:, 0], np.where(j < 57, j, j + 2)] = c
    return e


def many_geometry(ov):
    """(samples per stream, the four 1-based starts): four bursts 150 symbols apart, the smallest layout"""
    starts = [MANY_LEAD + 1 + 150 * ov * fr for fr in range(4)]
    return last_read(starts[3], ov), starts


def many_streams(count, ov, f=200.0, first=0):
    """`count` streams of the smallest length, one noiseless block each, stream i carrying si3_octets(cell identity i mod 65536, MCC
    100 + i div 65536, MNC 1, LAC i mod 1000).  Returns (s (count, n) complex, octets (count, 23), pos_info (5, 2)).
    The modulator is synth.gmsk_modulate's, evaluated through a table (tests/test_bcch_decode_cpu.py compares the two): the
    phase at sample i of symbol n is pi/2 times the sum of the pre-coded symbols up to n - 4, whose pulses are complete, plus the
    partial pulses of the last four, so a sample takes one of 17 * 4 * 16 * 148 * ov values per burst."""
    i = first + np.arange(count, dtype=np.int64)
    octets = np.tile(synth.si3_octets(0, 100, 1, 0), (count, 1)).astype(np.int64)
    cid, lac, mcc = i % 65536, i % 1000, 100 + i // 65536
    octets[:, 3], octets[:, 4] = cid >> 8, cid & 255
    octets[:, 5], octets[:, 6] = ((mcc // 10) % 10) << 4 | (mcc // 100), 0xF0 | (mcc % 10)
    octets[:, 8], octets[:, 9] = lac >> 8, lac & 255
    e = encode_many(octets)
    n, starts = many_geometry(ov)
    bits = np.zeros((count, 4, 156), dtype=np.int8)                    # 4 guard bits, the burst, 4 guard bits
    bits[:, :, 7:65], bits[:, :, 65:91], bits[:, :, 91:149] = e[:, :, :58], synth.TSC[MANY_TSC][None, None, :], e[:, :, 58:]
    one = np.ones((count, 4, 156), dtype=np.int8)                      # the pre-coded bits: 1 where the bit equals its predecessor
    one[:, :, 1:] = bits[:, :, 1:] == bits[:, :, :-1]
    one[:, :, 0] = bits[:, :, 0] == 0
    done = np.cumsum(2 * one - 1, axis=2, dtype=np.int32)              # the sum of the pre-coded symbols +-1 up to each bit
    quarter = done[:, :, 0:148] & 3                                    # symbol n = bit n + 4: pi/2 times the sum up to n, modulo 2 pi
    pat = sum(one[:, :, 4 - d:152 - d].astype(np.int32) << d for d in range(4))
    G = np.concatenate([np.cumsum(synth.gmsk_frequency_pulse(sps=ov)), [0.5]])
    dd, ii = np.arange(4)[None, :, None], np.arange(ov)[None, None, :]
    sign = 2.0 * ((np.arange(16)[:, None, None] >> dd) & 1) - 1.0
    phi = math.pi * np.sum(sign * G[dd * ov + ii], axis=1)             # (16, ov): the last four symbols' partial pulses
    s = np.zeros((count, n), dtype=np.complex128)
    for fr in range(4):
        t_abs = starts[fr] - 1 + np.arange(148 * ov).reshape(148, ov)
        tab = np.exp(1j * (0.37 * np.arange(17)[:, None, None, None, None] + 0.5 * math.pi * np.arange(4)[None, :, None, None, None] +
                           phi[None, None, :, None, :] + (2.0 * math.pi * f / (synth.SYMBOL_RATE * ov)) * t_abs[None, None, None, :, :]))
        idx = (((((i + fr) % 17).astype(np.int32)[:, None] * 4 + quarter[:, fr]) * 16 + pat[:, fr]) * 148 + np.arange(148, dtype=np.int32)[None, :])
        keep = min(148 * ov, n - (starts[fr] - 1))                       # the stream ends at the last burst's symbol 144
        s[:, starts[fr] - 1:starts[fr] - 1 + keep] = tab.reshape(-1, ov)[idx].reshape(count, 148 * ov)[:, :keep]
    pos = np.array([(1.0, 1.0)] + [(float(p), 2.0) for p in starts])
    return s, octets.astype(np.uint8), pos


def many_streams_direct(count, ov, f=200.0, first=0):
    """many_streams through synth.gmsk_modulate, burst by burst (for small counts: the check of the table above)"""
    _, octets, pos = many_streams(1, ov)
    n, starts = many_geometry(ov)
    g = synth.gmsk_frequency_pulse(sps=ov)
    out = []
    for i in range(first, first + count):
        o = synth.si3_octets(i % 65536, 100 + i // 65536, 1, i % 1000)
        e = synth.bcch_block_encode(o)
        s = np.zeros(n + 4 * ov, dtype=np.complex128)
        for fr in range(4):
            padded = np.concatenate([np.zeros(4, np.int8), burst_bits(e[fr], MANY_TSC), np.zeros(4, np.int8)])
            s[starts[fr] - 1:starts[fr] - 1 + 148 * ov] = synth.gmsk_modulate(synth.diff_precode(padded), ov, g)[4 * ov:152 * ov] * np.exp(0.37j * ((i + fr) % 17))
        out.append(s[:n] * np.exp(2j * np.pi * f * np.arange(n) / (synth.SYMBOL_RATE * ov)))
    return np.stack(out)


# ---- the exits and edges the GPU test walks through (tests/test_bcch_decode_cpu.py asserts the margins of every one) ---------
def repeat_blocks(pos, count):
    """`count` blocks that all point at the designed stream's four bursts: count * 5 rows"""
    return np.concatenate([pos] * count)


def edge_cases(ov):
    """name -> (s, pos_info, tsc): the designed stream at `ov` and its variations"""
    s, pos, tsc, _ = designed_case(ov, "clean")
    odd = [np.nan, -5.0, 0.0, 1e300, np.inf, float(len(s))]
    rows = []
    for q, bad in enumerate(odd):                                      # one bad start per block, at burst q mod 4
        blk = pos.copy()
        blk[1 + q % 4, 0] = bad
        rows.append(blk)
    return {
        "wrong_tsc": (s, pos, (tsc + 1) % 8),
        "no_type2": (s, np.array([[1.0, 0.0], [500.0, 1.0]]), tsc),
        "run_of_three": (s, pos[:4], tsc),
        "run_of_three_then_other": (s, np.concatenate([pos[:4], [[700.0, 0.0]], pos]), tsc),
        "blocks24": (s, repeat_blocks(pos, 24), tsc),
        "one_short": (s[:-1], pos, tsc),
        "odd_positions": (s, np.concatenate(rows + [pos]), tsc),
    }
