"""fp64 restatement of SCH_decode, written line by line from its definition, for the SCH_decode tests.

This is the project's own function, not a port: SCH_demod.m has no outputs and demodulates with Communications Toolbox code.
The definition, per type-1 row of pos_info with 1-based start p and ov in {2, 4, 8}:
    1  y_k = s(p + k*ov + delta) * (-j)^k for k = 3..144, delta = (5*ov - 1) div 2; a burst whose reads leave the stream (or whose
       p is NaN or < 1) is not evaluated: NaN columns, no error
    2  a_i = 1 - 2*SCH_TRAINING_BITS[i]; h1 = sum_{i<32} y_{42+i} a_i, h2 = sum_{i>=32} y_{42+i} a_i, h = h1 + h2,
       slope = angle(h2 conj(h1)) / 32, amp = |h| / 64
    3  soft_k = Re(y_k conj(h)/|h| exp(-j slope (k - 73.5))), positive = bit 0
    4  a 16-state soft Viterbi over the 78 values soft[3..41], soft[106..144]: from state 0 to state 0, branch metric
       (+-soft[2k]) + (+-soft[2k+1]) added to the path metric, a strict > keeps the candidate whose older bit is 0
    5  ok: CRC remainder all ones, tail bits zero, T3' <= 4, T2 <= 25; ts_err: hard errors in the 64 training bits; corrected:
       Hamming distance between the hard channel bits and the re-encoded word
and per stream the consistency rule: among the ok bursts c_i counts the ok bursts j (i included) with the same BSIC and
(fn_j - fn_i - round((p_j - p_i)/(1250 ov))) mod 2715648 == 0; the anchor is the smallest i with the largest c_i; status 0 iff
c_anchor >= 2, else 14.

`sch_decode` returns a dict: status, num_sch, num_ok, num_consistent, bsic, fn_anchor, pos_anchor, mean_slope (the mean of
slope[] over the ok bursts, left to right; NaN without one) and per type-1 row (NaN where not evaluated) ok, bsic_b, fn, ts_err,
corrected, slope, amp; soft (num_sch, 148) NaN outside 3..144; u (num_sch, 39) uint8, 255 where not evaluated;
min_merge_margin per burst: the smallest metric difference at a compare-select along the surviving path (restatement only: the
GPU tests compare only bursts whose margin is at least MARGIN * amp).

Also here: the inputs the CPU and the GPU tests share."""
import importlib
import math

import numpy as np

synth = importlib.import_module("multi-rtl-sdr-calibration_amd.synth")

MAX_HITS = 24
HYPER = 2715648
S_POST_NO_POS, S_SCH_NO_DECODE, E_CAPACITY, E_UNSUPPORTED, E_ARG = 10, 14, -4, -6, -1
MARGIN = 1e-6                                                         # min_merge_margin >= MARGIN * amp for every compared burst
FC = 957.4e6


def matlab_round(x):
    return math.copysign(math.floor(abs(x) + 0.5), x)


def delta(ov):
    return (5 * ov - 1) // 2


def viterbi(soft78):
    """-> (u (39,) int8, min_merge_margin).  State = u(k-1)<<3 | u(k-2)<<2 | u(k-3)<<1 | u(k-4)."""
    pm = [-math.inf] * 16
    pm[0] = 0.0
    hist = [0] * 16                                                  # bit k of hist[s] = u(k) of the survivor into state s
    marg = [math.inf] * 16                                           # the smallest compare-select difference along that survivor
    for k in range(39):
        s0, s1 = float(soft78[2 * k]), float(soft78[2 * k + 1])
        npm, nh, nm = [0.0] * 16, [0] * 16, [0.0] * 16
        for ns in range(16):
            b = ns >> 3
            cand = []
            for old in (0, 1):                                       # the predecessor whose oldest bit u(k-4) is `old`
                p = ((ns & 7) << 1) | old
                c0 = b ^ ((p >> 1) & 1) ^ (p & 1)                    # u(k) + u(k-3) + u(k-4)
                c1 = c0 ^ ((p >> 3) & 1)                             # ... + u(k-1)
                bm = (-s0 if c0 else s0) + (-s1 if c1 else s1)
                cand.append(pm[p] + bm)
            take = 1 if cand[1] > cand[0] else 0                     # strict: the first candidate stays
            p = ((ns & 7) << 1) | take
            npm[ns] = cand[take]
            nh[ns] = hist[p] | (b << k)
            d = abs(cand[0] - cand[1]) if (cand[0] > -math.inf and cand[1] > -math.inf) else math.inf
            nm[ns] = min(marg[p], d)
        pm, hist, marg = npm, nh, nm
    u = np.array([(hist[0] >> k) & 1 for k in range(39)], dtype=np.int8)
    return u, marg[0]


def decode_burst(s, p, ov):
    """one type-1 row: None when it is not evaluated, else a dict of the per-burst results"""
    n = len(s)
    if not (p >= 1):                                                 # NaN or < 1
        return None
    dl = delta(ov)
    if not (p + 144 * ov + dl <= n):
        return None
    p = int(p)
    k = np.arange(3, 145)
    y = np.full(148, np.nan + 0j)
    y[3:145] = s[p + k * ov + dl - 1] * (-1j) ** (k % 4)             # 1
    a = 1.0 - 2.0 * synth.SCH_TRAINING_BITS.astype(np.float64)
    h1 = np.sum(y[42:74] * a[:32])                                   # 2
    h2 = np.sum(y[74:106] * a[32:])
    h = h1 + h2
    slope = np.angle(h2 * np.conj(h1)) / 32.0
    amp = abs(h) / 64.0
    kk = np.arange(148, dtype=np.float64)
    soft = np.real(y * (np.conj(h) / abs(h)) * np.exp(-1j * slope * (kk - 73.5)))     # 3
    soft78 = np.concatenate([soft[3:42], soft[106:145]])
    u, margin = viterbi(soft78)                                      # 4
    rem = synth.sch_crc_remainder(u[:35])                            # 5
    f = synth.sch_fields(u[:25])
    ok = rem == 0x3FF and not np.any(u[35:]) and f["t3p"] <= 4 and f["t2"] <= 25
    hard = (soft78 < 0).astype(np.int8)
    return {"ok": bool(ok), "bsic": f["bsic"], "fn": f["fn"], "fields": f, "crc": rem,
            "ts_err": int(np.sum((soft[42:106] < 0).astype(np.int8) != synth.SCH_TRAINING_BITS)),
            "corrected": int(np.sum(hard != synth.sch_conv_encode(u))), "slope": float(slope), "amp": float(amp),
            "soft": soft, "u": u.astype(np.uint8), "margin": margin}


def sch_decode(s, pos_info, ov, r_len=None):
    pos_info = np.atleast_2d(np.asarray(pos_info, dtype=np.float64))
    if ov not in (2, 4, 8):
        return {"status": E_UNSUPPORTED}
    s = np.asarray(s, dtype=np.complex128).ravel()
    if r_len is not None:
        s = s[:max(int(r_len), 0)]
    out = {"status": 0, "num_sch": 0, "num_ok": 0, "num_consistent": 0, "bsic": -1, "fn_anchor": -1, "pos_anchor": -1,
           "mean_slope": math.nan}
    if len(s) < 1 or np.all(pos_info == -1):
        out["status"] = S_POST_NO_POS
        return _pad(out, 0)
    pos = pos_info[pos_info[:, 1] == 1, 0]
    nb = len(pos)
    out["num_sch"] = nb
    if nb > MAX_HITS:
        out["status"] = E_CAPACITY
        return _pad(out, 0)
    _pad(out, nb)
    for i, p in enumerate(pos):
        b = decode_burst(s, p, ov)
        if b is None:
            continue
        out["ok"][i] = float(b["ok"])
        if b["ok"]:
            out["bsic_b"][i], out["fn"][i] = b["bsic"], b["fn"]
        for name in ("ts_err", "corrected", "slope", "amp"):
            out[name][i] = b[name]
        out["soft"][i], out["u"][i], out["min_merge_margin"][i] = b["soft"], b["u"], b["margin"]
    oks = [i for i in range(nb) if out["ok"][i] == 1.0]
    out["num_ok"] = len(oks)
    if oks:
        acc = 0.0
        for i in oks:
            acc += out["slope"][i]
        out["mean_slope"] = acc / len(oks)
    best, anchor = 0, -1
    for i in oks:
        c = 0
        for j in oks:
            dfr = matlab_round((pos[j] - pos[i]) / (1250.0 * ov))
            c += out["bsic_b"][j] == out["bsic_b"][i] and (out["fn"][j] - out["fn"][i] - dfr) % HYPER == 0
        if c > best:
            best, anchor = c, i
    out["num_consistent"] = best
    if best >= 2:
        out["bsic"], out["fn_anchor"], out["pos_anchor"] = int(out["bsic_b"][anchor]), int(out["fn"][anchor]), float(pos[anchor])
    else:
        out["status"] = S_SCH_NO_DECODE
    return out


def _pad(out, nb):
    for name in ("ok", "bsic_b", "fn", "ts_err", "corrected", "slope", "amp", "min_merge_margin"):
        out[name] = np.full(nb, np.nan)
    out["soft"] = np.full((nb, 148), np.nan)
    out["u"] = np.full((nb, 39), 255, dtype=np.uint8)
    return out


def report(res):
    """the lines gsmcal_SCH_decode leaves in the call report"""
    if res["status"] == S_POST_NO_POS:
        return ""
    head = "SCH bursts %d decoded %d consistent %d\n" % (res["num_sch"], res["num_ok"], res["num_consistent"])
    if res["status"] == 0:
        return head + "BSIC %d frame number %d at sample %d\n" % (res["bsic"], res["fn_anchor"], res["pos_anchor"])
    return head + "Fail to decode the SCH bursts.\n"


def sch_alignment(rows, ov, ref=0):
    """restatement of api.sch_alignment on a list of sch_decode results"""
    out = np.full(len(rows), np.nan)
    if rows[ref]["status"] != 0:
        return out
    for d, r in enumerate(rows):
        if r["status"] == 0:
            w = (r["fn_anchor"] - rows[ref]["fn_anchor"] + HYPER // 2) % HYPER - HYPER // 2
            out[d] = r["pos_anchor"] - rows[ref]["pos_anchor"] - w * 1250.0 * ov
    return out


# ---- inputs shared by the CPU and the GPU tests ------------------------------------------------------------------------------
def decimate_by_2(r, pos_info):
    """the 8x stream and its table at 4x (tests/bcch_demod_ref.py has the same)"""
    pi4 = np.array(pos_info, dtype=np.float64)
    pi4[:, 0] = np.floor((pi4[:, 0] - 1) / 2) + 1
    return np.ascontiguousarray(np.asarray(r)[::2]), pi4


CHAIN_CASES = (("d0", 0, 7), ("d3", 3, 1000), ("d5", 5, 31000), ("d3wrap", 3, None))


def chain_stream_args(name):
    """make_stream arguments of one chain case: bsic = 8*dongle + 5, fn0 a whole number of multiframes plus the stream's own
    start_frame; the case "d3wrap" starts three multiframes before the hyperframe wrap."""
    _, dongle, mf = next(c for c in CHAIN_CASES if c[0] == name)
    sf = synth.make_stream(dongle=dongle, num_frames=1)[1]["start_frame"]
    fn0 = (HYPER - 3 * 51 + sf) if mf is None else 51 * mf + sf
    return dict(dongle=dongle, bsic=8 * dongle + 5, fn0=fn0)


def expected_fn(truth, pos, ov, delay=23):
    """the frame number of the SCH burst at 1-based sample `pos` of the corrected stream at `ov`: the capture starts frac_start
    8x-samples into frame fn0, the front end's FIR delays by `delay` samples, the chain takes the clock error out"""
    p8 = (np.asarray(pos, dtype=np.float64) - 1.0) * (8 // ov) + 1.0
    return (truth["fn0"] + np.floor((p8 + delay + truth["frac_start"]) / 10000.0 + 0.5).astype(np.int64)) % HYPER


def burst_bits(coded):
    """the 148 bits of an SCH burst around 78 coded bits"""
    c = np.asarray(coded, dtype=np.int8)
    return np.concatenate([np.zeros(3, np.int8), c[:39], synth.SCH_TRAINING_BITS, c[39:], np.zeros(3, np.int8)])


def coded_with_fields(bsic, t1, t2, t3p):
    """a word with a valid CRC whose fields are set directly (for T3' = 6)"""
    val = {"BSIC": bsic, "T1": t1, "T2": t2, "T3P": t3p}
    d = np.array([(val[f] >> b) & 1 for f, b in synth.SCH_INFO_MAP], dtype=np.int8)
    rem = synth.sch_crc_remainder(np.concatenate([d, np.zeros(10, np.int8)])) ^ 0x3FF
    par = np.array([(rem >> (9 - i)) & 1 for i in range(10)], dtype=np.int8)
    return synth.sch_conv_encode(np.concatenate([d, par, np.zeros(4, np.int8)]))


def designed_stream(ov, coded_list, frames, f=300.0, noise=0.02, seed=0, lead=40):
    """SCH bursts carrying coded_list[i] at frame offsets frames[i] (1250*ov samples per frame) from sample `lead`, each modulated
    between 4 guard bits, mixed with exp(2 pi i f n / fs) and with complex white noise of standard deviation `noise` per
    component.  Returns (s, pos_info): type-1 rows, 1-based starts.  The stream ends with the last burst's 148th symbol."""
    rng = np.random.default_rng(1000 * ov + seed)
    g = synth.gmsk_frequency_pulse(sps=ov)
    blen, fl = 148 * ov, 1250 * ov
    n = lead + frames[-1] * fl + blen
    s = np.zeros(n, dtype=np.complex128)
    pos = np.zeros((len(frames), 2))
    for i, (c, fr) in enumerate(zip(coded_list, frames)):
        padded = np.concatenate([np.zeros(4, np.int8), burst_bits(c), np.zeros(4, np.int8)])
        st = lead + fr * fl
        s[st:st + blen] = synth.gmsk_modulate(synth.diff_precode(padded), ov, g)[4 * ov:4 * ov + blen] * np.exp(1j * rng.uniform(0, 6.28))
        pos[i] = st + 1, 1
    s = s * np.exp(2j * np.pi * f * np.arange(n) / (synth.SYMBOL_RATE * ov))
    s = s + noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return s, pos


DESIGNED_FRAMES = (0, 10, 20, 40, 51)
DESIGNED_FN0 = 51 * 1234 + 1
DESIGNED_BSIC = 43


DESIGNED_KINDS = ("clean", "flipped", "t3p6", "wrong_fn", "other_bsic", "wrap")


def designed_case(ov, kind):
    """the five-burst designed stream with one burst altered -> (s, pos_info, expectation dict)
    kind: "clean", "flipped" (burst 2: a run of coded bits flipped, the CRC fails), "t3p6" (burst 1: valid CRC, T3' = 6),
    "wrong_fn" (burst 3: valid CRC, a frame number one multiframe off its position), "other_bsic" (burst 4), "wrap" (clean, the
    last burst behind the hyperframe wrap)."""
    fn0 = HYPER - 50 if kind == "wrap" else DESIGNED_FN0
    fns = [(fn0 + f) % HYPER for f in DESIGNED_FRAMES]
    coded = [synth.sch_encode(DESIGNED_BSIC, fn) for fn in fns]
    ok, same = [1] * 5, [1] * 5
    if kind == "flipped":
        coded[2] = coded[2].copy()
        coded[2][20:34] ^= 1
        ok[2] = 0
    elif kind == "t3p6":
        coded[1] = coded_with_fields(DESIGNED_BSIC, 4, 3, 6)
        ok[1] = 0
    elif kind == "wrong_fn":
        coded[3] = synth.sch_encode(DESIGNED_BSIC, fns[3] + 51)
        same[3] = 0
    elif kind == "other_bsic":
        coded[4] = synth.sch_encode(DESIGNED_BSIC ^ 9, fns[4])
        same[4] = 0
    s, pos = designed_stream(ov, coded, DESIGNED_FRAMES, seed=DESIGNED_KINDS.index(kind))
    return s, pos, {"ok": ok, "num_ok": sum(ok), "num_consistent": sum(o and m for o, m in zip(ok, same)), "fn0": fns[0]}


def single_burst_stream(ov, fn=DESIGNED_FN0, bsic=DESIGNED_BSIC, seed=9):
    return designed_stream(ov, [synth.sch_encode(bsic, fn)], (0,), seed=seed)


def last_read(pos, ov):
    """1-based index of the last sample the burst at `pos` reads: symbol 144"""
    return int(pos) + 144 * ov + delta(ov)


# ---- many one-burst streams, encoded and modulated in one vectorised pass ----------------------------------------------------
def encode_many(bsic, fn):
    """sch_encode for arrays, written independently of it: the CRC as the XOR of the remainders of the set bits"""
    bsic, fn = np.asarray(bsic, dtype=np.int64), np.asarray(fn, dtype=np.int64)
    val = {"BSIC": bsic, "T1": fn // 1326, "T2": fn % 26, "T3P": (fn % 51 - 1) // 10}
    d = np.stack([(val[f] >> b) & 1 for f, b in synth.SCH_INFO_MAP], axis=1).astype(np.int64)
    unit = np.array([synth.sch_crc_remainder(np.eye(35, dtype=np.int8)[i]) for i in range(25)], dtype=np.int64)
    rem = np.bitwise_xor.reduce(d * unit[None, :], axis=1) ^ 0x3FF
    par = (rem[:, None] >> (9 - np.arange(10))[None, :]) & 1
    u = np.concatenate([d, par, np.zeros((len(fn), 4), np.int64)], axis=1)
    z = np.concatenate([np.zeros((len(fn), 4), np.int64), u], axis=1)
    c = np.empty((len(fn), 78), dtype=np.int8)
    c[:, 0::2] = z[:, 4:] ^ z[:, 1:-3] ^ z[:, :-4]
    c[:, 1::2] = z[:, 4:] ^ z[:, 3:-1] ^ z[:, 1:-3] ^ z[:, :-4]
    return c


MANY_LEAD = 10


def many_streams(count, ov, f=200.0):
    """`count` streams of 160*ov samples, one noiseless SCH burst each from sample MANY_LEAD, stream i with bsic i mod 64 and its
    own frame number.  Returns (s (count, 160*ov) complex, bsic, fn)."""
    i = np.arange(count, dtype=np.int64)
    fn = 51 * ((i * 41) % (HYPER // 51)) + 10 * (i % 5) + 1
    bsic = i % 64
    c = encode_many(bsic, fn)
    bits = np.zeros((count, 156), dtype=np.int8)
    bits[:, 7:46], bits[:, 46:110], bits[:, 110:149] = c[:, :39], synth.SCH_TRAINING_BITS[None, :], c[:, 39:]
    prev = np.concatenate([np.zeros((count, 1), np.int8), bits[:, :-1]], axis=1)
    a = 2.0 * (1 - np.abs(bits - prev)).astype(np.float64) - 1.0
    g = synth.gmsk_frequency_pulse(sps=ov)
    up = np.zeros((count, 156 * ov))
    up[:, ::ov] = a
    fq = np.zeros_like(up)
    for j, gj in enumerate(g):
        fq[:, j:] += gj * up[:, :up.shape[1] - j]
    ph = math.pi * np.cumsum(fq, axis=1)[:, 4 * ov:152 * ov]
    n = 160 * ov
    s = np.zeros((count, n), dtype=np.complex128)
    s[:, MANY_LEAD:MANY_LEAD + 148 * ov] = np.exp(1j * (ph + 0.37 * (i % 17)[:, None]))
    s *= np.exp(2j * np.pi * f * np.arange(n) / (synth.SYMBOL_RATE * ov))[None, :]
    return s, bsic, fn


TX_PAIR = dict(tx_key=7, start_frame=4, bsic=52, fn0=51 * 300 + 4)      # two dongles (0 and 3) that receive one transmission
