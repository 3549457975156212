"""Shared inputs of the impaired-capture tests: 102-frame captures of dongles 0 and 3 with planted payloads, impaired at byte
level the way a real front end and a real band impair them -- a second cell on the channel, a neighbour carrier, echoes,
clipping, a faint signal, fades and drop-outs, a CW spur on and off the FCCH tone, DC steps and offsets, I/Q imbalance, a
carrier and a noise level at and beyond what synth draws -- and nothing cut.  Every other capture of the suite is one GSM carrier
in white noise at 70 LSB (synth.make_stream) or a byte-level cut of one (tests/exit_paths.py): the certified shortcuts of the
chain (the coarse detector's certified scan and the early stop of its SNR rounds, the Parseval certificate of k_fine_cert, the
hop-window decisions, the DC-residue floor of snr_from_power) are argued from bounds on the data, and these are the data that
strain the bounds.

All impairments are deterministic:
    to_c(raw)   (I - 127.5) + 1j (Q - 127.5)
    to_raw(y)   clip(floor(re/im + dc + 0.5), 0, 255), dc = (127.4, 127.6) unless given
    a = to_c(base capture), t = sample index, N = 1 020 000
The base captures carry a planted training sequence code, BSIC, frame number and system information, so that the follow-up
family (FCCH_demod, BCCH_demod, SCH_decode, BCCH_decode, pair_coherence) has a truth to be held to on the cases that calibrate.
Each case names the exit it is DESIGNED to take (include/gsmcal.h GSMCAL_S_*, 0 = calibrates); tests/test_impaired_cpu.py holds
the oracle to that design, so a change of synth cannot empty the GPU test unnoticed.  Where planting the payloads or the
re-quantisation moved a case across a threshold against the un-planted design, its gain was changed by a small amount until the
designed exit was back; those cases say so.

Plain module: numpy, synth and the oracle only (the follow-up workers at the end import the restatements of tests/*_ref.py when
they run) -- nothing here touches the GPU, so it is safe in spawned pool workers."""
import math

import numpy as np

from gsmcal import synth
from oracle import gsmcal_oracle as oracle

FC = 957.4e6
NUM_FRAMES = 102
N = NUM_FRAMES * synth.FRAME_OV
DC = (127.4, 127.6)
# what the base captures carry: name -> (dongle, tsc, bsic, multiframes before the first frame, cell identity); the BSIC's low
# three bits are the colour code = the training sequence code; SI3 and SI4 alternate from multiframe to multiframe
PLANTED = {"d0": (0, 5, 0o15, 700, 4017), "d3": (3, 2, 0o32, 31000, 7017)}
MCC, MNC, LAC = 262, 3, 0x1234


def coef():
    return synth.fir1(46, 200e3 / synth.FS)


def planted_args(base):
    """synth.make_stream arguments of a base capture with its payloads planted"""
    dongle, tsc, bsic, mf, cell = PLANTED[base]
    sf = synth.make_stream(dongle=dongle, num_frames=1)[1]["start_frame"]
    si = np.stack([synth.si3_octets(cell, MCC, MNC, LAC), synth.si4_octets(MCC, MNC, LAC)])
    return dict(dongle=dongle, tsc=tsc, bsic=bsic, fn0=51 * mf + sf, start_frame=sf, si=si)


def to_c(raw):
    raw = np.asarray(raw, dtype=np.float64)
    return (raw[0::2] - 127.5) + 1j * (raw[1::2] - 127.5)


def to_raw(y, dc=DC):
    out = np.empty(2 * len(y), dtype=np.float64)
    out[0::2] = y.real + dc[0]
    out[1::2] = y.imag + dc[1]
    return np.clip(np.floor(out + 0.5), 0, 255).astype(np.uint8)


def db(x):
    return 10.0 ** (x / 20.0)


def delayed(a, d):
    out = np.zeros_like(a)
    out[d:] = a[:len(a) - d]
    return out


def gated(a, level):
    """the two gates of the dropout cases on one capture each: [300000, 420000) and [330000, 360000)"""
    long_, short = a.copy(), a.copy()
    long_[300000:420000] *= level
    short[330000:360000] *= level
    return long_, short


# the pair_coherence partners of "plain": the same transmission through another channel, so lag0 = 0
PAIR_PARTNERS = ("echo8", "echo24", "echo3", "adjacent0", "adjacent+10", "cochannel-10", "fade", "clip3", "clip10")


def build():
    """-> list of case dicts {name, raw, status, group, base, follow, truth}: group "mixed" = the N-sample cases of the one
    batch, "own" = a length of its own; base = the planted capture the case comes from ("d0" / "d3"); follow: the case takes
    part in the follow-up tests (status 0 with planted payloads); truth: synth's truth dict of the base capture"""
    made = {b: synth.make_stream(num_frames=NUM_FRAMES, **planted_args(b)) for b in PLANTED}
    a, a3 = to_c(made["d0"][0]), to_c(made["d3"][0])
    t = np.arange(N, dtype=np.float64)
    cases = []

    def add(name, raw, status, base="d0", group="mixed", truth=None):
        cases.append({"name": name, "raw": np.ascontiguousarray(raw), "status": status, "group": group, "base": base,
                      "follow": status == 0, "truth": made[base][1] if truth is None else truth})

    add("plain", to_raw(a), 0)                                   # the re-quantised twin of the base capture
    # another cell on the channel, with its own FCCH timing
    b = to_c(synth.make_stream(dongle=5, seed=99, num_frames=NUM_FRAMES)[0])
    # (-10 and -9 dB move the total sampling ppm by 1.09: the fine stage's estimate goes from 33.70 to 38.04, the SCH stage takes
    # 5.43 back; at -8 dB the two stages still cancel to 2e-4.  -9 dB was added for that: with the payloads planted the move
    # sits there and at -10 dB, not at -8 dB)
    for g_db, status in ((-20, 0), (-10, 0), (-9, 0), (-8, 0), (-6, 2), (-5, 2), (-3, 1), (0, 1)):
        add(f"cochannel{g_db}" if g_db else "cochannel0", to_raw(a + db(g_db) * b), status)
    # a traffic-only carrier 200 kHz up
    tr = to_c(synth.make_stream(dongle=6, seed=98, num_frames=NUM_FRAMES, bcch=False)[0]) * np.exp(2j * math.pi * 200e3 / synth.FS * t)
    add("adjacent0", to_raw(0.5 * a + 0.5 * tr), 0)
    add("adjacent+10", to_raw(0.5 * a + 0.5 * db(10) * tr), 0)
    for d, g in ((8, 0.5), (24, 0.9), (3, 1.0)):
        add(f"echo{d}", to_raw(0.6 * (a + g * np.exp(1.3j) * delayed(a, d))), 0)
    add("d3plain", to_raw(a3), 0, base="d3")                     # the twin the dongle-3 cases are measured against
    add("d3echo40", to_raw(0.5 * (a3 + 0.7 * np.exp(2.1j) * delayed(a3, 40))), 0, base="d3")
    add("clip3", to_raw(3.0 * a), 0)                             # most bytes on the rails
    add("clip10", to_raw(10.0 * a), 0)
    add("d3clip10", to_raw(10.0 * a3), 0, base="d3")
    # 2.1 ... 0.7 LSB of signal.  faint0.015 runs at a gain of 0.0155: with the payloads planted 0.015 leaves at 7 like 0.01, and
    # 0.0155 brings the designed SCH spacing exit (9) back.  faint0.0195 was added: the only case here that fails the fine
    # stage's SNR gate (6)
    for name, k, status in (("faint0.03", 0.03, 0), ("faint0.02", 0.02, 4), ("faint0.0195", 0.0195, 6), ("faint0.015", 0.0155, 9),
                            ("faint0.01", 0.01, 7)):
        add(name, to_raw(k * a), status)
    add("fade", to_raw(a * (0.55 + 0.45 * np.cos(2 * math.pi * t / 230000.0))), 0)
    # a stretch of constant bytes inside a live capture / the same two gates at 0.02 instead of 0
    for tag, level, st in (("dropout", 0.0, (4, 0)), ("deepfade", 0.02, (0, 0))):
        for which, y, status in zip(("120k", "30k"), gated(a, level), st):
            add(f"{tag}{which}", to_raw(y), status)
    # a CW on the FCCH tone (+67.7 kHz), on its image and elsewhere in the band
    for name, f, g_db, status in (("spur+67-30", 67708.33, -30, 0), ("spur+67-20", 67708.33, -20, 4), ("spur+67-15", 67708.33, -15, 4),
                                  ("spur+67-10", 67708.33, -10, 4), ("spur+67+0", 67708.33, 0, 1), ("spur-67+0", -67708.33, 0, 1),
                                  ("spur+30+0", 30000.0, 0, 1)):
        add(name, to_raw(0.5 * (a + 70.0 * db(g_db) * np.exp(2j * math.pi * f / synth.FS * t))), status)
    for name, step, status in (("dcstep5", 5.0, 4), ("dcstep10", 10.0, 4), ("dcstep20", 20.0, 4), ("dcstep30+20j", 30.0 + 20.0j, 1)):
        add(name, to_raw(0.6 * a + step * (t >= N // 2)), status)
    add("dc+60", to_raw(0.5 * a, dc=(187.0, 70.0)), 0)
    # what synth.make_stream can impair itself, at and beyond the range it draws from
    for name, kw in (("iq1.2_10deg", dict(iq_gain=1.2, iq_phase_deg=10.0)), ("carrier+39.9", dict(carrier_ppm=39.9)),
                     ("carrier-70", dict(carrier_ppm=-70.0)), ("snr3", dict(snr_db=3.0)), ("snr0", dict(snr_db=0.0))):
        raw, truth = synth.make_stream(num_frames=NUM_FRAMES, **planted_args("d0"), **kw)
        add(name, raw, 0, truth=truth)
    # shorter captures, each a length of its own: 62 frames is the shortest that calibrates here
    for frames in (62, 72):
        raw, truth = synth.make_stream(num_frames=frames, **planted_args("d0"))
        add(f"plain{frames}", raw, 0, group="own", truth=truth)
    for c in cases:
        assert c["group"] != "mixed" or len(c["raw"]) == 2 * N, (c["name"], len(c["raw"]))
    return cases


def ordered(cases):
    """the mixed cases ordered so that neighbouring streams leave at different stages where the counts allow it (greedy: the most
    frequent status left that is not the last one's, as tests/test_gpu_exit_paths.py orders its batch)"""
    rest = [k for k in cases if k["group"] == "mixed"]
    mixed = []
    while rest:
        last = mixed[-1]["status"] if mixed else None
        count = {}
        for k in rest:
            count[k["status"]] = count.get(k["status"], 0) + 1
        pick = max((st for st in count if st != last), key=lambda st: count[st], default=last)
        nxt = next(k for k in rest if k["status"] == pick)
        rest.remove(nxt)
        mixed.append(nxt)
    return mixed


def calibrates(orc):
    """status 0, or 11 with a table"""
    return orc["status"] == 0 or (orc["status"] == 11 and not np.all(orc["pos_info"] == -1))


def window_powers(raw, c):
    """the power spectra of every 16-point window of the decimated stream, in the reference's operation order"""
    s = oracle.matlab_filter(c, oracle.raw2iq(np.asarray(raw, dtype=np.float64)))[0::64]
    return oracle._power_spectra(s, 1, len(s) - 15, 16)


def residue_floor(raw, c):
    """the total window power at or below which the batch path takes a 16-point window for rounding residue of its DC removal and
    returns NaN (kernels_detect.h snr_from_power, DecView::floor2): (16 |mean sum(coef)| 2^-46)^2"""
    raw = np.asarray(raw, dtype=np.float64)
    return 256.0 * (np.mean(raw[0::2]) ** 2 + np.mean(raw[1::2]) ** 2) * float(np.sum(c)) ** 2 * 2.0 ** -92


def scan_job(job):
    """job = (raw, coef) -> oracle.scan_capture dict plus every window's SNR, the counts of +inf / -inf / NaN among them, and the
    smallest non-zero total window power beside the DC-residue floor (pool worker)"""
    import os
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    raw, c = job
    out = oracle.scan_capture(raw, c)
    p = window_powers(raw, c)
    w = oracle._window_snr(p)
    tot = np.sum(p, axis=1)
    out["windows"] = w
    out["window_kinds"] = (int(np.sum(np.isposinf(w))), int(np.sum(np.isneginf(w))), int(np.sum(np.isnan(w))))
    out["min_power"], out["zero_power"], out["floor"] = float(np.min(tot[tot > 0])), int(np.sum(tot == 0)), residue_floor(raw, c)
    return out


# ---- the follow-up family on the cases that calibrate ------------------------------------------------------------------------
# Each restatement carries a guard that keeps a decision off a tie, and the GPU tests compare only what passes it:
#   SCH_decode     min_merge_margin >= sch_decode_ref.MARGIN * amp, per burst
#   BCCH_decode    bcch_decode_ref.margins_ok: every |soft| and the merge margin >= MARGIN * amp, per block
#   BCCH_demod     winner / runner-up >= bcch_demod_ref.MIN_RATIO, per burst
#   FCCH_demod     |noise_power / band_power| >= 1e-3, per burst (the SNR's NaN decision)
#   pair_coherence pair_coherence_ref.ties_ok's three conditions, per burst
# guard_counts() says how many of a stream's bursts each guard would exclude.
MAX_POS_ROWS = 144


def raw_table(pos_info):
    """pos_info (rows, 2) -> the (2, MAX_POS_ROWS) table the batch forms read, -1 behind the rows"""
    t = -np.ones((2, MAX_POS_ROWS))
    pi = np.atleast_2d(np.asarray(pos_info, dtype=np.float64))
    t[:, :len(pi)] = pi.T
    return t


def followup_job(job):
    """job = (r, pos_info, tsc, keep_r) -> {"fcch", "bcch", "sch", "si"}: the four single-stream restatements at 8x on one corrected
    stream and its table (pool worker); BCCH_demod's rotated stream is dropped unless keep_r"""
    import os
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    import bcch_decode_ref
    import bcch_demod_ref
    import fcch_demod_ref
    import sch_decode_ref
    r, pos_info, tsc, keep_r = job
    out = {"fcch": fcch_demod_ref.fcch_demod(r, pos_info, 8, FC),
           "bcch": bcch_demod_ref.bcch_demod(r, pos_info, synth.normal_training_sequences(8), 8, FC),
           "sch": sch_decode_ref.sch_decode(r, pos_info, 8),
           "si": bcch_decode_ref.bcch_decode(r, pos_info, tsc, 8)}
    if not keep_r:
        out["bcch"]["r"] = None
    return out


def pair_job(job):
    """job = (r_a, r_b, pos_info_a, pos_info_b) -> pair_coherence_ref.pair_coherence of the pair (a, b) at 8x with lag0 = 0 and
    the default lag range (pool worker)"""
    import os
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    import pair_coherence_ref
    ra, rb, pa, pb = job
    r = np.zeros((2, max(len(ra), len(rb))), dtype=np.complex128)
    r[0, :len(ra)], r[1, :len(rb)] = ra, rb
    pi = np.stack([raw_table(pa), raw_table(pb)])
    return pair_coherence_ref.pair_coherence(r, np.array([len(ra), len(rb)], dtype=np.int64), pi, 8, 0, 1, 0)


def guard_counts(res):
    """followup_job's result -> {function: (bursts looked at, bursts its guard excludes)}"""
    import bcch_decode_ref
    import bcch_demod_ref
    import sch_decode_ref
    out = {}
    w = res["sch"]
    ev = ~np.isnan(w["ok"])
    out["sch"] = (int(np.sum(ev)), int(np.sum(w["min_merge_margin"][ev] < sch_decode_ref.MARGIN * w["amp"][ev])))
    w = res["si"]
    ev = ~np.isnan(w["ok"])
    bad = np.any(w["min_soft"][ev] < bcch_decode_ref.MARGIN, axis=1) | (w["min_merge_margin"][ev] < bcch_decode_ref.MARGIN)
    out["si"] = (int(np.sum(ev)), int(np.sum(bad)))
    w = res["bcch"]
    done = ~np.isnan(w["max_idx"])
    out["bcch"] = (int(np.sum(done)), int(np.sum(w["ratio"][done] < bcch_demod_ref.MIN_RATIO)))
    w = res["fcch"]
    out["fcch"] = (len(w["noise_ratio"]), int(np.sum(np.abs(w["noise_ratio"]) < 1e-3)))
    return out


def pair_guard_counts(want, gap=1e-6, curvature=1e-4, coh=1e-6):
    """pair_job's result -> (bursts evaluated, bursts pair_coherence_ref.ties_ok's conditions exclude)"""
    ev = want["evaluated"]
    inner = ev & ~want["edge"]
    with np.errstate(invalid="ignore"):
        bad = (ev & (want["gap"] < gap)) | (inner & ((want["curvature"] < curvature) | (want["coh_margin"] < coh)))
    return int(np.sum(ev)), int(np.sum(bad))


def recovered(k, pos_info, res):
    """does each restatement find what was planted in case k?  -> {"sch": BSIC and every decoded frame number, "tsc": the training
    sequence code BCCH_demod settles on, "si": every block that passes the Fire code is a planted one and at least one does}"""
    import sch_decode_ref
    truth = k["truth"]
    tsc = PLANTED[k["base"]][1]
    sch, si, bc = res["sch"], res["si"], res["bcch"]
    sp = pos_info[pos_info[:, 1] == 1, 0]
    ok = sch["ok"] == 1.0
    want_fn = sch_decode_ref.expected_fn(truth, sp, 8)
    out = {"sch": bool(sch["status"] == 0 and sch["bsic"] == truth["bsic"] and np.any(ok) and np.all(sch["bsic_b"][ok] == truth["bsic"])
                       and np.array_equal(sch["fn"][ok], want_fn[ok])),
           "tsc": bool(bc["status"] == 0 and bc["idx"] == tsc + 1)}
    good = np.nonzero(si["ok"] == 1.0)[0]
    out["si"] = bool(si["status"] == 0 and len(good) >= 1 and all(any(np.array_equal(si["octets"][i], b) for b in truth["si"]) for i in good))
    return out


# the cases in which a restatement does NOT find the planted payload, run on the oracle's corrected stream: name -> the functions
# of recovered() that miss.  None here does: every case that calibrates still decodes.  tests/test_impaired_cpu.py pins this;
# tests/test_gpu_impaired.py asserts the planted truth on the GPU wherever the restatement recovers it.
NOT_RECOVERED = {}
