"""Shared inputs of the exit-path tests: captures built so that the batch chain leaves at a chosen early exit, or cuts its
pos_info table short at a chosen row, from raw bytes and with the default thresholds.

Two seeded 102-frame captures (dongles 0 and 3) are edited at byte level:
  cut    the capture ends `delta` samples behind the fifth first-round FCCH position p5 of the oracle's fine stage
         (FCCH_fine_correction.m:35 / SCH_corr_rate_correction.m:40 breaks, the slot-fit tests of :150-175).  For
         dongle 0 the cut is a head offset, raw[2a : 2(a+N)] with a + N = p5 + delta, so that all those cases share one N and
         go through ONE batch call; dongle 3's first FCCH sits too early in the capture for that: plain tail cuts, own lengths
  drop   k samples removed half-way between FCCH 3 and FCCH 4: the spacing classes of both stages, the SNR gate
  move   SCH burst 3 moved earlier (k > 0) or later (k < 0): k samples deleted 3000 samples ahead of it and k samples
         duplicated 3000 samples behind it (or the other way round), so nothing else shifts
  slow   captures with a sampling error of -600 / -1200 ppm cut right behind the first length the :35 test lets the last burst
         through: the :135 drop of the last burst, with nine bursts left (calibrates) and with four (GSMCAL_S_FINE_FEW_BURSTS --
         a plain cut of dongle 0 cannot reach it: the fine peak would have to sit 437 samples behind its coarse position)
  sf42   a capture that starts on the first FCCH of a multiframe (see SOURCES)
Cases on a threshold: the SCH spacing test at 40 / 39 samples, the slot-fit test at ep == len(r) / len(r) + 1 (build()).
Every position used comes from the oracle's own first-round positions of the unedited capture (one oracle run per dongle,
`scan()`).  Each case names the exit it is DESIGNED to take (include/gsmcal.h GSMCAL_S_*, 0 = calibrates) and, where it
matters, the shape of its pos_info table; tests/test_exit_paths_cpu.py holds the oracle to that design, so a change of synth
cannot empty the GPU test unnoticed.

Not reachable through the batch chain with these inputs:
  GSMCAL_E_INDEX in the fine stage (a coarse hit inside the first 64 symbols, FCCH_fine_correction.m:40-43)  the moving average
         of move_fft_snr_runtime_avg.m:11 is seeded with 999 dB, so the first hit cannot come before window ~mv_len = 160, symbol
         1240: head cuts that put the first FCCH into the first 64 symbols make the detector hit the SECOND burst (HEAD_CUTS).
         The index error the batch can reach is the capture shorter than 23 frames (FCCH_coarse_position.m:25), which
         tests/test_gpu_parity.py covers; the fine stage's is covered at function level with hand-given positions
  GSMCAL_S_POST_NO_POS (10) is never the FIRST exit met (an earlier stage has left before); it is asserted per stage.

Plain module: numpy, synth and the oracle only -- nothing here touches the GPU, so it is safe in spawned pool workers."""
import numpy as np

from gsmcal import synth
from oracle import gsmcal_oracle as oracle

FC = 957.4e6
NUM_FRAMES = 102
# the captures the cases are cut from: name -> synth.make_stream arguments
#   slow1200 / slow600  a sampling error of -1200 / -600 ppm: the fine stage stretches the stream (e < 0, max_len = len(s),
#            FCCH_fine_correction.m:118-122), so the regenerated last burst moves back by p_last * |e| > 437 samples and a cut
#            that the :35 test still lets through makes it overrun len(r): the :135 drop
#   sf42     first FCCH = the first of a 51-multiframe: the 11-frame gap is the FIFTH (b_idx = 5), so the BCCH block behind
#            SCH 1 is flagged by BCCH_flag(b_idx(b_idx>=5)-4) alone (SCH_corr_rate_correction.m:141)
SOURCES = {"d0": dict(dongle=0), "d3": dict(dongle=3), "slow1200": dict(dongle=0, sampling_ppm=-1200.0),
           "slow600": dict(dongle=0, sampling_ppm=-600.0), "sf42": dict(dongle=0, start_frame=42)}


def coef():
    return synth.fir1(46, 200e3 / synth.FS)


def scan():
    """{source: (raw, first-round FCCH positions, first-round SCH positions, coarse positions)} of the unedited captures: one
    oracle run each"""
    c, ts = coef(), synth.sch_training_sequence()
    out = {}
    for name, kw in SOURCES.items():
        raw = synth.make_stream(num_frames=NUM_FRAMES, **kw)[0]
        orc = oracle.calibrate_stream(raw, c, ts, FC)
        assert orc["status"] == 0 and len(orc["fine_first_round_pos"]) >= 8, "the unedited captures must calibrate"
        out[name] = (raw, orc["fine_first_round_pos"].astype(np.int64), orc["sch_first_round_pos"].astype(np.int64),
                     orc["coarse_pos"].astype(np.int64))
    return out


def len_r_after_fine(n, orc):
    """length of the stream the SCH stage cuts its table against when that stage measures no sampling error: the fine stage's
    max_len (FCCH_fine_correction.m:118-122)"""
    e = orc["sampling_ppm"][0] * 1e-6
    assert orc["sampling_ppm"][1] == 0.0, "the SCH stage resamples: len(r) is not the fine stage's"
    return int(np.floor(n / (1 + e))) if e >= 0 else n


def samples(raw, lo, hi):
    return raw[2 * lo:2 * hi]


def drop(raw, at, k):
    """k samples removed at sample `at`"""
    return np.concatenate([raw[:2 * at], raw[2 * (at + k):]])


def move(raw, burst, k):
    """the burst at sample `burst` k samples earlier (k > 0) or later (k < 0); the length stays"""
    lo, hi = burst - 3000, burst + 3000
    if k > 0:
        return np.concatenate([raw[:2 * lo], raw[2 * (lo + k):2 * hi], raw[2 * (hi - k):2 * hi], raw[2 * hi:]])
    k = -k
    return np.concatenate([raw[:2 * lo], raw[2 * (lo - k):2 * lo], raw[2 * lo:2 * (hi - k)], raw[2 * hi:]])


# (name, delta behind p5, designed status, designed table: None or (rows, type of the last row, BCCH rows))
CUTS_D0 = [("cut+1100", 1100, 2, None), ("cut+1300", 1300, 3, None), ("cut+2000", 2000, 8, (15, -1, 0)),
           ("cut+10800", 10800, 8, (15, -1, 0)), ("cut+11000", 11000, 11, (9, 0, 0)), ("cut+11500", 11500, 11, (10, 1, 0)),
           ("cut+21000", 21000, 11, (10, 1, 0)), ("cut+25000", 25000, 11, (11, 2, 1)), ("cut+35000", 35000, 11, (12, 2, 2)),
           ("cut+45000", 45000, 11, (13, 2, 3)), ("cut+60000", 60000, 0, (14, 2, 4))]
FULL_DELTA = 60000          # the cut the splices are applied to: it calibrates when left alone
# (name, kind, k, designed status)
SPLICES_D0 = [("drop200", "drop", 200, 9), ("drop390", "drop", 390, 6), ("drop410", "drop", 410, 4), ("drop1000", "drop", 1000, 2),
              ("sch3-50", "move", 50, 9), ("sch3-66", "move", 66, 7), ("sch3+28", "move", -28, 7), ("sch3-30", "move", 30, 0),
              ("sch3+15", "move", -15, 0)]
# dongle 3, tail cuts with lengths of their own: (name, delta, status, table)
CUTS_D3 = [("d3cut+11000", 11000, 0, (13, 0, 4)), ("d3cut+1300", 1300, 3, None)]
HEAD_CUTS = (0, 200, 400)   # first FCCH this many samples into the capture (dongle 0): inside the first 64 symbols


def build(sc=None):
    """-> (N of the mixed batch, list of case dicts {name, raw, status, table, group}); group "mixed" = the equal-N cases"""
    sc = sc or scan()
    raw0, p0, s0, _ = sc["d0"]
    p5 = int(p0[4])
    n_mixed = p5 + CUTS_D0[0][1]
    cases = []

    def add(name, raw, status, table, group):
        cases.append({"name": name, "raw": np.ascontiguousarray(raw), "status": status, "table": table, "group": group})

    for name, delta, status, table in CUTS_D0:
        end = p5 + delta
        add(name, samples(raw0, end - n_mixed, end), status, table, "mixed")
    end = p5 + FULL_DELTA
    a = end - n_mixed
    mid34 = int(p0[2] + p0[3]) // 2
    for name, kind, k, status in SPLICES_D0:
        if kind == "drop":
            add(name, drop(samples(raw0, a, end + k), mid34 - a, k), status, None, "mixed")
        else:
            add(name, move(samples(raw0, a, end), int(s0[2]) - a, k), status, None, "mixed")
    rng = np.random.default_rng(7)
    add("noise", np.clip(np.round(127.5 + 20 * rng.standard_normal(2 * n_mixed)), 0, 255).astype(np.uint8), 1, None, "mixed")
    add("plain+62000", samples(raw0, p5 + 62000 - n_mixed, p5 + 62000), 0, None, "mixed")
    for h in HEAD_CUTS:     # the detector locks on the second burst and runs out of capture after four: FEW_HITS, no index error
        first = int(p0[0]) - h
        add(f"head{h}", samples(raw0, first, first + n_mixed), 2, None, "mixed")
    # on the threshold of the SCH spacing test (SCH_corr_rate_correction.m:94-104, abs(diff - d_ov) < max_th = 40): SCH 3 moved so
    # that the first-round spacing SCH 2 -> 3 is exactly 40 short of ten frames (fails) and exactly 39 short (passes)
    k40 = int(s0[2] - s0[1]) - (100000 - 40)
    add("sch3-th40", move(samples(raw0, a, end), int(s0[2]) - a, k40), 9, (15, -1, 0), "mixed")
    add("sch3-th39", move(samples(raw0, a, end), int(s0[2]) - a, k40 - 1), 0, (14, 2, 4), "mixed")
    # on the threshold of the slot-fit test (:150-175, ep <= len(r)): the cut moved until the last row of a reference cut ends
    # exactly on the last sample of r (fits) and one sample behind it (does not); for an SCH row and for a BCCH row
    c_, ts_ = coef(), synth.sch_training_sequence()
    for tag, ref_delta, fit, nofit in (("sch", 11500, (10, 1, 0), (9, 0, 0)), ("bcch", 35000, (12, 2, 2), (11, 2, 1))):
        ref_end = p5 + ref_delta
        orc = oracle.calibrate_stream(samples(raw0, ref_end - n_mixed, ref_end), c_, ts_, FC)
        assert table_shape(orc["pos_info"]) == fit, (tag, table_shape(orc["pos_info"]))
        ep = int(orc["pos_info"][-1, 0]) + 1250 - 1
        fit_end = ref_end + ep - len_r_after_fine(n_mixed, orc)
        add(f"fit-{tag}", samples(raw0, fit_end - n_mixed, fit_end), 11, fit, "mixed")
        add(f"nofit-{tag}", samples(raw0, fit_end - 1 - n_mixed, fit_end - 1), 11, nofit, "mixed")
    raw3, p3, _, _ = sc["d3"]
    for name, delta, status, table in CUTS_D3:
        add(name, samples(raw3, 0, int(p3[4]) + delta), status, table, "own")
    # the full-length capture with 200 samples dropped: the fine stage resamples by -200 / (80 frames), the regenerated grid
    # drifts off the bursts and an SCH peak lands on the edge of its search window
    add("full-drop200", drop(raw0, mid34, 200), 7, None, "own")
    # the :135 drop of the last burst: leaving four bursts (FINE_FEW_BURSTS) and leaving nine (calibrates)
    for src, idx, name, status in (("slow1200", 4, "fewbursts", 5), ("slow600", 9, "drop135", 0)):
        raw, _, _, cp = sc[src]
        add(name, samples(raw, 0, (int(cp[idx]) + 211) * 8 + 40), status, None, "own")   # :35 passes from (position + 211) symbols on
    # six SCH hits with the 11-frame gap fifth: whole, and cut inside the BCCH block behind SCH 6
    raw42, p42, _, _ = sc["sf42"]
    assert p42[5] - p42[4] > 105000 and np.all(np.diff(p42[:5]) < 105000), "sf42: the 11-frame gap should be the fifth"
    add("sf42-full", raw42, 0, (28, 1, 8), "own")
    add("sf42-cut", samples(raw42, 0, int(p42[5]) + 35000), 0, (18, 2, 6), "own")
    for c in cases:
        assert c["group"] != "mixed" or len(c["raw"]) == 2 * n_mixed, (c["name"], len(c["raw"]), 2 * n_mixed)
    return n_mixed, cases


def table_shape(pos_info):
    """(rows, type of the last row or -1 for a sentinel, BCCH rows)"""
    pi = np.atleast_2d(pos_info)
    if np.all(pi == -1):
        return len(pi), -1, 0
    return len(pi), int(pi[-1, 1]), int(np.sum(pi[:, 1] == 2))


def oracle_job_r(job):
    """job = (raw, coef, ts, fc) -> (oracle.calibrate_stream dict WITH the corrected stream, None), or (None, message) where the
    reference would stop with an index error (pool worker, see parity.pool_map)"""
    import os
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    raw, c, ts, fc = job
    try:
        return oracle.calibrate_stream(raw, c, ts, fc, keep_r=True), None
    except oracle.MatlabIndexError as e:
        return None, str(e)


def literal_job(job):
    """job = (raw, coef, ts, fc) -> the literal oracle's calibrate_stream dict without the stream (pool worker)"""
    import os
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    from oracle import gsmcal_oracle_literal as lit
    raw, c, ts, fc = job
    try:
        out = lit.calibrate_stream(raw, c, ts, fc)
    except IndexError as e:
        return None, str(e)
    out.pop("r")
    return out, None


def scan_job(job):
    """job = (raw, coef) -> oracle.scan_capture dict (pool worker)"""
    import os
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    raw, c = job
    return oracle.scan_capture(raw, c)
