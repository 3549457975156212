"""Shared inputs of the threshold tests (tests/test_params_cpu.py, tests/test_gpu_params.py): the captures and the
gsmcal_params settings they run under.

The captures are those of tests/exit_paths.py -- the 102-frame captures of dongles 0 and 3, the -1200 ppm capture and the
edited cases (cut, drop, SCH move, slow, sf42) -- plus what the thresholds need and the exits did not: a full-length
noise-only capture, a traffic-only carrier (bcch=False), drops that shorten ONE gap between two coarse hits by 40 and 60
1x symbols, and a capture the detector hits exactly twice.  Every position comes from the oracle (exit_paths.scan()).

A parameter set is (name, {field: value}, [capture names]); SETS holds the calibration chain's, SCAN_SETS the scanner's.
The sets whose value depends on an oracle figure (the SNR gate either side of a burst's SNR, the scanner's tolerance either
side of a gap's deviation) are built by `gate_sets` / `scan_tol_sets` from default-parameter oracle results.
tests/test_params_cpu.py holds every set to being non-vacuous: it changes some capture's outcome, leaves another's alone,
and each boundary pair flips the oracle's decision.

Plain module: numpy, synth and the oracles only -- nothing here touches the GPU, so it is safe in spawned pool workers."""
import numpy as np

import exit_paths as ep

FC = ep.FC
TUNABLE = ("coarse_th_db", "min_hits", "fine_max_ppm", "fine_gate_snr_db", "sch_max_ppm", "post_min_bcch", "scan_min_hits",
           "scan_spacing", "scan_spacing_idle", "scan_tol")
GEOMETRY = {"coarse_mv_factor": 10, "coarse_max_offset": 5, "fine_max_offset": 64, "fine_noise_bw_hz": 200e3, "sch_max_offset": 8}
SCAN_DROPS = (40, 60)           # 1x symbols taken out of one FCCH gap
EXACT_SHORT = (410, 390)
CUT6 = (2000, 11000)


def captures(sc=None):
    """-> {name: uint8 capture}"""
    sc = sc or ep.scan()
    _, cases = ep.build(sc)
    caps = {k["name"]: k["raw"] for k in cases}
    raw0, p0, _, c0 = sc["d0"]
    caps["d0"], caps["d3"], caps["slow1200"] = raw0, sc["d3"][0], sc["slow1200"][0]
    rng = np.random.default_rng(11)
    caps["noise-full"] = np.clip(np.round(127.5 + 20 * rng.standard_normal(len(raw0))), 0, 255).astype(np.uint8)
    # every byte 128: raw2iq.m:8 leaves exact zeros, every window's SNR is 0/0 = NaN and no comparison with NaN holds -- the one
    # capture whose outcome no coarse threshold can move
    caps["const"] = np.full(len(raw0), 128, dtype=np.uint8)
    caps["nobcch"] = ep.synth.make_stream(dongle=0, num_frames=ep.NUM_FRAMES, bcch=False)[0]
    mid34 = int(p0[2] + p0[3]) // 2
    # drops that put the gap FCCH 3 -> 4 of the fine stage's first round exactly 410 and exactly 390 samples short of ten frames
    # (max_th = floor(100000 * max_ppm * 1e-6) is 410 at 4100 ppm and 390 at 3900: the strict < refuses them there); built like
    # exit_paths' drop cases, so they share the mixed batch's length
    n_mixed, p5 = int(p0[4]) + ep.CUTS_D0[0][1], int(p0[4])
    end = p5 + ep.FULL_DELTA
    gap = int(p0[3] - p0[2])
    for short in EXACT_SHORT:
        k = short + (gap - 100000)
        caps[f"short{short}"] = ep.drop(ep.samples(raw0, end - n_mixed, end + k), mid34 - (end - n_mixed), k)
    # tail cuts behind the SIXTH first-round FCCH position: six fine positions with five and with six SCH positions
    for delta in CUT6:
        caps[f"cut6+{delta}"] = ep.samples(raw0, 0, int(p0[5]) + delta)
    # the scanner's captures share one length: the longest drop's
    n_scan = len(raw0) // 2 - 8 * max(SCAN_DROPS)
    for k in SCAN_DROPS:
        caps[f"s-drop{k}"] = ep.samples(ep.drop(raw0, mid34, 8 * k), 0, n_scan)
    for name in ("d0", "d3", "noise-full"):
        caps["s-" + name] = ep.samples(caps[name], 0, n_scan)
    # two hits: the capture ends 2000 samples ahead of the third FCCH the detector would walk to
    end = int(p0[2]) - 2000
    assert end >= 232000, "23 frames are needed by FCCH_coarse_position.m:25"
    caps["twohit"] = ep.samples(raw0, 0, end)
    # ... and two hits either side of the idle frame: from 25000 samples ahead of FCCH 4 to 2000 ahead of FCCH 6
    assert p0[4] - p0[3] > 105000, "d0: the eleven-frame gap should be the fourth"
    caps["twohit-idle"] = ep.samples(raw0, int(p0[3]) - 25000, int(p0[5]) - 2000)
    return {k: np.ascontiguousarray(v) for k, v in caps.items()}


# ---- the calibration chain ---------------------------------------------------------------------------------------------------
SETS = []


def add(name, params, names):
    assert all(k in TUNABLE for k in params), params
    SETS.append((name, params, list(names)))


# min_hits: FCCH_fine_correction.m:12,69,142, SCH_corr_rate_correction.m:11,84.  fewbursts: four bursts left by the :135 drop;
# cut+2000 / cut+10800 ... : five and six first-round positions in the two stages (test_params_cpu.py asserts the counts)
MIN_HITS_CASES = ["fewbursts", "cut+1100", "cut+1300", "cut+2000", "cut+11000", "cut+21000", "head0", "noise", "cut6+2000", "cut6+11000"]
for mh in (2, 4, 6, 9):
    add(f"min_hits={mh}", {"min_hits": mh}, MIN_HITS_CASES + (["d0"] if mh == 9 else []))       # (ten hits: 9 lets them through)
# fine_max_ppm: max_th = floor(100000 * ppm * 1e-6) against |gap - 100000| of the drop cases (strict <)
FINE_CASES = ["drop410", "drop390", "short410", "short390", "plain+62000"]
for ppm, names in ((4100.0, FINE_CASES), (4110.0, FINE_CASES), (3800.0, FINE_CASES), (3900.0, FINE_CASES),
                   # above 50000 ppm the two classes overlap; at 100000 every ten-frame gap passes BOTH tests and is counted twice (:95)
                   (60000.0, FINE_CASES + ["drop1000"]), (100000.0, FINE_CASES + ["drop1000"])):
    add(f"fine_max_ppm={ppm:.0f}", {"fine_max_ppm": ppm}, names)
for ppm in (390.0, 400.0, 410.0):
    add(f"sch_max_ppm={ppm:.0f}", {"sch_max_ppm": ppm}, ["sch3-th39", "sch3-th40", "sch3-30", "sch3-50"])
add("fine_gate_snr_db=-100", {"fine_gate_snr_db": -100.0}, ["drop390", "short390", "plain+62000"])
for nb in (0, 1, 4, 6, 30):
    # BCCH rows: cut+11000 none (left out at 0), nofit-bcch 1, fit-bcch 2, cut+60000 4, the unedited capture of dongle 3 eight -- it
    # still calibrates at 6 and no longer at 30 (run at those two)
    add(f"post_min_bcch={nb}", {"post_min_bcch": nb}, ["fit-bcch", "nofit-bcch", "cut+60000"] + ([] if nb == 0 else ["cut+11000"]) + (["d3"] if nb >= 6 else []))
COARSE_TH = (0.0, 4.0, 7.0, 14.0, 25.0)
COARSE_CASES = ["d0", "d3", "slow1200", "noise-full", "const"]
for th in COARSE_TH:
    add(f"coarse_th_db={th:.0f}", {"coarse_th_db": th}, COARSE_CASES)
MIXED = {"min_hits": 4, "fine_max_ppm": 4110.0, "sch_max_ppm": 390.0, "post_min_bcch": 6}
add("mixed", MIXED, ["cut+1300", "drop410", "sch3-th39", "sch3-30", "cut+45000", "plain+62000", "noise", "cut+60000", "d3"])
# a gap that passes BOTH class tests and still gets through the :95 count: only hand-given base positions reach it (function level).
# Coarse hits 1, 2, 4, 6, 7 of d0 are 10, 20, 21 and 10 frames apart; at 100000 ppm the ten-frame gaps pass both tests, the other
# two pass neither, so sum(a) + sum(b) = 2 + 2 = 4 = last_idx - 1.  Where both passed the eleven-frame class wins (:129-130) and
# a gap in no class gets step 0: the regenerated grid is first + [0, 110000, 110000, 110000, 220000].  (The gate is opened so that the
# grid comes back.)
BOTH_CLASSES = {"fine_max_ppm": 100000.0, "fine_gate_snr_db": -1000.0}
BOTH_HITS = (0, 1, 3, 5, 6)
BOTH_GRID = (0.0, 110000.0, 110000.0, 110000.0, 220000.0)
INDEX_SET = ("coarse_th_db=-2000", {"coarse_th_db": -2000.0}, ["d0"])      # the fine stage's index error: a call of its own

# boundary pairs of fixed sets: (set a, set b, capture) -- the oracle's status differs between the two
PAIRS = [("fine_max_ppm=4100", "fine_max_ppm=4110", "short410"), ("fine_max_ppm=3800", "fine_max_ppm=3900", "drop390"),
         ("fine_max_ppm=3900", "default", "short390"),
         ("sch_max_ppm=390", "sch_max_ppm=400", "sch3-th39"), ("sch_max_ppm=400", "sch_max_ppm=410", "sch3-th40"),
         ("post_min_bcch=1", "post_min_bcch=4", "nofit-bcch"), ("post_min_bcch=4", "post_min_bcch=6", "cut+60000"),
         ("post_min_bcch=6", "post_min_bcch=30", "d3"),
         ("min_hits=4", "min_hits=6", "cut+2000"), ("min_hits=4", "min_hits=6", "fewbursts")]
GATE_CASE = "plain+62000"          # its weakest burst is stronger than cut+60000's: that one fails either gate


def gate_sets(orc_default, margin):
    """the SNR gate `margin` below and above the lowest per-burst gate SNR of GATE_CASE (oracle, default parameters)"""
    m = float(np.min(orc_default["fine_gate_snr"]))
    return [("gate-below", {"fine_gate_snr_db": m - margin}, [GATE_CASE, "cut+60000", "noise"]),
            ("gate-above", {"fine_gate_snr_db": m + margin}, [GATE_CASE, "cut+60000", "noise"])]


# ---- the scanner -------------------------------------------------------------------------------------------------------------
SCAN_CASES = ["s-d0", "s-d3", "s-drop40", "s-drop60", "s-noise-full", "twohit", "twohit-idle", "drop1000", "head0"]   # (walks of 3 and 4)
SCAN_SETS = [(f"scan_min_hits={n}", {"scan_min_hits": n}, SCAN_CASES) for n in (1, 2, 3, 5)]
# one spacing moved out of reach (two hits suffice, so that the captures with ONE gap decide): only the gap across the idle
# frame (:176) still fits, or only the plain ones (:170)
SCAN_SETS += [("scan_spacing+100", {"scan_spacing": 12600.0, "scan_min_hits": 2}, SCAN_CASES),
              ("scan_spacing_idle+100", {"scan_spacing_idle": 13850.0, "scan_min_hits": 2}, SCAN_CASES)]


def scan_dev(coarse_pos, spacing=12500.0, idle=13750.0):
    """largest distance of a gap from the nearer of the two spacings (integers: positions are 1 + 8k)"""
    d = np.diff(np.asarray(coarse_pos, dtype=np.float64))
    return float(np.max(np.minimum(np.abs(d - spacing), np.abs(d - idle))))


def scan_tol_sets(scan_default):
    """{capture: oracle.scan_capture dict at default parameters} -> for each drop case the tolerance ON its largest deviation
    (strict >: accepted) and one below (refused)"""
    out = []
    for k in SCAN_DROPS:
        dev = scan_dev(scan_default[f"s-drop{k}"]["coarse_pos"])
        assert dev == int(dev) and dev >= 8
        # (two hits suffice: a tolerance below the reference's 50 alone could only refuse more than the default rule does)
        out.append((f"scan_tol=dev{k}", {"scan_tol": dev, "scan_min_hits": 2}, SCAN_CASES))
        out.append((f"scan_tol=dev{k}-1", {"scan_tol": dev - 1.0, "scan_min_hits": 2}, SCAN_CASES))
    return out


SCAN_SET_NAMES = [name for name, _, _ in SCAN_SETS] + [f"scan_tol=dev{k}{s}" for k in SCAN_DROPS for s in ("", "-1")]


# ---- pool workers ------------------------------------------------------------------------------------------------------------
def _oracle(which):
    if which == "literal":
        from oracle import gsmcal_oracle_literal as mod
    else:
        from oracle import gsmcal_oracle as mod
    return mod


def calib_job(job):
    """job = (which oracle, raw, coef, ts, [params, ...]) -> [(dict without streams, None) or (None, index-error text), ...]; the
    front end does not depend on the thresholds and is computed once"""
    import os
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    which, raw, coef, ts, plist = job
    mod = _oracle(which)
    front = mod.front_end(raw, coef)
    out = []
    for params in plist:
        try:
            res = mod.calibrate_stream(raw, coef, ts, FC, params=params, front=front)
        except IndexError as e:           # (MatlabIndexError is one)
            out.append((None, str(e)))
            continue
        res.pop("r", None)
        out.append((res, None))
    return out


def scan_job(job):
    """job = (which oracle, raw, coef, [params, ...]) -> [scan_capture dict, ...]"""
    import os
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    which, raw, coef, plist = job
    mod = _oracle(which)
    front = mod.front_end(raw, coef)
    return [mod.scan_capture(raw, coef, params=params, front=front) for params in plist]


def _job(job):
    fn, args = job
    return fn(args)


def run(which, caps, groups):
    """groups: [(worker, [(capture name, params dict or None), ...], extra arguments, parameter sets per job), ...] -> one
    {(capture name, key(params)): result} per group, all through ONE pool_map; a job is one capture with up to `chunk` parameter
    sets (the front end is computed once per job, the pool stays balanced)"""
    import parity
    jobs, index = [], []
    for g, (fn, wanted, extra, chunk) in enumerate(groups):
        by_cap = {}
        for name, params in wanted:
            lst = by_cap.setdefault(name, [])
            if params not in lst:
                lst.append(params)
        for name, plist in by_cap.items():
            for i in range(0, len(plist), chunk):
                jobs.append((fn, (which, caps[name]) + extra + (plist[i:i + chunk],)))
                index.append((g, name, plist[i:i + chunk]))
    res = parity.pool_map(_job, jobs, max_workers=16)
    out = [{} for _ in groups]
    for (g, name, plist), rs in zip(index, res):
        for params, r in zip(plist, rs):
            out[g][(name, key(params))] = r
    return out


def run_jobs(fn, which, caps, wanted, extra, chunk):
    return run(which, caps, [(fn, wanted, extra, chunk)])[0]


def run_both(which, caps, coef, ts, calib_wanted, scan_wanted, chunk=4):
    """the chain's and the scanner's runs in one pool -> (chain results, scanner results)"""
    return run(which, caps, [(calib_job, calib_wanted, (coef, ts), chunk), (scan_job, scan_wanted, (coef,), 16)])


def key(params):
    return tuple(sorted((params or {}).items()))
