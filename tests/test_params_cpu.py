"""CPU tests (no marker) of the threshold cases of tests/params_cases.py, with the oracles alone.

The reference hard-codes every threshold, so no reference run and no golden vector can check a moved one: the two independent
restatements (oracle/gsmcal_oracle.py, oracle/gsmcal_oracle_literal.py), each with the literal replaced by its gsmcal_params
field, are held to each other here on every capture of every parameter set tests/test_gpu_params.py runs.  The rest are
conditions on the INPUTS: every set changes some capture's outcome and leaves another's alone, every boundary pair flips the
oracle's decision, the counts the min_hits cases were built for are the counts they have -- so a change of synth fails
here instead of silently emptying the GPU test."""
import math

import numpy as np
import pytest

import exit_paths as ep
import params_cases as pc
import parity
from oracle import gsmcal_oracle as o
from oracle import gsmcal_oracle_literal as lit


@pytest.fixture(scope="module")
def built():
    caps = pc.captures()
    coef, ts = ep.coef(), ep.synth.sch_training_sequence()
    used = sorted({n for _, _, names in pc.SETS for n in names} | {pc.GATE_CASE, "d0", "cut+60000", "noise", "nobcch"})
    base = pc.run_jobs(pc.calib_job, "vector", caps, [(n, None) for n in used], (coef, ts), 4)
    sets = pc.SETS + pc.gate_sets(base[(pc.GATE_CASE, ())][0], 10 * parity.SNR_ATOL) + [pc.INDEX_SET]
    wanted = [(n, p) for _, p, names in sets for n in names]
    vec = pc.run_jobs(pc.calib_job, "vector", caps, wanted, (coef, ts), 4)
    vec.update(base)
    literal = pc.run_jobs(pc.calib_job, "literal", caps, wanted + [("nobcch", None)], (coef, ts), 6)
    sbase = pc.run_jobs(pc.scan_job, "vector", caps, [(n, None) for n in pc.SCAN_CASES], (coef,), 16)
    ssets = pc.SCAN_SETS + pc.scan_tol_sets({n: sbase[(n, ())] for n in pc.SCAN_CASES})
    swanted = [(n, p) for _, p, names in ssets for n in names]
    svec = pc.run_jobs(pc.scan_job, "vector", caps, swanted, (coef,), 16)
    svec.update(sbase)
    slit = pc.run_jobs(pc.scan_job, "literal", caps, swanted + [(n, None) for n in pc.SCAN_CASES], (coef,), 16)
    return {"caps": caps, "sets": sets, "vec": vec, "lit": literal, "ssets": ssets, "svec": svec, "slit": slit}


def outcome(res):
    orc, err = res
    return "index error" if orc is None else (orc["status"], orc["n_fcch"], orc["n_pos_rows"])


def close(x, y):
    return (math.isinf(x) and math.isinf(y)) or abs(x - y) <= 1e-9 * abs(x) + 1e-12      # as tests/test_oracle_cpu.py


def test_params_omitted_none_and_the_defaults_are_the_same_thing(built):
    """bit-identical results without `params`, with None, with {} and with the reference's literals spelt out"""
    raw, coef, ts = built["caps"]["cut+60000"], ep.coef(), ep.synth.sch_training_sequence()
    a = o.calibrate_stream(raw, coef, ts, pc.FC)
    for params in (None, {}, dict(o.PARAM_DEFAULTS)):
        b = o.calibrate_stream(raw, coef, ts, pc.FC, params=params, front=o.front_end(raw, coef))
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (params, k)
    sa, sb = o.scan_capture(raw, coef), o.scan_capture(raw, coef, params=dict(o.PARAM_DEFAULTS))
    assert all(np.array_equal(sa[k], sb[k]) for k in ("coarse_pos", "coarse_snr", "snr", "num_hit"))
    assert set(o.PARAM_DEFAULTS) == set(pc.TUNABLE) == set(lit.TUNABLE)


@pytest.mark.parametrize("field", sorted(pc.GEOMETRY))
def test_geometry_fields_are_refused_by_both_oracles(field):
    for call in (lambda p: o.scanner_accept([1.0, 12501.0, 25001.0], [9.0, 9.0, 9.0], params=p),
                 lambda p: lit.scanner_accept([1.0, 12501.0, 25001.0], [9.0, 9.0, 9.0], params=p),
                 lambda p: o.carrier_correct_post_SCH(-1.0, [[1.0, 0.0]], 8, pc.FC, params=p),
                 lambda p: lit.carrier_correct_post_SCH(-1.0, [[1.0, 0.0]], 8, pc.FC, params=p),
                 lambda p: o.FCCH_fine_correction(np.zeros(8), [1.0], 8, pc.FC, params=p),
                 lambda p: lit.FCCH_fine_correction(np.zeros(8), [1.0], 8, pc.FC, params=p)):
        with pytest.raises(ValueError):
            call({field: pc.GEOMETRY[field]})
        call({"min_hits": 5})


def test_params_objects_are_read_or_refused_never_ignored():
    """a dataclass is read like a mapping; a ctypes structure (whose fields vars() does not show) is a TypeError in both oracles,
    not a silent run at the defaults"""
    import ctypes
    import dataclasses

    @dataclasses.dataclass
    class P:
        scan_min_hits: int = 2

    class S(ctypes.Structure):
        _fields_ = [("scan_min_hits", ctypes.c_int)]

    for mod in (o, lit):
        assert mod.scanner_accept([1.0, 12501.0], [9.0, 7.0]) == (0.0, 0.0)
        assert mod.scanner_accept([1.0, 12501.0], [9.0, 7.0], params=P()) == (8.0, 2.0)
        assert mod.scanner_accept([1.0, 12501.0], [9.0, 7.0], params={"scan_min_hits": 2}) == (8.0, 2.0)
        with pytest.raises(TypeError):
            mod.scanner_accept([1.0, 12501.0], [9.0, 7.0], params=S(2))


def test_the_two_oracles_agree_at_every_parameter_set(built):
    n = 0
    for name, params, names in built["sets"] + [("default", None, ["nobcch"])]:
        for cap in names:
            (a, ea), (b, eb) = built["vec"][(cap, pc.key(params))], built["lit"][(cap, pc.key(params))]
            what = (name, cap)
            n += 1
            if a is None or b is None:
                assert a is None and b is None, (what, ea, eb)
                continue
            assert list(a["stage_exit"]) == list(b["stage_exit"]) and a["status"] == b["status"], (what, a["stage_exit"], b["stage_exit"])
            assert (a["n_fcch"], a["n_pos_rows"], a["first_fcch_pos"]) == (b["n_fcch"], b["n_pos_rows"], b["first_fcch_pos"]), what
            assert np.array_equal(a["coarse_pos"], b["coarse_pos"]), what
            assert np.array_equal(a["fine_first_round_pos"], b["first"]), what
            assert np.array_equal(a["fcch_pos"], b["fcch_pos"]), what
            if not a["sch_edge_abort"]:
                assert np.array_equal(a["sch_first_round_pos"], b["sch_first"]), what
            assert a["pos_info"].shape == b["pos_info"].shape and np.array_equal(a["pos_info"], b["pos_info"]), what
            assert np.allclose(a["coarse_snr"], b["coarse_snr"], rtol=0, atol=1e-9), what
            assert a["fine_gate_snr"].shape == b["fine_gate_snr"].shape and np.allclose(a["fine_gate_snr"], b["fine_gate_snr"], rtol=0, atol=1e-9), what
            for x, y in zip(list(a["sampling_ppm"]) + list(a["carrier_ppm"]) + [a["total_sampling_ppm"], a["total_carrier_ppm"]],
                            b["sp"] + b["cp"] + b["tot"]):
                assert close(x, y), (what, x, y)
    print(n, "capture x parameter-set runs compared")


def test_the_two_oracles_agree_on_the_scanner_rule(built):
    for name, params, names in built["ssets"] + [("default", None, pc.SCAN_CASES)]:
        for cap in names:
            a, b = built["svec"][(cap, pc.key(params))], built["slit"][(cap, pc.key(params))]
            assert np.array_equal(a["coarse_pos"], b["coarse_pos"]), (name, cap)
            assert a["num_hit"] == b["num_hit"] and abs(a["snr"] - b["snr"]) <= 1e-9, (name, cap, a["snr"], b["snr"], a["num_hit"], b["num_hit"])


def test_every_parameter_set_changes_one_outcome_and_leaves_another(built):
    """(status, n_fcch, n_pos_rows) against the default-parameter oracle; a set that spells out the defaults changes nothing"""
    for name, params, names in built["sets"]:
        diff = [cap for cap in names if outcome(built["vec"][(cap, pc.key(params))]) != outcome(built["vec"][(cap, ())])]
        print(name, "changes", diff, "of", names)
        if all(o.PARAM_DEFAULTS[k] == v for k, v in params.items()):
            assert not diff, (name, diff)
            continue
        assert diff, f"{name}: no capture's outcome differs from the default parameters'"
        if (name, params, names) != pc.INDEX_SET:
            assert len(diff) < len(names), f"{name}: every capture's outcome differs"


def test_every_scanner_set_changes_one_outcome_and_leaves_another(built):
    for name, params, names in built["ssets"]:
        diff = [cap for cap in names if built["svec"][(cap, pc.key(params))]["num_hit"] != built["svec"][(cap, ())]["num_hit"]]
        print(name, "changes", diff)
        if all(o.PARAM_DEFAULTS[k] == v for k, v in params.items()):
            assert not diff, (name, diff)
        else:
            assert diff and len(diff) < len(names), (name, diff)


def test_every_boundary_pair_flips_the_decision(built):
    by = {name: params for name, params, _ in built["sets"]}
    by["default"] = None
    for a, b, cap in pc.PAIRS:
        sa, sb = (built["vec"][(cap, pc.key(by[x]))][0]["status"] for x in (a, b))
        print(a, b, cap, sa, sb)
        assert sa != sb, (a, b, cap, sa)
    below, above = (built["vec"][(pc.GATE_CASE, pc.key(by[x]))][0] for x in ("gate-below", "gate-above"))
    assert below["status"] == 0 and above["status"] == 6, (below["status"], above["status"])
    # the scanner's tolerance ON the largest deviation accepts (strict >), one below refuses
    tol = sorted((p["scan_tol"], name) for name, p, _ in built["ssets"] if "scan_tol" in p)
    assert len(tol) >= 2
    for k in pc.SCAN_DROPS:
        cap = f"s-drop{k}"
        dev = pc.scan_dev(built["svec"][(cap, ())]["coarse_pos"])
        on, under = (built["svec"][(cap, pc.key({"scan_tol": t, "scan_min_hits": 2}))] for t in (dev, dev - 1.0))
        assert on["num_hit"] == len(on["coarse_pos"]) >= 3 and under["num_hit"] == 0, (cap, dev, on["num_hit"], under["num_hit"])


def test_the_fine_spacing_cases_sit_exactly_on_their_thresholds(built):
    """max_th = floor(d_ov * max_ppm * 1e-6) lands on 410 at 4100 ppm, 411 at 4110, 390 at 3900 (a product next to an integer), and
    the gap FCCH 3 -> 4 of short410 / short390 is exactly that far from ten frames: `<=` for `<` would let them through"""
    assert [math.floor(100000.0 * p * 1e-6) for p in (4100.0, 4110.0, 3800.0, 3900.0, 4000.0)] == [410, 411, 380, 390, 400]
    for short in pc.EXACT_SHORT:
        d = built["vec"][(f"short{short}", ())][0]["fine_first_round_diff"]
        dev = np.minimum(np.abs(d - 100000.0), np.abs(d - 110000.0))
        assert dev[2] == short and d[2] < 100000 and np.all(np.delete(dev, 2) < 100), (short, d)
    by = {name: params for name, params, _ in built["sets"]}
    st = {(n, cap): built["vec"][(cap, pc.key(by[n]))][0]["status"] for n in by if n.startswith("fine_max_ppm") for cap in pc.FINE_CASES}
    assert st[("fine_max_ppm=4100", "short410")] == 4 and st[("fine_max_ppm=4110", "short410")] != 4
    assert st[("fine_max_ppm=3900", "short390")] == 4 and built["vec"][("short390", ())][0]["status"] != 4
    # above 90 900 ppm a ten-frame gap passes the eleven-frame test as well and is counted twice: the :95 exit
    assert all(st[("fine_max_ppm=100000", cap)] == 4 for cap in pc.FINE_CASES)


def test_a_gap_in_both_spacing_classes_counts_twice_and_eleven_frames_win(built):
    sc = ep.scan()
    raw0, _, _, c0 = sc["d0"]
    coef = ep.coef()
    base = c0[list(pc.BOTH_HITS)].astype(np.float64)
    ia, ib = {}, {}
    a = o.FCCH_fine_correction(o.front_end(raw0, coef), base, 8, pc.FC, ia, pc.BOTH_CLASSES)
    b = lit.FCCH_fine_correction(lit.front_end(raw0, coef), base, 8, pc.FC, ib, pc.BOTH_CLASSES)
    assert ia["exit"] == ib["exit"] == 0
    d = ia["first_round_diff"]
    assert [int(round(x / 10000.0)) for x in d] == [10, 20, 21, 10], d
    assert np.array_equal(a[0], b[0]) and tuple(a[0] - a[0][0]) == pc.BOTH_GRID, (a[0], b[0])
    assert close(a[2], b[2]) and close(a[3], b[3]) and a[2] > 4e5, (a[2], b[2], a[3], b[3])
    # at the default 4000 ppm the same positions leave at the spacing exit
    assert o.FCCH_fine_correction(o.front_end(raw0, coef), base, 8, pc.FC, ia)[0] == -1.0 and ia["exit"] == 4


def test_the_min_hits_cases_have_the_counts_they_were_built_for(built):
    """first-round counts of five and of six in both stages, and four bursts left behind the :135 drop: with min_hits in
    {4, 6} every `<` of FCCH_fine_correction.m:12,69,142 and SCH_corr_rate_correction.m:11,84 meets a count on either side"""
    def counts(cap):
        r = built["vec"][(cap, ())][0]
        return len(r["coarse_pos"]), len(r["fine_first_round_pos"]), r["n_fcch"], len(r["sch_first_round_pos"])
    assert counts("cut+2000") == (5, 5, 5, 4) and counts("cut+11000") == (5, 5, 5, 5)
    assert counts("cut6+2000") == (6, 6, 6, 5) and counts("cut6+11000") == (6, 6, 6, 6)
    assert counts("cut+1100")[0] == 4 and counts("cut+1300")[:2] == (5, 4)
    few = built["vec"][("fewbursts", ())][0]
    assert len(few["fine_first_round_pos"]) == 5 and few["n_fcch"] == 4 and few["status"] == 5
    st = lambda cap, mh: built["vec"][(cap, pc.key({"min_hits": mh}))][0]["stage_exit"]          # noqa: E731
    assert list(st("cut6+2000", 6))[:3] == [0, 0, 8] and list(st("cut6+11000", 6))[:3] == [0, 0, 0]       # SCH :84 at 5 and at 6
    assert st("cut+2000", 6)[1] == 2 and st("cut+2000", 4)[2] == 0                                  # fine :12; SCH :84 at 4
    assert st("cut+1300", 4)[1] == 0 and st("cut+1300", 6)[1] == 2                                  # fine :69 at 4
    assert st("fewbursts", 4)[1] == 0 and built["vec"][("fewbursts", pc.key({"min_hits": 4}))][0]["n_fcch"] == 4   # :142 at 4


def test_the_post_and_coarse_cases(built):
    bcch = lambda cap: int(np.sum(built["vec"][(cap, ())][0]["pos_info"][:, 1] == 2))           # noqa: E731
    assert [bcch(c) for c in ("cut+11000", "nofit-bcch", "fit-bcch", "cut+60000", "d3")] == [0, 1, 2, 4, 8]
    at = lambda nb: built["vec"][("d3", pc.key({"post_min_bcch": nb}))][0]["status"]           # noqa: E731
    assert (at(6), at(30)) == (0, 11), "a capture that still calibrates above the default, and one value that stops it"
    zero = [n for name, p, names in built["sets"] if p == {"post_min_bcch": 0} for n in names]
    assert zero and all(bcch(c) >= 1 for c in zero)
    # the threshold runs from below the screening level to above every capture's peak; the lowest one makes noise hit
    n_hits = {th: [len(built["vec"][(cap, pc.key({"coarse_th_db": th}))][0]["coarse_pos"]) for cap in pc.COARSE_CASES] for th in pc.COARSE_TH}
    print(n_hits)
    assert built["vec"][("noise-full", pc.key({"coarse_th_db": 0.0}))][0]["status"] != 1
    assert all(built["vec"][(cap, pc.key({"coarse_th_db": 25.0}))][0]["status"] == 1 for cap in pc.COARSE_CASES)
    assert all(built["vec"][("const", pc.key({"coarse_th_db": th}))][0]["status"] == 1 for th in pc.COARSE_TH)
    assert built["vec"][("nobcch", ())][0]["status"] == 1
    assert built["vec"][("d0", pc.key(pc.INDEX_SET[1]))] [0] is None, "the 999 dB seed lets window 1 hit at -2000 dB: sp < 1 in the fine stage"


def test_scanner_cases(built):
    d = {cap: built["svec"][(cap, ())] for cap in pc.SCAN_CASES}
    assert len(d["twohit"]["coarse_pos"]) == 2 and d["twohit"]["num_hit"] == 0
    assert d["s-noise-full"]["coarse_pos"][0] == -1.0
    two = built["svec"][("twohit", pc.key({"scan_min_hits": 2}))]
    assert two["num_hit"] == 2 and two["snr"] == (d["twohit"]["coarse_snr"][0] + d["twohit"]["coarse_snr"][1]) / 2
    # scan_min_hits = 1 on "nothing found": FCCH_pos = -1 has one element and no gap to refuse (the literal rule, :168-173)
    one = built["svec"][("s-noise-full", pc.key({"scan_min_hits": 1}))]
    assert (one["snr"], one["num_hit"]) == (-1.0, 1.0)
    # + 100 on one spacing: a capture with gaps of both kinds is refused either way, the captures with one gap tell the two apart
    assert len(d["twohit-idle"]["coarse_pos"]) == 2 and abs(np.diff(d["twohit-idle"]["coarse_pos"])[0] - 13750) <= 50
    hits = {name: [built["svec"][(cap, pc.key(p))]["num_hit"] for cap in ("s-d0", "twohit", "twohit-idle")]
            for name, p, _ in built["ssets"] if name.endswith("+100")}
    assert hits == {"scan_spacing+100": [0, 0, 2], "scan_spacing_idle+100": [0, 2, 0]}, hits
    assert d["s-d0"]["num_hit"] == 10
