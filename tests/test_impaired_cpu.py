"""CPU tests (no marker) of the impaired-capture case set, with the oracles and the restatements alone: every case of
tests/impaired.py takes the exit it was designed for in the vectorised oracle and in the literal one, the set as a whole holds
what tests/test_gpu_impaired.py relies on -- the spread of exits, impairments that reach the ppm estimators, a non-finite
scanner SNR, a capture without a hit --, and the follow-up family's restatements, run on the ORACLE's corrected streams, stay
off their own tie guards and find the planted payloads (all but what impaired.NOT_RECOVERED lists).  These are conditions on the INPUTS:
a change of synth that moved a case across a threshold fails here, not silently in the GPU test."""
import math

import numpy as np
import pytest

import exit_paths as ep
import impaired as im
import parity


@pytest.fixture(scope="module")
def built():
    cases = im.build()
    c, ts = im.coef(), im.synth.sch_training_sequence()
    jobs = [(k["raw"], c, ts, im.FC) for k in cases]
    orcs = parity.pool_map(ep.oracle_job_r, jobs, max_workers=16)
    lits = parity.pool_map(ep.literal_job, jobs, max_workers=16)
    scans = parity.pool_map(im.scan_job, [(k["raw"], c) for k in cases], max_workers=16)
    return cases, orcs, lits, scans


@pytest.fixture(scope="module")
def follow(built):
    """the restatements of the follow-up family on the oracle's r_correct and pos_info of every case flagged for them"""
    cases, orcs, _, _ = built
    flagged = [(k, orc) for k, (orc, _) in zip(cases, orcs) if k["follow"]]
    assert all(orc is not None and orc["status"] == 0 for _, orc in flagged)
    res = parity.pool_map(im.followup_job, [(orc["r_correct"], orc["pos_info"], im.PLANTED[k["base"]][1], False) for k, orc in flagged],
                          max_workers=16)
    by = {k["name"]: orc for k, orc in flagged}
    pairs = parity.pool_map(im.pair_job, [(by["plain"]["r_correct"], by[x]["r_correct"], by["plain"]["pos_info"], by[x]["pos_info"])
                                          for x in im.PAIR_PARTNERS], max_workers=16)
    return flagged, res, pairs


def test_every_case_takes_its_designed_exit(built):
    cases, orcs, _, _ = built
    for k, (orc, err) in zip(cases, orcs):
        assert orc is not None, (k["name"], err)
        print(k["name"], orc["status"], list(orc["stage_exit"]), ep.table_shape(orc["pos_info"]), orc["sampling_ppm"], orc["carrier_ppm"])
        assert orc["status"] == k["status"], (k["name"], orc["status"], k["status"])
        assert orc["n_fcch"] == len(orc["fcch_pos"]) and orc["n_pos_rows"] == len(orc["pos_info"])
        assert (orc["status"] == 0) == (orc["r_len"] > 0)


def test_the_literal_oracle_agrees_on_every_case(built):
    cases, orcs, lits, _ = built
    for k, (a, _), (b, err) in zip(cases, orcs, lits):
        assert b is not None, (k["name"], err)
        name = k["name"]
        assert list(a["stage_exit"]) == list(b["stage_exit"]) and a["status"] == b["status"], (name, a["stage_exit"], b["stage_exit"])
        assert (a["n_fcch"], a["n_pos_rows"], a["first_fcch_pos"]) == (b["n_fcch"], b["n_pos_rows"], b["first_fcch_pos"]), name
        assert np.array_equal(a["coarse_pos"], b["coarse_pos"]), name
        assert np.array_equal(a["fine_first_round_pos"], b["first"]), name
        assert np.array_equal(a["fcch_pos"], b["fcch_pos"]), name
        assert a["pos_info"].shape == b["pos_info"].shape and np.array_equal(a["pos_info"], b["pos_info"]), name
        for x, y in zip(list(a["sampling_ppm"]) + list(a["carrier_ppm"]) + [a["total_sampling_ppm"], a["total_carrier_ppm"]],
                        b["sp"] + b["cp"] + b["tot"]):
            assert (math.isinf(x) and math.isinf(y)) or abs(x - y) <= 1e-9 * abs(x) + 1e-12, (name, x, y)


def test_the_set_spreads_over_the_exits_and_reaches_the_estimators(built):
    cases, orcs, _, _ = built
    met = {orc["status"] for orc, _ in orcs}
    assert met >= {0, 1, 2, 4, 6, 7, 9}, met
    mixed = im.ordered(cases)
    assert len(mixed) >= 40 and all(len(k["raw"]) == 2 * im.N for k in mixed)
    assert sum(im.calibrates(orc) for orc, _ in orcs) >= 15
    # the impairment reached the estimator: the total sampling ppm of a calibrating case is off its un-impaired twin's (the
    # re-quantised base capture of the same dongle and length)
    by = {k["name"]: orc for k, (orc, _) in zip(cases, orcs)}
    twin = {"d0": by["plain"]["total_sampling_ppm"], "d3": by["d3plain"]["total_sampling_ppm"]}
    moved = [(k["name"], orc["total_sampling_ppm"] - twin[k["base"]]) for k, (orc, _) in zip(cases, orcs)
             if k["group"] == "mixed" and im.calibrates(orc) and abs(orc["total_sampling_ppm"] - twin[k["base"]]) > 1e-3]
    print("total sampling ppm moved by the impairment:", moved)
    assert len(moved) >= 3, moved
    # ... and the first stage's estimate alone moves in many more (the SCH stage takes most of it back)
    first = [k["name"] for k, (orc, _) in zip(cases, orcs)
             if k["group"] == "mixed" and im.calibrates(orc) and abs(orc["sampling_ppm"][0] - by["plain" if k["base"] == "d0" else "d3plain"]["sampling_ppm"][0]) > 0.5]
    assert len(first) >= 8, first


def test_the_scanner_meets_a_non_finite_snr_and_a_capture_without_a_hit(built):
    cases, _, _, scans = built
    for k, sc in zip(cases, scans):
        print(k["name"], "scanner snr", sc["snr"], "num_hit", sc["num_hit"], "hop walk", len(sc["coarse_pos"]),
              "windows +inf / -inf / NaN", sc["window_kinds"])
    assert any(not math.isfinite(sc["snr"]) for sc in scans), "no case with a non-finite scanner SNR"
    assert any(sc["num_hit"] == 0 for sc in scans), "no case without a hit"
    by = {k["name"]: sc for k, sc in zip(cases, scans)}
    # the stretch of constant bytes: windows whose noise power is exactly zero, inside a capture whose detector still hits
    assert by["dropout120k"]["window_kinds"][0] + by["dropout120k"]["window_kinds"][2] > 0 and by["dropout120k"]["num_hit"] > 0


def test_no_window_of_the_set_comes_near_the_dc_residue_floor(built):
    """The batch path answers NaN for a window whose total power is at or below (16 |mean sum(coef)| 2^-46)^2 (snr_from_power,
    DecView::floor2): a threshold, not a construction.  What reaches it is a window whose samples all equal the capture's mean,
    where the reference computes an exact 0/0.  A stretch constant at another byte value is at least 1/N off the mean (the mean is
    an integer sum over N samples), 1e-6 here against the 1.8e-12 the floor stands for, and a window that is not constant holds
    integers a whole LSB apart.  None of the impaired captures -- 0.7 LSB of signal, a gate to constant bytes, both rails -- has a
    window of exactly zero power, and the weakest window of the set stays more than ten orders of magnitude above the floor."""
    cases, _, _, scans = built
    margin = min(sc["min_power"] / sc["floor"] for sc in scans)
    for k, sc in zip(cases, scans):
        print(k["name"], "smallest window power", sc["min_power"], "floor", sc["floor"], "windows of zero power", sc["zero_power"])
    print(f"smallest window power / floor over the set: {margin:.3e}")
    assert all(sc["zero_power"] == 0 for sc in scans)
    assert margin > 1e10, margin


def test_the_follow_ups_stay_off_their_tie_guards(follow):
    """over the whole set at most 1 burst in 50 is excluded by a restatement's own guard, and no case loses more than one"""
    flagged, res, pairs = follow
    total = {}
    for (k, _), r in zip(flagged, res):
        counts = im.guard_counts(r)
        print(k["name"], counts)
        for fn, (n, bad) in counts.items():
            assert bad <= 1, (k["name"], fn, bad)
            total[fn] = tuple(np.add(total.get(fn, (0, 0)), (n, bad)))
    for x, want in zip(im.PAIR_PARTNERS, pairs):
        n, bad = im.pair_guard_counts(want)
        print("plain ->", x, (n, bad), "status", want["row"][0], "used", want["row"][3])
        assert bad == 0, f"pair (plain, {x}): a decision on a tie -- replace the pair, do not skip it"
        assert n >= 10 and want["row"][0] == 0.0, (x, n, want["row"][0])
        total["pair"] = tuple(np.add(total.get("pair", (0, 0)), (n, bad)))
    print("bursts looked at / excluded per function:", total)
    for fn, (n, bad) in total.items():
        assert n >= 20 and 50 * bad <= n, (fn, n, bad)


def test_the_restatements_recover_the_planted_payloads_where_pinned(follow):
    flagged, res, _ = follow
    seen = {}
    for (k, orc), r in zip(flagged, res):
        seen[k["name"]] = im.recovered(k, orc["pos_info"], r)
        print(k["name"], seen[k["name"]], "sch ok", r["sch"]["ok"].tolist(), "si ok", r["si"]["ok"].tolist(), "tsc idx", r["bcch"]["idx"])
    for name, got in seen.items():
        missed = tuple(fn for fn, hit in got.items() if not hit)
        assert missed == tuple(im.NOT_RECOVERED.get(name, ())), (name, got)
    assert set(im.NOT_RECOVERED) <= set(seen) and sum(all(v.values()) for v in seen.values()) >= 15
