"""CPU tests (no marker) of the exit-path case set, with the oracles alone: every case of tests/exit_paths.py takes exactly
the early exit and builds exactly the pos_info shape it was designed for, in the vectorised oracle and in the literal one,
and the set as a whole holds what tests/test_gpu_exit_paths.py relies on.  These are conditions on the INPUTS: a change of
synth that moved a burst would fail here, not silently empty the GPU test."""
import math

import numpy as np
import pytest

import exit_paths as ep
import parity


@pytest.fixture(scope="module")
def built():
    n_mixed, cases = ep.build()
    c, ts = ep.coef(), ep.synth.sch_training_sequence()
    jobs = [(k["raw"], c, ts, ep.FC) for k in cases]
    orcs = parity.pool_map(ep.oracle_job_r, jobs, max_workers=16)
    lits = parity.pool_map(ep.literal_job, jobs, max_workers=16)
    return n_mixed, cases, orcs, lits


def test_every_case_takes_its_designed_exit_and_table_shape(built):
    _, cases, orcs, _ = built
    for k, (orc, err) in zip(cases, orcs):
        assert orc is not None, (k["name"], err)
        print(k["name"], orc["status"], list(orc["stage_exit"]), ep.table_shape(orc["pos_info"]), orc["sampling_ppm"])
        assert orc["status"] == k["status"], (k["name"], orc["status"], k["status"])
        if k["table"] is not None:
            assert ep.table_shape(orc["pos_info"]) == k["table"], (k["name"], ep.table_shape(orc["pos_info"]), k["table"])
        # the four new values follow from the outputs the oracle had before
        assert orc["n_fcch"] == len(orc["fcch_pos"]) and orc["n_pos_rows"] == len(orc["pos_info"])
        assert orc["first_fcch_pos"] == orc["pos_info"][0, 0]
        assert (orc["status"] == 0) == (orc["r_len"] > 0)


def test_the_literal_oracle_agrees_on_every_case(built):
    _, cases, orcs, lits = built
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


def test_the_set_reaches_every_exit_the_chain_can_meet_first(built):
    _, cases, orcs, _ = built
    met = {orc["status"] for orc, _ in orcs}
    assert met >= {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11}, met
    mixed = {orc["status"] for k, (orc, _) in zip(cases, orcs) if k["group"] == "mixed"}
    assert mixed >= {0, 1, 2, 3, 4, 6, 7, 8, 9, 11}, f"the one mixed batch should leave at every stage: {mixed}"
    # POST_NO_POS (10) is never the first exit: per stage
    post = [orc["stage_exit"][3] for orc, _ in orcs]
    assert 10 in post and all((e == 10) == (orc["status"] not in (0, 11)) for e, (orc, _) in zip(post, orcs))
    # ... and FEW_HITS of the SCH stage behind every fine-stage exit that hands on a sentinel or too few positions
    assert all(orc["stage_exit"][2] == 2 for orc, _ in orcs if orc["stage_exit"][1] in (2, 3, 4, 6))


def test_the_set_holds_the_table_endings_and_a_resampling_sch_stage(built):
    _, cases, orcs, _ = built
    shapes = [ep.table_shape(orc["pos_info"]) for orc, _ in orcs]
    assert any(s[1] == 0 for s in shapes), "a table ending on an FCCH row"
    assert any(s[1] == 1 for s in shapes), "a table ending on an SCH row"
    for nb in (1, 2, 3):
        assert any(s[1] == 2 and s[2] == nb for s in shapes), f"a table ending on BCCH row {nb} of its block"
    assert any(s == (1, -1, 0) for s in shapes) and any(s[1] == -1 and s[0] == 15 for s in shapes), "both sentinel shapes"
    assert any(orc["status"] == 0 and orc["sampling_ppm"][1] != 0 for orc, _ in orcs), "OP_LERP behind the SCH stage (e != 0)"
    assert any(orc["status"] == 11 and orc["sampling_ppm"][1] != 0 for orc, _ in orcs)
    n_mixed = built[0]
    assert any(len(k["raw"]) % 16 for k in cases if k["group"] == "own"), "a length with 2N off a 16-byte boundary"
    assert sum(k["group"] == "mixed" for k in cases) >= 30 and all(len(k["raw"]) == 2 * n_mixed for k in cases if k["group"] == "mixed")


def test_a_first_burst_in_the_first_64_symbols_is_not_hit(built):
    """The fine stage's index error (FCCH_fine_correction.m:40-43, sp < 1) needs a coarse hit inside the first 64 symbols.  The
    moving average is seeded with 999 dB (move_fft_snr_runtime_avg.m:11), so no window before ~mv_len = 160 (symbol 1240) can
    hit: with the first FCCH at the very start of the capture the detector locks on the second one.  The batch chain cannot
    reach that exit from raw bytes; it stays covered at function level."""
    _, cases, orcs, _ = built
    heads = [(k, orc) for k, (orc, _) in zip(cases, orcs) if k["name"].startswith("head")]
    assert len(heads) == len(ep.HEAD_CUTS)
    for k, orc in heads:
        assert orc is not None and orc["coarse_pos"][0] > 10000 and len(orc["coarse_pos"]) == 4, (k["name"], orc["coarse_pos"])


def by_name(built):
    _, cases, orcs, _ = built
    return {k["name"]: (k, orc) for k, (orc, _) in zip(cases, orcs)}


def test_the_drop_of_the_last_burst_with_nine_and_with_four_bursts_left(built):
    """FCCH_fine_correction.m:135: the regenerated last burst overruns len(r) and is dropped.  drop135 keeps nine of ten and
    calibrates; fewbursts keeps four of five: positions and the resampled stream come back, the carrier block is skipped
    (GSMCAL_S_FINE_FEW_BURSTS).  No other case of the set takes the drop."""
    cases = by_name(built)
    took = [n for n, (_, orc) in cases.items() if orc["stage_exit"][1] in (0, 5) and len(orc["fine_first_round_pos"]) >= 5
            and len(orc["fcch_pos"]) == len(orc["fine_first_round_pos"]) - 1]
    assert sorted(took) == ["drop135", "fewbursts"], took
    _, orc = cases["drop135"]
    assert orc["status"] == 0 and len(orc["fine_first_round_pos"]) == 10 and orc["n_fcch"] == 9 and orc["r_len"] > 0
    _, orc = cases["fewbursts"]
    assert orc["status"] == 5 and list(orc["stage_exit"]) == [0, 5, 2, 10]
    assert len(orc["fine_first_round_pos"]) == 5 and orc["n_fcch"] == 4 and orc["fcch_pos"][0] != -1.0
    assert math.isfinite(orc["sampling_ppm"][0]) and math.isinf(orc["carrier_ppm"][0]) and orc["r_len"] == -1


def test_the_cases_on_a_threshold_sit_exactly_on_it(built):
    """a `<=` for `<` in the spacing test, or a `<` for `<=` in the slot-fit test, changes the outcome of one case of each pair"""
    cases = by_name(built)
    n_mixed = built[0]
    d40 = np.diff(cases["sch3-th40"][1]["sch_first_round_pos"])
    d39 = np.diff(cases["sch3-th39"][1]["sch_first_round_pos"])
    max_th = math.floor(100000 * 400 * 1e-6)                                       # SCH_corr_rate_correction.m:94-95
    assert max_th == 40 and np.max(np.abs(d40[:3] - 100000)) == 40 and np.max(np.abs(d39[:3] - 100000)) == 39, (d40, d39)
    assert cases["sch3-th40"][1]["status"] == 9 and cases["sch3-th39"][1]["status"] == 0
    for tag in ("sch", "bcch"):
        fit, nofit = cases[f"fit-{tag}"][1], cases[f"nofit-{tag}"][1]
        len_r = ep.len_r_after_fine(n_mixed, fit)
        assert len_r == ep.len_r_after_fine(n_mixed, nofit)
        assert fit["pos_info"][-1, 0] + 1250 - 1 == len_r, (tag, fit["pos_info"][-1], len_r)    # ep == len(r): the row is kept
        assert len(nofit["pos_info"]) == len(fit["pos_info"]) - 1
        assert np.array_equal(nofit["pos_info"], fit["pos_info"][:-1] + [1.0, 0.0]), tag          # ep == len(r) + 1: it is not
    assert cases["fit-bcch"][1]["pos_info"][-1, 1] == 2 and cases["fit-sch"][1]["pos_info"][-1, 1] == 1


def test_a_bcch_block_flagged_by_the_gap_four_hits_later_only(built):
    """sf42: the 11-frame gap is the fifth, so BCCH_flag(1) comes from b_idx(b_idx>=5)-4 alone (SCH_corr_rate_correction.m:141):
    the four BCCH rows right behind SCH 1; the cut one ends inside the block behind SCH 6"""
    cases = by_name(built)
    for name in ("sf42-full", "sf42-cut"):
        orc = cases[name][1]
        d = np.diff(orc["sch_first_round_pos"])
        assert len(d) >= 5 and np.all(np.abs(d[:4] - 100000) < 40) and abs(d[4] - 110000) < 44, (name, d)
        assert list(orc["pos_info"][:7, 1]) == [0, 1, 2, 2, 2, 2, 0], (name, orc["pos_info"][:7])
    pi = cases["sf42-cut"][1]["pos_info"]
    assert len(cases["sf42-cut"][1]["sch_first_round_pos"]) == 6 and list(pi[-4:, 1]) == [0, 1, 2, 2]
