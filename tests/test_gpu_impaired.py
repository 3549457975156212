"""GPU tests (-m gpu) of the batch chain and its follow-up family on impaired captures: the cases of tests/impaired.py
(tests/test_impaired_cpu.py holds them to their designed exits and the restatements to their tie guards with the CPU alone) --
a second cell on the channel, a neighbour carrier, echoes, clipping, faint signals, fades, drop-outs to constant bytes, CW spurs,
DC steps, I/Q imbalance, carrier and noise beyond the drawn range -- in ONE batch against the live oracle, every route through
the chain bit for bit (GSMCAL_CERT=0 is the chain without the Parseval certificate: equality is the certificate's soundness on
these inputs), each case alone, the scanner with its window SNRs (the +inf of a constant stretch included), and FCCH_demod,
BCCH_demod, SCH_decode, BCCH_decode and pair_coherence in their batch forms on the GPU's own corrected streams against their
restatements and the planted payloads.
No bar of its own: positions, counts and status exact, ppm parity.PPM_RTOL / PPM_ATOL, SNR parity.SNR_ATOL with non-finite values
equal in kind, corrected streams STREAM_RTOL of their peak, the follow-ups through the compare functions of their own test files."""
import numpy as np
import pytest

import exit_paths as ep
import impaired as im
import parity
from test_gpu_bcch_decode import compare as compare_si
from test_gpu_bcch_demod import compare as compare_bcch
from test_gpu_exit_paths import ROUTES, check_against_oracle, run_dev, same_all
from test_gpu_fcch_demod import compare as compare_fcch
from test_gpu_general_taps import STREAM_RTOL, context_under, same_answer
from test_gpu_pair_coherence import compare as compare_pair, worst as pair_worst
from test_gpu_sch_decode import compare as compare_sch

pytestmark = pytest.mark.gpu

FC = im.FC
WINDOW_CASES = ("dropout120k", "dropout30k", "faint0.02", "faint0.01", "spur+67-15", "spur+67-10", "spur+67+0")
SINGLES = ("echo24", "cochannel-10")             # the two impaired streams whose batch rows are held to the single-stream calls


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


@pytest.fixture(scope="module")
def built():
    """the cases with their oracle results (corrected stream included) and the scanner's, the mixed batch in im.ordered's order"""
    cases = im.build()
    coef, ts = im.coef(), im.synth.sch_training_sequence()
    orcs = parity.pool_map(ep.oracle_job_r, [(k["raw"], coef, ts, FC) for k in cases], max_workers=16)
    scans = parity.pool_map(im.scan_job, [(k["raw"], coef) for k in cases], max_workers=16)
    for k, (orc, err), sc in zip(cases, orcs, scans):
        assert orc is not None and orc["status"] == k["status"], (k["name"], err)
        k["orc"], k["scan"] = orc, sc
    mixed = im.ordered(cases)
    print("mixed batch:", [(k["name"], k["status"]) for k in mixed])
    return {"mixed": mixed, "own": [k for k in cases if k["group"] == "own"], "coef": coef, "ts": ts,
            "raw": np.stack([k["raw"] for k in mixed]), "at": {k["name"]: i for i, k in enumerate(mixed)}}


@pytest.fixture(scope="module")
def mixed_ref(g, built):
    """the mixed batch on a fresh profiled context (device-pointer call, NaN pre-fill): (output, details, kernel launches)"""
    res, det, names = run_dev(g, built["raw"], built["coef"], built["ts"], profile=True)
    return res[0], det, names


def worst_over_tolerance(cases, out, det):
    """largest deviation / tolerance per quantity over the streams of one call (for the record: DESIGN.md quotes them)"""
    w = {"ppm": 0.0, "coarse_snr": 0.0, "r_correct": 0.0}
    for i, k in enumerate(cases):
        orc = k["orc"]
        want = list(orc["sampling_ppm"]) + list(orc["carrier_ppm"]) + [orc["total_sampling_ppm"], orc["total_carrier_ppm"]]
        for a, b in zip(out["table"][i, :6], want):
            if np.isfinite(b):
                w["ppm"] = max(w["ppm"], abs(a - b) / (parity.PPM_RTOL * abs(b) + parity.PPM_ATOL))
        n = det["counts"][i][0]
        if n and orc["coarse_pos"][0] != -1.0:
            with np.errstate(invalid="ignore"):                             # (+inf on both sides: compare_stream holds the kind)
                d = np.abs(det["coarse_snr"][i, :n] - orc["coarse_snr"])
            w["coarse_snr"] = max(w["coarse_snr"], float(np.max(d[np.isfinite(d)], initial=0.0)) / parity.SNR_ATOL)
        if orc["r_len"] > 0:
            ref = orc["r_correct"]
            w["r_correct"] = max(w["r_correct"], float(np.max(np.abs(out["r_correct"][i, :len(ref)] - ref)) / (STREAM_RTOL * np.max(np.abs(ref)))))
    return w


# ---- (a) one mixed batch against the oracle -------------------------------------------------------------------------------
def test_mixed_batch_against_the_oracle(built, mixed_ref):
    out, det, _ = mixed_ref
    check_against_oracle(built["mixed"], out, det)
    st = [k["status"] for k in built["mixed"]]
    assert set(st) >= {0, 1, 2, 4, 6, 7, 9} and len(st) >= 40
    assert all(a != b or a == 0 for a, b in zip(st, st[1:])), f"streams that leave early should have a neighbour that leaves elsewhere: {st}"
    print("largest deviation / tolerance:", {k: f"{v:.3g}" for k, v in worst_over_tolerance(built["mixed"], out, det).items()})


def test_own_lengths_against_the_oracle(g, built):
    assert len(built["own"]) >= 2
    for k in built["own"]:
        res, det, _ = run_dev(g, k["raw"][None, :], built["coef"], built["ts"])
        check_against_oracle([k], res[0], det)


# ---- (b) every route, bit for bit -----------------------------------------------------------------------------------------
# ROUTES of test_gpu_exit_paths (the four-launch tail, the chain without the certificate, four lanes, two tail slots) and the
# throughput detector, whose SNR rounds stop at the first certified hit (k_coarse_scan computes the window SNRs itself)
@pytest.mark.parametrize("env", ROUTES + [{"GSMCAL_SNR_FULL": "0"}], ids=lambda e: ",".join(f"{k[7:]}={v}" for k, v in e.items()))
def test_routes_agree(g, built, mixed_ref, env):
    res, _, _ = run_dev(g, built["raw"], built["coef"], built["ts"], env=env)
    same_all(mixed_ref[0], res[0], str(env))


def test_graph_replay_agrees(g, built, mixed_ref):
    """GSMCAL_GRAPH=2 over three host-pointer calls on one context: eager, capture + replay, replay"""
    ref = mixed_ref[0]
    cx = context_under(g, {"GSMCAL_GRAPH": "2"})
    try:
        for k in range(3):
            out = g.calibrate_batch(built["raw"], built["coef"], built["ts"], FC, want_r=True, ctx=cx)
            same_answer(ref, out)
            assert np.array_equal(ref["r_len"], out["r_len"]), k
            for i, L in enumerate(ref["r_len"]):
                if L > 0:
                    assert np.array_equal(ref["r_correct"][i, :L], out["r_correct"][i, :L]), (k, i)
    finally:
        cx.close()


def test_four_calls_in_flight_agree(g, built, mixed_ref):
    """four device-pointer calls four deep, each into its own outputs"""
    res, _, _ = run_dev(g, built["raw"], built["coef"], built["ts"], calls=4, depth=4)
    for k, out in enumerate(res):
        same_all(mixed_ref[0], out, f"call {k}")


# ---- (c) each case alone ---------------------------------------------------------------------------------------------------
def test_each_case_alone_gives_the_row_of_the_mixed_batch(g, built, mixed_ref):
    ref = mixed_ref[0]
    for i, k in enumerate(built["mixed"]):
        one = g.calibrate_batch(built["raw"][i:i + 1], built["coef"], built["ts"], FC, want_r=True)
        assert np.array_equal(one["table"][0], ref["table"][i], equal_nan=True), (k["name"], one["table"][0], ref["table"][i])
        assert np.array_equal(one["pos_info"][0], ref["pos_info"][i]), k["name"]
        assert one["r_len"][0] == ref["r_len"][i], k["name"]
        L = int(ref["r_len"][i])
        if L > 0:
            assert np.array_equal(one["r_correct"][0, :L], ref["r_correct"][i, :L]), k["name"]


# ---- (d) the scanner and its window SNRs ----------------------------------------------------------------------------------
def snr_same(got, want):
    """SNRs at the bar; a non-finite value must be the same kind of non-finite value"""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    fin = np.isfinite(want)
    return bool(got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want))
                and np.array_equal(np.isneginf(got), np.isneginf(want)) and np.all(np.abs(got[fin] - want[fin]) <= parity.SNR_ATOL))


def test_scanner_against_the_oracle(g, built):
    coef = built["coef"]
    cases = built["mixed"] + built["own"]
    outs = [g.fcch_scan_batch(built["raw"], coef)] + [g.fcch_scan_batch(k["raw"][None, :], coef) for k in built["own"]]
    kinds = set()
    for j, k in enumerate(cases):
        out, i = (outs[0], j) if j < len(built["mixed"]) else (outs[1 + j - len(built["mixed"])], 0)
        live, n = k["scan"], out["counts"][i]
        print(k["name"], "scanner snr", out["snr"][i], live["snr"], "num_hit", out["num_hit"][i], live["num_hit"])
        assert live["num_hit"] == out["num_hit"][i], (k["name"], live["num_hit"], out["num_hit"][i])
        assert snr_same(out["snr"][i], live["snr"]), (k["name"], out["snr"][i], live["snr"])
        kinds.add("finite" if np.isfinite(live["snr"]) else "non-finite")
        if live["coarse_pos"][0] == -1.0:
            assert n == 0 and out["positions"][i, 0] == -1.0, k["name"]
            kinds.add("no hit")
        else:
            parity.assert_positions(out["positions"][i, :n], live["coarse_pos"], f"scan positions ({k['name']})")
            assert snr_same(out["pos_snr"][i, :n], live["coarse_snr"]), (k["name"], out["pos_snr"][i, :n], live["coarse_snr"])
    assert kinds == {"finite", "non-finite", "no hit"}, kinds


@pytest.mark.parametrize("env", [{}, {"GSMCAL_SNR_FULL": "0", "GSMCAL_SNR_INLINE_KEEP": "1"}], ids=["table", "inline_kept"])
def test_window_snrs_of_the_dropout_faint_and_spur_cases(g, built, env):
    """every window SNR the detector built -- the full table of a latency batch, and the moving search's 3 579 windows that the
    throughput detector computes inside k_coarse_scan -- against the oracle's value: the +inf of the windows inside the stretch of
    constant bytes as +inf, no NaN where the reference has none, and a window ruled out without a spectrum (-inf) below the
    screening level of 5 dB in the reference"""
    names = WINDOW_CASES
    raw = np.stack([built["raw"][built["at"][n]] for n in names])
    cx = context_under(g, env)
    try:
        g.calibrate_batch(raw, built["coef"], built["ts"], FC, ctx=cx)
        tabs = [g.last_batch_snr(i, ctx=cx) for i in range(len(raw))]
    finally:
        cx.close()
    worst, n_inf = 0.0, 0
    for name, (tab, n_mov) in zip(names, tabs):
        want = built["mixed"][built["at"][name]]["scan"]["windows"]
        assert n_mov == 3579 and len(tab) in (n_mov, len(want)), (name, n_mov, len(tab), len(want))
        want = want[:len(tab)]
        screened = np.isneginf(tab)
        assert not screened[:n_mov].any(), name                               # the moving search's windows are all computed
        assert np.all(want[screened] < 5.0), (name, want[screened][~(want[screened] < 5.0)][:4])
        got, ref = tab[~screened], want[~screened]
        assert snr_same(got, ref), (name, "kinds", int(np.sum(np.isposinf(got))), int(np.sum(np.isposinf(ref))), int(np.sum(np.isnan(got))),
                                    int(np.sum(np.isnan(ref))), "worst", np.max(np.abs(got - ref)[np.isfinite(ref) & np.isfinite(got)], initial=0.0))
        fin = np.isfinite(ref)
        worst = max(worst, float(np.max(np.abs(got[fin] - ref[fin]), initial=0.0)))
        n_inf += int(np.sum(np.isposinf(got)))
        print(name, "windows", len(tab), "computed", int(np.sum(~screened)), "+inf", int(np.sum(np.isposinf(got))))
    print(f"largest window SNR difference {worst:.3e} dB = {worst / parity.SNR_ATOL:.3g} of the bar")
    # (the stretch starts at sample 300 000, window 4 687: behind the moving search's windows, inside the full table alone)
    assert n_inf > 0 or env, "the constant stretch should give windows with an SNR of +inf"


# ---- (e) the follow-up family on the GPU's own corrected streams ----------------------------------------------------------
@pytest.fixture(scope="module")
def followed(g, built, mixed_ref):
    """the flagged streams of the mixed batch, as the GPU returned them, with the four single-stream restatements of each"""
    out = mixed_ref[0]
    idx = [i for i, k in enumerate(built["mixed"]) if k["follow"]]
    assert len(idx) >= 15 and all(out["r_len"][i] > 0 for i in idx)
    streams = {i: (np.ascontiguousarray(out["r_correct"][i, :int(out["r_len"][i])]), out["pos_info"][i]) for i in idx}
    tsc = [im.PLANTED[k["base"]][1] for k in built["mixed"]]
    wants = parity.pool_map(im.followup_job, [(streams[i][0], streams[i][1], tsc[i], True) for i in idx], max_workers=16)
    return {"idx": idx, "streams": streams, "tsc": tsc, "want": dict(zip(idx, wants)), "got": {}}


def same_bits(a, b):
    a, b = (np.ascontiguousarray(v, dtype=np.float64).view(np.uint64) for v in (a, b))
    return a.shape == b.shape and np.array_equal(a, b)


def check_no_stream_rows(built, out, status_col):
    """a stream the chain returned no r for: the POST_NO_POS row of every batch form (10)"""
    gone = [i for i, k in enumerate(built["mixed"]) if out["r_len"][i] < 0]
    assert len(gone) >= 15 and np.all(status_col[gone] == 10.0), status_col[gone]


def test_fcch_demod_batch(g, built, mixed_ref, followed):
    out = mixed_ref[0]
    table = g.fcch_demod_batch(out["r_correct"], out["r_len"], out["pos_info_raw"], 8, FC)
    t = g.demod_rows(table)
    check_no_stream_rows(built, out, t["status"])
    for i in followed["idx"]:
        k = int(t["num_fcch"][i])
        got = {"freq": t["freq"][i, :k], "snr": t["snr"][i, :k], "max_idx": t["max_idx"][i, :k].astype(np.int64),
               "mean_freq": float(t["mean_freq"][i]), "carrier_ppm": float(t["carrier_ppm"][i])}
        print(built["mixed"][i]["name"])
        assert t["status"][i] == 0.0
        compare_fcch(got, followed["want"][i]["fcch"])
        followed["got"].setdefault(i, {})["fcch"] = got
    for name in SINGLES:
        i = built["at"][name]
        one = g.FCCH_demod(*followed["streams"][i], 8, FC)
        got = followed["got"][i]["fcch"]
        assert all(same_bits(one[f], got[f]) for f in ("freq", "snr", "mean_freq", "carrier_ppm")) and np.array_equal(one["max_idx"], got["max_idx"]), name


def test_bcch_demod_batch(g, built, mixed_ref, followed):
    out = mixed_ref[0]
    nts = g.synth.normal_training_sequences(8)
    res = g.bcch_demod_batch(out["r_correct"], out["r_len"], out["pos_info_raw"], 8, nts, FC, want_corr=True, want_r=True)
    t = g.bcch_rows(res["table"])
    check_no_stream_rows(built, out, t["status"])
    assert np.array_equal(res["r_len"], out["r_len"])
    for i in followed["idx"]:
        k, case = int(t["num_bcch"][i]), built["mixed"][i]
        got = {"status": int(t["status"][i]), "idx": int(t["tsc_idx"][i]), "num_bcch": k, "num_agree": t["num_agree"][i],
               "mean_fo": float(t["mean_fo"][i]), "carrier_ppm": float(t["carrier_ppm"][i]), "corr_val": res["corr"][i, :4].T,
               "r": res["r"][i, :int(out["r_len"][i])]}
        for f in ("max_idx", "peak", "runner_up", "phase"):
            got[f] = t[f][i, :k]
        print(case["name"])
        s, pos = followed["streams"][i]
        compare_bcch(got, followed["want"][i]["bcch"], s, pos, 8)
        if "tsc" not in im.NOT_RECOVERED.get(case["name"], ()):
            assert got["status"] == 0 and got["idx"] == followed["tsc"][i] + 1, (case["name"], got["idx"])
    for name in SINGLES:
        i = built["at"][name]
        one = g.BCCH_demod(*followed["streams"][i], nts, 8, FC)
        assert same_bits(res["table"][i], one["row"]), name
        assert same_bits(res["r"][i, :len(one["r"])].view(np.float64), one["r"].view(np.float64)), name


def test_sch_decode_batch(g, built, mixed_ref, followed):
    out = mixed_ref[0]
    res = g.sch_decode_batch(out["r_correct"], out["r_len"], out["pos_info_raw"], 8, built["ts"], want_soft=True, want_u=True)
    t = g.sch_rows(res["table"])
    check_no_stream_rows(built, out, t["status"])
    for i in followed["idx"]:
        k, case = int(t["num_sch"][i]), built["mixed"][i]
        got = {"status": int(t["status"][i]), "bsic": int(t["bsic"][i]), "fn_anchor": int(t["fn_anchor"][i]), "pos_anchor": int(t["pos_anchor"][i]),
               "num_sch": k, "num_ok": int(t["num_ok"][i]), "num_consistent": int(t["num_consistent"][i]), "mean_slope": float(t["mean_slope"][i]),
               "u": res["u"][i, :k], "soft": res["soft"][i, :k]}
        for f in ("ok", "bsic_b", "fn", "ts_err", "corrected", "slope", "amp"):
            got[f] = t[f][i, :k]
        print(case["name"])
        s, pos = followed["streams"][i]
        compare_sch(got, followed["want"][i]["sch"], s, pos, 8)
        followed["got"].setdefault(i, {})["sch"] = got
        if "sch" not in im.NOT_RECOVERED.get(case["name"], ()):
            hit = im.recovered(case, pos, {"sch": got, "si": followed["want"][i]["si"], "bcch": followed["want"][i]["bcch"]})
            assert hit["sch"] and got["bsic"] == im.PLANTED[case["base"]][2], (case["name"], got["bsic"], got["fn"])
    for name in SINGLES:
        i = built["at"][name]
        one = g.SCH_decode(*followed["streams"][i], built["ts"], 8, want_soft=True)
        k = one["num_sch"]
        assert same_bits(res["table"][i], one["row"]) and same_bits(res["soft"][i, :k], one["soft"]) and np.array_equal(res["u"][i, :k], one["u"]), name


def test_bcch_decode_batch(g, built, mixed_ref, followed):
    out = mixed_ref[0]
    res = g.bcch_decode_batch(out["r_correct"], out["r_len"], out["pos_info_raw"], 8, followed["tsc"], want_soft=True)
    t = g.si_rows(res["table"])
    check_no_stream_rows(built, out, t["status"])
    for i in followed["idx"]:
        k, case = int(t["num_blocks"][i]), built["mixed"][i]
        got = {"status": int(t["status"][i]), "num_blocks": k, "num_ok": int(t["num_ok"][i]), "first_ok": int(t["first_ok"][i]),
               "octets": res["octets"][i, :k], "soft": res["soft"][i, :k]}
        for f in g.SI_BLOCK_FIELDS:
            got[f] = t[f][i, :k]
        print(case["name"])
        s, pos = followed["streams"][i]
        compare_si(got, followed["want"][i]["si"], s, pos, 8)
        if "si" not in im.NOT_RECOVERED.get(case["name"], ()):
            hit = im.recovered(case, pos, {"sch": followed["want"][i]["sch"], "si": got, "bcch": followed["want"][i]["bcch"]})
            assert hit["si"], (case["name"], got["ok"])
            f = g.si_fields(got["octets"][got["first_ok"] - 1])
            assert f["valid"] == 1 and (f["mcc"], f["mnc"], f["lac"]) == (im.MCC, im.MNC, im.LAC), (case["name"], f)
            assert f["cell_id"] == (im.PLANTED[case["base"]][4] if f["si_type"] == 3 else -1), (case["name"], f)
    for name in SINGLES:
        i = built["at"][name]
        one = g.BCCH_decode(*followed["streams"][i], followed["tsc"][i], 8, want_soft=True)
        k = one["num_blocks"]
        assert same_bits(res["table"][i], one["row"]) and same_bits(res["soft"][i, :k], one["soft"]) and np.array_equal(res["octets"][i, :k], one["octets"]), name


def test_pair_coherence_batch(g, built, mixed_ref, followed):
    """(plain, X): the same transmission through another channel, lag0 = 0, the default lag range"""
    out = mixed_ref[0]
    a = built["at"]["plain"]
    pairs = [(a, built["at"][x]) for x in im.PAIR_PARTNERS]
    st = followed["streams"]
    wants = parity.pool_map(im.pair_job, [(st[a][0], st[b][0], st[a][1], st[b][1]) for _, b in pairs], max_workers=16)
    res = g.pair_coherence_batch(out["r_correct"], out["r_len"], out["pos_info_raw"], 8, pairs, 0, want_corr=True)
    t = g.pair_rows(res["table"])
    for q, (x, want) in enumerate(zip(im.PAIR_PARTNERS, wants)):
        print(f"plain -> {x}: used {int(t['num_used'][q])} delay0 {t['delay0'][q]:.4f} coherence mean {t['mean_coherence'][q]:.4f} min {t['min_coherence_seen'][q]:.4f} "
              f"carrier {t['rel_carrier_hz'][q]:.3f} Hz")
        compare_pair(res["table"][q], res["corr"][q], want, f"plain -> {x}")
        assert t["status"][q] == 0 and t["num_eval"][q] >= 10
    for q in (1, 5):                                                     # echo24, cochannel-10
        _, b = pairs[q]
        one = g.pair_coherence(st[a][0], st[b][0], st[a][1], 8, 0, want_corr=True)
        k = one["num_bursts"]
        assert same_bits(res["table"][q], one["row"]) and same_bits(res["corr"][q, :k].view(np.float64), one["corr"].view(np.float64)), im.PAIR_PARTNERS[q]
    print("largest deviation / tolerance:", {k: f"{v:.3g}" for k, v in pair_worst.items()})


# ---- (f) for the record ---------------------------------------------------------------------------------------------------
def test_record_of_the_kernels_that_ran(built, mixed_ref):
    """Not asserted beyond the default route's tail: which kernels the mixed batch launched, and per case what the chain left.
    (The certificate's open-chunk count is not exposed by gsmcal_last_batch_details or the profile.)"""
    out, det, names = mixed_ref
    print("mixed batch kernels:", sorted(names.items()))
    for i, k in enumerate(built["mixed"]):
        print(f"{k['name']}: status {out['table'][i, 9]:.0f} coarse {det['counts'][i][0]} fine first {det['counts'][i][1]} fcch {det['counts'][i][2]} "
              f"sch first {det['counts'][i][3]} rows {out['table'][i, 7]:.0f} r_len {out['r_len'][i]}")
    assert [k for k in names if "k_post_chain_r" in k] == ["(k_post_chain_r<8, 512, 47>)"], names
