"""GPU tests (-m gpu) of gsmcal_params: every tunable threshold moved, on the captures and parameter sets of
tests/params_cases.py (tests/test_params_cpu.py holds the two oracles to each other on all of them and proves that no set is
vacuous).  One batch call per set and capture length on a fresh context with set_params(...); every row against
oracle.calibrate_stream(..., params=...) through parity.compare_stream (columns 6..9 exact), pos_info as
tests/test_gpu_exit_paths.py compares it.  The coarse threshold additionally on every route through the detector; the scanner
rule on fcch_scan_batch; both tails, the chain function by function with its console lines, no stale parameters in a captured
graph or behind a call in flight, and the contract of set_params."""
import math

import numpy as np
import pytest

import exit_paths as ep
import params_cases as pc
import parity
from oracle import gsmcal_oracle as o
from test_gpu_exit_paths import as_out, dev_call
from test_gpu_general_taps import same_answer, stream_close

pytestmark = pytest.mark.gpu

FC = pc.FC
MARGIN = 10 * parity.SNR_ATOL


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


@pytest.fixture(scope="module")
def data():
    """captures, parameter sets and the oracle's answer to every (capture, set): two pool runs (the sets on an oracle figure --
    the SNR gate, the scanner's tolerance -- need the default-parameter results first)"""
    caps = pc.captures()
    coef, ts = ep.coef(), ep.synth.sch_training_sequence()
    stale = [(n, p) for n in STALE_CASES for p in (None, STALE_PARAMS)]
    base, sbase = pc.run_both("vector", caps, coef, ts, [(pc.GATE_CASE, None)] + stale, [(n, None) for n in pc.SCAN_CASES])
    sets = pc.SETS + pc.gate_sets(base[(pc.GATE_CASE, ())][0], MARGIN)
    ssets = pc.SCAN_SETS + pc.scan_tol_sets({n: sbase[(n, ())] for n in pc.SCAN_CASES})
    orc, sorc = pc.run_both("vector", caps, coef, ts, [(n, p) for _, p, names in sets + [pc.INDEX_SET] for n in names],
                            [(n, p) for _, p, names in ssets for n in names])
    orc.update(base)
    sorc.update(sbase)
    return {"caps": caps, "coef": coef, "ts": ts, "sets": {name: (p, names) for name, p, names in sets},
            "ssets": {name: (p, names) for name, p, names in ssets}, "orc": orc, "sorc": sorc}


def by_length(caps, names):
    """[(names, stacked captures)] per capture length, at most 8 captures a call"""
    groups = {}
    for n in names:
        groups.setdefault(len(caps[n]), []).append(n)
    out = []
    for ns in groups.values():
        for i in range(0, len(ns), 8):
            out.append((ns[i:i + 8], np.stack([caps[n] for n in ns[i:i + 8]])))
    return out


def new_context(g, monkeypatch, env, params):
    """a context created under `env` (the switches are read when a context is created) with `params` set"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cx = g.Context(0)
    for k in env:
        monkeypatch.delenv(k)
    if params:
        cx.set_params(**params)
    return cx


def run_set(g, data, monkeypatch, params, names, env=None):
    """-> [(names, calibrate_batch output, last_batch_details)] per length, each call on a context of its own"""
    res = []
    for ns, raw in by_length(data["caps"], names):
        cx = new_context(g, monkeypatch, env or {}, params)
        try:
            out = g.calibrate_batch(raw, data["coef"], data["ts"], FC, ctx=cx)
            det = g.last_batch_details(len(raw), ctx=cx)
        finally:
            cx.close()
        res.append((ns, out, det))
    return res


def check_rows(data, params, res, what):
    bad = []
    for ns, out, det in res:
        for i, n in enumerate(ns):
            orc, err = data["orc"][(n, pc.key(params))]
            row = out["table"][i]
            print(f"{what} {n}: gpu status {row[9]:.0f} n_fcch {row[6]:.0f} rows {row[7]:.0f} | oracle "
                  + (f"{orc['status']} {orc['n_fcch']} {orc['n_pos_rows']}" if orc else f"index error ({err})"))
            try:
                if orc is None:
                    assert row[9] == g_E_INDEX, row[9]
                else:
                    parity.compare_stream(orc, row, det, i, out["pos_info"][i])
            except AssertionError as e:
                bad.append(f"{what}, capture {n}: {e}")
    assert not bad, "\n".join(bad)


g_E_INDEX = -5.0            # GSMCAL_E_INDEX

CHAIN_SETS = [name for name, p, _ in pc.SETS if "coarse_th_db" not in p] + ["gate-below", "gate-above"]


# ---- (a) min_hits, fine_max_ppm, sch_max_ppm, fine_gate_snr_db, post_min_bcch and the mixed set against the oracle -----------
@pytest.mark.parametrize("name", CHAIN_SETS)
def test_parameter_set_against_the_oracle(g, data, monkeypatch, name):
    params, names = data["sets"][name]
    res = run_set(g, data, monkeypatch, params, names)
    check_rows(data, params, res, name)
    if name.startswith("gate-"):
        st = {n: out["table"][i, 9] for ns, out, _ in res for i, n in enumerate(ns)}
        assert st[pc.GATE_CASE] == (0 if name == "gate-below" else 6), (name, st)


# ---- (b) the coarse threshold on every route through the detector -------------------------------------------------------------
COARSE_ENVS = [{"GSMCAL_SNR_FULL": "0"}, {"GSMCAL_SNR_SCREEN_DB": "-300"}, {"GSMCAL_SNR_SCREEN_DB": "30"}, {"GSMCAL_CERT": "0"},
               {"GSMCAL_SNR_FULL": "0", "GSMCAL_SNR_INLINE_MIN": "0"}]


def kernels_launched(g, data, monkeypatch, params, names, env):
    """{kernel: launches} of one profiled call under `env`: the switches do select other kernels"""
    (_, raw), = by_length(data["caps"], names)
    cx = new_context(g, monkeypatch, env, params)
    try:
        cx.profile_enable()
        g.calibrate_batch(raw, data["coef"], data["ts"], FC, ctx=cx)
        return {k: v[1] for k, v in cx.profile_get().items()}
    finally:
        cx.close()


@pytest.mark.parametrize("th", pc.COARSE_TH)
def test_coarse_threshold_on_every_detector_route(g, data, monkeypatch, th):
    """the table path (default), the inline detector, an unscreened table, a screening level above every threshold (the hop walk
    falls back to its own spectra), no certificate, own spectra: the default context's rows are the oracle's, every other
    context's table, pos_info and coarse positions are the default's bit for bit"""
    params, names = data["sets"][f"coarse_th_db={th:.0f}"]
    ref = run_set(g, data, monkeypatch, params, names)
    check_rows(data, params, ref, f"th={th}")
    if th == 7.0:
        launches = [kernels_launched(g, data, monkeypatch, params, names, env) for env in ({}, COARSE_ENVS[0], COARSE_ENVS[4])]
        print("kernels: default, inline detector, own spectra:", launches)
        assert launches[0] != launches[1] and launches[0] != launches[2] and launches[1] != launches[2], launches
    for env in COARSE_ENVS:
        res = run_set(g, data, monkeypatch, params, names, env=env)
        for (ns, a, da), (_, b, db) in zip(ref, res):
            same_answer(a, b)
            assert np.array_equal(da["counts"], db["counts"]), (env, da["counts"], db["counts"])
            for i in range(len(ns)):
                k = da["counts"][i, 0]
                assert np.array_equal(da["coarse_pos"][i, :k], db["coarse_pos"][i, :k]), (env, ns[i])
                assert np.allclose(da["coarse_snr"][i, :k], db["coarse_snr"][i, :k], rtol=0, atol=parity.SNR_ATOL), (env, ns[i])


def test_coarse_threshold_below_the_seed_of_the_moving_average(g, data, monkeypatch):
    """coarse_th_db = -2000: 999 dB of seed no longer keep window 1 from hitting, the fine stage is handed a position inside the
    first 64 symbols: MATLAB stops with an index error (the oracle raises), the table says GSMCAL_E_INDEX"""
    _, params, names = pc.INDEX_SET
    assert data["orc"][(names[0], pc.key(params))][0] is None
    res = run_set(g, data, monkeypatch, params, names)
    check_rows(data, params, res, "th=-2000")
    _, out, det = res[0]
    assert out["table"][0, 9] == g_E_INDEX and det["coarse_pos"][0, 0] == 1.0


# ---- (c) the scanner's rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.SCAN_SET_NAMES)
def test_scanner_rule_against_the_oracle(g, data, monkeypatch, name):
    params, names = data["ssets"][name]
    for ns, raw in by_length(data["caps"], names):
        cx = new_context(g, monkeypatch, {}, params)
        try:
            out = g.fcch_scan_batch(raw, data["coef"], ctx=cx)
        finally:
            cx.close()
        for i, n in enumerate(ns):
            live = data["sorc"][(n, pc.key(params))]
            k = out["counts"][i]
            print(f"{name} {n}: gpu snr {out['snr'][i]:.6f} num_hit {out['num_hit'][i]:.0f} | oracle {live['snr']:.6f} {live['num_hit']:.0f}")
            assert live["num_hit"] == out["num_hit"][i], (name, n, live["num_hit"], out["num_hit"][i])
            assert abs(live["snr"] - out["snr"][i]) < parity.SNR_ATOL, (name, n, live["snr"], out["snr"][i])
            if live["coarse_pos"][0] == -1.0:
                assert k == 0 and out["positions"][i, 0] == -1.0, (name, n)
            else:
                parity.assert_positions(out["positions"][i, :k], live["coarse_pos"], f"scan positions ({name}, {n})")
                assert np.allclose(out["pos_snr"][i, :k], live["coarse_snr"], rtol=0, atol=parity.SNR_ATOL), (name, n)


# ---- (d) both tails, both entry styles ----------------------------------------------------------------------------------------
def test_four_launch_tail_under_the_mixed_set(g, data, monkeypatch):
    params, names = data["sets"]["mixed"]
    ref = run_set(g, data, monkeypatch, params, names)
    res = run_set(g, data, monkeypatch, params, names, env={"GSMCAL_FUSE_POST": "0"})
    for (_, a, _), (_, b, _) in zip(ref, res):
        same_answer(a, b)


def chain(mod, r, ts, params=None, ctx=None):
    """the four MATLAB-signature calls of gsm_sync_demod.m:117-120 -> (outputs, reports or infos)"""
    if mod is o:
        i0, i1, i2, i3 = {}, {}, {}, {}
        pos, _ = o.FCCH_coarse_position(r[0::64], 8, i0, params)
        fp, r1, sp1, cp1 = o.FCCH_fine_correction(r, pos, 8, FC, i1, params)
        pi, r2, sp2 = o.SCH_corr_rate_correction(r1, fp, ts, 8, i2, params)
        r3, cp2 = o.carrier_correct_post_SCH(r2, pi, 8, FC, i3, params)
        return (pos, fp, r1, sp1, cp1, pi, r2, sp2, r3, cp2), [i0, i1, i2, i3]
    reps = []
    pos, _ = mod.FCCH_coarse_position(r[0::64], 8, ctx=ctx)
    reps.append(mod.last_call_report(ctx))
    fp, r1, sp1, cp1 = mod.FCCH_fine_correction(r, pos, 8, FC, ctx=ctx)
    reps.append(mod.last_call_report(ctx))
    pi, r2, sp2 = mod.SCH_corr_rate_correction(r1, fp, ts, 8, ctx=ctx)
    reps.append(mod.last_call_report(ctx))
    r3, cp2 = mod.carrier_correct_post_SCH(r2, pi, 8, FC, ctx=ctx)
    reps.append(mod.last_call_report(ctx))
    return (pos, fp, r1, sp1, cp1, pi, r2, sp2, r3, cp2), reps


def compare_chain(got, want, name):
    pos, fp, r1, sp1, cp1, pi, r2, sp2, r3, cp2 = got
    o_pos, o_fp, o_r1, o_sp1, o_cp1, o_pi, o_r2, o_sp2, o_r3, o_cp2 = want
    parity.assert_positions(pos, o_pos, f"{name}: coarse position")
    parity.assert_positions(fp, o_fp, f"{name}: FCCH_pos")
    assert np.ndim(fp) == np.ndim(o_fp), name
    parity.assert_positions(pi, o_pi, f"{name}: pos_info")
    for a, b, what in ((sp1, o_sp1, "sampling_ppm(1)"), (cp1, o_cp1, "carrier_ppm(1)"), (sp2, o_sp2, "sampling_ppm(2)"),
                       (cp2, o_cp2, "carrier_ppm(2)")):
        parity.assert_ppm(a, b, f"{name}: {what}")
    for a, b in ((r1, o_r1), (r2, o_r2), (r3, o_r3)):
        if isinstance(b, np.ndarray):
            stream_close(a, b)
        else:
            assert np.ndim(a) == 0 and a == -1.0 and b == -1.0, name


@pytest.mark.parametrize("cap", ["cut+1300", "sch3-30", "short410"])
def test_chain_function_by_function_under_the_mixed_set(g, data, monkeypatch, cap):
    """the four MATLAB-signature calls on a context with the mixed set: every stage output is the oracle's, and the exits taken
    differ from the default parameters' (cut+1300: four first-round positions now suffice; sch3-30: four BCCH rows no longer do;
    short410: a gap 410 short passes max_th = 411)"""
    r = o.front_end(data["caps"][cap], data["coef"])
    want, infos = chain(o, r, data["ts"], pc.MIXED)
    dflt, infos0 = chain(o, r, data["ts"])
    assert [i["exit"] for i in infos] != [i["exit"] for i in infos0], cap
    cx = new_context(g, monkeypatch, {}, pc.MIXED)
    try:
        got, reps = chain(g, r, data["ts"], ctx=cx)
    finally:
        cx.close()
    print(cap, [i["exit"] for i in infos0], "->", [i["exit"] for i in infos])
    compare_chain(got, want, cap)
    if infos[3]["exit"] == 11:
        assert "post SCH: Warning! The number of BCCH bursts is less than 4!" in reps[3].split("\n")


def test_spacing_exit_lines_follow_fine_max_ppm(g, data, monkeypatch):
    """FCCH_fine_correction.m:96-99 prints max_th and the per-gap distances; the library rebuilds those lines on the host from
    gsmcal_params.fine_max_ppm.  short410 under 4100 ppm: max_th = 410 / 451, the gap 410 short is counted out"""
    n2s = g.num2str
    params = {"fine_max_ppm": 4100.0}
    r = o.front_end(data["caps"]["short410"], data["coef"])
    want, infos = chain(o, r, data["ts"], params)
    assert [i["exit"] for i in infos][:2] == [0, 4]
    cx = new_context(g, monkeypatch, {}, params)
    try:
        got, reps = chain(g, r, data["ts"], ctx=cx)
    finally:
        cx.close()
    compare_chain(got, want, "short410 at 4100 ppm")
    d = np.diff(infos[1]["first_round_pos"])
    a, b = np.abs(d - 100000.0), np.abs(d - 110000.0)
    lines = [" ", f"FCCH fine: first round diff {n2s(d)}", "FCCH fine: Warning! Kinds of pos diff more than 2!",
             f"Expected len {n2s(len(d))}. Actual {n2s([np.sum(a < 410), np.sum(b < 451)])}",
             f"diff intra multiframe max th 410 actual {n2s(a)}", f"diff inter multiframe max th 451 actual {n2s(b)}", ""]
    assert np.sum(a < 410) + np.sum(b < 451) == len(d) - 1 and 410.0 in a
    assert reps[1].split("\n") == lines, (reps[1], lines)


def test_a_gap_in_both_spacing_classes_is_beyond_the_geometry(g, data, monkeypatch):
    """fine_max_ppm = 100000 with hand-given base positions (params_cases.BOTH_CLASSES): two gaps pass both class tests, two pass
    neither, the :95 count still fits, the reference would resample by e = 0.45 (both oracles: tests/test_params_cpu.py).  The
    tile and window buffers behind the resampling stages are sized for the reference's 4000 ppm: a stretch above 4400 ppm is
    answered with GSMCAL_E_UNSUPPORTED, decided from e before a sample is read (kernels_estim.h GSMCAL_MAX_STRETCH_FINE)"""
    sc_pos = data["orc"][("d0", pc.key({"min_hits": 9}))][0]["coarse_pos"]
    base = sc_pos[list(pc.BOTH_HITS)]
    r = o.front_end(data["caps"]["d0"], data["coef"])
    info = {}
    o_fp, o_r1, o_sp, o_cp = o.FCCH_fine_correction(r, base, 8, FC, info, pc.BOTH_CLASSES)
    assert info["exit"] == 0 and tuple(o_fp - o_fp[0]) == pc.BOTH_GRID, o_fp
    assert o_sp > 4400.0
    cx = new_context(g, monkeypatch, {}, pc.BOTH_CLASSES)
    try:
        with pytest.raises(g.GsmcalError, match="GSMCAL_E_UNSUPPORTED"):
            g.FCCH_fine_correction(r, base, 8, FC, ctx=cx)
        # the same context still serves: the same positions minus the twenty-frame gaps, inside the geometry
        fp, _, sp, _ = g.FCCH_fine_correction(r, sc_pos[:6], 8, FC, ctx=cx, want_r=False)
        want = o.FCCH_fine_correction(r, sc_pos[:6], 8, FC, None, pc.BOTH_CLASSES)
        parity.assert_positions(fp, want[0], "FCCH_pos")
        parity.assert_ppm(sp, want[2], "sampling_ppm")
    finally:
        cx.close()


def test_sch_stage_stretch_beyond_the_geometry(g, data, monkeypatch):
    """the same construction one stage on: FCCH positions 1, 2, 4, 6, 7 of d0 under sch_max_ppm = 100000 -- the SCH stage's
    first-round gaps are 10, 20, 21 and 10 frames, the :106 count fits, the reference resamples by e = 0.43; above 440 ppm the
    stage answers GSMCAL_E_UNSUPPORTED (kernels_estim.h GSMCAL_MAX_STRETCH_SCH).  All ten positions: the oracle's row"""
    params = {"sch_max_ppm": 100000.0}
    r = o.front_end(data["caps"]["d0"], data["coef"])
    pos, _ = o.FCCH_coarse_position(r[0::64], 8)
    fp, r1, _, _ = o.FCCH_fine_correction(r, pos, 8, FC)
    assert len(fp) == 10
    info = {}
    o_pi, _, o_sp = o.SCH_corr_rate_correction(r1, fp[list(pc.BOTH_HITS)], data["ts"], 8, info, params)
    assert info["exit"] == 0 and o_sp > 4e5 and [int(round(x / 10000.0)) for x in info["first_round_diff"]] == [10, 20, 21, 10], (info, o_sp)
    cx = new_context(g, monkeypatch, {}, params)
    try:
        with pytest.raises(g.GsmcalError, match="GSMCAL_E_UNSUPPORTED"):
            g.SCH_corr_rate_correction(r1, fp[list(pc.BOTH_HITS)], data["ts"], 8, ctx=cx)
        pi, _, sp = g.SCH_corr_rate_correction(r1, fp, data["ts"], 8, ctx=cx, want_r=False)
        want = o.SCH_corr_rate_correction(r1, fp, data["ts"], 8, None, params)
        parity.assert_positions(pi, want[0], "pos_info")
        parity.assert_ppm(sp, want[2], "sampling_ppm")
    finally:
        cx.close()


# ---- (e) no stale parameters ----------------------------------------------------------------------------------------------------
STALE_CASES = ["short410", "plain+62000", "noise", "sch3-th39"]
STALE_PARAMS = {"fine_max_ppm": 4110.0, "sch_max_ppm": 390.0}


def oracle_tables_differ(data):
    a = [data["orc"][(n, ())][0]["status"] for n in STALE_CASES]
    b = [data["orc"][(n, pc.key(STALE_PARAMS))][0]["status"] for n in STALE_CASES]
    assert a != b and any(x == y for x, y in zip(a, b)), (a, b)


def check_table(data, params, out, det):
    for i, n in enumerate(STALE_CASES):
        parity.compare_stream(data["orc"][(n, pc.key(params))][0], out["table"][i], det, i, out["pos_info"][i])


@pytest.mark.parametrize("graph", [None, "2"], ids=["graph-default", "GRAPH=2"])
def test_set_params_between_calls_on_the_same_buffers(g, data, monkeypatch, graph):
    """calibrate_batch_dev into the SAME device buffers, graph capture at its default setting and with GSMCAL_GRAPH=2 (which
    captures one-lane plans as well: eager, capture + replay, replay): three calls, set_params, one call -- the new parameters'
    table, not a replay of the old graph (its key carries params_epoch) --, the defaults again, one call -- the first table bit
    for bit"""
    if graph:
        monkeypatch.setenv("GSMCAL_GRAPH", graph)
    import torch
    oracle_tables_differ(data)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    raw = np.stack([data["caps"][n] for n in STALE_CASES])
    d, n = raw.shape[0], raw.shape[1] // 2
    with torch.cuda.stream(st):
        cx = g.Context(0, stream=st.cuda_stream)
        monkeypatch.delenv("GSMCAL_GRAPH", raising=False)
        try:
            raw_t = torch.from_numpy(raw).to(dev)
            tab = torch.zeros((d, g.TABLE_COLS), dtype=torch.float64, device=dev)
            pos = torch.zeros((d, 2, g.MAX_POS_ROWS), dtype=torch.float64, device=dev)
            rl = torch.zeros((d,), dtype=torch.int64, device=dev)
            st.synchronize()

            def call():
                g.calibrate_batch_dev(raw_t.data_ptr(), d, n, data["coef"], data["ts"], FC, tab.data_ptr(), pos.data_ptr(), None,
                                      rl.data_ptr(), ctx=cx)
                cx.sync()
                return as_out(tab, pos, rl, None), g.last_batch_details(d, ctx=cx)
            first = [call() for _ in range(3)]
            for out, _ in first[1:]:
                same_answer(first[0][0], out)
            check_table(data, None, *first[2])
            cx.set_params(**STALE_PARAMS)
            moved = call()
            check_table(data, STALE_PARAMS, *moved)
            assert not np.array_equal(moved[0]["table"][:, 9], first[0][0]["table"][:, 9])
            again = call()
            same_answer(moved[0], again[0])
            cx.set_params(**{k: o.PARAM_DEFAULTS[k] for k in STALE_PARAMS})
            back = call()
            same_answer(first[0][0], back[0])
            assert np.array_equal(first[0][0]["r_len"], back[0]["r_len"])
        finally:
            cx.close()


def test_set_params_behind_a_call_in_flight(g, data):
    """pipeline depth 2: call A, set_params, call B into buffers of their own; after sync A holds the old parameters' table and
    B the new one"""
    import torch
    oracle_tables_differ(data)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    raw = np.stack([data["caps"][n] for n in STALE_CASES])
    with torch.cuda.stream(st):
        cx = g.Context(0, stream=st.cuda_stream)
        try:
            raw_t = torch.from_numpy(raw).to(dev)
            st.synchronize()
            cx.set_pipeline_depth(2)
            a = dev_call(g, cx, raw_t, data["coef"], data["ts"], with_r=False)
            cx.set_params(**STALE_PARAMS)
            b = dev_call(g, cx, raw_t, data["coef"], data["ts"], with_r=False)
            cx.sync()
            det_b = g.last_batch_details(len(raw), ctx=cx)
            out_a, out_b = as_out(*a), as_out(*b)
            check_table(data, STALE_PARAMS, out_b, det_b)
            # (the details describe the most recent call: A's rows against the oracle's table columns and pos_info)
            for i, n in enumerate(STALE_CASES):
                orc = data["orc"][(n, ())][0]
                row = out_a["table"][i]
                for c, want in enumerate(list(orc["sampling_ppm"]) + list(orc["carrier_ppm"]) + [orc["total_sampling_ppm"], orc["total_carrier_ppm"]]):
                    parity.assert_ppm(row[c], want, f"call A, {n}, column {c}")
                assert [float(v) for v in row[6:10]] == [float(orc["n_fcch"]), float(orc["n_pos_rows"]), float(orc["first_fcch_pos"]),
                                                         float(orc["status"])], (n, row[6:10])
                if not np.all(orc["pos_info"] == -1):
                    parity.assert_positions(out_a["pos_info"][i], orc["pos_info"], f"call A, {n}: pos_info")
            assert not np.array_equal(out_a["table"][:, 9], out_b["table"][:, 9])
        finally:
            cx.close()


# ---- (f) the contract of set_params --------------------------------------------------------------------------------------------
def params_tuple(p):
    return tuple(getattr(p, k) for k, _ in p._fields_)


def test_set_params_refuses_and_keeps_what_it_had(g, data):
    """out-of-range counts and NaN thresholds: GSMCAL_E_ARG; a geometry field off its default: GSMCAL_E_UNSUPPORTED; after every
    refusal get_params() returns the previous values and a batch call the previous table"""
    raw = np.stack([data["caps"][n] for n in ("short410", "noise")])
    cx = g.Context(0)
    try:
        cx.set_params(fine_max_ppm=4110.0, min_hits=4, scan_min_hits=1, post_min_bcch=0)       # (the ends of the ranges are accepted)
        cx.set_params(min_hits=2)
        cx.set_params(min_hits=g.MAX_HITS)
        cx.set_params(min_hits=4, coarse_th_db=math.inf)
        cx.set_params(coarse_th_db=10.0)
        prev = params_tuple(cx.get_params())
        ref = g.calibrate_batch(raw, data["coef"], data["ts"], FC, ctx=cx)
        assert ref["table"][0, 9] == 6                                                         # (4110 ppm: not the default's 4)
        arg, geo = "GSMCAL_E_ARG", "GSMCAL_E_UNSUPPORTED"
        bad = [({"min_hits": 1}, arg), ({"min_hits": g.MAX_HITS + 1}, arg), ({"scan_min_hits": 0}, arg), ({"post_min_bcch": -1}, arg)]
        bad += [({k: float("nan")}, arg) for k in pc.TUNABLE if isinstance(o.PARAM_DEFAULTS[k], float)]
        bad += [({k: type(v)(v + 1)}, geo) for k, v in pc.GEOMETRY.items()] + [({"fine_max_offset": 32}, geo)]
        assert len(bad) == 4 + 7 + 6
        for kw, code in bad:
            with pytest.raises(g.GsmcalError, match=code):
                cx.set_params(**kw)
            assert params_tuple(cx.get_params()) == prev, kw
            out = g.calibrate_batch(raw, data["coef"], data["ts"], FC, ctx=cx)
            assert np.array_equal(out["table"], ref["table"], equal_nan=True), kw
        with pytest.raises(AttributeError):
            cx.set_params(no_such_field=1)
    finally:
        cx.close()
