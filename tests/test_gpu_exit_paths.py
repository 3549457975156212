"""GPU tests (-m gpu) of the batch chain's early exits and end-of-capture branches, from raw bytes and with the default
thresholds: the cases of tests/exit_paths.py (tests/test_exit_paths_cpu.py holds them to their designed exits with the oracle
alone) in ONE batch whose neighbouring streams leave at different stages, against the live oracle -- the status column and
the counts of columns 6..8 included (parity.compare_stream) --, each case alone, every route through the tail bit for bit,
the chain function by function with the warnings of the exits, and the scanner's hop walk at the cut ends.
Bars as everywhere (tests/parity.py, test_gpu_general_taps.py): positions bit-exact, ppm 1e-6 relative + 1e-9, corrected
streams 2e-8 of their peak."""
import math

import numpy as np
import pytest

import exit_paths as ep
import parity
from oracle import gsmcal_oracle as o
from test_gpu_general_taps import context_under, launches, same_answer, stream_close

pytestmark = pytest.mark.gpu

FC = ep.FC


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


@pytest.fixture(scope="module")
def built():
    """the cases with their oracle results (corrected stream included), the mixed batch ordered so that neighbours leave at
    different stages"""
    n_mixed, cases = ep.build()
    coef, ts = ep.coef(), ep.synth.sch_training_sequence()
    orcs = parity.pool_map(ep.oracle_job_r, [(k["raw"], coef, ts, FC) for k in cases], max_workers=16)
    for k, (orc, err) in zip(cases, orcs):
        assert orc is not None and orc["status"] == k["status"], (k["name"], err)
        k["orc"] = orc
    rest = [k for k in cases if k["group"] == "mixed"]
    mixed = []
    while rest:                                  # greedy: the most frequent status left that is not the last one's
        last = mixed[-1]["status"] if mixed else None
        count = {}
        for k in rest:
            count[k["status"]] = count.get(k["status"], 0) + 1
        pick = max((st for st in count if st != last), key=lambda st: count[st], default=last)
        nxt = next(k for k in rest if k["status"] == pick)
        rest.remove(nxt)
        mixed.append(nxt)
    print("mixed batch:", [(k["name"], k["status"]) for k in mixed])
    return {"n": n_mixed, "mixed": mixed, "own": [k for k in cases if k["group"] == "own"], "coef": coef, "ts": ts,
            "raw": np.stack([k["raw"] for k in mixed])}


def dev_call(g, cx, raw_t, coef, ts, with_r=True):
    """one gsmcal_calibrate_batch_dev call into fresh outputs; r_correct pre-filled with NaN"""
    import torch
    d, n = raw_t.shape[0], raw_t.shape[1] // 2
    dev = raw_t.device
    tab = torch.zeros((d, g.TABLE_COLS), dtype=torch.float64, device=dev)
    pos = torch.zeros((d, 2, g.MAX_POS_ROWS), dtype=torch.float64, device=dev)
    rl = torch.zeros((d,), dtype=torch.int64, device=dev)
    rc = torch.full((d, n, 2), float("nan"), dtype=torch.float64, device=dev) if with_r else None
    g.calibrate_batch_dev(raw_t.data_ptr(), d, n, coef, ts, FC, tab.data_ptr(), pos.data_ptr(),
                          rc.data_ptr() if with_r else None, rl.data_ptr(), ctx=cx)
    return tab, pos, rl, rc


def as_out(tab, pos, rl, rc):
    """device outputs -> the dict g.calibrate_batch returns (r_correct keeps the NaN pre-fill behind r_len)"""
    table, p = tab.cpu().numpy(), pos.cpu().numpy()
    rows = []
    for i in range(len(table)):
        k = int(table[i, 7])
        rows.append(-np.ones((k, 2)) if table[i, 8] == -1.0 else p[i, :, :k].T.copy())
    r = None
    if rc is not None:
        r = rc.cpu().numpy()
        r = r[..., 0] + 1j * r[..., 1]
    return {"table": table, "pos_info": rows, "pos_info_raw": p, "r_len": rl.cpu().numpy(), "r_correct": r}


def run_dev(g, raw, coef, ts, env=None, calls=1, depth=1, with_r=True, profile=False):
    """`calls` device-pointer calls on a fresh context on a torch stream -> (list of outputs, details of the last call, profile)"""
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        cx = context_under(g, env or {}, stream=st.cuda_stream)
        try:
            if profile:
                cx.profile_enable()
            raw_t = torch.from_numpy(raw).to(dev)
            st.synchronize()
            if depth > 1:
                cx.set_pipeline_depth(depth)
            outs = [dev_call(g, cx, raw_t, coef, ts, with_r) for _ in range(calls)]
            cx.sync()
            det = g.last_batch_details(len(raw), ctx=cx)
            names = {k: v[1] for k, v in cx.profile_get().items()} if profile else None
            res = [as_out(*x) for x in outs]
        finally:
            cx.close()
    return res, det, names


def same_all(ref, out, what=""):
    """table, pos_info, r_len and every sample of r_correct (NaN pre-fill included) bit for bit"""
    same_answer(ref, out)
    assert np.array_equal(ref["r_len"], out["r_len"]), what
    if ref["r_correct"] is not None and out["r_correct"] is not None:
        assert np.array_equal(ref["r_correct"], out["r_correct"], equal_nan=True), what


def check_against_oracle(cases, out, det):
    """every row through parity.compare_stream (columns 6..9 included); r_len exact; r_correct within the stream bar where the
    reference returns a stream and untouched (still NaN) where it returns -1; behind r_len nothing is written either"""
    for i, k in enumerate(cases):
        orc, row = k["orc"], out["table"][i]
        print(f"{k['name']}: gpu status {row[9]:.0f} n_fcch {row[6]:.0f} rows {row[7]:.0f} first {row[8]:.0f} | oracle {orc['status']} "
              f"{orc['n_fcch']} {orc['n_pos_rows']} {orc['first_fcch_pos']:.0f} r_len {out['r_len'][i]} / {orc['r_len']}")
    bad = []
    for i, k in enumerate(cases):                                # (every case is looked at: the message names all that fail)
        orc = k["orc"]
        try:
            parity.compare_stream(orc, out["table"][i], det, i, out["pos_info"][i])
            assert out["table"][i, 9] == k["status"], out["table"][i, 9]
            assert out["r_len"][i] == orc["r_len"], (out["r_len"][i], orc["r_len"])
            r = out["r_correct"][i]
            if orc["r_len"] > 0:
                L = orc["r_len"]
                stream_close(r[:L], orc["r_correct"])
                assert np.all(np.isnan(r[L:])), "samples written behind r_len"
            else:
                assert np.all(np.isnan(r)), "the reference returns r = -1, yet the slice of this stream was written to"
        except AssertionError as e:
            bad.append(f"case {k['name']} (stream {i}): {e}")
    assert not bad, "\n".join(bad)


@pytest.fixture(scope="module")
def mixed_ref(g, built):
    """the mixed batch on a fresh profiled context (device-pointer call, NaN pre-fill): (output, details, kernel launches)"""
    res, det, names = run_dev(g, built["raw"], built["coef"], built["ts"], profile=True)
    print("mixed batch kernels:", sorted(names.items()))
    return res[0], det, names


# ---- (a) one mixed batch against the oracle -------------------------------------------------------------------------------
def test_mixed_batch_against_the_oracle(built, mixed_ref):
    out, det, names = mixed_ref
    check_against_oracle(built["mixed"], out, det)
    st = [k["status"] for k in built["mixed"]]
    assert set(st) >= {0, 1, 2, 3, 4, 6, 7, 8, 9, 11}
    assert all(a != b for a, b in zip(st, st[1:])), f"neighbouring streams should leave at different stages: {st}"
    # the default route: the fused tail with the reference geometry compiled in
    assert [k for k in names if "k_post_chain_r" in k] == ["(k_post_chain_r<8, 512, 47>)"], names
    assert launches(names, "k_burst_tone") == 0 and launches(names, "k_window_sch") == 0, names


def test_host_pointer_call_gives_the_same_batch(g, built, mixed_ref):
    out = g.calibrate_batch(built["raw"], built["coef"], built["ts"], FC, want_r=True)
    ref = mixed_ref[0]
    same_answer(ref, out)
    assert np.array_equal(ref["r_len"], out["r_len"])
    for i, L in enumerate(ref["r_len"]):
        if L > 0:
            assert np.array_equal(ref["r_correct"][i, :L], out["r_correct"][i, :L]), i


# ---- (b) the cut lengths of their own, one call per length ----------------------------------------------------------------
def test_other_cut_lengths_against_the_oracle(g, built):
    assert any(len(k["raw"]) % 16 for k in built["own"])
    for k in built["own"]:
        res, det, _ = run_dev(g, k["raw"][None, :], built["coef"], built["ts"])
        check_against_oracle([k], res[0], det)


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


# ---- (d) every route through the tail, bit for bit ------------------------------------------------------------------------
def assert_several_lanes(names):
    """a call split over lanes never takes the fused tail (host_plan.h: n_lanes_used == 1): every lane launches the four-launch
    tail of its own -- two k_burst_tone and one k_window_sch per lane"""
    assert launches(names, "k_post_chain_r") == 0, names
    n_lanes = launches(names, "k_window_sch")
    assert n_lanes >= 2 and launches(names, "k_burst_tone") == 2 * n_lanes, names


ROUTES = [{"GSMCAL_FUSE_POST": "0"}, {"GSMCAL_CERT": "0"}, {"GSMCAL_LANES": "4", "GSMCAL_LANE_MIN": "2"}, {"GSMCAL_POST_SLOTS": "2"}]


@pytest.mark.parametrize("env", ROUTES, ids=lambda e: ",".join(f"{k[7:]}={v}" for k, v in e.items()))
def test_routes_agree(g, built, mixed_ref, env):
    four_launch = env == {"GSMCAL_FUSE_POST": "0"}
    lanes = "GSMCAL_LANES" in env
    res, _, names = run_dev(g, built["raw"], built["coef"], built["ts"], env=env, profile=four_launch or lanes)
    same_all(mixed_ref[0], res[0], str(env))
    if lanes:
        print("four-lane kernels:", sorted(names.items()))
        assert_several_lanes(names)
    if four_launch:
        print("four-launch tail kernels:", sorted(names.items()))
        for want in ("(k_burst_tone<1, 8, 47>)", "(k_window_sch<8, 512, 47>)", "(k_burst_tone<0, 8, 47>)"):
            assert names.get(want) == 1, (want, names)
        assert launches(names, "k_post_chain_r") == 0 and launches(names, "k_burst_tone") == 2, names


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


def test_pipelined_calls_agree(g, built, mixed_ref):
    """six device-pointer calls three deep, each into its own outputs"""
    res, _, _ = run_dev(g, built["raw"], built["coef"], built["ts"], calls=6, depth=3)
    for k, out in enumerate(res):
        same_all(mixed_ref[0], out, f"call {k}")


def test_tiled_past_one_lane_agrees(g, built, mixed_ref):
    """the mixed batch tiled to more than 128 streams: it leaves the one-lane path"""
    reps = -(-129 // len(built["raw"]))
    raw = np.concatenate([built["raw"]] * reps)
    assert len(raw) > 128
    res, _, names = run_dev(g, raw, built["coef"], built["ts"], with_r=False, profile=True)
    print("tiled batch kernels:", sorted(names.items()))
    assert_several_lanes(names)
    out, ref = res[0], mixed_ref[0]
    d = len(built["raw"])
    for t in range(reps):
        assert np.array_equal(out["table"][t * d:(t + 1) * d], ref["table"], equal_nan=True), t
        assert np.array_equal(out["r_len"][t * d:(t + 1) * d], ref["r_len"]), t
        assert all(np.array_equal(a, b) for a, b in zip(out["pos_info"][t * d:(t + 1) * d], ref["pos_info"])), t


# ---- (e) function by function ----------------------------------------------------------------------------------------------
WARN = {(0, 1): "FCCH coarse: No FCCH found!",
        (1, 2): "FCCH fine: Warning! Length of hits is smaller than 5!", (1, 4): "FCCH fine: Warning! Kinds of pos diff more than 2!",
        (1, 6): "FCCH fine: Warning! Some FCCH SNR seems pretty low!",
        (2, 2): "SCH: Warning! Length of hits is smaller than 5!", (2, 7): "SCH:  Warning! No peak around base position is found!",
        (2, 9): "SCH: Warning! Kinds of pos diff more than 2!",
        (3, 10): "post SCH: Warning! No valid position information!",
        (3, 11): "post SCH: Warning! The number of BCCH bursts is less than 4!"}


def test_chain_function_by_function_at_every_exit(g, built):
    """test_gpu_parity.py's test_chain_function_by_function sequence on one case per status: sentinel shapes, r = s at the
    spacing exits and -1 at the others, and the warning line of every exit abi_report.h has text for"""
    ts, coef = built["ts"], built["coef"]
    subset, seen_warn = {}, set()
    for k in built["mixed"] + built["own"]:
        subset.setdefault(k["status"], k)
    assert set(subset) >= {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11}
    for status, k in sorted(subset.items()):
        r = o.matlab_filter(coef, o.raw2iq(k["raw"]))
        i0, i1, i2, i3 = {}, {}, {}, {}
        o_pos, _ = o.FCCH_coarse_position(r[0::64], 8, i0)
        o_fp, o_r1, o_sp1, o_cp1 = o.FCCH_fine_correction(r, o_pos, 8, FC, i1)
        o_pi, o_r2, o_sp2 = o.SCH_corr_rate_correction(o_r1, o_fp, ts, 8, i2)
        o_r3, o_cp2 = o.carrier_correct_post_SCH(o_r2, o_pi, 8, FC, i3)
        exits = [i0["exit"], i1["exit"], i2["exit"], i3["exit"]]
        assert next((c for c in exits if c), 0) == status, (k["name"], exits)
        reps = []
        pos, _ = g.FCCH_coarse_position(r[0::64], 8)
        reps.append(g.last_call_report())
        fp, r1, sp1, cp1 = g.FCCH_fine_correction(r, pos, 8, FC)
        reps.append(g.last_call_report())
        pi, r2, sp2 = g.SCH_corr_rate_correction(r1, fp, ts, 8)
        reps.append(g.last_call_report())
        r3, cp2 = g.carrier_correct_post_SCH(r2, pi, 8, FC)
        reps.append(g.last_call_report())
        name = k["name"]
        parity.assert_positions(pos, o_pos, f"{name}: coarse position")
        parity.assert_positions(fp, o_fp, f"{name}: FCCH_pos")                # (the -1 sentinel included)
        assert np.ndim(fp) == np.ndim(o_fp), name
        parity.assert_ppm(sp1, o_sp1, f"{name}: sampling_ppm(1)")
        parity.assert_ppm(cp1, o_cp1, f"{name}: carrier_ppm(1)")
        parity.assert_positions(pi, o_pi, f"{name}: pos_info")                # ([-1 -1] or -ones(3K, 2): same shape)
        parity.assert_ppm(sp2, o_sp2, f"{name}: sampling_ppm(2)")
        parity.assert_ppm(cp2, o_cp2, f"{name}: carrier_ppm(2)")
        for got, want in ((r1, o_r1), (r2, o_r2), (r3, o_r3)):
            if isinstance(want, np.ndarray):
                stream_close(got, want)
            else:
                assert np.ndim(got) == 0 and got == -1.0 and want == -1.0, name
        if exits[1] == 5:
            # FCCH_fine_correction.m:135-142: the last burst dropped, four left: the positions and the resampled stream come
            # back, the carrier block is skipped
            assert np.shape(fp) == (4,) and isinstance(r1, np.ndarray) and len(r1) == len(o_r1) == len(r), name
            assert math.isfinite(sp1) and math.isfinite(o_sp1) and cp1 == math.inf and o_cp1 == math.inf, (name, sp1, cp1)
            assert any(line.startswith("FCCH fine: sampling error ppm") for line in reps[1].split("\n")), reps[1]
            assert "FCCH freq" not in reps[1] and "carrier error" not in reps[1], reps[1]
        if exits[1] == 4:
            assert isinstance(r1, np.ndarray) and len(r1) == len(r), "FCCH_fine_correction.m:72,95: r = s at the spacing exit"
        if exits[2] == 9:
            assert isinstance(r2, np.ndarray) and len(r2) == len(o_r1), "SCH_corr_rate_correction.m:87,106: r = s at the spacing exit"
        for stage, code in enumerate(exits):
            line = WARN.get((stage, code))
            if line is not None:
                assert line in reps[stage].split("\n"), (name, stage, code, reps[stage])
                seen_warn.add((stage, code))
            elif code == 0:
                assert "Warning" not in reps[stage], (name, stage, reps[stage])
    assert seen_warn == set(WARN), f"every warning abi_report.h has text for should have been met: missing {set(WARN) - seen_warn}"


# ---- (f) the scanner's hop walk at the cut ends ---------------------------------------------------------------------------
def test_scanner_on_the_cut_captures(g, built):
    """FCCH_coarse_position.m:49 / :67: the hop walk stops where the next window would leave the capture"""
    coef = built["coef"]
    cases = built["mixed"] + built["own"]
    lives = parity.pool_map(ep.scan_job, [(k["raw"], coef) for k in cases], max_workers=16)
    outs = [g.fcch_scan_batch(built["raw"], coef)] + [g.fcch_scan_batch(k["raw"][None, :], coef) for k in built["own"]]
    for j, (k, live) in enumerate(zip(cases, lives)):
        out, i = (outs[0], j) if j < len(built["mixed"]) else (outs[1 + j - len(built["mixed"])], 0)
        n = out["counts"][i]
        assert live["num_hit"] == out["num_hit"][i], (k["name"], live["num_hit"], out["num_hit"][i])
        assert abs(live["snr"] - out["snr"][i]) < parity.SNR_ATOL, k["name"]
        if live["coarse_pos"][0] == -1.0:
            assert n == 0 and out["positions"][i, 0] == -1.0, k["name"]
        else:
            parity.assert_positions(out["positions"][i, :n], live["coarse_pos"], f"scan positions ({k['name']})")
            assert np.allclose(out["pos_snr"][i, :n], live["coarse_snr"], rtol=0, atol=parity.SNR_ATOL), k["name"]
    counts = {len(live["coarse_pos"]) for live in lives if live["coarse_pos"][0] != -1.0}
    assert {3, 4, 5} <= counts and max(counts) >= 9, f"walks of three, four, five and nine or more hits: {counts}"
