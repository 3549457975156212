"""GPU tests (-m gpu) of the batch chain with channel filters other than the drivers' 47 mirrored taps: the any-geometry
instantiations behind gsmcal_calibrate_batch -- k_post_chain_r<0, 0, 0>, k_burst_tone<., 0, 0>, k_window_sch<0, 0, 0>,
k_fine_cert<0, 0> building its windows from the raw bytes, k_stream_tile<0>, the k_gather routes for filters too long for
a staging pass / a stream tile -- and the non-mirrored branches of the 47-tap ones, on raw bytes, against the live oracle.
The filters and streams are tests/general_taps.py's; tests/test_general_taps_cpu.py shows with the oracle alone that the
ramp filters tell a reversed tap order apart at these bars.  Bars as everywhere (tests/parity.py, test_gpu_parity.py):
positions bit-exact, ppm 1e-6 relative + 1e-9, SNRs 1e-8 dB, corrected streams 2e-8 of their peak (the derotation
argument behind that bar does not involve the tap count)."""
import os

import numpy as np
import pytest

import general_taps as gt
import parity
from oracle import gsmcal_oracle as o

pytestmark = pytest.mark.gpu

FC = gt.FC
STREAM_RTOL = 2e-8
# (filter, unaligned cut), by increasing tap count; the cut sends 31 and 47 taps to k_front_fused and starts streams off a
# 16-byte boundary
CASES = [(name, False) for name in gt.FILTERS] + [(name, True) for name in ("fir31", "ramp47", "ramp66")]
CASES.sort(key=lambda c: (len(gt.FILTERS[c[0]]), list(gt.FILTERS).index(c[0]), c[1]))
CASE_IDS = [f"{n}-unaligned" if u else n for n, u in CASES]
TAIL_KERNELS = ("k_post_chain_r", "k_burst_tone", "k_window_sch")


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


@pytest.fixture(scope="module")
def streams():
    return gt.make_streams()


@pytest.fixture(scope="module")
def ts():
    return gt.synth.sch_training_sequence()


def stream_close(a, b):
    assert isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape, (np.shape(a), np.shape(b))
    scale = np.max(np.abs(b))
    err = np.max(np.abs(a - b))
    print(f"   r_correct: max abs err / peak {err / scale:.3e}")
    assert err <= STREAM_RTOL * scale, f"stream mismatch: max abs err {err} at scale {scale}"


@pytest.fixture(scope="module")
def profiled(g, streams, ts):
    """(filter, unaligned) -> (calibrate_batch output with r_correct, last_batch_details, {kernel name: launches}) of ONE call on
    a fresh context with the per-kernel profile on; computed once per case.  (A profile does not change the plan of a
    one-lane call at pipeline depth 1 -- it only keeps a call out of graph capture and out of the pipeline, host_plan.h
    run_maybe_graph / abi_calls.h gsmcal_calibrate_batch_dev; test_variants_agree compares these very tables bit for bit
    with an unprofiled context's.)"""
    cache = {}

    def run(name, unaligned):
        if (name, unaligned) not in cache:
            raw = gt.cut(streams, unaligned)
            cx = g.Context(0)
            try:
                cx.profile_enable()
                out = g.calibrate_batch(raw, gt.FILTERS[name], ts, FC, want_r=True, ctx=cx)
                det = g.last_batch_details(len(raw), ctx=cx)
                names = {k: v[1] for k, v in cx.profile_get().items()}
            finally:
                cx.close()
            print(name, "unaligned" if unaligned else "aligned", "kernels:", sorted(names.items()))
            cache[(name, unaligned)] = (out, det, names)
        return cache[(name, unaligned)]
    return run


def launches(names, part):
    return sum(n for k, n in names.items() if part in k)


# ---- (a) every row against the live oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,unaligned", CASES, ids=CASE_IDS)
def test_batch_chain_against_the_oracle(g, streams, ts, profiled, name, unaligned):
    """Every row through parity.compare_stream, every corrected stream within 2e-8 of its peak.  (The one-tap case is the
    one that found the contracted interpolation weight -- chain_ops.h lerp_pos: on unfiltered samples an ulp of the
    query position k*(1+e) moved the tone estimate by 2e-11 ppm and the end of r_correct by 4.3e-8 of its peak.)"""
    raw = gt.cut(streams, unaligned)
    coef = gt.FILTERS[name]
    out, det, _ = profiled(name, unaligned)
    assert np.all(out["table"][:, 9] >= 0), out["table"][:, 9]             # no error status: every tap count here is served
    orcs = parity.pool_map(gt.oracle_job_r, [(raw[i], coef, ts, FC) for i in range(len(raw))], max_workers=16)
    n_r = 0
    for i, orc in enumerate(orcs):
        parity.compare_stream(orc, out["table"][i], det, i, out["pos_info"][i])
        if isinstance(orc.get("r_correct"), np.ndarray):
            n_r += 1
            L = int(out["r_len"][i])
            assert L == len(orc["r_correct"]), (i, L, len(orc["r_correct"]))
            stream_close(out["r_correct"][i, :L], orc["r_correct"])
        else:
            assert out["r_len"][i] == -1, i
    assert n_r >= 4, "the set should hold at least four streams the reference algorithm calibrates"
    assert n_r < len(raw), "... and at least one it does not (sentinel rows)"


# ---- (b) ... and on the kernels the case is there for --------------------------------------------------------------------
@pytest.mark.parametrize("name,unaligned", CASES, ids=CASE_IDS)
def test_the_general_geometry_kernels_ran(profiled, name, unaligned):
    """What a 6-stream call launches, by tap count (host_plan.h run_fine / front_fused, abi_calls.h launch_r_correct):
       tail          47 taps: k_post_chain_r<8, 512, 47>; any other count: k_post_chain_r<0, 0, 0> (one lane, 48 workgroups: fused)
       fine windows  up to 436 taps a staging pass of k_fine_cert fits the LDS its later phases use (17 904 bytes at 8x): it
                     filters the raw bytes itself -- <8, 47> for 47 taps, <0, 0> otherwise -- and no k_gather runs in front of it;
                     769 taps: k_gather writes the windows and k_fine_cert only reads them back (that form has no taps in it
                     and is launched as <8, 47>, host_plan.h `g.ov == 8 && (!fg.raw || fg.ntaps == 47)`)
       r_correct     k_stream_tile<47> / <0>; 769 taps (stream_tile_lds > 64 KiB): the level-4 tile gather, a second k_gather
       front end     k_front_fast<47|31> for aligned captures, sym only for exactly mirrored taps; else k_front_fused"""
    _, _, names = profiled(name, unaligned)
    ntaps = len(gt.FILTERS[name])
    coef = gt.FILTERS[name]
    mirrored = np.array_equal(coef, coef[::-1])
    tail = [k for k in names if any(t in k for t in TAIL_KERNELS)]
    if ntaps == 47:
        assert tail == ["(k_post_chain_r<8, 512, 47>)"], names
        assert launches(names, "k_fine_cert<8, 47>") == 1 and launches(names, "k_gather") == 0, names
        assert launches(names, "k_stream_tile<47>") == 1 and launches(names, "k_stream_tile_s47") == 0, names     # not mirrored
    else:
        assert tail == ["(k_post_chain_r<0, 0, 0>)"], names
        assert not any("8, 47>" in k or "8, 512, 47>" in k for k in tail), names
        if ntaps == 769:
            assert launches(names, "k_gather") == 2, names                     # fine windows + r_correct
            assert launches(names, "k_fine_cert") == 1, names
            assert launches(names, "k_stream_tile") == 0, names
        else:
            assert launches(names, "k_gather") == 0, names
            assert launches(names, "k_fine_cert<0, 0>") == 1 and launches(names, "k_fine_cert") == 1, names
            assert launches(names, "k_stream_tile<0>") == 1 and launches(names, "k_stream_tile") == 1, names
    if ntaps in (31, 47) and not unaligned:
        want = f"k_front_fast{ntaps}" + ("_sym" if mirrored else "")
        assert names.get(want) == 1 and launches(names, "k_front_f") == 1, names
    else:
        assert names.get("k_front_fused") == 1 and launches(names, "k_front_f") == 1, names


# ---- (c) the other routes through the chain give the same table ----------------------------------------------------------
VARIANT_FILTERS = ("fir31", "ramp47", "ramp200")
EXACT_ENVS = [{"GSMCAL_CERT": "0"}, {"GSMCAL_PRESCREEN": "0"}, {"GSMCAL_LANES": "4", "GSMCAL_LANE_MIN": "2"},
              {"GSMCAL_FUSE_GATHER": "0"}, {"GSMCAL_FUSE_POST": "0"}, {"GSMCAL_POST_SLOTS": "2"}, {"GSMCAL_SNR_FULL": "0"},
              {"GSMCAL_GRAPH": "2"}, {}]


def context_under(g, env, **kw):
    """a context created under `env` (the switches are read when a context is created)"""
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return g.Context(0, **kw)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def default_out(g, streams, ts):
    """filter -> the session's default context's answer (no profile)"""
    cache = {}

    def run(name):
        if name not in cache:
            cache[name] = g.calibrate_batch(streams, gt.FILTERS[name], ts, FC, want_r=True)
        return cache[name]
    return run


def same_answer(ref, out):
    assert np.array_equal(ref["table"], out["table"], equal_nan=True)
    assert len(ref["pos_info"]) == len(out["pos_info"])
    assert all(np.array_equal(a, b) for a, b in zip(ref["pos_info"], out["pos_info"]))


@pytest.mark.parametrize("name", VARIANT_FILTERS)
def test_profiled_and_default_context_agree(default_out, profiled, name):
    ref, out = default_out(name), profiled(name, False)[0]
    same_answer(ref, out)
    assert np.array_equal(ref["r_len"], out["r_len"])
    for i, L in enumerate(ref["r_len"]):
        if L > 0:
            assert np.array_equal(ref["r_correct"][i, :L], out["r_correct"][i, :L]), i


@pytest.mark.parametrize("env", EXACT_ENVS, ids=lambda e: ",".join(f"{k[7:]}={v}" for k, v in e.items()) or "repeat")
@pytest.mark.parametrize("name", VARIANT_FILTERS)
def test_variants_agree(g, streams, ts, default_out, name, env):
    """No certificate, plain fp64 search, four lanes, fine windows through k_gather, the four-launch tail (k_burst_tone /
    k_window_sch with the raw-source gather in front of them), two post-chain slots per CU, the hop walk on its own spectra;
    and three calls in a row on one context -- plain (eager each time) and under GSMCAL_GRAPH=2 (eager, capture + replay,
    replay): table and pos_info bit for bit the default context's."""
    ref = default_out(name)
    ntaps = len(gt.FILTERS[name])
    cx = context_under(g, env)
    try:
        four_launch = env == {"GSMCAL_FUSE_POST": "0"}
        if four_launch:
            cx.profile_enable()
        for _ in range(3 if env in ({}, {"GSMCAL_GRAPH": "2"}) else 1):
            same_answer(ref, g.calibrate_batch(streams, gt.FILTERS[name], ts, FC, ctx=cx))
        if four_launch:
            names = {k: v[1] for k, v in cx.profile_get().items()}
            print(name, "four-launch tail kernels:", sorted(names.items()))
            geo = ("8, 47>", "8, 512, 47>") if ntaps == 47 else ("0, 0>", "0, 0, 0>")
            for want in (f"(k_burst_tone<1, {geo[0]})", f"(k_window_sch<{geo[1]})", f"(k_burst_tone<0, {geo[0]})"):
                assert names.get(want) == 1, (want, names)
            assert launches(names, "k_post_chain_r") == 0 and launches(names, "k_burst_tone") == 2, names
    finally:
        cx.close()


@pytest.mark.parametrize("name", VARIANT_FILTERS)
def test_generic_front_kernel_agrees(g, streams, ts, default_out, name):
    """GSMCAL_FRONT_GENERIC=1: k_front_fused where the aligned 31- and 47-tap cases take k_front_fast; it sums in another
    order, so the bar is test_front_end_variants_agree's"""
    ref = default_out(name)
    cx = context_under(g, {"GSMCAL_FRONT_GENERIC": "1"})
    try:
        out = g.calibrate_batch(streams, gt.FILTERS[name], ts, FC, ctx=cx)
    finally:
        cx.close()
    assert np.array_equal(ref["table"][:, 6:], out["table"][:, 6:])           # counts, status
    np.testing.assert_allclose(ref["table"][:, :6], out["table"][:, :6], rtol=1e-9, atol=1e-12)
    assert all(np.array_equal(a, b) for a, b in zip(ref["pos_info"], out["pos_info"]))


@pytest.mark.parametrize("name", VARIANT_FILTERS)
def test_pipelined_calls_agree(g, streams, ts, default_out, name):
    """Six calibrate_batch_dev calls three deep (gsmcal_ctx_set_pipeline_depth), each into its own output set: table, pos_info,
    r_len and every sample of r_correct bit for bit what the default context wrote."""
    import torch
    dev = torch.device("cuda", 0)
    ref = default_out(name)
    d, n = streams.shape[0], streams.shape[1] // 2
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        cx = g.Context(0, stream=st.cuda_stream)
        try:
            raw_t = torch.from_numpy(streams).to(dev)
            tabs = [torch.zeros((d, g.TABLE_COLS), dtype=torch.float64, device=dev) for _ in range(6)]
            poss = [torch.zeros((d, 2, g.MAX_POS_ROWS), dtype=torch.float64, device=dev) for _ in range(6)]
            rls = [torch.zeros((d,), dtype=torch.int64, device=dev) for _ in range(6)]
            rcs = [torch.full((d, n, 2), float("nan"), dtype=torch.float64, device=dev) for _ in range(6)]
            cx.set_pipeline_depth(3)
            for k in range(6):
                g.calibrate_batch_dev(raw_t.data_ptr(), d, n, gt.FILTERS[name], ts, FC, tabs[k].data_ptr(), poss[k].data_ptr(),
                                      rcs[k].data_ptr(), rls[k].data_ptr(), ctx=cx)
            cx.sync()
            for k in range(6):
                tab = tabs[k].cpu().numpy()
                assert np.array_equal(tab, ref["table"], equal_nan=True), k
                rl = rls[k].cpu().numpy()
                assert np.array_equal(rl, ref["r_len"]), k
                pk = poss[k].cpu().numpy()
                got = rcs[k].cpu().numpy()
                for i in range(d):
                    if tab[i, 8] != -1.0:
                        assert np.array_equal(pk[i, :, :int(tab[i, 7])].T, ref["pos_info"][i]), (k, i)
                    L = int(rl[i])
                    if L > 0:
                        assert np.array_equal(got[i, :L, 0] + 1j * got[i, :L, 1], ref["r_correct"][i, :L]), (k, i)
        finally:
            cx.close()


# ---- (d) the scanner path ------------------------------------------------------------------------------------------------
SCAN_FILTERS = ("one", "fir5", "fir48", "fir64", "fir65", "ramp66", "ramp200")


@pytest.fixture(scope="module")
def captures(g):
    """64-frame captures: FCCH one frame in / at the very start / one frame in at another multiframe phase (the first windows
    and the head rows matter), one carrier without a BCCH, one at a seeded start"""
    s = g.synth
    caps = [s.make_stream(dongle=80, arfcn=i, num_frames=64, bcch=True, start_frame=s0, frac_start=100.0)[0]
            for i, s0 in enumerate((49, 0, 9))]
    caps.append(s.make_stream(dongle=81, num_frames=64, bcch=False)[0])
    caps.append(s.make_stream(dongle=82, num_frames=64)[0])
    return np.stack(caps)


@pytest.mark.parametrize("name", SCAN_FILTERS)
def test_scanner_against_the_oracle(g, captures, name):
    coef = gt.FILTERS[name]
    out = g.fcch_scan_batch(captures, coef)
    lives = parity.pool_map(gt.scan_job, [(c, coef) for c in captures], max_workers=16)
    for i, live in enumerate(lives):
        n = out["counts"][i]
        assert live["num_hit"] == out["num_hit"][i], (i, live["num_hit"], out["num_hit"][i])
        assert abs(live["snr"] - out["snr"][i]) < parity.SNR_ATOL, (i, live["snr"], out["snr"][i])
        if live["coarse_pos"][0] == -1.0:
            assert n == 0 and out["positions"][i, 0] == -1.0, i
        else:
            parity.assert_positions(out["positions"][i, :n], live["coarse_pos"], f"scan positions ({name}, capture {i})")
            assert np.allclose(out["pos_snr"][i, :n], live["coarse_snr"], rtol=0, atol=parity.SNR_ATOL), i
    # the detector input itself: the first decimated rows (the head rows take partial tap sums of the DC term)
    fe = g.frontend_batch(captures, coef, 64)
    want = o.matlab_filter(coef, o.raw2iq(captures.T.astype(np.float64)))[0::64]
    assert np.max(np.abs(fe.T[:8] - want[:8])) < 1e-11


def test_the_scanner_set_sees_a_carrier_and_none(captures):
    """(the oracle alone) the captures hold accepted carriers and one that is not"""
    hits = [o.scan_capture(c, gt.FILTERS["fir48"])["num_hit"] for c in captures]
    assert sum(h > 0 for h in hits) >= 3 and any(h == 0 for h in hits), hits
