"""GPU tests (-m gpu) of the window gathers of the four-launch tail: k_burst_tone<1|0, 8, 47> run burst_gather_fast against
an LDS copy of their stream's state, k_window_sch<8, 512, 47> builds its window with sch_gather_fast; the fused tail
k_post_chain_r keeps gather_core for the SCH window, and the generic instantiations keep it everywhere.

Every batch of tests/tail_gathers.py runs three ways -- the default fused tail, GSMCAL_FUSE_POST=0 (the four launches) and
four calls in flight (which take the four-launch tail as well) -- and the table, pos_info, r_len and last_batch_details of
the three are compared BIT FOR BIT (the details of calls in flight through a reference taken with their own coarse detector:
COARSE_SNR_BOUND_DB below): equality of the fused and the four-launch answers is the check of the new SCH gather against the
old one.  The fused answer is held against the live oracle (parity.compare_stream; bars of tests/parity.py), and
each batch must take a stream through the SCH stage in the oracle, so that no comparison is empty
(tests/test_tail_gathers_cpu.py holds the same on the CPU)."""
import numpy as np
import pytest

import parity
import tail_gathers as tg
from tail_gathers import context_under, launches

pytestmark = pytest.mark.gpu

FC = tg.FC
FOUR = {"GSMCAL_FUSE_POST": "0"}


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


@pytest.fixture(scope="module")
def ts(g):
    return g.synth.sch_training_sequence()


@pytest.fixture(scope="module")
def batches():
    return tg.build()


def dev_call(g, cx, raw_t, coef, ts):
    """one gsmcal_calibrate_batch_dev call into fresh outputs"""
    import torch
    d, n = raw_t.shape[0], raw_t.shape[1] // 2
    dev = raw_t.device
    tab = torch.zeros((d, g.TABLE_COLS), dtype=torch.float64, device=dev)
    pos = torch.zeros((d, 2, g.MAX_POS_ROWS), dtype=torch.float64, device=dev)
    rl = torch.zeros((d,), dtype=torch.int64, device=dev)
    g.calibrate_batch_dev(raw_t.data_ptr(), d, n, coef, ts, FC, tab.data_ptr(), pos.data_ptr(), None, rl.data_ptr(), ctx=cx)
    return tab, pos, rl


def as_out(tab, pos, rl):
    table, p = tab.cpu().numpy(), pos.cpu().numpy()
    rows = []
    for i in range(len(table)):
        k = int(table[i, 7])
        rows.append(-np.ones((k, 2)) if table[i, 8] == -1.0 else p[i, :, :k].T.copy())
    return {"table": table, "pos_info": rows, "r_len": rl.cpu().numpy()}


def run_dev(g, ts, order, env=None, depth=1, profile=False):
    """device-pointer calls on the batches of `order` (a list of (raw, taps)), one after the other on a fresh context on a torch
    stream, each into outputs of its own -> (outputs per call, details of the last call, {kernel: launches} or None)"""
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        cx = context_under(g, env or {}, stream=st.cuda_stream)
        try:
            if profile:
                cx.profile_enable()
            dev_raw = {}
            for raw, _ in order:
                if id(raw) not in dev_raw:
                    dev_raw[id(raw)] = torch.from_numpy(raw).to(dev)
            st.synchronize()
            if depth > 1:
                cx.set_pipeline_depth(depth)
            outs = [dev_call(g, cx, dev_raw[id(raw)], taps, ts) for raw, taps in order]
            cx.sync()
            det = g.last_batch_details(len(order[-1][0]), ctx=cx)
            names = {k: v[1] for k, v in cx.profile_get().items()} if profile else None
            res = [as_out(*x) for x in outs]
        finally:
            cx.close()
    return res, det, names


def same_bits(ref, out, what):
    assert np.array_equal(ref["table"], out["table"], equal_nan=True), what
    assert len(ref["pos_info"]) == len(out["pos_info"]), what
    assert all(np.array_equal(a, b) for a, b in zip(ref["pos_info"], out["pos_info"])), what
    assert np.array_equal(ref["r_len"], out["r_len"]), what


def same_details(ref, det, what, but=()):
    assert set(ref) == set(det), what
    for k in ref:
        if k not in but:
            assert np.array_equal(ref[k], det[k], equal_nan=True), (what, k)


# Calls in flight take the four-launch tail AND another coarse detector in front of it: k_coarse_scan_inl computes the moving
# search's SNRs itself, where a call alone reads them from the full table of k_coarse_snr (host_plan.h: snr_nwin, no_fuse_now).
# Each detector forms the 16-point spectrum of a window and adds up bin powers itself, in an order of its own, so the SNRs they
# REPORT (coarse_snr of the details; no decision differs, every position is compared exactly) may differ by rounding.  Worst
# case per detector: a bin is a 16-term complex dot product, its power carries 2 * 16 eps of relative error, a sum of up to
# 16 powers 15 eps more: 47 eps for the signal power and for the total alike; the ratio of the two, compared between two
# detectors: 4 * 47 eps.  10*log10 turns a relative error r into 10 / ln(10) * r dB, plus an ulp of the result on either side
# (3.6e-15 dB at 16..32 dB):
COARSE_SNR_BOUND_DB = 10.0 / np.log(10.0) * 188 * 2.0 ** -53 + 2 * 3.6e-15     # 9.8e-14 dB
# The details of calls in flight are therefore compared BIT FOR BIT with a reference taken with the same detector -- the
# same depth-4 context with a profile on, which runs one call at a time with the kernels the calls in flight run
# (abi_calls.h: same_kernels_unpipelined) --, and that reference with the fused one: every field but coarse_snr bit for bit,
# coarse_snr within the bound above.


def same_details_but_snr(ref, det, what):
    d = float(np.max(np.abs(ref["coarse_snr"] - det["coarse_snr"])))
    print(f"{what}: coarse_snr of the two detectors: max abs difference {d:.3e} dB (bound {COARSE_SNR_BOUND_DB:.3e})")
    same_details(ref, det, what, but=("coarse_snr",))
    assert d <= COARSE_SNR_BOUND_DB, (what, d)


@pytest.fixture(scope="module")
def fused(g, ts, batches):
    """name -> (output, details, kernel launches) of ONE default call on a fresh profiled context; computed once per batch"""
    cache = {}

    def run(name):
        if name not in cache:
            res, det, names = run_dev(g, ts, [batches[name]], profile=True)
            cache[name] = (res[0], det, names)
        return cache[name]
    return run


@pytest.fixture(scope="module")
def alone4(g, ts, batches, fused):
    """name -> (output, details) of ONE call on a fresh depth-4 context with a profile on: one call at a time, with the kernels
    of calls in flight -- the four-launch tail behind k_coarse_scan_inl; held to the fused reference here, once per batch"""
    cache = {}

    def run(name):
        if name not in cache:
            res, det, names = run_dev(g, ts, [batches[name]], depth=4, profile=True)
            print(f"{name}: kernels of a call in flight {sorted(names.items())}")
            assert launches(names, "k_post_chain_r") == 0 and launches(names, "k_burst_tone") == 2 and launches(names, "k_window_sch") == 1, names
            # the two detectors: the table kernel in front of the fused call, none in front of a call in flight
            assert launches(names, "k_coarse_scan_inl") == 1 and launches(names, "k_coarse_snr") == 0, names
            assert launches(fused(name)[2], "k_coarse_scan_inl") == 0 and launches(fused(name)[2], "k_coarse_snr") == 1, fused(name)[2]
            ref, dref, _ = fused(name)
            same_bits(ref, res[0], f"{name}: the kernels of calls in flight, one call")
            same_details_but_snr(dref, det, f"{name}: the kernels of calls in flight, one call")
            cache[name] = (res[0], det)
        return cache[name]
    return run


@pytest.fixture(scope="module")
def oracles(batches):
    cache = {}

    def run(name):
        if name not in cache:
            cache[name] = tg.oracle_batch(*batches[name])
        return cache[name]
    return run


CASES = ("plain", "ppm", "ends", "copy", "fir31", "ramp47")


@pytest.mark.parametrize("name", CASES)
def test_three_routes_agree_bit_for_bit(g, ts, batches, fused, alone4, oracles, name):
    raw, taps = batches[name]
    assert 3 <= len(raw) <= 4 and raw.shape[1] <= 2 * tg.NUM_FRAMES * 10000
    ref, det, names = fused(name)
    print(f"{name}: fused-route kernels {sorted(names.items())}")
    # the default route is the fused tail; the reference geometry compiled in where the filter is the drivers'
    assert launches(names, "k_post_chain_r") == 1 and launches(names, "k_burst_tone") == 0 and launches(names, "k_window_sch") == 0, names
    assert ("(k_post_chain_r<8, 512, 47>)" in names) == (name not in tg.GENERIC), names
    # ---- against the oracle ----
    orcs = oracles(name)
    assert any(o is not None and tg.through_sch(o) for o in orcs), f"{name}: no stream reaches the SCH stage in the oracle"
    for i, o in enumerate(orcs):
        assert o is not None, (name, i)
        print(f"   stream {i}: status {o['status']} SCH windows {len(o['sch_first_round_pos'])} sampling ppm {o['sampling_ppm']} "
              f"| gpu row {ref['table'][i]}")
        parity.compare_stream(o, ref["table"][i], det, i, ref["pos_info"][i])
        assert ref["r_len"][i] == o["r_len"], (name, i, ref["r_len"][i], o["r_len"])
    # ---- the four launches ----
    res4, det4, names4 = run_dev(g, ts, [batches[name]], env=FOUR, profile=True)
    print(f"{name}: four-launch kernels {sorted(names4.items())}")
    assert launches(names4, "k_post_chain_r") == 0 and launches(names4, "k_burst_tone") == 2 and launches(names4, "k_window_sch") == 1, names4
    if name not in tg.GENERIC:
        for want in ("(k_burst_tone<1, 8, 47>)", "(k_window_sch<8, 512, 47>)", "(k_burst_tone<0, 8, 47>)"):
            assert names4.get(want) == 1, (want, names4)
    else:
        for want in ("(k_burst_tone<1, 0, 0>)", "(k_window_sch<0, 0, 0>)", "(k_burst_tone<0, 0, 0>)"):
            assert names4.get(want) == 1, (want, names4)
    same_bits(ref, res4[0], f"{name}: four launches")
    same_details(det, det4, f"{name}: four launches")
    # ---- four calls in flight ----
    ref4, dref4 = alone4(name)
    for i, o in enumerate(orcs):                                   # (the other detector's coarse_snr against the oracle as well)
        parity.compare_stream(o, ref4["table"][i], dref4, i, ref4["pos_info"][i])
    resp, detp, _ = run_dev(g, ts, [batches[name]] * 5, depth=4)
    for k, out in enumerate(resp):
        same_bits(ref, out, f"{name}: call {k} of five, four in flight")
    same_details(dref4, detp, f"{name}: four in flight")


def test_two_batches_alternating_four_deep(g, ts, batches, fused, alone4):
    """`plain` and `other` (same shape, different captures) alternate on one context at pipeline depth 4: every output set
    equals the same batch alone"""
    a, b = batches["plain"], batches["other"]
    assert a[0].shape == b[0].shape and not np.array_equal(a[0], b[0])
    ref_a, det_a, _ = fused("plain")
    ref_b, det_b, _ = fused("other")
    assert not np.array_equal(ref_a["table"], ref_b["table"], equal_nan=True)
    res, det, _ = run_dev(g, ts, [a, b] * 4, depth=4)
    for k, out in enumerate(res):
        same_bits(ref_b if k % 2 else ref_a, out, f"call {k}")
    same_details(alone4("other")[1], det, "the last call's details")
