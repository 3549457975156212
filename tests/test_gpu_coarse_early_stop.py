"""k_coarse_scan<.., INL> decides every window of the moving search in the round (256 windows) that computes it and stops
behind the first certified hit (-m gpu).  Captures whose first hit -- computed here with the oracle, never taken from frame
arithmetic -- lies on either side of the boundaries between rounds 1|2 and 2|3, early in round 1, in rounds 7 and 8, nowhere
(no BCCH carrier), or behind windows the certificate cannot decide (NaN and +inf SNRs: the exact replay, every round) run as
ONE batch through the three routes of the detector: window SNRs inside the scan kernel (early stop), the same with the table
kept (every round), and the table kernel k_coarse_snr + table scan.  All three must agree bit for bit, with the oracle, with
calls in flight and in the scanner.  The synthesiser reaches every hit index asked for; a case it could not reach would be
replaced by the nearest index the search found (see _capture_with_hit) and the coverage test says which rounds are met."""
import numpy as np
import pytest

import parity
import worstcase as wc
from oracle import gsmcal_oracle as o

pytestmark = pytest.mark.gpu

FC = 957.4e6
FRAMES = 26                      # 24 is the fewest that give the moving search its 3 594 rows
ROUND = 256                      # windows per round of the in-kernel SNR loop
# name -> (start_frame, first guess of frac_start, wanted 0-based window of the first hit or None: take what comes)
HIT_CASES = {
    "round1_200": (8, 7488.0, 200),
    "hit_255": (8, 3968.0, 255), "hit_256": (8, 3904.0, 256), "hit_257": (8, 3840.0, 257),
    "hit_511": (6, 7616.0, 511), "hit_512": (6, 7552.0, 512), "hit_513": (6, 7488.0, 513),
    "late": (39, 3600.0, None),                 # burst at window ~100, inside the seeded history; the next one 11 frames on
    "seeded_history": (0, 0.0, None),           # burst at window 0: the reference misses it and hits ten frames later
}


def _first_hit(raw, coef):
    """0-based window of move_fft_snr_runtime_avg's first hit on the capture's decimated stream, None without one"""
    r = o.front_end(raw, coef)
    hf, hidx, _, _ = o.move_fft_snr_runtime_avg(r[0::64][:3594], 160, 16, 10.0)
    return int(hidx) - 1 if hf else None


def _capture_with_hit(synth, coef, dongle, start_frame, frac_start, want):
    """frac_start is moved by 64 raw samples per window until the oracle's first hit is `want`; the nearest index met
    otherwise -> (capture, hit)"""
    best = None
    fs = frac_start
    for _ in range(8):
        raw = synth.make_stream(dongle=dongle, num_frames=FRAMES, start_frame=start_frame, frac_start=fs)[0]
        h = _first_hit(raw, coef)
        assert h is not None
        if want is None or h == want:
            return raw, h
        if best is None or abs(h - want) < abs(best[1] - want):
            best = (raw, h)
        fs = min(max(fs + 64.0 * (h - want), 0.0), 19000.0)
    return best


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


@pytest.fixture(scope="module")
def setup(g):
    s = g.synth
    return {"coef": s.fir1(46, 200e3 / s.FS), "coef31": s.fir1(30, 200e3 / s.FS), "ts": s.sch_training_sequence()}


@pytest.fixture(scope="module")
def batch(g, setup):
    """names, captures (one batch of 12), the oracle's first hit per capture, the oracle's calibrate_stream per capture"""
    names, caps, hits = [], [], []
    for k, (name, (sf, fs, want)) in enumerate(HIT_CASES.items()):
        raw, h = _capture_with_hit(g.synth, setup["coef"], 60 + k, sf, fs, want)
        names.append(name); caps.append(raw); hits.append(h)
    names.append("no_bcch")
    caps.append(g.synth.make_stream(dongle=75, num_frames=FRAMES, bcch=False)[0])
    hits.append(_first_hit(caps[-1], setup["coef"]))
    # dropped samples at decimated rows 200..240, in front of a hit near window 512: exact zeros (NaN SNRs) / a constant (+inf).
    # (the dither that makes the means exact needs a capture whose I and Q levels both lie close to one byte value)
    for dg in range(80, 200):
        base = g.synth.make_stream(dongle=dg, num_frames=FRAMES, start_frame=6, frac_start=7552.0)[0]
        mi, mq = float(np.mean(base[0::2])), float(np.mean(base[1::2]))
        if round(mi) == round(mq) and max(abs(mi - round(mi)), abs(mq - round(mq))) < 0.4:
            break
    assert _first_hit(base, setup["coef"]) > ROUND
    stretch = wc.constant_stretch_captures(base, starts=(200 * 64,), level=int(round(mi)))
    for k in ("exact_mean_200", "near_mean_200"):
        names.append(k); caps.append(stretch[k]); hits.append(_first_hit(stretch[k], setup["coef"]))
    raw = np.stack(caps)
    orc = [o.calibrate_stream(c, setup["coef"], setup["ts"], FC) for c in caps]      # (26 frames: a second for all twelve)
    return {"names": names, "raw": raw, "hits": hits, "orc": orc}


@pytest.fixture(scope="module")
def routes(g, setup, batch):
    """The batch through the three detector routes, one context each (the switches are read when a context is created;
    GSMCAL_SNR_FULL=0 sends a batch this small down the throughput path) -> name -> outputs"""
    mp = pytest.MonkeyPatch()
    made, out = {}, {}
    try:
        for name, env in (("kernel", {"GSMCAL_SNR_INLINE_MIN": "0"}), ("inline_kept", {"GSMCAL_SNR_INLINE_KEEP": "1"}), ("inline", {})):
            mp.setenv("GSMCAL_SNR_FULL", "0")
            for k, v in env.items():
                mp.setenv(k, v)
            made[name] = g.Context(0)
            for k in list(env) + ["GSMCAL_SNR_FULL"]:
                mp.delenv(k)
        d = len(batch["raw"])
        for name, cx in made.items():
            cal = g.calibrate_batch(batch["raw"], setup["coef"], setup["ts"], FC, ctx=cx)
            det = g.last_batch_details(d, ctx=cx)
            tabs = None if name == "inline" else [g.last_batch_snr(i, ctx=cx) for i in range(d)]
            out[name] = {"cal": cal, "det": det, "snr": tabs}
        yield out
    finally:
        mp.undo()
        for cx in made.values():
            cx.close()


def test_the_first_hits_lie_on_both_sides_of_round_boundaries(batch):
    """What the other tests stand on: the oracle's first hits cover at least five rounds and both sides of a boundary, one
    lies in round 1, one past window 1 792, the burst inside the seeded history is missed, the traffic carrier never hits."""
    hit = dict(zip(batch["names"], batch["hits"]))
    print({k: (v, None if v is None else v // ROUND + 1) for k, v in hit.items()})
    found = [h for h in batch["hits"] if h is not None]
    assert len({h // ROUND for h in found}) >= 5
    sides = {(h + 1) // ROUND for h in found if (h + 1) % ROUND == 0} & {h // ROUND for h in found if h % ROUND == 0}
    assert sides, "no pair of hits at windows 256 k - 1 and 256 k"
    assert [hit[k] for k in ("hit_255", "hit_256", "hit_257", "hit_511", "hit_512", "hit_513")] == [255, 256, 257, 511, 512, 513]
    assert 155 <= hit["round1_200"] < ROUND and hit["late"] > 1792
    assert hit["seeded_history"] > 1500            # (a burst at window 0 would be hit at once were it not for the 999 seeds)
    assert hit["no_bcch"] is None
    assert hit["exact_mean_200"] is None           # the NaN stays in the reference's running sum for good
    assert hit["near_mean_200"] is not None and hit["near_mean_200"] < 256


def test_the_three_routes_agree_bit_for_bit(batch, routes):
    ref = routes["kernel"]
    for name in ("inline_kept", "inline"):
        got = routes[name]
        assert np.array_equal(ref["cal"]["table"], got["cal"]["table"], equal_nan=True), name
        assert np.array_equal(ref["cal"]["r_len"], got["cal"]["r_len"]), name
        assert all(np.array_equal(a, b) for a, b in zip(ref["cal"]["pos_info"], got["cal"]["pos_info"])), name
        assert np.array_equal(ref["det"]["counts"], got["det"]["counts"]), name
        # coarse_pos[0] / coarse_snr[0] are mv_hit_idx (as a position) and mv_hit_snr; the rest is the hop walk
        for k in ("coarse_pos", "coarse_snr"):
            assert np.array_equal(ref["det"][k], got["det"][k], equal_nan=True), (name, k)
    for i, nm in enumerate(batch["names"]):
        (ta, na), (tb, nb) = ref["snr"][i], routes["inline_kept"]["snr"][i]
        assert na == nb == 3579 and len(ta) == len(tb) == 3579
        assert np.array_equal(ta, tb, equal_nan=True), f"{nm}: kept window SNRs differ from k_coarse_snr's"
    no = batch["names"].index("no_bcch")
    assert routes["inline"]["cal"]["table"][no, 9] == float(o.S_NO_FCCH)
    assert routes["inline"]["det"]["counts"][no, 0] == 0


def test_the_early_stop_route_matches_the_oracle(batch, routes):
    got = routes["inline"]
    for i, nm in enumerate(batch["names"]):
        h = batch["hits"][i]
        if h is not None:                          # mv_hit_idx, as FCCH_coarse_position.m:91 reports it
            assert got["det"]["coarse_pos"][i, 0] == float(h * 8 + 1), nm
        parity.compare_stream(batch["orc"][i], got["cal"]["table"][i], got["det"], i, got["cal"]["pos_info"][i])


def test_calls_in_flight_with_early_and_late_hits_mixed(g, setup, batch, routes, monkeypatch):
    """Eight calls four deep over two orders of the batch (early hits leave their rounds while a neighbour call's late ones
    still run): every output set bit for bit the one-call-at-a-time result."""
    import torch
    dev = torch.device("cuda", 0)
    raws = [batch["raw"], np.ascontiguousarray(batch["raw"][::-1])]
    d, n = raws[0].shape[0], raws[0].shape[1] // 2
    one = routes["inline"]["cal"]
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        monkeypatch.setenv("GSMCAL_SNR_FULL", "0")
        cx = g.Context(0, stream=st.cuda_stream)
        monkeypatch.delenv("GSMCAL_SNR_FULL")
        try:
            raw_t = [torch.from_numpy(r_).to(dev) for r_ in raws]
            tabs = [torch.zeros((d, g.TABLE_COLS), dtype=torch.float64, device=dev) for _ in range(8)]
            poss = [torch.zeros((d, 2, g.MAX_POS_ROWS), dtype=torch.float64, device=dev) for _ in range(8)]
            rls = [torch.zeros((d,), dtype=torch.int64, device=dev) for _ in range(8)]
            cx.set_pipeline_depth(4)
            for k in range(8):
                g.calibrate_batch_dev(raw_t[k & 1].data_ptr(), d, n, setup["coef"], setup["ts"], FC, tabs[k].data_ptr(),
                                      poss[k].data_ptr(), None, rls[k].data_ptr(), ctx=cx)
            cx.sync()
            for k in range(8):
                order = np.arange(d)[::-1] if k & 1 else np.arange(d)
                assert np.array_equal(tabs[k].cpu().numpy(), one["table"][order], equal_nan=True), k
                assert np.array_equal(rls[k].cpu().numpy(), one["r_len"][order]), k
                assert np.array_equal(poss[k].cpu().numpy(), one["pos_info_raw"][order], equal_nan=True), k
        finally:
            cx.close()


def test_the_scanner_with_early_stop_matches_the_table_route(g, setup, batch, monkeypatch):
    """fcch_scan_batch_dev on the same captures: snr and num_hit bit for bit those of the table-kernel route."""
    import torch
    dev = torch.device("cuda", 0)
    d, n = batch["raw"].shape[0], batch["raw"].shape[1] // 2
    monkeypatch.setenv("GSMCAL_SNR_FULL", "0")
    inl = g.Context(0)
    monkeypatch.setenv("GSMCAL_SNR_INLINE_MIN", "0")
    ker = g.Context(0)
    monkeypatch.delenv("GSMCAL_SNR_INLINE_MIN")
    monkeypatch.delenv("GSMCAL_SNR_FULL")
    try:
        want = g.fcch_scan_batch(batch["raw"], setup["coef31"], ctx=ker)
        raw_t = torch.from_numpy(batch["raw"]).to(dev)
        sn = torch.full((d, 2), float("nan"), dtype=torch.float64, device=dev)
        pos = torch.zeros((d, g.MAX_HITS), dtype=torch.float64, device=dev)
        psn = torch.zeros((d, g.MAX_HITS), dtype=torch.float64, device=dev)
        cnt = torch.zeros((d,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        g.fcch_scan_batch_dev(raw_t.data_ptr(), d, n, setup["coef31"], sn.data_ptr(), pos.data_ptr(), psn.data_ptr(), cnt.data_ptr(), ctx=inl)
        inl.sync()
        got = sn.cpu().numpy()
        assert np.array_equal(got[:, 0], want["snr"], equal_nan=True)
        assert np.array_equal(got[:, 1], want["num_hit"], equal_nan=True)
        assert np.array_equal(cnt.cpu().numpy(), want["counts"])
        assert np.array_equal(pos.cpu().numpy(), want["positions"], equal_nan=True)
        assert np.array_equal(psn.cpu().numpy(), want["pos_snr"], equal_nan=True)
        assert want["num_hit"][batch["names"].index("no_bcch")] == 0.0
    finally:
        inl.close()
        ker.close()


@pytest.mark.parametrize("delta", [1e-9, -1e-9, 1e-7, -1e-7])
def test_per_function_detector_with_the_first_window_on_the_threshold(g, delta):
    """FCCH_coarse_position(s, 8) on a decimated stream of 15 938 samples whose first candidate window sits |delta| from the
    threshold, inside the certificate's margin: an undecided window in front of every decided one, settled by the exact replay
    (one call at a time: the table scan, which this form of the kernel leaves as it was)."""
    s, info = wc.coarse_threshold_stream(delta, "first")
    want_p, want_s = o.FCCH_coarse_position(s, 8)
    got_p, got_s = g.FCCH_coarse_position(s, 8)
    parity.assert_positions(got_p, want_p, f"coarse positions (margin {info['margin']:g})")
    assert np.allclose(got_s, want_s, rtol=0, atol=parity.SNR_ATOL)
    assert (got_p[0] == 1000 * 8 + 1) == (delta > 0)          # window 1000 hits on the + side only
