"""The hop walk of k_coarse_scan on its own 16-point spectra (-m gpu): every window of a hop's 11-candidate group is decided
inside the DPP row that computed its spectrum and every wave walks on from the group's 11 records.  26-frame captures (two or
three hops) built so that each branch of the walk is taken -- which branch a capture takes is read off the ORACLE's positions
(test_the_captures_take_the_branches_they_are_named_for), never assumed:

  cand_0 / cand_10   a stretch of samples taken out / doubled between the first two bursts: the second hit is the first / last
                     candidate of the +10-frame group
  idle_frame         the capture starts four frames in front of frame 40: the +10-frame group misses, the +11-frame group hits
  both_miss          the second burst (both groups) overwritten with traffic: the walk stops, n_coarse stays 1
  g1_off_hit/_miss   the second hit lies so late that the +11-frame group of the third hop would run past the end of the capture
                     (nx1 > limit): only the +10-frame group is looked at; it hits / (third burst overwritten) misses
  inf_stretch        dropped samples filled with the rounded DC level over the +10-frame candidates of the second hop: windows
  nan_stretch        with ONE non-zero bin (no noise: +inf in the reference) / exact zeros (0/0) -- a candidate the ratio test
                     cannot settle sends the stream through the exact replay
  inf_edge/nan_edge  the same stretch ending among the candidates: windows that are part constant, part burst
  snr_5 .. snr_8     5, 6.5 and 8 dB streams: decisions close to the threshold
  constant           a capture of one byte value: every window below the residue floor, no hit
  no_bcch            a traffic carrier: the moving search finds nothing

All captures run as ONE batch through: the calibration entry at depth 1 (full SNR table, the one-wave table walk), at depth 4
(k_coarse_scan<INL>: the moving search's SNRs in the kernel, the walk on its own spectra), the scanner, and -- the other
instantiations of the walk -- the calibration entry and the scanner of a context without the full table (GSMCAL_SNR_FULL=0), with
and without the in-kernel moving search (GSMCAL_SNR_INLINE_MIN=0).  Positions, hit counts and status match the oracle exactly,
SNRs and ppm within tests/parity.py's tolerances; the routes agree with each other bit for bit."""
import numpy as np
import pytest

import parity
import worstcase as wc
from oracle import gsmcal_oracle as o

pytestmark = pytest.mark.gpu

FC = 957.4e6
FRAMES = 26
D0, D1 = 1563, 1719              # round(12500 / 8), round(13750 / 8): the hops of FCCH_coarse_position.m:35-36 in windows
LIMIT = 4063 - 15 - 5            # last window a candidate group may start from (:49, :67), 26 frames


def _windows(pos):
    """1-based windows of the oracle's coarse positions, [] without a hit"""
    pos = np.atleast_1d(pos)
    return [] if pos[0] == -1.0 else [int(v) for v in (pos - 1) / 8 + 1]


def _hops(w):
    """per hop (group, candidate): group 0 = +10 frames, 1 = +11 frames (across the idle frame)"""
    out = []
    for a, b in zip(w[:-1], w[1:]):
        out.append((0, b - a - D0 + 5) if abs(b - a - D0) <= 5 else (1, b - a - D1 + 5))
    return out


def _shift(raw, at_window, k):
    """k > 0: the 64 k samples in front of window at_window once more (what follows moves k windows later, the tail drops
    out); k < 0: 64 |k| samples taken out (the tail is filled from the samples in front of it)"""
    b = raw.reshape(-1, 2)
    p = at_window * 64
    if k > 0:
        b = np.concatenate([b[:p], b[p - 64 * k:p], b[p:]])[:len(b)]
    elif k < 0:
        b = np.concatenate([b[:p], b[p + 64 * -k:], b[len(b) - 2000 - 64 * -k:len(b) - 2000]])
    return np.ascontiguousarray(b).reshape(-1)


def _overwrite(raw, lo_window, hi_window, src_window):
    """windows [lo, hi) (and the 16 samples a window spans) overwritten with the traffic that starts at src_window"""
    b = raw.reshape(-1, 2).copy()
    n = (hi_window - lo_window + 16) * 64
    b[lo_window * 64: lo_window * 64 + n] = b[src_window * 64: src_window * 64 + n]
    return b.reshape(-1)


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


@pytest.fixture(scope="module")
def setup(g):
    s = g.synth
    return {"coef": s.fir1(46, 200e3 / s.FS), "ts": s.sch_training_sequence()}


@pytest.fixture(scope="module")
def batch(g, setup):
    """names, captures, per capture the oracle's calibrate_stream and scan_capture (computed once, never changed)"""
    s, coef = g.synth, setup["coef"]

    def win(raw):
        return _windows(o.FCCH_coarse_position(o.front_end(raw, coef)[0::64], 8)[0])

    caps = {}
    base = s.make_stream(dongle=0, num_frames=FRAMES, start_frame=5, frac_start=2000.0)[0]
    w = win(base)
    nominal = _hops(w)[0][1]
    caps["cand_0"] = _shift(base, w[0] + 800, 0 - nominal)
    caps["cand_10"] = _shift(base, w[0] + 800, 10 - nominal)
    caps["idle_frame"] = s.make_stream(dongle=1, num_frames=FRAMES, start_frame=36, frac_start=2000.0)[0]
    caps["both_miss"] = _overwrite(base, w[0] + D0 - 8, w[0] + D1 + 8, w[0] + 300)
    late = s.make_stream(dongle=2, num_frames=FRAMES, start_frame=5, frac_start=200.0)[0]
    wl = win(late)
    caps["g1_off_hit"] = late
    caps["g1_off_miss"] = _overwrite(late, wl[1] + D0 - 8, wl[1] + D0 + 8, wl[0] + 300)
    # 40 windows of dropped samples over all the +10-frame candidates of the second hop (inf_ / nan_stretch), and ending among
    # them in front of the burst (inf_ / nan_edge: windows that are part constant, part signal)
    mi = float(np.mean(base[0::2]))
    for tag, start in (("stretch", w[0] + D0 - 8), ("edge", w[0] + D0 - 5 - 36)):
        made = wc.constant_stretch_captures(base, starts=(start * 64,), level=int(round(mi)))
        caps["inf_" + tag] = next(v for k, v in made.items() if k.startswith("near_mean"))
        caps["nan_" + tag] = next(v for k, v in made.items() if k.startswith("exact_mean"))
    for name, snr in (("snr_5", 5.0), ("snr_6p5", 6.5), ("snr_8", 8.0)):
        caps[name] = s.make_stream(dongle=10 + int(snr), num_frames=FRAMES, snr_db=snr)[0]
    caps["constant"] = wc.degenerate_captures(FRAMES)["constant_128"]
    caps["no_bcch"] = s.make_stream(dongle=3, num_frames=FRAMES, bcch=False)[0]
    names = list(caps)
    raw = np.stack([caps[k] for k in names])
    orc = [o.calibrate_stream(c, coef, setup["ts"], FC) for c in raw]
    return {"names": names, "raw": raw, "orc": orc, "scan": [o.scan_capture(c, coef) for c in raw]}


@pytest.fixture(scope="module")
def routes(g, setup, batch):
    """name -> outputs of the batch through one route (see the module's docstring); the switches are read when a context is made"""
    import torch
    dev = torch.device("cuda", 0)
    mp = pytest.MonkeyPatch()
    made, out = {}, {}
    raw, coef, ts = batch["raw"], setup["coef"], setup["ts"]
    d, n = raw.shape[0], raw.shape[1] // 2
    try:
        for name, env in (("own_inl", {"GSMCAL_SNR_FULL": "0"}), ("own_table", {"GSMCAL_SNR_FULL": "0", "GSMCAL_SNR_INLINE_MIN": "0"})):
            for k, v in env.items():
                mp.setenv(k, v)
            made[name] = g.Context(0)
            for k in env:
                mp.delenv(k)
        cal = g.calibrate_batch(raw, coef, ts, FC)
        out["depth1"] = {"cal": cal, "det": g.last_batch_details(d)}
        out["scan"] = g.fcch_scan_batch(raw, coef)
        for name, cx in made.items():
            cal = g.calibrate_batch(raw, coef, ts, FC, ctx=cx)
            out[name] = {"cal": cal, "det": g.last_batch_details(d, ctx=cx)}
            out["scan_" + name] = g.fcch_scan_batch(raw, coef, ctx=cx)
        st = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(st):
            cx = made["depth4"] = g.Context(0, stream=st.cuda_stream)
            raw_t = torch.from_numpy(raw).to(dev)
            tabs = [torch.zeros((d, g.TABLE_COLS), dtype=torch.float64, device=dev) for _ in range(4)]
            poss = [torch.zeros((d, 2, g.MAX_POS_ROWS), dtype=torch.float64, device=dev) for _ in range(4)]
            rls = [torch.zeros((d,), dtype=torch.int64, device=dev) for _ in range(4)]
            cx.set_pipeline_depth(4)
            for k in range(4):                     # four calls in flight, the details are those of the last
                g.calibrate_batch_dev(raw_t.data_ptr(), d, n, coef, ts, FC, tabs[k].data_ptr(), poss[k].data_ptr(), None, rls[k].data_ptr(), ctx=cx)
            det = g.last_batch_details(d, ctx=cx)
            cx.sync()
            out["depth4"] = {"det": det, "calls": [{"table": tabs[k].cpu().numpy(), "pos_info_raw": poss[k].cpu().numpy(),
                                                    "r_len": rls[k].cpu().numpy()} for k in range(4)]}
        yield out
    finally:
        mp.undo()
        for cx in made.values():
            cx.close()


def test_the_captures_take_the_branches_they_are_named_for(batch):
    w = {k: _windows(r["coarse_pos"]) for k, r in zip(batch["names"], batch["orc"])}
    h = {k: _hops(v) for k, v in w.items()}
    print({k: (w[k], h[k]) for k in w})
    assert h["cand_0"][0] == (0, 0) and h["cand_10"][0] == (0, 10)
    assert h["idle_frame"][0][0] == 1                                   # group 0 missed, taken across the idle frame
    assert len(w["both_miss"]) == 1 and w["both_miss"][0] + D1 <= LIMIT  # both groups were looked at
    for k in ("g1_off_hit", "g1_off_miss"):
        assert w[k][1] + D0 <= LIMIT < w[k][1] + D1, k                  # third hop: nx0 inside, nx1 past the limit
    assert len(w["g1_off_hit"]) == 3 and len(w["g1_off_miss"]) == 2
    print({k: r["coarse_snr"] for k, r in zip(batch["names"], batch["orc"]) if k[:4] in ("inf_", "nan_")})
    snr = dict(zip(batch["names"], (np.atleast_1d(r["coarse_snr"]) for r in batch["orc"])))
    assert np.isposinf(snr["inf_stretch"][1])                           # a window without noise is a hit in the reference
    assert len(w["nan_stretch"]) == 1                                   # 0/0 at every +10-frame candidate: misses; nothing 11 frames on
    assert len(w["inf_edge"]) >= 2 and len(w["nan_edge"]) >= 2
    assert w["constant"] == [] and w["no_bcch"] == []
    assert all(len(w[k]) >= 1 for k in ("snr_5", "snr_6p5", "snr_8"))


def _cut_pos_info(row, pos_raw):
    """pos_info of one stream in the oracle's shape, as calibrate_batch cuts it from the raw rows"""
    k = int(row[7])
    return -np.ones((k, 2)) if row[8] == -1.0 else pos_raw[:, :k].T.copy()


@pytest.mark.parametrize("route", ["depth1", "depth4", "own_inl", "own_table"])
def test_the_calibration_entry_matches_the_oracle(batch, routes, route):
    r = routes[route]
    cal = r["calls"][3] if route == "depth4" else r["cal"]             # (the details are those of the last call in flight)
    for i, nm in enumerate(batch["names"]):
        print(nm, r["det"]["counts"][i], cal["table"][i, 6:10])
        parity.compare_stream(batch["orc"][i], cal["table"][i], r["det"], i, _cut_pos_info(cal["table"][i], cal["pos_info_raw"][i]))


@pytest.mark.parametrize("route", ["scan", "scan_own_inl", "scan_own_table"])
def test_the_scanner_matches_the_oracle(batch, routes, route):
    got = routes[route]
    for i, nm in enumerate(batch["names"]):
        want = batch["scan"][i]
        w = _windows(want["coarse_pos"])
        assert int(got["counts"][i]) == len(w), nm
        parity.assert_positions(got["positions"][i, :len(w)], np.atleast_1d(want["coarse_pos"])[:len(w)], f"{nm}: scanner positions")
        assert np.allclose(got["pos_snr"][i, :len(w)], np.atleast_1d(want["coarse_snr"])[:len(w)], rtol=0, atol=parity.SNR_ATOL), nm
        assert got["num_hit"][i] == want["num_hit"], nm
        assert np.isclose(got["snr"][i], want["snr"], rtol=0, atol=parity.SNR_ATOL, equal_nan=True), nm


def _trim(a, counts):
    """entries behind a stream's count are not results (a replay leaves what its first pass wrote there)"""
    a = a.copy()
    for i, c in enumerate(counts):
        a[i, max(int(c), 0):] = 0.0
    return a


def test_every_route_gives_the_same_bits(batch, routes):
    """depth 4 against depth 1: table, pos_info, r_len, hit counts and coarse positions (the SNRs: the next test); the four calls
    in flight among themselves; the walk on its own spectra at depth 4 and with and without the in-kernel moving search; the
    scanner's two routes with the walk on its own spectra."""
    one, four = routes["depth1"], routes["depth4"]
    for k in range(4):
        c = four["calls"][k]
        assert np.array_equal(c["table"], one["cal"]["table"], equal_nan=True), k
        assert np.array_equal(c["r_len"], one["cal"]["r_len"]), k
        assert np.array_equal(c["pos_info_raw"], one["cal"]["pos_info_raw"], equal_nan=True), k
    nc = one["det"]["counts"][:, 0]
    for name in ("depth4", "own_inl", "own_table"):
        det = routes[name]["det"]
        assert np.array_equal(det["counts"], one["det"]["counts"]), name
        assert np.array_equal(_trim(det["coarse_pos"], nc), _trim(one["det"]["coarse_pos"], nc)), name
        assert np.array_equal(_trim(det["coarse_snr"], nc), _trim(four["det"]["coarse_snr"], nc), equal_nan=True), name
        assert np.allclose(_trim(det["coarse_snr"], nc), _trim(one["det"]["coarse_snr"], nc), rtol=0, atol=parity.SNR_ATOL, equal_nan=True), name
    for name in ("own_inl", "own_table"):
        assert np.array_equal(routes[name]["cal"]["table"], one["cal"]["table"], equal_nan=True), name
    a, b = routes["scan_own_inl"], routes["scan_own_table"]
    for key in ("snr", "num_hit", "counts"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
        assert np.allclose(a[key], routes["scan"][key], rtol=0, atol=parity.SNR_ATOL, equal_nan=True), key
    for key in ("positions", "pos_snr"):
        assert np.array_equal(_trim(a[key], a["counts"]), _trim(b[key], a["counts"]), equal_nan=True), key


def test_depth_4_reports_the_coarse_snrs_of_depth_1_bit_for_bit(batch, routes):
    """The SNR a hop reports is the value k_coarse_snr's table holds for its window, whichever way the hop was decided: depth 1
    reads it from the full table, the walk on its own spectra (depth 4, the contexts without the full table, the scanner's
    forms) evaluates that window once more with the table kernel's arithmetic behind the walk.  (The powers of the walk's direct
    DFTs, which decide, differ from the FFT's in the last places: reported from those, 15 of the 32 SNRs of these captures
    differed from depth 1's, by up to 3.7e-14 dB.)"""
    one = routes["depth1"]["det"]
    nc = one["counts"][:, 0]
    a = _trim(one["coarse_snr"], nc)
    for name in ("depth4", "own_inl", "own_table"):
        b = _trim(routes[name]["det"]["coarse_snr"], nc)
        fin = np.isfinite(a) & np.isfinite(b)
        print(name, "hops", int(np.sum(np.maximum(nc, 0))), "SNRs that differ", int(np.sum(a[fin] != b[fin])), "largest difference", float(np.max(np.abs(a[fin] - b[fin]))))
        assert np.array_equal(a, b, equal_nan=True), name
    for name in ("scan_own_inl", "scan_own_table"):
        for key in ("snr", "num_hit"):
            assert np.array_equal(routes[name][key], routes["scan"][key], equal_nan=True), (name, key)
        assert np.array_equal(_trim(routes[name]["pos_snr"], routes["scan"]["counts"]), _trim(routes["scan"]["pos_snr"], routes["scan"]["counts"]), equal_nan=True), name
