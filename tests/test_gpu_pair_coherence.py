"""GPU tests of pair_coherence (-m gpu): gsmcal_pair_coherence / gsmcal_pair_coherence_batch[_dev] (k_pair_xcorr, k_pair_finish)
against the fp64 restatement of the definition in tests/pair_coherence_ref.py, against the planted values of the designed pair and
against the truth of three calibrated dongles of one transmission.

Bounds against the restatement, with their origin:
  evaluated, edge, used, the counts, status, m*, pos          identical
  each corr value      1e-12 * sqrt(Ea_k * Eb_mk): the Cauchy-Schwarz bound of the Ls-term sum times 1e-12 (the rounding bound of
                       such a sum is about Ls * 1.1e-16 = 3e-14 of it at Ls = 296)
  delay                1e-8 sample
  phase, phase0        1e-9 rad, compared modulo 2 pi
  freq, rel_carrier_hz, burst_carrier_hz      1e-6 Hz
  rel_sampling_ppm     1e-6
  coherence (per burst, mean, min)            1e-12
  delay_rms, phase_rms                        1e-9
  delay0               1e-8 sample (as delay)
Every comparison first asserts on the restatement that no decision sits on a tie: the relative gap between the two largest y >=
1e-6, the parabola's curvature >= 1e-4, |coherence - min_coherence| >= 1e-6.  A test fails rather than leave a burst out.  Rows of
the batch forms equal the single call bit for bit."""
import numpy as np
import pytest

import pair_coherence_ref as ref

pytestmark = pytest.mark.gpu

FC = ref.FC
NB = ref.MAX_PAIR_BURSTS
TOL = {"delay": 1e-8, "freq": 1e-6, "coherence": 1e-12, "delay0": 1e-8, "rel_sampling_ppm": 1e-6, "delay_rms": 1e-9,
       "rel_carrier_hz": 1e-6, "burst_carrier_hz": 1e-6, "phase_rms": 1e-9, "mean_coherence": 1e-12, "min_coherence_seen": 1e-12}
TOL_PHASE = {"phase": 1e-9, "phase0": 1e-9}
IDENTICAL_HEAD = ("status", "num_bursts", "num_eval", "num_used", "num_adjacent", "lag0", "max_lag")
worst = {}


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


def same_bits(a, b):
    a, b = (np.ascontiguousarray(v, dtype=np.float64).view(np.uint64) for v in (a, b))
    return a.shape == b.shape and np.array_equal(a, b)


def note(name, dev, tol):
    dev = float(np.max(dev)) if np.size(dev) else 0.0
    worst[name] = max(worst.get(name, 0.0), dev / tol)
    return dev


def compare(row, corr, want, what=""):
    """one pair: a row of the table (and its corr block) against the restatement"""
    assert ref.ties_ok(want), (what, want["gap"][want["evaluated"]], want["curvature"][want["evaluated"]], want["coh_margin"][want["evaluated"]])
    w, c = want["row"], ref.col
    for k in IDENTICAL_HEAD:
        assert row[c(k)] == w[c(k)], (what, k, row[c(k)], w[c(k)])
    ev, edge = want["evaluated"], want["edge"]
    inner = ev & ~edge
    pos = row[c("pos"): c("pos") + NB]
    assert np.array_equal(~np.isnan(pos), ev) and np.array_equal(pos[ev], w[c("pos"): c("pos") + NB][ev]), (what, "pos")
    e = row[c("edge"): c("edge") + NB]
    assert np.array_equal(e[ev], edge[ev].astype(float)) and np.isnan(e[~ev]).all(), (what, "edge")
    for k in ("delay", "phase", "freq", "coherence"):
        assert np.array_equal(~np.isnan(row[c(k): c(k) + NB]), inner), (what, k, "which bursts have a value")
    used = inner & (np.nan_to_num(row[c("coherence"): c("coherence") + NB], nan=-1.0) >= 0.5)      # (every case here runs at min_coherence 0.5)
    assert np.array_equal(used, want["used"]), (what, "used")
    # m*: the delay is lag0 + m* + the parabola's offset, |offset| <= 0.5 (and from the GPU's own correlations below)
    assert np.all(np.abs(row[c("delay"): c("delay") + NB][inner] - w[c("lag0")] - want["mstar"][inner]) <= 0.5 + 1e-8), (what, "m*")
    if corr is not None:
        assert corr.shape == want["corr"].shape, (corr.shape, want["corr"].shape)
        assert np.isnan(corr[~ev]).all() and not np.isnan(corr[ev]).any(), (what, "corr NaN pattern")
        scale = np.sqrt(want["ea"][ev][:, None, :] * want["eb"][ev])
        dev = np.abs(corr[ev] - want["corr"][ev]) / scale
        note("corr", dev, 1e-12)
        assert np.all(dev <= 1e-12), (what, "corr", dev.max())
        # ... and m* itself, from the GPU's own correlations
        y = np.sum(np.abs(corr[ev]) ** 2, axis=2)
        assert np.array_equal(np.argmax(y, axis=1) - want["M"], want["mstar"][ev]), (what, "m*")
    for k, tol in TOL.items():
        sl = slice(c(k), c(k) + NB) if k in ref.BURST else slice(c(k), c(k) + 1)
        a, b = row[sl], w[sl]
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, k, a[:4], b[:4])
        m = ~np.isnan(b)
        assert np.all(np.abs(a[m] - b[m]) <= tol), (what, k, note(k, np.abs(a[m] - b[m]), tol), tol)
        note(k, np.abs(a[m] - b[m]), tol)
    for k, tol in TOL_PHASE.items():
        sl = slice(c(k), c(k) + NB) if k in ref.BURST else slice(c(k), c(k) + 1)
        a, b = row[sl], w[sl]
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, k)
        m = ~np.isnan(b)
        dev = np.abs(ref.wrap(a[m] - b[m]))
        note(k, dev, tol)
        assert np.all(dev <= tol), (what, k, dev.max())


def single(g, r, r_len, pi, ov, a, b, lag0, M, want_corr=True, min_coherence=0.5):
    """gsmcal_pair_coherence on streams a and b of a batch-shaped input"""
    rows = int(np.max(np.nonzero(np.any(pi[a] != -1.0, axis=0))[0])) + 1
    return g.pair_coherence(r[a, :int(r_len[a])], r[b, :int(r_len[b])], pi[a][:, :rows].T, ov, lag0, M, min_coherence, want_corr=want_corr)


@pytest.mark.parametrize("ov", [2, 4, 8])
def test_designed_pair_single_batch_and_dev(g, ctx, ov):
    import torch
    r, r_len, pi, plant = ref.designed_streams(ov)
    bound = ref.designed_bounds(ov, plant)
    c = ref.col
    for M in (1, 3, 4 * ov):
        lag0 = 11 if M == 1 else 10                                     # M >= 3: the maximum one lag off the centre
        want = ref.pair_coherence(r, r_len, pi, ov, 0, 1, lag0, M)
        one = single(g, r, r_len, pi, ov, 0, 1, lag0, M)
        compare(one["row"], np.concatenate([one["corr"], np.full((NB - 3, 2 * M + 1, 4), np.nan + 1j * np.nan)]), want, f"single ov {ov} M {M}")
        assert one["status"] == 0 and one["num_used"] == 3 and one["delay"].shape == (3,) and one["corr"].shape == (3, 2 * M + 1, 4)
        res = g.pair_coherence_batch(r, r_len, pi, ov, [(0, 1)], lag0, M, want_corr=True)
        compare(res["table"][0], res["corr"][0], want, f"batch ov {ov} M {M}")
        assert same_bits(res["table"][0], one["row"]) and same_bits(res["corr"][0, :3].view(np.float64), one["corr"].view(np.float64))
        assert same_bits(g.pair_coherence_batch(r, r_len, pi, ov, [(0, 1)], lag0, M)[0], one["row"])      # without corr: the same row
        # ---- the device form ----
        d_r = torch.from_numpy(r).to("cuda:0")
        d_len, d_pos = torch.from_numpy(r_len).to("cuda:0"), torch.from_numpy(pi).to("cuda:0")
        d_out = torch.full((1, g.PAIR_COLS), -7.0, dtype=torch.float64, device="cuda:0")
        d_corr = torch.full((1, NB, 2 * M + 1, 4), -7.0, dtype=torch.complex128, device="cuda:0")
        torch.cuda.synchronize()
        g.pair_coherence_batch_dev(d_r.data_ptr(), r.shape[1], d_len.data_ptr(), d_pos.data_ptr(), 2, ov, [(0, 1)], [lag0], d_out.data_ptr(),
                                   max_lag=M, d_corr=d_corr.data_ptr(), ctx=ctx)
        ctx.sync()
        assert same_bits(d_out.cpu().numpy()[0], one["row"]) and same_bits(d_corr.cpu().numpy().view(np.float64), res["corr"].view(np.float64))
        # ---- what was planted (the bounds of tests/test_pair_coherence_cpu.py) ----
        row = one["row"]
        assert np.all(np.abs(one["delay"] - plant["delay"]) <= bound["delay"]) and abs(row[c("delay0")] - plant["delay"]) <= bound["delay"]
        assert np.all(np.abs(ref.wrap(one["phase"] - plant["phase"])) <= bound["phase"])
        assert np.all(np.abs(one["freq"] - plant["freq"]) <= bound["freq"]) and abs(row[c("rel_carrier_hz")] - plant["freq"]) <= bound["rel_carrier_hz"]
        assert abs(ref.wrap(row[c("phase0")] - plant["phase"][0])) <= bound["phase"] and abs(row[c("rel_sampling_ppm")]) <= bound["rel_sampling_ppm"]
    assert "pair delay" in g.last_call_report() and "pair coherence mean" in g.last_call_report()
    print("largest deviation / tolerance so far:", {k: f"{v:.3g}" for k, v in worst.items()})


def test_window_boundaries_exactly_at_and_one_past_each_limit(g):
    """Evaluated iff 0 <= p, p + L <= len_a, 0 <= p + lag0 - M, p + lag0 + M + L <= len_b: one burst on each limit, one a sample past it."""
    ov, M = 2, 3
    L = 148 * ov
    r, _, _, _ = ref.designed_streams(ov)
    n = r.shape[1]
    cases = []                                                           # (pos, lag0, len_a, len_b, evaluated)
    cases += [(1.0, M, n, n, True), (0.0, M + 1, n, n, False)]          # 0 <= p (p = 0 / -1, the b window kept inside)
    cases += [(201.0, 11, 200 + L, n, True), (201.0, 11, 200 + L - 1, n, False)]                       # p + L <= len_a
    cases += [(201.0, M - 200, n, n, True), (201.0, M - 201, n, n, False)]                             # 0 <= p + lag0 - M
    cases += [(201.0, 11, n, 200 + 11 + M + L, True), (201.0, 11, n, 200 + 11 + M + L - 1, False)]     # p + lag0 + M + L <= len_b
    for pos, lag0, len_a, len_b, evaluated in cases:
        pi = np.stack([ref.raw_table([(pos, 1.0), (2701.0, 2.0), (5201.0, 2.0)]), ref.raw_table([])])
        rl = np.array([len_a, len_b], dtype=np.int64)
        want = ref.pair_coherence(r, rl, pi, ov, 0, 1, lag0, M)
        assert want["evaluated"][0] == evaluated, (pos, lag0, len_a, len_b)
        res = g.pair_coherence_batch(r, rl, pi, ov, [(0, 1)], lag0, M, want_corr=True)
        t = g.pair_rows(res["table"])
        assert (not np.isnan(t["pos"][0, 0])) == evaluated, (pos, lag0, len_a, len_b, t["pos"][0, :3])
        assert np.isnan(res["corr"][0, 0]).all() == (not evaluated)
        if not evaluated:
            assert all(np.isnan(t[k][0, 0]) for k in ref.BURST)
        compare(res["table"][0], res["corr"][0], want, f"boundary {pos} {lag0} {len_a} {len_b}")


def test_exits(g):
    ov, M = 2, 3
    r, r_len, pi, _ = ref.designed_streams(ov)
    c = ref.col
    # lag0 off by M + 2: every maximum at the edge of the lag range
    want = ref.pair_coherence(r, r_len, pi, ov, 0, 1, 11 + M + 2, M)
    res = g.pair_coherence_batch(r, r_len, pi, ov, [(0, 1)], 11 + M + 2, M, want_corr=True)
    compare(res["table"][0], res["corr"][0], want, "all edge")
    t = g.pair_rows(res["table"])
    assert t["status"][0] == g.S_PAIR_FEW == 16 and t["edge"][0, :3].tolist() == [1.0, 1.0, 1.0] and t["num_used"][0] == 0
    assert np.isnan(res["table"][0, c("delay0"): c("max_lag")]).all()
    one = single(g, r, r_len, pi, ov, 0, 1, 11 + M + 2, M)
    assert one["status"] == 16 and same_bits(one["row"], res["table"][0]) and "Fewer than two bursts" in g.last_call_report()
    # a stream with r_len = -1 (as a or as b), and one with an all -1 table: nothing to read
    gone = np.array([r_len[0], -1], dtype=np.int64)
    res = g.pair_coherence_batch(r, gone, pi, ov, [(0, 1), (1, 0), (0, 0)], [11, -11, 0], M, want_corr=True)
    t = g.pair_rows(res["table"])
    assert t["status"].tolist() == [10.0, 10.0, 0.0] and t["num_bursts"].tolist() == [0.0, 0.0, 3.0]
    res2 = g.pair_coherence_batch(r, r_len, pi, ov, [(1, 0)], -11, M, want_corr=True)                    # b's table is all -1
    for row, corr, a, b, rl in ((res["table"][0], res["corr"][0], 0, 1, gone), (res["table"][1], res["corr"][1], 1, 0, gone),
                                (res2["table"][0], res2["corr"][0], 1, 0, r_len)):
        compare(row, corr, ref.pair_coherence(r, rl, pi, ov, a, b, int(row[c("lag0")]), M), "no pos")
        assert row[0] == 10 and np.isnan(row[c("delay0"): c("max_lag")]).all() and np.isnan(row[16:]).all() and np.isnan(corr).all()
    assert g.pair_coherence(r[1], r[0], -np.ones((1, 2)), ov, -11, M) is None
    # 120 rows pass, 121 are more than the row holds
    for count, status in ((120, 0.0), (121, -4.0)):
        many = np.stack([ref.raw_table([(201.0 + 40 * i, 1.0 + (i & 1)) for i in range(count)]), pi[1]])
        want = ref.pair_coherence(r, r_len, many, ov, 0, 1, 11, M)
        res = g.pair_coherence_batch(r, r_len, many, ov, [(0, 1)], 11, M, want_corr=True)
        assert res["table"][0, 0] == status and res["table"][0, 1] == count
        compare(res["table"][0], res["corr"][0], want, f"{count} rows")
        assert (want["evaluated"].sum() == 120) == (count == 120)
    # arguments
    for kw, code in ((dict(pairs=[(0, 2)]), "-1"), (dict(pairs=[(-1, 0)]), "-1"), (dict(ov=3), "-6"), (dict(M=4 * ov + 1), "-1"),
                     (dict(M=-1), "-1"), (dict(minc=1.5), "-1")):
        with pytest.raises(g.GsmcalError, match=f"failed with {code} "):
            g.pair_coherence_batch(r, r_len, pi, kw.get("ov", ov), kw.get("pairs", [(0, 1)]), 11, kw.get("M", M), kw.get("minc", 0.5))
    with pytest.raises(g.GsmcalError, match="failed with -6 "):
        g.pair_coherence(r[0], r[1], pi[0][:, :4].T, 3, 11, 3)
    # a stream against itself (tests/pair_coherence_ref.py periodic_self_stream: y is even in the lag there)
    rs, ls, ps = ref.periodic_self_stream(ov)
    want = ref.pair_coherence(rs, ls, ps, ov, 0, 0, 0, M)
    res = g.pair_coherence_batch(rs, ls, ps, ov, [(0, 0)], 0, M, want_corr=True)
    compare(res["table"][0], res["corr"][0], want, "self")
    t = g.pair_rows(res["table"])
    print("self pair: |coherence - 1|", np.abs(t["coherence"][0, :3] - 1).max(), "|delay|", np.abs(t["delay"][0, :3]).max(), "|phase|",
          np.abs(t["phase"][0, :3]).max())
    assert t["status"][0] == 0 and t["num_used"][0] == 3
    assert np.all(np.abs(t["coherence"][0, :3] - 1) <= 1e-12) and np.all(np.abs(t["delay"][0, :3]) <= 1e-8) and np.all(np.abs(t["phase"][0, :3]) <= 1e-9)
    assert abs(t["delay0"][0]) <= 1e-8 and abs(t["phase0"][0]) <= 1e-9


def test_a_row_is_the_same_bits_wherever_it_is_computed(g):
    """The row of pair (a, b) in a batch of 1 pair and of 6, in either list order, among d = 2 and d = 5 streams, from the single
    call, and from call to call."""
    ov, M = 4, 5
    r, r_len, pi, _ = ref.designed_streams(ov)
    one = single(g, r, r_len, pi, ov, 0, 1, 11, M)
    alone = g.pair_coherence_batch(r, r_len, pi, ov, [(0, 1)], 11, M, want_corr=True)
    assert same_bits(alone["table"][0], one["row"]) and one["status"] == 0
    # five streams: the pair's two in places 3 and 1, three others around them (one of them empty)
    rng = np.random.Generator(np.random.Philox(key=[7, 7]))
    other = rng.standard_normal((3, r.shape[1])) + 1j * rng.standard_normal((3, r.shape[1]))
    r5 = np.stack([other[0], r[1], other[1], r[0], other[2]])
    l5 = np.array([r.shape[1], r_len[1], -1, r_len[0], r.shape[1] - 7], dtype=np.int64)
    p5 = np.stack([pi[0], pi[1], pi[0], pi[0], ref.raw_table([(301.0, 2.0), (5301.0, 1.0)])])
    pairs = [(0, 4), (3, 1), (4, 0), (3, 3), (2, 3), (1, 3)]
    lags = [0, 11, 0, 0, 0, -11]
    six = g.pair_coherence_batch(r5, l5, p5, ov, pairs, lags, M, want_corr=True)
    assert same_bits(six["table"][1], one["row"]) and same_bits(six["corr"][1].view(np.float64), alone["corr"][0].view(np.float64))
    back = g.pair_coherence_batch(r5, l5, p5, ov, pairs[::-1], lags[::-1], M, want_corr=True)
    assert same_bits(back["table"], six["table"][::-1]) and same_bits(back["corr"].view(np.float64), six["corr"][::-1].view(np.float64))
    again = g.pair_coherence_batch(r5, l5, p5, ov, pairs, lags, M, want_corr=True)
    assert same_bits(again["table"], six["table"]) and same_bits(again["corr"].view(np.float64), six["corr"].view(np.float64))
    assert g.pair_rows(six["table"])["status"].tolist() == [16.0, 0.0, 16.0, 0.0, 10.0, 10.0]
    # every row against the restatement (noise against noise included: a maximum somewhere, coherence far below the threshold)
    for q, (a, b) in enumerate(pairs):
        compare(six["table"][q], six["corr"][q], ref.pair_coherence(r5, l5, p5, ov, a, b, lags[q], M), f"pair {a}->{b} of six")


@pytest.fixture(scope="module")
def triple(g):
    """three dongles on one transmission, calibrated in one batch through a context of its own"""
    s = g.synth
    coef, ts = s.fir1(46, 200e3 / s.FS), s.sch_training_sequence()
    made = [s.make_stream(**ref.triple_stream_args(i)) for i in range(3)]
    raw = np.stack([m[0] for m in made])
    own = g.Context(0)
    out = g.calibrate_batch(raw, coef, ts, FC, want_r=True, ctx=own)
    own.close()
    assert out["table"][:, 9].tolist() == [0.0] * 3
    return {"raw": raw, "out": out, "truth": [m[1] for m in made], "coef": coef, "ts": ts}


def test_calibrated_triple_all_six_ordered_pairs(g, ctx, triple):
    import torch
    out, truth = triple["out"], triple["truth"]
    r, r_len, pi = out["r_correct"], out["r_len"], out["pos_info_raw"]
    sch = g.sch_decode_batch(r, r_len, pi, 8, triple["ts"])
    assert g.sch_rows(sch)["status"].tolist() == [0.0] * 3
    pairs = [(a, b) for a in range(3) for b in range(3) if a != b]
    lag0 = g.pair_lag0(sch, pairs, 8)
    # the SCH positions are whole samples: the difference of two of them sits within two samples of what was planted
    assert all(abs(int(lag0[q]) - ref.triple_planted_delay(a, b)) <= 2.0 for q, (a, b) in enumerate(pairs)), lag0
    assert all(lag0[pairs.index((b, a))] == -lag0[q] for q, (a, b) in enumerate(pairs))
    res = g.pair_coherence_batch(r, r_len, pi, 8, pairs, lag0, want_corr=True)
    t = g.pair_rows(res["table"])
    c = ref.col
    # ---- against the restatement run on the GPU's own r_correct ----
    for q, (a, b) in enumerate(pairs):
        compare(res["table"][q], res["corr"][q], ref.pair_coherence(r, r_len, pi, 8, a, b, int(lag0[q])), f"triple {a}->{b}")
    # ---- against the truth, at the bars of tests/test_pair_coherence_cpu.py ----
    table = out["table"]
    for q, (a, b) in enumerate(pairs):
        planted = ref.triple_planted_delay(a, b)
        left_hz, left_ppm = ref.triple_left_by_the_chain(truth, table[:, 4], table[:, 5], a, b)
        ev = ~np.isnan(t["pos"][q])
        rev = pairs.index((b, a))
        print(f"pair {a}->{b}: eval {int(t['num_eval'][q])} used {int(t['num_used'][q])} coherence {t['coherence'][q][ev].min():.4f} delay0 {t['delay0'][q]:.4f} "
              f"planted {planted} carrier {t['rel_carrier_hz'][q]:.3f} left {left_hz:.3f} ppm {t['rel_sampling_ppm'][q]:.4f} left {left_ppm:.4f}")
        assert t["status"][q] == 0 and t["num_eval"][q] >= 16 and t["num_used"][q] == t["num_eval"][q] and not np.any(t["edge"][q][ev] == 1.0)
        assert np.all(t["coherence"][q][ev] >= 0.9)
        assert abs(t["delay0"][q] - planted) <= 0.15
        assert abs(t["rel_carrier_hz"][q] - left_hz) <= 6.0
        assert abs(t["rel_sampling_ppm"][q] - left_ppm) <= 0.1
        assert abs(t["delay0"][rev] + t["delay0"][q]) <= 0.02 and abs(t["rel_carrier_hz"][rev] + t["rel_carrier_hz"][q]) <= 0.5
    # ---- the device form enqueued behind calibrate_batch_dev, no synchronisation in between ----
    D, n = triple["raw"].shape[0], triple["raw"].shape[1] // 2
    d_raw = torch.from_numpy(triple["raw"]).to("cuda:0")
    b = {"table": torch.zeros((D, g.TABLE_COLS), dtype=torch.float64, device="cuda:0"),
         "pos": torch.zeros((D, 2, g.MAX_POS_ROWS), dtype=torch.float64, device="cuda:0"),
         "r": torch.zeros((D, n), dtype=torch.complex128, device="cuda:0"),
         "len": torch.zeros(D, dtype=torch.int64, device="cuda:0"),
         "pair": torch.full((len(pairs), g.PAIR_COLS), -7.0, dtype=torch.float64, device="cuda:0")}
    torch.cuda.synchronize()
    g.calibrate_batch_dev(d_raw.data_ptr(), D, n, triple["coef"], triple["ts"], FC, b["table"].data_ptr(), b["pos"].data_ptr(),
                          b["r"].data_ptr(), b["len"].data_ptr(), ctx=ctx)
    g.pair_coherence_batch_dev(b["r"].data_ptr(), n, b["len"].data_ptr(), b["pos"].data_ptr(), D, 8, pairs, lag0, b["pair"].data_ptr(), ctx=ctx)
    ctx.sync()
    assert same_bits(b["pair"].cpu().numpy(), res["table"])
    print("largest deviation / tolerance:", {k: f"{v:.3g}" for k, v in worst.items()})
