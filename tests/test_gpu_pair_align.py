"""GPU tests of pair_align (-m gpu): gsmcal_pair_align / gsmcal_pair_align_batch[_dev] (k_pair_align, k_pair_align_info) against
the fp64 restatement of the definition in tests/pair_align_ref.py, and the closed loop measure -> align -> measure on three
calibrated dongles of one transmission.

Bounds against the restatement, with their origin:
  statuses, first_valid, end_valid, num_valid, the sum's row, which samples are zero        identical (x is formed by the same
                       individually rounded operations on both sides, so floor(x) is the same number)
  each valid sample    1e-11 * sum_k |h_k| |s_k|: the 16-term tap sum rounds near 16 * 1.1e-16 of that, the taps differ by a few
                       1e-16 (sin pi mu and angle-addition constants against np.sinc and np.cos), and the de-rotation's argument
                       reaches ~1e4 rad at these sizes, where one ulp is 2e-12
  combined             1e-11 * sum_g |w_g| sum_k |h_k| |s_k|
  identity (integer delay, no drift, no carrier)     1e-15 * sum_k |h_k| |s_k|: mu = 0 selects the sample itself
  combined in reversed list order                    1e-14 * sum_g |w_g aligned_g|: the order of the sum is part of the definition
Before comparing, every case asserts on the restatement that no x sits within 1e-9 of an integer (a last-bit difference could
floor it the other way) -- but for rows with an integer delay and no drift, whose x is exact: a test fails rather than leave a
sample out.  Bars of the closed loop on the calibrated triple:
pair_align_ref.TRIPLE_AFTER (twice what the restatement gave on the oracle's r_correct).
Largest deviation / bound seen on an MI355X: see DESIGN.md section 20."""
import numpy as np
import pytest

import pair_align_ref as ref
import pair_coherence_ref as pc

pytestmark = pytest.mark.gpu

FC = pc.FC
worst = {}


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


def same_bits(a, b):
    a, b = (np.ascontiguousarray(v).view(np.float64).view(np.uint64) if np.iscomplexobj(v) else np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
            for v in (a, b))
    return a.shape == b.shape and np.array_equal(a, b)


def note(name, dev, scale, tol):
    m = scale > 0
    ratio = float(np.max(dev[m] / (tol * scale[m]))) if m.any() else 0.0
    worst[name] = max(worst.get(name, 0.0), ratio)
    return ratio


def compare(got, want, what, tol=1e-11):
    """a pair_align_batch result (dict with info and aligned and / or combined) against the restatement's"""
    assert ref.no_x_near_an_integer(want["x"][~want["exact"]]), (what, "an x within 1e-9 of an integer")
    assert np.array_equal(got["info"], want["info"]), (what, got["info"], want["info"])
    if "aligned" in got:
        a, w, sc = got["aligned"], want["aligned"], want["scale"]
        assert a.shape == w.shape, (what, a.shape, w.shape)
        assert np.array_equal(a == 0, sc == 0) and np.array_equal(w == 0, sc == 0), (what, "which samples are exactly zero")
        assert same_bits(a[sc == 0], np.zeros(int((sc == 0).sum()), dtype=np.complex128)), (what, "zeros are +0 + 0j")
        dev = np.abs(a - w)
        ratio = note("aligned", dev, sc, tol)
        assert np.all(dev <= tol * sc), (what, "aligned", ratio)
    if "combined" in got:
        dev = np.abs(got["combined"] - want["combined"])
        ratio = note("combined", dev, want["comb_scale"], tol)
        assert np.all(dev <= tol * want["comb_scale"]), (what, "combined", ratio)


def dev_form(g, ctx, r, r_len, ov, members, params, out_len, aligned=True, combined=True):
    import torch
    G = len(members)
    d_r, d_len = torch.from_numpy(np.ascontiguousarray(r)).to("cuda:0"), torch.from_numpy(np.asarray(r_len, dtype=np.int64)).to("cuda:0")
    d_info = torch.full((G + 1, g.ALIGN_INFO_COLS), -7.0, dtype=torch.float64, device="cuda:0")
    d_al = torch.full((G, out_len), -7.0, dtype=torch.complex128, device="cuda:0") if aligned else None
    d_cb = torch.full((out_len,), -7.0, dtype=torch.complex128, device="cuda:0") if combined else None
    torch.cuda.synchronize()
    g.pair_align_batch_dev(d_r.data_ptr(), r.shape[1], d_len.data_ptr(), r.shape[0], ov, members, params, out_len, d_info.data_ptr(),
                           d_aligned=d_al.data_ptr() if aligned else None, d_combined=d_cb.data_ptr() if combined else None, ctx=ctx)
    ctx.sync()
    out = {"info": d_info.cpu().numpy()}
    if aligned:
        out["aligned"] = d_al.cpu().numpy()
    if combined:
        out["combined"] = d_cb.cpu().numpy()
    return out


def parameter_sets(ov, n):
    """the rows of test 1: the measured one, the largest drifts either way (base moves 30 samples against n across the stream and
    across tile boundaries), a negative delay, a carrier of 3 kHz"""
    measured, _ = ref.measured_row(ov, weight=0.3)
    return np.array([measured,
                     [11.2503717, 1000.0, 300.0, 0.7, 0.0, 0.2],               # (delays chosen so that no x of a case is an integer)
                     [40.3137, -1000.0, -120.0, -2.1, n / 2.0, 0.15],
                     [-25.6, 3.7, 40.0, 0.1, 1000.0, 0.25],
                     [3.4, -0.9, 3000.0, 1.3, 333.0, 0.1]])


@pytest.mark.parametrize("ov", [2, 4, 8])
def test_parity_with_the_restatement_host_dev_and_single(g, ctx, ov):
    r, r_len, _, _ = pc.designed_streams(ov)
    n = r.shape[1]
    params = np.vstack([ref.ref_row(0.5), parameter_sets(ov, n)])
    members = [0, 1, 1, 0, 1, 1]
    for out_len in (n - 7, n + 300):                               # 7 493 at ov 2: no multiple of the tile; and longer than the streams
        want = ref.pair_align_batch(r, r_len, ov, members, params, out_len)
        assert want["info"][:6, 0].tolist() == [0.0] * 6 and np.all(want["info"][:6, 3] > n - 200)
        got = g.pair_align_batch(r, r_len, ov, members, params, out_len)
        compare(got, want, f"host ov {ov} out_len {out_len}")
        dev = dev_form(g, ctx, r, r_len, ov, members, params, out_len)
        compare(dev, want, f"dev ov {ov} out_len {out_len}")
        assert same_bits(dev["aligned"], got["aligned"]) and same_bits(dev["combined"], got["combined"]) and same_bits(dev["info"], got["info"])
        for q in (1, 2, 5):                                        # the single form: the same bits as the member's row
            out, info = g.pair_align(r[members[q], :r_len[members[q]]], ov, params[q], out_len)
            assert same_bits(out, got["aligned"][q]), (ov, out_len, q)
            assert [info[k] for k in g.ALIGN_INFO_FIELDS] == got["info"][q].tolist()
    assert "align member 0 stream" in g.last_call_report()
    # a shorter r_len than the row (the stride): len = min(r_len, stride) bounds the valid interval
    rl = np.array([n, n - 1000], dtype=np.int64)
    want = ref.pair_align_batch(r, rl, ov, [0, 1], params[:2], n)
    assert want["info"][1, 2] < n - 1000
    compare(g.pair_align_batch(r, rl, ov, [0, 1], params[:2], n), want, f"short r_len ov {ov}")
    print("largest deviation / bound so far:", {k: f"{v:.3g}" for k, v in worst.items()})


def test_identity_returns_the_samples(g):
    ov = 4
    r, r_len, _, _ = pc.designed_streams(ov)
    n = r.shape[1]
    for delay in (0, 9, -13):
        row = [float(delay), 0.0, 0.0, 0.0, 0.0, 1.0]
        want = ref.pair_align(r[1], n, ov, row, n)
        out, info = g.pair_align(r[1], ov, row, n)
        lo, hi = info["first_valid"], info["end_valid"]
        assert (info["status"], lo, hi) == (0, want["first_valid"], want["end_valid"]) == (0, max(7 - delay, 0), min(n, n - 8 - delay))
        shifted = r[1][lo + delay: hi + delay]
        assert np.all(np.abs(out[lo:hi] - shifted) <= 1e-15 * want["scale"][lo:hi])
        assert np.all(out[:lo] == 0) and np.all(out[hi:] == 0)


def test_bit_identity_of_rows_and_of_the_sum(g, ctx):
    ov = 4
    r2, l2, _, _ = pc.designed_streams(ov)
    n = r2.shape[1]
    rng = np.random.Generator(np.random.Philox(key=[20, 20]))
    other = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
    r = np.stack([other[0], r2[1], other[1], r2[0], other[2]])
    r_len = np.array([n, n, n - 50, n, n - 7], dtype=np.int64)
    sets = parameter_sets(ov, n)
    members, params = [3, 1, 0, 4, 1], np.vstack([ref.ref_row(0.2), sets[0], sets[2], sets[3], sets[1]])
    out_len = n - 3
    five = g.pair_align_batch(r, r_len, ov, members, params, out_len)
    compare(five, ref.pair_align_batch(r, r_len, ov, members, params, out_len), "five members")
    for q in range(5):                                             # alone (with and without the sum), and from the single call
        alone = g.pair_align_batch(r, r_len, ov, [members[q]], params[q:q + 1], out_len)
        assert same_bits(alone["aligned"][0], five["aligned"][q]) and same_bits(alone["info"][0], five["info"][q]), q
        bare = g.pair_align_batch(r, r_len, ov, [members[q]], params[q:q + 1], out_len, want_combined=False)
        assert "combined" not in bare and same_bits(bare["aligned"][0], five["aligned"][q]), q
        single, _ = g.pair_align(r[members[q], :r_len[members[q]]], ov, params[q], out_len)
        assert same_bits(single, five["aligned"][q]), q
    no_sum = g.pair_align_batch(r, r_len, ov, members, params, out_len, want_combined=False)
    assert same_bits(no_sum["aligned"], five["aligned"]) and same_bits(no_sum["info"][:5], five["info"][:5])
    only_sum = g.pair_align_batch(r, r_len, ov, members, params, out_len, want_aligned=False)
    assert "aligned" not in only_sum and same_bits(only_sum["combined"], five["combined"]) and same_bits(only_sum["info"], five["info"])
    again = g.pair_align_batch(r, r_len, ov, members, params, out_len)
    assert same_bits(again["aligned"], five["aligned"]) and same_bits(again["combined"], five["combined"]) and same_bits(again["info"], five["info"])
    dev = dev_form(g, ctx, r, r_len, ov, members, params, out_len)
    assert same_bits(dev["combined"], five["combined"]) and same_bits(dev["aligned"], five["aligned"]) and same_bits(dev["info"], five["info"])
    back = g.pair_align_batch(r, r_len, ov, members[::-1], params[::-1], out_len)
    assert same_bits(back["aligned"], five["aligned"][::-1]) and same_bits(back["info"][:5], five["info"][:5][::-1])
    scale = np.sum(np.abs(params[:, 5:6] * five["aligned"]), axis=0)
    assert np.all(np.abs(back["combined"] - five["combined"]) <= 1e-14 * scale)
    assert np.array_equal(back["info"][5, :3], five["info"][5, :3]) and abs(back["info"][5, 3] - five["info"][5, 3]) <= 1e-15


def test_exits(g):
    ov = 2
    r, r_len, _, _ = pc.designed_streams(ov)
    n = r.shape[1]
    good = parameter_sets(ov, n)[0]
    nan_row = g.pair_align_params(np.full(g.PAIR_COLS, np.nan), ov, weights=0.25)[0]          # a failed pair_coherence row passes through
    assert np.isnan(nan_row[:5]).all() and nan_row[5] == 0.25
    beyond = np.array([float(n), 0.0, 0.0, 0.0, 0.0, 0.25])
    members, params = [0, 1, 1, 1, 1], np.vstack([ref.ref_row(0.25), good, nan_row, good, beyond])
    rl = np.array([n, n], dtype=np.int64)
    gone = np.array([n, -1], dtype=np.int64)
    for lens, status in ((rl, [0.0, 0.0, 17.0, 0.0, 0.0]), (gone, [0.0, 10.0, 10.0, 10.0, 10.0])):
        want = ref.pair_align_batch(r, lens, ov, members, params, n)
        got = g.pair_align_batch(r, lens, ov, members, params, n)
        compare(got, want, f"exits {status}")
        t = g.align_rows(got["info"])
        assert t["status"].tolist() == status and t["members_used"] == status.count(0.0)
        for q, s in enumerate(status):
            if s != 0.0:
                assert not got["aligned"][q].any() and got["info"][q].tolist() == [s, 0.0, 0.0, 0.0]
    t = g.align_rows(g.pair_align_batch(r, rl, ov, members, params, n)["info"])
    assert t["num_valid"][4] == 0 and t["status"][4] == 0 and (t["combined_first"], t["combined_end"]) == (7, 7) and t["weight_sum"] == 0.25 + 0.3 + 0.3 + 0.25
    # the sum leaves the skipped member out: the same bits as the list without it
    a = g.pair_align_batch(r, rl, ov, members[:4], params[:4], n)
    b = g.pair_align_batch(r, rl, ov, [0, 1, 1], params[[0, 1, 3]], n)
    assert same_bits(a["combined"], b["combined"]) and g.align_rows(a["info"])["members_used"] == 3
    out, info = g.pair_align(-1, ov, good, 64)                                                 # the r = -1 sentinel: an empty stream
    assert info["status"] == g._lib.S_POST_NO_POS == 10 and not out.any()
    out, info = g.pair_align(r[1], ov, nan_row, 64)
    assert info["status"] == g.S_ALIGN_SKIPPED == 17 and not out.any()
    # arguments: decided before anything is enqueued
    ok = dict(ov=ov, members=[0, 1], params=np.vstack([ref.ref_row(0.5), good]), out_len=n)
    for kw, code in ((dict(members=[0, 2]), "-1"), (dict(members=[-1, 1]), "-1"), (dict(out_len=0), "-1"),
                     (dict(params=np.vstack([ref.ref_row(0.5), [0.0, 1000.5, 0.0, 0.0, 0.0, 0.5]])), "-1"),
                     (dict(params=np.vstack([ref.ref_row(0.5), [0.0, -1001.0, 0.0, 0.0, 0.0, 0.5]])), "-1"),
                     (dict(want_aligned=False, want_combined=False), "-1"), (dict(ov=3), "-6"), (dict(ov=1), "-6"), (dict(ov=16), "-6")):
        a = dict(ok, **kw)
        with pytest.raises(g.GsmcalError, match=f"failed with {code} "):
            g.pair_align_batch(r, rl, a["ov"], a["members"], a["params"], a["out_len"], want_aligned=a.get("want_aligned", True),
                               want_combined=a.get("want_combined", True))
    with pytest.raises(g.GsmcalError, match="failed with -6 "):
        g.pair_align(r[1], 3, good, 64)
    # 64 members pass, 65 are refused
    many = np.tile(good, (65, 1))
    many[:, 0] += 0.37 * np.arange(65)
    many[:, 5] = 1.0 / 64
    mem = [i & 1 for i in range(65)]
    want = ref.pair_align_batch(r, rl, ov, mem[:64], many[:64], 1000)
    compare(g.pair_align_batch(r, rl, ov, mem[:64], many[:64], 1000), want, "64 members")
    with pytest.raises(g.GsmcalError, match="failed with -1 "):
        g.pair_align_batch(r, rl, ov, mem, many, 1000)
    # |slope_ppm| = 1000 exactly is inside
    assert g.pair_align_batch(r, rl, ov, [1], [[0.0, -1000.0, 0.0, 0.0, 0.0, 1.0]], 100)["info"][0, 0] == 0


@pytest.fixture(scope="module")
def triple(g):
    """three dongles on one transmission, calibrated in one batch through a context of its own"""
    s = g.synth
    coef, ts = s.fir1(46, 200e3 / s.FS), s.sch_training_sequence()
    made = [s.make_stream(**pc.triple_stream_args(i)) for i in range(3)]
    raw = np.stack([m[0] for m in made])
    own = g.Context(0)
    out = g.calibrate_batch(raw, coef, ts, FC, want_r=True, ctx=own)
    own.close()
    assert out["table"][:, 9].tolist() == [0.0] * 3
    return {"raw": raw, "out": out, "coef": coef, "ts": ts}


def test_closed_loop_on_the_calibrated_triple(g, ctx, triple):
    import torch
    out = triple["out"]
    r, r_len, pi = out["r_correct"], out["r_len"], out["pos_info_raw"]
    n = r.shape[1]
    sch = g.sch_decode_batch(r, r_len, pi, 8, triple["ts"])
    res = g.coherent_combine(r, r_len, pi, 8, sch, ref=0, want_aligned=True)
    t = g.align_rows(res["info"])
    assert t["status"].tolist() == [0.0] * 3 and t["members_used"] == 3 and abs(t["weight_sum"] - 1.0) <= 1e-15
    assert res["members"].tolist() == [0, 1, 2] and res["params"].shape == (3, 6) and res["combined"].shape == (n,)
    assert same_bits(res["aligned"][0, 7:r_len[0] - 8], r[0, 7:r_len[0] - 8])                  # the reference stream passes unchanged
    before = g.pair_rows(res["pair_table"])
    c = pc.col
    # ---- every step against the restatement on the same r_correct ----
    lag0 = g.pair_lag0(sch, [(0, 1), (0, 2)], 8)
    for q, m in enumerate((1, 2)):
        want = ref.pair_align_params(pc.pair_coherence(r, r_len, pi, 8, 0, m, int(lag0[q]))["row"], 8, 0.5, 1.0 / 3)
        assert np.allclose(res["params"][q + 1], want, rtol=1e-7, atol=1e-7), (m, res["params"][q + 1], want)      # (pair_coherence's own bounds)
    compare({k: res[k] for k in ("info", "aligned", "combined")}, ref.pair_align_batch(r, r_len, 8, [0, 1, 2], res["params"], n), "triple")
    # ---- measured again: stream 0 against each aligned member at lag0 = 0 (an aligned row ends at its end_valid: zeros follow) ----
    r2 = np.stack([r[0], res["aligned"][1], res["aligned"][2]])
    l2 = np.array([r_len[0], t["end_valid"][1], t["end_valid"][2]], dtype=np.int64)
    after = g.pair_rows(g.pair_coherence_batch(r2, l2, pi, 8, [(0, 1), (0, 2)], 0))
    for q in range(2):
        print(f"member {q + 1}: delay0 {before['delay0'][q]:.4f} -> {after['delay0'][q]:+.4f}  carrier {before['rel_carrier_hz'][q]:.3f} -> {after['rel_carrier_hz'][q]:+.4f} Hz  "
              f"phase0 {before['phase0'][q]:.4f} -> {after['phase0'][q]:+.4f}  coherence {before['mean_coherence'][q]:.5f} -> {after['mean_coherence'][q]:.5f}  "
              f"ppm {before['rel_sampling_ppm'][q]:+.4f} -> {after['rel_sampling_ppm'][q]:+.4f}")
        assert after["status"][q] == 0
        assert after["mean_coherence"][q] >= before["mean_coherence"][q]
        assert abs(after["delay0"][q]) <= ref.TRIPLE_AFTER["delay0"]
        assert abs(after["rel_carrier_hz"][q]) <= ref.TRIPLE_AFTER["rel_carrier_hz"]
    # ---- the device chain: calibrate -> pair_coherence -> pair_align enqueued back to back.  The parameter rows are host arrays, so
    # the one synchronisation sits between pair_coherence_batch_dev and pair_align_batch_dev (its table is read there) ----
    D, raw = 3, triple["raw"]
    ns = raw.shape[1] // 2
    d_raw = torch.from_numpy(raw).to("cuda:0")
    b = {"table": torch.zeros((D, g.TABLE_COLS), dtype=torch.float64, device="cuda:0"),
         "pos": torch.zeros((D, 2, g.MAX_POS_ROWS), dtype=torch.float64, device="cuda:0"),
         "r": torch.zeros((D, ns), dtype=torch.complex128, device="cuda:0"),
         "len": torch.zeros(D, dtype=torch.int64, device="cuda:0"),
         "pair": torch.full((2, g.PAIR_COLS), -7.0, dtype=torch.float64, device="cuda:0"),
         "info": torch.full((4, g.ALIGN_INFO_COLS), -7.0, dtype=torch.float64, device="cuda:0"),
         "aligned": torch.full((3, ns), -7.0, dtype=torch.complex128, device="cuda:0"),
         "combined": torch.full((ns,), -7.0, dtype=torch.complex128, device="cuda:0")}
    torch.cuda.synchronize()
    g.calibrate_batch_dev(d_raw.data_ptr(), D, ns, triple["coef"], triple["ts"], FC, b["table"].data_ptr(), b["pos"].data_ptr(),
                          b["r"].data_ptr(), b["len"].data_ptr(), ctx=ctx)
    g.pair_coherence_batch_dev(b["r"].data_ptr(), ns, b["len"].data_ptr(), b["pos"].data_ptr(), D, 8, [(0, 1), (0, 2)], lag0, b["pair"].data_ptr(), ctx=ctx)
    ctx.sync()                                                     # the one synchronisation: the parameters pass through the host
    params = np.vstack([ref.ref_row(1.0 / 3), g.pair_align_params(b["pair"].cpu().numpy(), 8, 1.0 / 3)])
    g.pair_align_batch_dev(b["r"].data_ptr(), ns, b["len"].data_ptr(), D, 8, [0, 1, 2], params, ns, b["info"].data_ptr(),
                           d_aligned=b["aligned"].data_ptr(), d_combined=b["combined"].data_ptr(), ctx=ctx)
    ctx.sync()
    assert ns == n and same_bits(params, res["params"])
    assert same_bits(b["info"].cpu().numpy(), res["info"]) and same_bits(b["combined"].cpu().numpy(), res["combined"])
    assert same_bits(b["aligned"].cpu().numpy(), res["aligned"])
    print("largest deviation / bound:", {k: f"{v:.3g}" for k, v in worst.items()})
