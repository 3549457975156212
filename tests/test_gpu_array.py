"""GPU tests of optimal combining (-m gpu): gsmcal_array_covariance_batch[_dev] (k_array_cov, k_array_cov_reduce) and
gsmcal_array_combine_batch[_dev] (k_array_combine) against the fp64 restatement in tests/array_ref.py, and the chain
covariance -> weights -> beam on the designed case and on three calibrated dongles of one transmission.

Bounds against the restatement, with their origin:
  covariance   every entry within (len + 8) 2^-53 sum_n (|Re x_i| + |Im x_i|)(|Re x_j| + |Im x_j|): the a-priori bound of an fp64 sum in
               any order, with or without fused multiply-adds; a dropped or doubled sample misses it by nine orders of magnitude
  beams        every sample within (G + 4) 2^-52 sum_g (|Re w| + |Im w|)(|Re x| + |Im x|)
  exact        conjugate symmetry, a +0 imaginary diagonal, an all-zero matrix at len = 0, bit equality of a window alone / in two
               lists / between two calls / between the host and _dev forms, and of a beam alone / among others / twice / both forms
  designed     weights within the bar of tests/test_array_cpu.py of the restatement's (same inputs, same maths: rounding only), the
               combined stream's measured SINR within 0.01 dB of the restatement's
Largest deviation / bound seen on an MI355X: see DESIGN.md section 21 (printed by the tests)."""
import ctypes as C

import numpy as np
import pytest

import array_ref as ref
from test_gpu_pair_align import same_bits, triple  # noqa: F401  (the calibrated triple: a fixture of that module)

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 5, 17, 64)
D = 70
worst = {}


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


@pytest.fixture(scope="module")
def data(g):
    """random rows, the window list of the shapes test and the rows per G (one index repeated from G = 2 on); built once"""
    chunk = g.COV_CHUNK
    assert chunk % 64 == 0
    stride = 3 * chunk + 200
    rng = np.random.Generator(np.random.Philox(key=[21, 70]))
    x = rng.standard_normal((D, stride)) + 1j * rng.standard_normal((D, stride))
    x *= np.exp(rng.uniform(-3.0, 3.0, (D, 1)))                    # rows of different power
    wins = []
    for ln in (0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 7):
        odd = 37 if 37 + ln <= stride else 1
        for start in (0, odd, stride - ln):                        # at 0, at an odd offset, ending exactly at stride (193 for the longest: odd)
            wins.append((start, ln))
    rows = {}
    for G in SIZES:
        r = rng.permutation(D)[:G]
        if G >= 2:
            r[-1] = r[0]                                           # a row named twice
        rows[G] = r.astype(np.int32)
    return {"x": x, "stride": stride, "chunk": chunk, "windows": np.array(wins, dtype=np.int64), "rows": rows,
            "d_x": None}


def dev_x(data):
    import torch
    if data["d_x"] is None:
        data["d_x"] = torch.from_numpy(data["x"]).to("cuda:0")
        torch.cuda.synchronize()
    return data["d_x"]


def cov_dev(g, ctx, data, rows, windows):
    import torch
    W, G = len(windows), len(rows)
    d_cov = torch.full((W, G, G), -7.0, dtype=torch.complex128, device="cuda:0")
    torch.cuda.synchronize()
    g.array_covariance_dev(dev_x(data).data_ptr(), data["stride"], D, rows, windows, d_cov.data_ptr(), ctx=ctx)
    ctx.sync()
    return d_cov.cpu().numpy()


def combine_dev(g, ctx, data, rows, weights, out_len):
    import torch
    B = np.atleast_2d(weights).shape[0]
    d_out = torch.full((B, out_len), -7.0, dtype=torch.complex128, device="cuda:0")
    torch.cuda.synchronize()
    g.array_combine_dev(dev_x(data).data_ptr(), data["stride"], D, rows, weights, out_len, d_out.data_ptr(), ctx=ctx)
    ctx.sync()
    return d_out.cpu().numpy()


def check_cov(got, x, rows, windows, what):
    want, bound = ref.array_covariance(x, rows, windows), ref.covariance_bound(x, rows, windows)
    assert got.shape == want.shape, (what, got.shape)
    dev = np.abs(got - want)
    m = bound > 0
    ratio = float(np.max(dev[m] / bound[m])) if m.any() else 0.0
    worst["covariance"] = max(worst.get("covariance", 0.0), ratio)
    assert np.all(dev <= bound), (what, ratio)
    # exact: Hermitian, the diagonal's imaginary part +0, len = 0 all zero
    assert np.array_equal(got, np.conj(np.swapaxes(got, 1, 2))), (what, "conjugate symmetry")
    di = np.diagonal(got, axis1=1, axis2=2).imag
    assert np.all(di == 0.0) and not np.signbit(di).any(), (what, "the diagonal's imaginary part is +0")
    for w, (_, ln) in enumerate(np.asarray(windows).reshape(-1, 2)):
        if ln == 0:
            assert not got[w].any(), (what, "len = 0")
    return ratio


@pytest.mark.parametrize("G", SIZES)
def test_covariance_against_the_restatement(g, ctx, data, G):
    x, rows, wins = data["x"], data["rows"][G], data["windows"]
    host = g.array_covariance(x, rows, wins)
    ratio = check_cov(host, x, rows, wins, f"host G {G}")
    dev = cov_dev(g, ctx, data, rows, wins)
    assert same_bits(dev, host), "host and _dev forms"
    assert same_bits(g.array_covariance(x, rows, wins), host), "two calls"
    # one window alone, and inside two other lists (reversed; between overlapping neighbours)
    rev = g.array_covariance(x, rows, wins[::-1])
    assert same_bits(rev, host[::-1])
    for k in (4, 10, 17, 22, 26):                                  # len 1 and 64 at an odd start, chunk - 1 ending at stride, chunk + 1, the longest
        alone = g.array_covariance(x, rows, wins[k:k + 1])
        assert same_bits(alone[0], host[k]), (G, k)
        start, ln = wins[k]
        around = np.array([[max(start - 5, 0), min(ln + 9, data["stride"] - max(start - 5, 0))], wins[k], [start, max(ln // 2, 0)], [0, data["stride"]]])
        among = g.array_covariance(x, rows, around)
        assert same_bits(among[1], host[k]), (G, k, "among overlapping windows")
        check_cov(among, x, rows, around, f"overlapping G {G} k {k}")
    print(f"G {G}: largest deviation / bound {ratio:.3g}; so far {worst}")


def test_covariance_of_256_windows_in_one_call(g, ctx, data):
    rng = np.random.Generator(np.random.Philox(key=[21, 256]))
    stride, chunk = data["stride"], data["chunk"]
    ln = rng.integers(0, 2 * chunk + 100, 256)
    ln[:4] = (0, stride, chunk, 1)
    start = (rng.uniform(0.0, 1.0, 256) * (stride - ln + 1)).astype(np.int64)
    wins = np.stack([start, ln], axis=1).astype(np.int64)
    assert np.all(wins[:, 0] + wins[:, 1] <= stride)
    rows = data["rows"][17]
    got = g.array_covariance(data["x"], rows, wins)
    check_cov(got, data["x"], rows, wins, "256 windows")
    assert same_bits(cov_dev(g, ctx, data, rows, wins), got)
    some = [1, 2, 77, 255]
    assert same_bits(g.array_covariance(data["x"], rows, wins[some]), got[some])
    with pytest.raises(g.GsmcalError, match="failed with -1 "):
        g.array_covariance(data["x"], rows, np.vstack([wins, wins[:1]]))      # 257


def test_nan_reaches_its_row_and_column_in_the_windows_that_cover_it(g, data):
    x = data["x"].copy()
    G = 17
    rows = data["rows"][G]                                         # rows[16] == rows[0]
    chunk = data["chunk"]
    hit, n0 = 5, 2 * chunk + 100
    x[rows[hit], n0] = complex(np.nan, 1.0)
    wins = np.array([[0, data["stride"]], [n0, 1], [n0 - 70, 71], [0, n0], [n0 + 1, 90], [n0 - chunk - 6, chunk + 100]], dtype=np.int64)
    covers = [True, True, True, False, False, True]
    got = g.array_covariance(x, rows, wins)
    touched = np.zeros((G, G), bool)
    touched[hit, :] = True
    touched[:, hit] = True
    for w, c in enumerate(covers):
        assert np.array_equal(np.isnan(got[w]), touched if c else np.zeros((G, G), bool)), w
    # the same with the repeated row: both of its places
    x = data["x"].copy()
    x[rows[0], 7] = complex(np.inf, 0.0)
    got = g.array_covariance(x, rows, [[0, 64], [8, 64]])
    touched = np.zeros((G, G), bool)
    touched[[0, 16], :] = True
    touched[:, [0, 16]] = True
    assert np.array_equal(~np.isfinite(got[0]), touched) and np.all(np.isfinite(got[1]))


def weights_for(G, B, seed):
    rng = np.random.Generator(np.random.Philox(key=[21, 1000 + seed]))
    return rng.standard_normal((B, G)) + 1j * rng.standard_normal((B, G))


@pytest.mark.parametrize("G", SIZES)
def test_combine_against_the_restatement(g, ctx, data, G):
    x, rows, stride = data["x"], data["rows"][G], data["stride"]
    w16 = weights_for(G, 16, G)
    for B in (1, 3, 16):
        w = w16[:B]
        for out_len in (1, 255, 256, 257, stride):
            got = g.array_combine(x, rows, w, out_len)
            want, bound = ref.array_combine(x, rows, w, out_len), ref.combine_bound(x, rows, w, out_len)
            assert got.shape == want.shape == (B, out_len)
            dev = np.abs(got - want)
            worst["combine"] = max(worst.get("combine", 0.0), float(np.max(dev / bound)))
            assert np.all(dev <= bound), (G, B, out_len, float(np.max(dev / bound)))
            if out_len in (257, stride):
                assert same_bits(combine_dev(g, ctx, data, rows, w, out_len), got), "host and _dev forms"
                assert same_bits(g.array_combine(x, rows, w, out_len), got), "two calls"
    # a beam alone, among three, among sixteen (and at another place of the list): the same bits
    full = g.array_combine(x, rows, w16)
    for b in (0, 2, 7, 15):
        assert same_bits(g.array_combine(x, rows, w16[b]), full[b]), (G, b)
        assert same_bits(g.array_combine(x, rows, w16[[15, b, 3]])[1], full[b]), (G, b)
        assert same_bits(g.array_combine(x, rows, w16[[b, 1]])[0], full[b]), (G, b)
    assert g.array_combine(x, rows, w16[0]).shape == (stride,)
    print(f"G {G}: largest deviation / bound so far {worst}")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_argument_errors_leave_the_outputs_untouched(g, ctx, data):
    """every GSMCAL_E_ARG case of both entry points, host and _dev form: -1, and not a byte of the output written"""
    import torch
    lib, stride = ctx.lib, data["stride"]
    x = np.ascontiguousarray(data["x"][:6])
    d_x = torch.from_numpy(x).to("cuda:0")
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_long)
    rows_ok, wins_ok, w_ok = np.array([0, 5, 2], dtype=np.int32), np.array([[0, 100], [stride - 10, 10]], dtype=np.int64), np.ones((2, 3), dtype=np.complex128)
    cov = np.full((2, 3, 3), -7.0, dtype=np.complex128)
    d_cov = torch.full((2, 3, 3), -7.0, dtype=torch.complex128, device="cuda:0")
    out = np.full((2, 50), -7.0, dtype=np.complex128)
    d_out = torch.full((2, 50), -7.0, dtype=torch.complex128, device="cuda:0")
    torch.cuda.synchronize()

    def cov_call(dev, xnull=False, onull=False, stride_=stride, d=6, rows=rows_ok, G=3, wins=wins_ok, W=2):
        rp = rows.ctypes.data_as(ip) if rows is not None else None
        wp = wins.ctypes.data_as(lp) if wins is not None else None
        if dev:
            return lib.gsmcal_array_covariance_batch_dev(ctx.h, None if xnull else C.c_void_p(d_x.data_ptr()), stride_, d, rp, G, wp, W,
                                                         None if onull else C.c_void_p(d_cov.data_ptr()))
        return lib.gsmcal_array_covariance_batch(ctx.h, None if xnull else _dp(x), stride_, d, rp, G, wp, W, None if onull else _dp(cov))

    def comb_call(dev, xnull=False, onull=False, stride_=stride, d=6, rows=rows_ok, G=3, w=w_ok, B=2, out_len=50):
        rp = rows.ctypes.data_as(ip) if rows is not None else None
        wp = _dp(w) if w is not None else None
        if dev:
            return lib.gsmcal_array_combine_batch_dev(ctx.h, None if xnull else C.c_void_p(d_x.data_ptr()), stride_, d, rp, G, wp, B, out_len,
                                                      None if onull else C.c_void_p(d_out.data_ptr()))
        return lib.gsmcal_array_combine_batch(ctx.h, None if xnull else _dp(x), stride_, d, rp, G, wp, B, out_len, None if onull else _dp(out))

    def w_(a):
        return np.array(a, dtype=np.int64)

    many_rows = np.zeros(65, dtype=np.int32)
    many_wins = np.tile(np.array([[0, 1]], dtype=np.int64), (257, 1))
    cov_bad = [dict(rows=np.array([0, 6, 2], dtype=np.int32)), dict(rows=np.array([0, -1, 2], dtype=np.int32)), dict(G=0), dict(rows=many_rows, G=65),
               dict(W=0), dict(wins=many_wins, W=257), dict(wins=w_([[-1, 5], [0, 1]])), dict(wins=w_([[0, -1], [0, 1]])),
               dict(wins=w_([[0, 1], [stride - 9, 10]])), dict(wins=w_([[stride + 1, 0], [0, 1]])), dict(wins=w_([[0, stride + 1], [0, 1]])),
               dict(xnull=True), dict(onull=True), dict(rows=None), dict(wins=None), dict(d=0), dict(stride_=0)]
    comb_bad = [dict(rows=np.array([0, 6, 2], dtype=np.int32)), dict(rows=np.array([-1, 1, 2], dtype=np.int32)), dict(G=0), dict(rows=many_rows, G=65),
                dict(B=0), dict(B=17), dict(out_len=0), dict(out_len=stride + 1), dict(out_len=-3), dict(xnull=True), dict(onull=True),
                dict(rows=None), dict(w=None), dict(d=0), dict(stride_=0)]
    for dev in (False, True):
        for kw in cov_bad:
            assert cov_call(dev, **kw) == -1, ("covariance", dev, kw)
        for kw in comb_bad:
            assert comb_call(dev, **kw) == -1, ("combine", dev, kw)
        assert lib.gsmcal_array_covariance_batch(None, _dp(x), stride, 6, rows_ok.ctypes.data_as(ip), 3, wins_ok.ctypes.data_as(lp), 2, _dp(cov)) == -1
        assert lib.gsmcal_array_combine_batch(None, _dp(x), stride, 6, rows_ok.ctypes.data_as(ip), 3, _dp(w_ok), 2, 50, _dp(out)) == -1
    ctx.sync()
    for buf in (cov, out, d_cov.cpu().numpy(), d_out.cpu().numpy()):
        assert np.all(buf == -7.0), "an output was written"
    # ... and the same calls with nothing wrong succeed (the limits themselves are inside)
    for dev in (False, True):
        assert cov_call(dev) == 0 and comb_call(dev) == 0
    ctx.sync()
    assert not np.any(cov == -7.0) and not np.any(out == -7.0) and not np.any(d_cov.cpu().numpy() == -7.0) and not np.any(d_out.cpu().numpy() == -7.0)
    assert g.array_covariance(x, np.zeros(64, dtype=np.int32), [[0, 3]]).shape == (1, 64, 64)
    assert g.array_combine(x, [1], np.ones((16, 1)), stride).shape == (16, stride)
    with pytest.raises(g.GsmcalError, match="failed with -1 "):
        g.array_combine(x, [1], np.ones((17, 1)))


def test_designed_case_end_to_end_on_the_device(g, ctx):
    import torch
    case = ref.designed_case(0)
    x, wins, s = case["x"], case["windows"], case["s"]
    n = x.shape[1]
    d_x = torch.from_numpy(x).to("cuda:0")
    d_cov = torch.zeros((2, 4, 4), dtype=torch.complex128, device="cuda:0")
    d_out = torch.zeros((2, n), dtype=torch.complex128, device="cuda:0")
    torch.cuda.synchronize()
    rows = [0, 1, 2, 3]
    g.array_covariance_dev(d_x.data_ptr(), n, 4, rows, wins, d_cov.data_ptr(), ctx=ctx)
    ctx.sync()                                                     # the one synchronisation: the weights are host arithmetic
    cov = d_cov.cpu().numpy()
    w, info = g.combine_weights(cov[0], cov[1], ref=0)
    assert info["status"] == 0
    g.array_combine_dev(d_x.data_ptr(), n, 4, rows, np.stack([w, ref.equal_gain_weights()]), n, d_out.data_ptr(), ctx=ctx)
    ctx.sync()
    y = d_out.cpu().numpy()
    # ---- the restatement on the same samples ----
    rcov = ref.array_covariance(x, rows, wins)
    want, winfo = ref.combine_weights(rcov[0], rcov[1], 0)
    tol = 100.0 * 4 * 2.0 ** -53 * np.linalg.cond(rcov[1]) / ((winfo["lambda_1"] - winfo["lambda_2"]) / winfo["lambda_1"])
    sin = ref.sin_angle(w, want)
    got_db, want_db = ref.measured_sinr_db(y[0, :ref.NWIN], s), ref.measured_sinr_db(ref.array_combine(x, rows, want)[0, :ref.NWIN], s)
    eg_db = ref.measured_sinr_db(y[1, :ref.NWIN], s)
    print(f"sin(angle to the restatement's weights) {sin:.3g} (bar {tol:.3g}); measured SINR {got_db:.4f} dB, restatement {want_db:.4f} dB, "
          f"equal gain {eg_db:.3f} dB, optimum {ref.optimum_sinr_db():.3f} dB")
    assert sin <= tol and abs(info["lambda_1"] - winfo["lambda_1"]) <= tol * winfo["lambda_1"]
    assert abs(got_db - want_db) <= 0.01
    assert ref.optimum_sinr_db() - ref.sinr_db(w) <= 0.1
    assert np.all(np.abs(y[0] - ref.array_combine(x, rows, w)[0]) <= ref.combine_bound(x, rows, w)[0])


def test_max_ratio_on_the_calibrated_triple(g, ctx, triple):  # noqa: F811
    out = triple["out"]
    r, r_len, pi = out["r_correct"], out["r_len"], out["pos_info_raw"]
    n = r.shape[1]
    sch = g.sch_decode_batch(r, r_len, pi, 8, triple["ts"])
    res = g.coherent_combine(r, r_len, pi, 8, sch, ref=0, weights="max_ratio", want_aligned=True)
    t = g.align_rows(res["info"])
    used = t["status"] == 0
    w = res["weights"]
    assert used.tolist() == [True] * 3 and w.shape == (3,) and np.all(np.isfinite(w[used]))
    assert abs(np.linalg.norm(w[used]) - 1.0) <= 1e-15 * 8 and w[0].imag == 0.0 and w[0].real >= 0.0
    assert res["cov"].shape == (3, 3) and np.array_equal(res["cov"], res["cov"].conj().T) and res["combined"].shape == (n,)
    print("weights: magnitudes", np.abs(w), "phases", np.angle(w))
    # every step against the restatement on the same aligned rows
    wins = g.burst_windows(pi[0], 8, res["info"])
    assert len(wins) >= 4 and np.all(wins[:, 1] == 148 * 8) and np.all(wins[:, 0] >= t["combined_first"]) and np.all(wins.sum(axis=1) <= t["combined_end"])
    rcov = ref.array_covariance(res["aligned"], [0, 1, 2], wins)
    bound = ref.covariance_bound(res["aligned"], [0, 1, 2], wins).sum(axis=0) + len(wins) * 2.0 ** -53 * np.abs(rcov).sum(axis=0)
    assert np.all(np.abs(res["cov"] - rcov.sum(axis=0)) <= bound)
    want, winfo = ref.combine_weights(res["cov"], None, 0)
    assert ref.sin_angle(w, want) <= 100.0 * 3 * 2.0 ** -53 / ((winfo["lambda_1"] - winfo["lambda_2"]) / winfo["lambda_1"])
    y = ref.array_combine(res["aligned"], [0, 1, 2], w)[0]
    assert np.all(np.abs(res["combined"] - y) <= ref.combine_bound(res["aligned"], [0, 1, 2], w)[0])
    # the combined stream decodes with the reference stream's pos_info, to what the reference stream itself carries
    one = g.sch_rows(g.sch_decode_batch(res["combined"][None, :], [t["combined_end"]], pi[:1], 8, triple["ts"]))
    own = g.sch_rows(sch[:1])
    assert one["status"][0] == 0 and own["status"][0] == 0
    assert one["bsic"][0] == own["bsic"][0] and one["fn_anchor"][0] == own["fn_anchor"][0]
    # weights=None: the bits of the chain spelled out as before this option existed
    plain = g.coherent_combine(r, r_len, pi, 8, sch, ref=0)
    assert "weights" not in plain and "cov" not in plain and "aligned" not in plain
    lag0 = g.pair_lag0(sch, [(0, 1), (0, 2)], 8)
    table = g.pair_coherence_batch(r, r_len, pi, 8, [(0, 1), (0, 2)], lag0, None, 0.5)
    params = np.vstack([[0.0, 0.0, 0.0, 0.0, 0.0, 1.0 / 3], g.pair_align_params(table, 8, 1.0 / 3, 0.5)])
    spelled = g.pair_align_batch(r, r_len, 8, [0, 1, 2], params, want_aligned=False)
    assert same_bits(plain["combined"], spelled["combined"]) and same_bits(plain["info"], spelled["info"]) and same_bits(plain["params"], params)
    assert same_bits(plain["pair_table"], table) and same_bits(res["params"], params) and same_bits(res["info"], spelled["info"])
