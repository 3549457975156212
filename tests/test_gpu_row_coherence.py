"""GPU tests of row_coherence (-m gpu): gsmcal_row_coherence_batch[_resident] (k_row_xcorr, k_row_finish) against the fp64 restatement
of the definition in tests/row_coherence_ref.py, against pair_coherence_batch on the designed GSM streams (the correlations bit for
bit), the bit equalities include/gsmcal.h promises, the discipline of DESIGN.md section 22 (guard bands, call history, refusals with
the outputs untouched), and the closed loop make_wideband -> apply_calibration_resident -> row_coherence_resident ->
apply_params_refine -> apply_calibration_resident -> row_coherence_resident -> array_covariance_dev on the device.

Bounds against the restatement, with their origin:
  evaluated, edge, used, the counts, status, m*, start, the echoed arguments        identical
  each corr value      (Ls + 8) 2^-53 sum_n (|Re b| + |Im b|)(|Re a| + |Im a|) over the segment: the a-priori rounding bound of an
                       Ls-term sum of products in any order (the bound tests/test_gpu_array.py uses)
  every other column   tests/test_gpu_pair_coherence.py's TOL / TOL_PHASE times max(1, Ls / 296): those bars were set at Ls <= 296, and
                       the rounding of an Ls-term sum grows with Ls
Every comparison first asserts on the restatement that no decision sits on a tie (row_coherence_ref.ties_ok); a test fails rather
than leave a window out."""
import ctypes as C

import numpy as np
import pytest

import apply_ref as ar
import pair_coherence_ref as pcr
import row_coherence_ref as rr
from test_gpu_pair_coherence import TOL as PAIR_TOL, TOL_PHASE as PAIR_TOL_PHASE

pytestmark = pytest.mark.gpu

SENT = -7.0
NW = rr.MAX_ROW_WINDOWS
RENAMED = {"burst_carrier_hz": "window_carrier_hz"}
TOL = {RENAMED.get(k, k): v for k, v in PAIR_TOL.items()}
TOL_PHASE = dict(PAIR_TOL_PHASE)
IDENTICAL_HEAD = ("status", "num_windows", "num_eval", "num_used", "num_adjacent", "lag0", "max_lag", "win_len", "sample_rate", "min_coherence", "max_gap")
worst = {}


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


def same_bits(a, b):
    a, b = (np.ascontiguousarray(v).view(np.uint64) for v in (a, b))
    return a.shape == b.shape and np.array_equal(a, b)


def note(name, dev, tol):
    dev = float(np.max(dev)) if np.size(dev) else 0.0
    worst[name] = max(worst.get(name, 0.0), dev / tol)
    return dev


def compare(row, corr, want, what=""):
    """one pair: a row of the table (and its corr block) against the restatement"""
    ev, edge = want["evaluated"], want["edge"]
    assert rr.ties_ok(want), (what, want["gap"][ev], want["curvature"][ev], want["coh_margin"][ev])
    w, c, W, Ls = want["row"], rr.col, len(ev), want["Ls"]
    grow = max(1.0, Ls / 296.0)
    for k in IDENTICAL_HEAD:
        assert row[c(k)] == w[c(k)], (what, k, row[c(k)], w[c(k)])
    inner = ev & ~edge
    for k in rr.WINDOW:
        assert np.isnan(row[c(k) + W: c(k) + NW]).all(), (what, k, "NaN at and beyond W")
    st = row[c("start"): c("start") + W]
    assert np.array_equal(~np.isnan(st), ev) and np.array_equal(st[ev], w[c("start"): c("start") + W][ev]), (what, "start")
    e = row[c("edge"): c("edge") + W]
    assert np.array_equal(e[ev], edge[ev].astype(float)) and np.isnan(e[~ev]).all(), (what, "edge")
    coh = row[c("coherence"): c("coherence") + W]
    for k in ("delay", "phase", "freq"):
        assert np.array_equal(~np.isnan(row[c(k): c(k) + W]), inner), (what, k, "which windows have a value")
    assert not np.any(~np.isnan(coh) & ~inner), (what, "coherence outside the inner windows")
    used = inner & (np.nan_to_num(coh, nan=-1.0) >= w[c("min_coherence")])
    assert np.array_equal(used, want["used"]), (what, "used")
    assert np.all(np.abs(row[c("delay"): c("delay") + W][inner] - w[c("lag0")] - want["mstar"][inner]) <= 0.5 + 1e-8 * grow), (what, "m*")
    if corr is not None:
        assert corr.shape == want["corr"].shape, (corr.shape, want["corr"].shape)
        assert np.isnan(corr[~ev]).all() and not np.isnan(corr[ev]).any(), (what, "corr NaN pattern")
        bound = (Ls + 8) * 2.0 ** -53 * want["babs"][ev]
        dev = np.maximum(np.abs(corr[ev].real - want["corr"][ev].real), np.abs(corr[ev].imag - want["corr"][ev].imag))
        ok = dev <= bound
        worst["corr"] = max(worst.get("corr", 0.0), float(np.max(dev[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0)
        assert np.all(ok), (what, "corr", float(np.max(dev / np.maximum(bound, 1e-300))))
        y = np.sum(np.abs(corr[ev]) ** 2, axis=2)
        assert np.array_equal(np.argmax(y, axis=1) - want["M"], want["mstar"][ev]), (what, "m* of the GPU's own correlations")
    for tols, phase in ((TOL, False), (TOL_PHASE, True)):
        for k, tol in tols.items():
            tol = tol * grow
            sl = slice(c(k), c(k) + W) if k in rr.WINDOW else slice(c(k), c(k) + 1)
            a, b = row[sl], w[sl]
            assert np.array_equal(np.isnan(a), np.isnan(b)), (what, k, a[:4], b[:4])
            m = ~np.isnan(b)
            dev = np.abs(rr.wrap(a[m] - b[m])) if phase else np.abs(a[m] - b[m])
            note(k, dev, tol)
            assert np.all(dev <= tol), (what, k, float(np.max(dev)), tol)


class Resident:
    """One call of the resident form with out and corr between guard bands of `pad` sentinel values and x uploaded once."""

    def __init__(self, g, ctx, x, P, W, M, want_corr=True, pad=9):
        import torch
        self.g, self.ctx, self.pad, self.P, self.W, self.M = g, ctx, pad, int(P), int(W), int(M)
        self.x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.complex128)
        self.d, self.stride = self.x.shape
        self.d_x = torch.from_numpy(self.x).to("cuda:0")
        self.nc = self.P * self.W * (2 * self.M + 1) * 4
        self.d_out = torch.full((2 * pad + self.P * g.ROW_COLS,), SENT, dtype=torch.float64, device="cuda:0")
        self.d_corr = torch.full((2 * (2 * pad + self.nc),), SENT, dtype=torch.float64, device="cuda:0") if want_corr else None
        torch.cuda.synchronize()

    def call(self, pairs, lag0, starts, win_len, fs, min_coh=0.5, max_gap=None, valid=None, raw=None):
        """raw: arguments of the C call that replace the ones built here (a NULL pointer, a count, a ctypes array)"""
        lp, ip = self.g._lib.c_long_p, self.g._lib.c_int_p
        pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        lg = np.ascontiguousarray(np.broadcast_to(np.asarray(lag0, dtype=np.int32).ravel(), (len(pr),)))
        st = np.ascontiguousarray(np.asarray(starts, dtype=np.int64).ravel())
        va = None if valid is None else np.ascontiguousarray(np.asarray(valid, dtype=np.int64).reshape(-1, 2))
        a = dict(d_x=self.d_x.data_ptr(), stride=self.stride, d=self.d, valid=va.ctypes.data_as(lp) if va is not None else None,
                 pairs=pr.ctypes.data_as(ip), lag0=lg.ctypes.data_as(ip), P=len(pr), starts=st.ctypes.data_as(lp), W=len(st), win_len=win_len, M=self.M,
                 min_coh=min_coh, max_gap=8.0 * win_len if max_gap is None else max_gap, fs=fs, d_out=self.d_out.data_ptr() + 8 * self.pad,
                 d_corr=self.d_corr.data_ptr() + 16 * self.pad if self.d_corr is not None else 0)
        a.update(raw or {})
        rc = self.ctx.lib.gsmcal_row_coherence_batch_resident(
            self.ctx.h, C.c_void_p(a["d_x"]), int(a["stride"]), int(a["d"]), a["valid"], a["pairs"], a["lag0"], int(a["P"]), a["starts"], int(a["W"]),
            int(a["win_len"]), int(a["M"]), float(a["min_coh"]), float(a["max_gap"]), float(a["fs"]), C.c_void_p(a["d_out"]),
            C.c_void_p(a["d_corr"]) if a["d_corr"] else None)
        self.ctx.sync()
        return rc

    def read(self):
        """-> (table (P, ROW_COLS), corr (P, W, 2M+1, 4) or None) after asserting that nothing else was written and x is unchanged"""
        o, p = self.d_out.cpu().numpy(), self.pad
        assert np.all(o[:p] == SENT) and np.all(o[p + self.P * self.g.ROW_COLS:] == SENT), "the doubles around out"
        corr = None
        if self.d_corr is not None:
            cc = self.d_corr.cpu().numpy()
            assert np.all(cc[:2 * p] == SENT) and np.all(cc[2 * p + 2 * self.nc:] == SENT), "the doubles around corr"
            corr = cc[2 * p: 2 * p + 2 * self.nc].copy().view(np.complex128).reshape(self.P, self.W, 2 * self.M + 1, 4)
        assert same_bits(self.d_x.cpu().numpy().view(np.float64), self.x.view(np.float64)), "x"
        return o[p: p + self.P * self.g.ROW_COLS].reshape(self.P, -1).copy(), corr

    def untouched(self):
        return bool(np.all(self.d_out.cpu().numpy() == SENT) and (self.d_corr is None or np.all(self.d_corr.cpu().numpy() == SENT)))


def resident(g, ctx, x, pairs, lag0, starts, win_len, fs, M, want_corr=True, **kw):
    r = Resident(g, ctx, x, len(pairs), len(starts), M, want_corr)
    assert r.call(pairs, lag0, starts, win_len, fs, **kw) == 0, ctx.lib.gsmcal_last_error(ctx.h)
    return r.read()


N_ROW, FS, PLANT_D = 70000, 2.4e6, 11.25


@pytest.fixture(scope="module")
def rows():
    """a (row 0), b = a delayed by 11.25 samples, turned and with noise (row 1), an all-zero row (2), noise (3)"""
    a, b, plant = rr.designed_rows(N_ROW, PLANT_D, 0.7, 300.0, FS, 20261021)
    rng = np.random.Generator(np.random.Philox(key=[24, 1]))
    return np.stack([a, b, np.zeros(N_ROW, dtype=np.complex128), rng.standard_normal(N_ROW) + 1j * rng.standard_normal(N_ROW)])


def spread(W, win_len, lo=100):
    """W ascending starts whose windows (and 80 samples of lag on either side) lie inside a row of N_ROW"""
    step = max(1, min(4 * (win_len // 4) + 13, (N_ROW - lo - win_len - 100) // max(W, 1)))
    return [lo + step * j for j in range(W)]


# (win_len, M, W, lag0): Ls = 4, 4, 512, 513, 1025, 1537 -- each side of a chunk boundary of the sums; every M, W and lag0 the
# definition names at least once; M = 64 at every Ls that takes another number of tiles
SHAPES = [(16, 1, 1, 11), (16, 7, 2, 11), (16, 64, 128, 0), (16, 16, 64, 3), (19, 8, 63, -3), (19, 15, 65, 11), (19, 63, 127, 11),
          (2048, 16, 127, 11), (2048, 17, 2, 0), (2048, 64, 5, 11), (2052, 32, 65, 11), (2052, 1, 1, 11), (2052, 7, 64, 3),
          (4100, 64, 9, 11), (4100, 15, 63, -3), (4100, 8, 128, 11), (6151, 63, 7, 11), (6151, 17, 2, 11), (6151, 32, 1, 0)]


@pytest.mark.parametrize("win_len,M,W,lag0", SHAPES)
def test_parity_with_the_restatement(g, ctx, rows, win_len, M, W, lag0):
    starts = spread(W, win_len)
    want = rr.row_coherence(rows, 0, 1, lag0, starts, win_len, FS, M)
    assert want["evaluated"].all()
    table, corr = resident(g, ctx, rows, [(0, 1)], lag0, starts, win_len, FS, M)
    compare(table[0], corr[0], want, f"win_len {win_len} M {M} W {W} lag0 {lag0}")
    if lag0 == 11 and M >= 2 and win_len >= 2048:
        assert table[0, 0] == (0 if W >= 2 else 16) and table[0, rr.col("num_used")] == W
        if W >= 2:
            assert abs(table[0, rr.col("delay0")] - PLANT_D) <= 0.1 and abs(table[0, rr.col("rel_carrier_hz")] - 300.0) <= 5.0
    host = g.row_coherence(rows, [(0, 1)], starts, win_len, FS, lag0=lag0, max_lag=M, want_corr=True, ctx=ctx)
    assert same_bits(host["table"], table) and same_bits(host["corr"].view(np.float64), corr.view(np.float64))
    print("largest deviation / bound so far:", {k: f"{v:.3g}" for k, v in worst.items()})


@pytest.mark.parametrize("M", [2, 16, 64])
def test_the_maximum_inside_and_on_each_edge_of_the_lag_range(g, ctx, rows, M):
    win_len, starts = 2052, spread(4, 2052, lo=200)
    for lag0, mstar, edge in ((11 - (M - 1), M - 1, False), (11 + (M - 1), -(M - 1), False), (11 - M, M, True), (11 + M, -M, True)):
        want = rr.row_coherence(rows, 0, 1, lag0, starts, win_len, FS, M)
        assert np.all(want["mstar"] == mstar) and np.all(want["edge"] == edge), (lag0, want["mstar"])
        table, corr = resident(g, ctx, rows, [(0, 1)], lag0, starts, win_len, FS, M)
        compare(table[0], corr[0], want, f"M {M} lag0 {lag0}")
        assert table[0, 0] == (16 if edge else 0) and table[0, rr.col("num_used")] == (0 if edge else 4)
        if edge:
            assert np.isnan(table[0, rr.col("delay0"): rr.col("max_lag")]).all()


def test_each_of_the_four_inequalities_met_and_one_sample_short(g, ctx, rows):
    win_len, M, lag0 = 2052, 7, 11                                   # Ls = 513: 2052 samples are used
    L4, n = 2052, N_ROW
    # (valid or None, start, evaluated)
    cases = [(None, n - L4 - lag0 - M, True), (None, n - L4 - lag0 - M + 1, False)]                       # p + lag0 + M + 4 Ls <= stride
    cases += [([[500, n], [0, n]], 500, True), ([[501, n], [0, n]], 500, False)]                          # first_a <= p
    cases += [(None, 0, True)]                                       # first_a <= p with valid NULL: p = 0 (a negative start is refused)
    cases += [([[0, 500 + L4], [0, n]], 500, True), ([[0, 500 + L4 - 1], [0, n]], 500, False)]            # p + 4 Ls <= end_a
    cases += [([[0, n], [500 + lag0 - M, n]], 500, True), ([[0, n], [500 + lag0 - M + 1, n]], 500, False)]                  # first_b <= p + lag0 - M
    cases += [([[0, n], [0, 500 + lag0 + M + L4]], 500, True), ([[0, n], [0, 500 + lag0 + M + L4 - 1]], 500, False)]        # ... <= end_b
    for valid, p, ev in cases:
        starts, at = [p], 0
        valid = valid if valid is None else valid + [[0, n], [0, 0]]          # (one interval per row of x)
        want = rr.row_coherence(rows, 0, 1, lag0, starts, win_len, FS, M, valid=valid)
        assert want["evaluated"][at] == ev, (valid, p)
        table, corr = resident(g, ctx, rows, [(0, 1)], lag0, starts, win_len, FS, M, valid=valid)
        compare(table[0], corr[0], want, f"valid {valid} start {p}")
        assert np.isnan(corr[0, at]).all() == (not ev) and np.isnan(table[0, rr.col("start") + at]) == (not ev)
    # lag0 negative: b's window starts before a's; 0 <= p + lag0 - M with valid NULL
    for p, ev in ((M + 5, True), (M + 4, False)):
        want = rr.row_coherence(rows, 1, 0, -5, [p, 30000], win_len, FS, M)
        assert want["evaluated"].tolist() == [ev, True]
        table, corr = resident(g, ctx, rows, [(1, 0)], -5, [p, 30000], win_len, FS, M)
        compare(table[0], corr[0], want, f"start {p} lag0 -5")
    # a's own limit with valid NULL: p + 4 Ls <= stride (lag0 + M <= 0 keeps b inside)
    for p, ev in ((n - L4, True), (n - L4 + 1, False)):
        want = rr.row_coherence(rows, 1, 0, -11, [30000, p], win_len, FS, M)
        assert want["evaluated"].tolist() == [True, ev]
        table, corr = resident(g, ctx, rows, [(1, 0)], -11, [30000, p], win_len, FS, M)
        compare(table[0], corr[0], want, f"start {p} lag0 -11")


def test_self_pair_zero_row_and_fewer_than_two_used(g, ctx, rows):
    win_len, M = 2048, 8
    starts = spread(5, win_len)
    pairs = [(0, 0), (0, 2), (2, 0), (2, 2), (0, 3)]
    table, corr = resident(g, ctx, rows, pairs, 0, starts, win_len, FS, M)
    for q, (a, b) in enumerate(pairs):
        compare(table[q], corr[q], rr.row_coherence(rows, a, b, 0, starts, win_len, FS, M), f"pair {a}->{b}")
    t = g.row_rows(table)
    assert t["status"].tolist() == [0.0, 16.0, 16.0, 16.0, 16.0] and t["num_eval"].tolist() == [5.0] * 5
    assert np.all(np.abs(t["coherence"][0, :5] - 1) <= 1e-12) and np.all(np.abs(t["delay"][0, :5]) <= 1e-2) and np.all(np.abs(t["phase"][0, :5]) <= 1e-9)
    # an all-zero row: every correlation an exact zero, the first lag is the maximum (an edge), coherence NaN, not used
    for q in (1, 2, 3):
        assert not corr[q].any() and t["edge"][q, :5].tolist() == [1.0] * 5 and np.isnan(t["coherence"][q, :5]).all() and t["num_used"][q] == 0
        assert np.isnan(table[q, rr.col("delay0"): rr.col("max_lag")]).all()
    assert t["num_used"][4] == 0 and not np.any(t["coherence"][4, :5] >= 0.2)                              # noise: far below the threshold
    # one used window of two (the other past b's valid end); min_coherence 1: none used
    one, _ = resident(g, ctx, rows, [(0, 1)], 11, [100, 60000], 2048, FS, 16, valid=[[0, N_ROW], [0, 50000], [0, N_ROW], [0, N_ROW]])
    assert one[0, 0] == 16 and one[0, rr.col("num_eval")] == 1 and one[0, rr.col("num_used")] == 1 and np.isnan(one[0, rr.col("delay0")])
    none, _ = resident(g, ctx, rows, [(0, 1)], 11, starts, 2048, FS, 16, min_coh=1.0)
    assert none[0, 0] == 16 and none[0, rr.col("num_eval")] == 5 and none[0, rr.col("num_used")] == 0 and none[0, rr.col("min_coherence")] == 1.0


@pytest.mark.parametrize("ov", [2, 4, 8])
def test_correlations_equal_pair_coherence_bit_for_bit(g, ctx, ov):
    """win_len = 148 ov: one chunk per segment, k_pair_xcorr's own order of the sums"""
    r, r_len, pi, _ = pcr.designed_streams(ov)
    frame, fs = 1250 * ov, pcr.fs_of(ov)
    starts = [200, 200 + frame, 200 + 2 * frame]
    for M in (1, 3, 4 * ov):
        lag0 = 11 if M == 1 else 10
        pair = g.pair_coherence_batch(r, r_len, pi, ov, [(0, 1)], lag0, M, want_corr=True, ctx=ctx)
        table, corr = resident(g, ctx, r, [(0, 1)], lag0, starts, 148 * ov, fs, M, max_gap=1875.0 * ov)
        assert same_bits(corr[0].view(np.float64), pair["corr"][0, :3].view(np.float64)), (ov, M)
        compare(table[0], corr[0], rr.row_coherence(r, 0, 1, lag0, starts, 148 * ov, fs, M, 0.5, 1875.0 * ov), f"ov {ov} M {M}")
        # the other columns: within the bars (fp contraction may differ between the two finishing kernels)
        p, t = pair["table"][0], table[0]
        for k, tol in list(PAIR_TOL.items()) + list(PAIR_TOL_PHASE.items()):
            mine = RENAMED.get(k, k)
            width = 3 if k in pcr.BURST else 1
            a, b = t[rr.col(mine): rr.col(mine) + width], p[pcr.col(k): pcr.col(k) + width]
            assert np.array_equal(np.isnan(a), np.isnan(b)), (k, a, b)
            dev = np.abs(rr.wrap(a - b)) if k in PAIR_TOL_PHASE else np.abs(a - b)
            assert np.all(dev[~np.isnan(b)] <= tol), (ov, M, k, a, b)
        assert t[0] == p[0] and np.array_equal(t[2:6], p[2:6]) and np.array_equal(t[rr.col("edge"): rr.col("edge") + 3], p[pcr.col("edge"): pcr.col("edge") + 3])


def test_a_row_is_the_same_bits_wherever_it_is_computed(g, ctx, rows):
    win_len, M = 4100, 17
    starts = spread(6, win_len)
    alone, alone_corr = resident(g, ctx, rows, [(0, 1)], 11, starts, win_len, FS, M)
    assert alone[0, 0] == 0
    pairs, lags = [(0, 3), (0, 1), (1, 0), (0, 1), (2, 2), (3, 1)], [0, 11, -11, 11, 0, 5]
    six, six_corr = resident(g, ctx, rows, pairs, lags, starts, win_len, FS, M)
    for q in (1, 3):                                                 # among others, and listed twice
        assert same_bits(six[q], alone[0]) and same_bits(six_corr[q].view(np.float64), alone_corr[0].view(np.float64))
    back, back_corr = resident(g, ctx, rows, pairs[::-1], lags[::-1], starts, win_len, FS, M)
    assert same_bits(back, six[::-1]) and same_bits(back_corr.view(np.float64), six_corr[::-1].view(np.float64))
    # twice in a row through the same buffers; without corr; the host form; other rows around the pair's two
    r = Resident(g, ctx, rows, 6, len(starts), M)
    for _ in range(2):
        assert r.call(pairs, lags, starts, win_len, FS) == 0
        again, again_corr = r.read()
        assert same_bits(again, six) and same_bits(again_corr.view(np.float64), six_corr.view(np.float64))
    bare, none = resident(g, ctx, rows, pairs, lags, starts, win_len, FS, M, want_corr=False)
    assert none is None and same_bits(bare, six)
    host = g.row_coherence(rows, pairs, starts, win_len, FS, lag0=lags, max_lag=M, want_corr=True, ctx=ctx)
    assert same_bits(host["table"], six) and same_bits(host["corr"].view(np.float64), six_corr.view(np.float64))
    assert same_bits(g.row_coherence(rows, pairs, starts, win_len, FS, lag0=lags, max_lag=M, ctx=ctx), six)
    moved, moved_corr = resident(g, ctx, rows[[3, 1, 2, 0]], [(3, 1)], 11, starts, win_len, FS, M)
    assert same_bits(moved[0], alone[0]) and same_bits(moved_corr.view(np.float64), alone_corr.view(np.float64))
    for q, (a, b) in enumerate(pairs):
        compare(six[q], six_corr[q], rr.row_coherence(rows, a, b, lags[q], starts, win_len, FS, M), f"pair {a}->{b} of six")


def test_call_history_leaves_no_trace(g, ctx, rows):
    """A, B, A with every argument array of B another size and content; a refused call between two good ones"""
    a_args = dict(pairs=[(0, 1), (1, 0)], lag0=[11, -11], starts=spread(3, 2052), win_len=2052, fs=FS)
    b_args = dict(pairs=[(3, 0)], lag0=[2], starts=spread(100, 19), win_len=19, fs=2.0e6, min_coh=0.3, max_gap=5.0, valid=[[7, 60000], [0, N_ROW], [0, 9], [50, N_ROW]])
    ra, rb = Resident(g, ctx, rows, 2, 3, 9), Resident(g, ctx, rows[[3, 2, 1, 0]], 1, 100, 40)
    assert ra.call(**a_args) == 0
    first = ra.read()
    assert rb.call(**b_args) == 0
    tb, cb = rb.read()
    compare(tb[0], cb[0], rr.row_coherence(rows[[3, 2, 1, 0]], 3, 0, 2, b_args["starts"], 19, 2.0e6, 40, 0.3, 5.0, b_args["valid"]), "B")
    ra2 = Resident(g, ctx, rows, 2, 3, 9)
    assert ra2.call(**a_args) == 0
    second = ra2.read()
    assert same_bits(second[0], first[0]) and same_bits(second[1].view(np.float64), first[1].view(np.float64))
    refused = Resident(g, ctx, rows, 2, 3, 9)
    assert refused.call(**dict(a_args, starts=[5, 5, 9])) == rr.E_ARG and refused.untouched()
    ra3 = Resident(g, ctx, rows, 2, 3, 9)
    assert ra3.call(**a_args) == 0
    third = ra3.read()
    assert same_bits(third[0], first[0]) and same_bits(third[1].view(np.float64), first[1].view(np.float64))
    for q, (a, b) in enumerate(a_args["pairs"]):
        compare(first[0][q], first[1][q], rr.row_coherence(rows, a, b, a_args["lag0"][q], a_args["starts"], 2052, FS, 9), "A")


def test_refusals_leave_the_outputs_untouched(g, ctx, rows):
    lp, ip = g._lib.c_long_p, g._lib.c_int_p
    starts = spread(3, 2052)
    good = dict(pairs=[(0, 1), (1, 0)], lag0=[11, -11], starts=starts, win_len=2052, fs=FS)
    bad_pairs = [np.array(p, dtype=np.int32) for p in ([[0, 4], [1, 0]], [[0, 1], [-1, 0]])]
    bad_starts = [np.array(s, dtype=np.int64) for s in ([-1, 5, 9], [5, 5, 9], [9, 5, 20])]
    bad_valid = [np.array(v, dtype=np.int64) for v in ([[-1, 9], [0, 9], [0, 9], [0, 9]], [[0, N_ROW + 1], [0, 9], [0, 9], [0, 9]], [[0, 9], [0, 9], [10, 9], [0, 9]])]
    cases = [("d_x NULL", dict(d_x=0)), ("pairs NULL", dict(pairs=None)), ("lag0 NULL", dict(lag0=None)), ("starts NULL", dict(starts=None)),
             ("d_out NULL", dict(d_out=0)), ("d 0", dict(d=0)), ("P 0", dict(P=0)), ("P -1", dict(P=-1)), ("W 0", dict(W=0)), ("W 129", dict(W=129)),
             ("stride 0", dict(stride=0)), ("win_len 15", dict(win_len=15)), ("win_len 65537", dict(win_len=65537)), ("M 0", dict(M=0)),
             ("M 65", dict(M=65)), ("fs 0", dict(fs=0.0)), ("fs < 0", dict(fs=-1.0)), ("fs inf", dict(fs=np.inf)), ("fs nan", dict(fs=np.nan)),
             ("min_coherence -0.1", dict(min_coh=-0.1)), ("min_coherence 1.5", dict(min_coh=1.5)), ("min_coherence nan", dict(min_coh=np.nan)),
             ("max_gap -1", dict(max_gap=-1.0)), ("max_gap nan", dict(max_gap=np.nan))]
    cases += [(f"pair {p.tolist()}", dict(pairs=p.ctypes.data_as(ip))) for p in bad_pairs]
    cases += [(f"starts {s.tolist()}", dict(starts=s.ctypes.data_as(lp))) for s in bad_starts]
    cases += [(f"valid {v.tolist()}", dict(valid=v.ctypes.data_as(lp))) for v in bad_valid]
    r = Resident(g, ctx, rows, 2, 3, 9)
    for what, kw in cases:
        named = {k: kw[k] for k in ("min_coh", "max_gap") if k in kw}
        assert r.call(good["pairs"], good["lag0"], good["starts"], good["win_len"], good["fs"], raw=kw, **named) == rr.E_ARG, what
        assert r.untouched(), what
    assert b"strictly ascending" in ctx.lib.gsmcal_last_error(ctx.h) or b"valid interval" in ctx.lib.gsmcal_last_error(ctx.h)
    # the edges are inside
    assert Resident(g, ctx, rows, 1, 1, 64).call([(0, 1)], 11, [100], 65536, FS, min_coh=0.0, max_gap=0.0) == 0
    assert Resident(g, ctx, rows, 1, 128, 1).call([(3, 3)], 0, list(range(128)), 16, FS, min_coh=1.0, valid=[[0, 0], [0, N_ROW], [5, 5], [0, N_ROW]]) == 0
    # the host form: the same refusals, its outputs untouched
    dp = g._lib.c_double_p
    out = np.full((2, g.ROW_COLS), SENT)
    corr = np.full((2, 3, 19, 4), SENT + 1j * SENT)
    x = np.ascontiguousarray(rows)
    pr, lg, st = np.array(good["pairs"], dtype=np.int32), np.array(good["lag0"], dtype=np.int32), np.array(starts, dtype=np.int64)

    def host(x_p=x.view(np.float64).ctypes.data_as(dp), stride=N_ROW, d=4, valid=None, pairs=pr.ctypes.data_as(ip), lag0=lg.ctypes.data_as(ip), P=2,
             starts_p=st.ctypes.data_as(lp), W=3, win_len=2052, M=9, min_coh=0.5, max_gap=1e4, fs=FS, out_p=out.ctypes.data_as(dp),
             corr_p=corr.view(np.float64).ctypes.data_as(dp)):
        return ctx.lib.gsmcal_row_coherence_batch(ctx.h, x_p, stride, d, valid, pairs, lag0, P, starts_p, W, win_len, M, min_coh, max_gap, fs, out_p, corr_p)
    for what, kw in (("x NULL", dict(x_p=None)), ("pairs NULL", dict(pairs=None)), ("lag0 NULL", dict(lag0=None)), ("starts NULL", dict(starts_p=None)),
                     ("out NULL", dict(out_p=None)), ("d 0", dict(d=0)), ("P 0", dict(P=0)), ("W 129", dict(W=129)), ("stride 0", dict(stride=0)),
                     ("win_len 15", dict(win_len=15)), ("M 65", dict(M=65)), ("fs nan", dict(fs=np.nan)), ("min_coherence", dict(min_coh=1.5)),
                     ("max_gap", dict(max_gap=-1.0)), ("pair", dict(pairs=bad_pairs[0].ctypes.data_as(ip))),
                     ("starts", dict(starts_p=bad_starts[1].ctypes.data_as(lp))), ("valid", dict(valid=bad_valid[2].ctypes.data_as(lp)))):
        assert host(**kw) == rr.E_ARG, what
        assert np.all(out == SENT) and np.all(corr == SENT + 1j * SENT), what
    assert host() == 0
    want = resident(g, ctx, rows, good["pairs"], good["lag0"], starts, 2052, FS, 9, max_gap=1e4)
    assert same_bits(out, want[0]) and same_bits(corr.view(np.float64), want[1].view(np.float64))
    with pytest.raises(g.GsmcalError, match="failed with -1 "):
        g.row_coherence(rows, [(0, 4)], starts, 2052, FS, ctx=ctx)
    with pytest.raises(ValueError):
        g.row_coherence(rows, [(0, 1)], starts, 2052, FS, valid=[[0, 9]], ctx=ctx)


def test_closed_loop_on_the_device(g, ctx):
    """three retuned dongles on one wideband transmission: the first pass leaves start offsets, a few hundred Hz and the tuners'
    phases between them; one refinement from the measured rows puts dongles 1 and 2 on dongle 0's time base, carrier and phase."""
    import torch
    raw, params = rr.loop_captures(g.synth)
    D, n, fs = 3, rr.LOOP_N, rr.LOOP_FS
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_out = [torch.full((D, n), SENT, dtype=torch.complex128, device="cuda:0") for _ in range(2)]
    d_info = [torch.full((D, g.APPLY_INFO_COLS), SENT, dtype=torch.float64, device="cuda:0") for _ in range(2)]
    d_tab = [torch.full((3, g.ROW_COLS), SENT, dtype=torch.float64, device="cuda:0") for _ in range(2)]
    d_cov = torch.full((len(rr.LOOP_STARTS), 3, 3), SENT, dtype=torch.complex128, device="cuda:0")
    torch.cuda.synchronize()
    tables, outs, infos, plist = [], [], [], [params]
    for i in range(2):
        g.apply_calibration_resident(d_raw.data_ptr(), D, n, plist[i], fs, n, n, d_out[i].data_ptr(), d_info[i].data_ptr(), ctx=ctx)
        ctx.sync()                                                   # (the valid intervals pass through the host)
        infos.append(d_info[i].cpu().numpy())
        g.row_coherence_resident(d_out[i].data_ptr(), n, D, rr.LOOP_PAIRS, rr.LOOP_STARTS, rr.LOOP_WIN, fs, d_tab[i].data_ptr(), lag0=rr.LOOP_LAG0,
                                 max_lag=rr.LOOP_M, valid=g.valid_of(infos[i]), ctx=ctx)
        if i == 1:
            g.array_covariance_dev(d_out[1].data_ptr(), n, D, [0, 1, 2], [(s, 4 * (rr.LOOP_WIN // 4)) for s in rr.LOOP_STARTS], d_cov.data_ptr(), ctx=ctx)
        ctx.sync()
        tables.append(d_tab[i].cpu().numpy())
        outs.append(d_out[i].cpu().numpy())
        if i == 0:
            refined = g.apply_params_refine(tables[0], params)
            refined[0] = params[0]                                   # the reference keeps its row
            want = np.stack([params[0]] + [rr.apply_params_refine(tables[0][b], params[b])[1] for b in (1, 2)])
            assert same_bits(refined, want)
            plist.append(refined)
    first, second = rr.loop_figures(tables[0]), rr.loop_figures(tables[1])
    print("after pass 1:", first)
    print("after one refinement:", second, "bars:", rr.LOOP_BARS)
    assert not rr.within_bars(first) and first["rel_carrier_hz"] >= 150.0
    assert rr.within_bars(second), (second, rr.LOOP_BARS)
    # every table within the parity bars of the restatement run on the GPU's own rows
    for i in range(2):
        for q, (a, b) in enumerate(rr.LOOP_PAIRS):
            want = rr.row_coherence(outs[i], a, b, rr.LOOP_LAG0[b], rr.LOOP_STARTS, rr.LOOP_WIN, fs, rr.LOOP_M, 0.5, None, infos[i][:, 1:3].astype(np.int64))
            compare(tables[i][q], None, want, f"pass {i + 1} pair {a}->{b}")
    # array_covariance takes the refined rows: in phase with the reference, as coherent as the restatement says
    cov = d_cov.cpu().numpy().sum(axis=0)
    L = 4 * (rr.LOOP_WIN // 4)
    seg = np.stack([np.concatenate([outs[1][i, s:s + L] for s in rr.LOOP_STARTS]) for i in range(3)])
    for m in (1, 2):
        rho = abs(cov[0, m]) / np.sqrt(cov[0, 0].real * cov[m, m].real)
        rho_ref = abs(np.vdot(seg[m], seg[0])) / np.sqrt(np.vdot(seg[0], seg[0]).real * np.vdot(seg[m], seg[m]).real)
        print(f"dongle {m}: arg cov {np.angle(cov[0, m]):+.5f} rad, coherence {rho:.6f} (restatement {rho_ref:.6f})")
        assert abs(np.angle(cov[0, m])) <= rr.LOOP_BARS["phase0"] and abs(rho - rho_ref) <= 1e-3 and rho >= 0.99
    # the wrapper does the same in one call
    out2, info2, refined2, table2 = g.retune_align(raw, params, fs, 0, rr.LOOP_STARTS, rr.LOOP_WIN, lag0=rr.LOOP_LAG0, max_lag=rr.LOOP_M, ctx=ctx)
    assert same_bits(table2, tables[0]) and same_bits(refined2, plist[1]) and same_bits(out2.view(np.float64), outs[1].view(np.float64))
    print("largest deviation / bound:", {k: f"{v:.3g}" for k, v in worst.items()})


def test_row_lag_search_finds_a_planted_start_offset(g, ctx):
    n, fs = 30000, rr.LOOP_FS
    raw = np.stack([g.synth.make_wideband(dongle=i, n=n, sample_rate=fs, start=st, tx_key=6)[0] for i, st in enumerate((0.0, 700.0))])
    params = np.stack([ar.identity_row(), ar.identity_row()])
    params[:, 6], params[:, 7] = 127.4, 127.6
    out, info = g.apply_calibration(raw, params, fs, ctx=ctx)
    starts = [2000 + 5000 * j for j in range(5)]
    # dongle 1 started 700 samples late: its content sits 700 samples EARLIER in its row
    assert g.row_lag_search(out, 0, 1, starts, 1184, fs, -1000, 1000, valid=g.valid_of(info), ctx=ctx) == -700
    assert g.row_lag_search(out, 1, 0, starts, 1184, fs, -1000, 1000, max_lag=16, valid=g.valid_of(info), ctx=ctx) == 700
    assert g.row_lag_search(out, 0, 1, starts, 1184, fs, -600, 600, valid=g.valid_of(info), ctx=ctx) is None
