"""GPU tests of the MEX gateway (-m gpu): the objects of tests/mex_gateway.py linked to libgsmcal.so itself.  Every output of every
target, in both complex-storage modes, is THE SAME BITS as the Python API function of the same name on the same input (the four
fused targets: calibrate_batch, fcch_scan_batch, band_power_batch, subband_power_batch, transposed to the MATLAB shape), and the
text the gateway mexPrintf()s is last_call_report() of the Python call.  Both bindings call the same ABI function on the same
device; the gateway makes a context of its own, which its recorded exit hook destroys (at most two gateway contexts exist at a
time).  So that a mistake the two bindings share cannot pass, raw2iq, FCCH_coarse_position, SCH_corr_rate_correction,
gsmcal_calibrate, BCCH_decode and pair_align are also held to numpy / the oracle / what was planted / the restatement, and the
chain is run gateway output into gateway input, sentinels included.

Inputs: one seeded 61-frame capture at 8x (dongle 0 with planted system information), its cut 2000 samples behind the fifth FCCH
(the SCH stage leaves with -ones(15,2)), a noise capture, dongle 3 cut to the same length (calibrates with 14 rows)."""
import contextlib
import os

import numpy as np
import pytest

import bcch_decode_ref
import mex_gateway as mg
import pair_align_ref
import parity
from oracle import gsmcal_oracle as o

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FC = 957.4e6
OV = 8


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


def col(v):
    return np.asarray(v).reshape(-1, 1)


def row(v):
    a = np.asarray(v)
    return (a if np.iscomplexobj(a) else a.astype(np.float64)).reshape(1, -1)


def sc(v):
    return np.array([[float(v)]])


def stream(r):
    """a stream as the Python API returns it -> the MATLAB value: a complex column, or the real 1 x 1 -1"""
    return col(r) if isinstance(r, np.ndarray) else sc(-1.0)


def same_bits(a, b):
    if isinstance(b, list):
        return isinstance(a, dict) and a["shape"] == (1, len(b)) and all(same_bits(x, y) for x, y in zip(a["cells"], b))
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.bool_:
        return np.array_equal(a, b)
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@contextlib.contextmanager
def gateways(target):
    """the target's two objects; their contexts (made at the first call) go through the exit hook when the block ends"""
    gs = [mg.gateway(target, m, "lib") for m in mg.MODES]
    try:
        yield gs
    finally:
        for x in gs:
            assert x.run_atexit() <= 1 and x.num_hooks() == 0


def both(target, args, want, nlhs=None, printed=None):
    """calls the target in both modes: no error, a clean stub, every output the bits of `want`, the printed text as given"""
    nlhs = len(want) if nlhs is None else nlhs
    with gateways(target) as gs:
        for x in gs:
            res = x.call(*args, nlhs=nlhs)
            assert res.err is None, (target, x.mode, res.err)
            assert res.failures == "", res.failures
            k = nlhs if target == "FCCH_demod" else max(nlhs, 1)                 # FCCH_demod.m returns nothing
            assert res.set_mask == [True] * k + [False] * (mg.MAX_OUT - k)
            for i, w in enumerate(want):
                assert same_bits(res.out[i], w), (target, x.mode, i, res.out[i], w)
            if printed is not None:
                assert res.printed == printed, (target, x.mode, res.printed, printed)
            assert x.num_hooks() == (0 if target == "total_ppm_calculation" else 1)
    return res


@pytest.fixture(scope="module")
def data(g):
    s = g.synth
    coef, ts = s.fir1(46, 200e3 / s.FS), s.sch_training_sequence()
    raw0, truth0 = s.make_stream(num_frames=61, **bcch_decode_ref.chain_stream_args("d0"))
    raw3, _ = s.make_stream(num_frames=61, **bcch_decode_ref.chain_stream_args("d3"))
    orc0 = o.calibrate_stream(raw0, coef, ts, FC)
    n_cut = int(orc0["fine_first_round_pos"][4]) + 2000
    rng = np.random.default_rng(7)
    noise = np.clip(np.round(127.5 + 20 * rng.standard_normal(2 * n_cut)), 0, 255).astype(np.uint8)
    d = {"coef": coef, "ts": ts, "raw0": raw0, "truth0": truth0, "orc0": orc0, "n_cut": n_cut, "cut": raw0[:2 * n_cut], "noise": noise,
         "full3": raw3[:2 * n_cut]}
    # the 8x stream of each capture as the driver has it (gsm_sync_demod.m:107,110): the Python API on the GPU
    for name in ("raw0", "cut", "noise"):
        d["r_" + name] = g.filter(coef, g.raw2iq(d[name]))
    # the calibrated stream and its table: the follow-ups' input
    pos, _ = g.FCCH_coarse_position(d["r_raw0"][0::64], 8)
    fp, r1, _, _ = g.FCCH_fine_correction(d["r_raw0"], pos, OV, FC)
    pi, r2, _ = g.SCH_corr_rate_correction(r1, fp, ts, OV)
    r3, _ = g.carrier_correct_post_SCH(r2, pi, OV, FC)
    assert isinstance(r3, np.ndarray) and pi.shape == (16, 2)
    d.update(coarse=pos, fcch_pos=fp, r1=r1, pos_info=pi, r2=r2, r3=r3)
    return d


# ---- the front end and the detectors --------------------------------------------------------------------------------------------
def test_raw2iq(g, data):
    a = np.stack([data["cut"][:4002], data["noise"][:4002], data["full3"][:4002]], axis=1)          # 2N x 3, columns differ
    want = g.raw2iq(a)
    assert np.array_equal(want, o.raw2iq(a.astype(np.float64)))                                     # numpy, exactly
    both("raw2iq", [a], [want], printed="")
    both("raw2iq", [a.astype(np.float64)], [want], printed="")                                      # the reference's doubles
    both("raw2iq", [a[:, :1]], [want[:, :1]])


def test_chn_filters(g, data):
    s = g.raw2iq(np.stack([data["cut"][:2 * 1501], data["noise"][:2 * 1501], data["full3"][:2 * 1501]], axis=1))   # odd n, D = 3
    both("chn_filter_8x_4x", [s], [g.chn_filter_8x_4x(s)], printed="")
    both("chn_filter_4x", [s], [g.chn_filter_4x(s)], printed="")
    both("chn_filter_8x_4x", [s[:, 1].real.reshape(-1, 1)], [col(g.chn_filter_8x_4x(s[:, 1].real + 0j))])      # a real column
    both("chn_filter_4x", [row(s[:5, 2])], [g.chn_filter_4x(row(s[:5, 2]))])                                   # a row is 1 x 5: n = 1, D = 5


def test_detectors(g, data):
    s = data["r_raw0"][0::64][:3594]
    hf, hi, ha, hs = g.move_fft_snr_runtime_avg(s, 160, 16, 10)
    assert hf
    both("move_fft_snr_runtime_avg", [col(s), 160.0, 16.0, 10.0], [np.array([[True]]), sc(hi), sc(ha), sc(hs)], printed="")
    both("move_fft_snr_runtime_avg", [row(s.real), 160.0, 16.0, 10.0],
         [np.array([[g.move_fft_snr_runtime_avg(s.real + 0j, 160, 16, 10)[0]]])], nlhs=1)
    nz = data["r_noise"][0::64][:600]
    nf = g.move_fft_snr_runtime_avg(nz, 160, 16, 10)
    res = both("move_fft_snr_runtime_avg", [col(nz), 160.0, 16.0, 10.0], [np.array([[False]])], nlhs=4)
    assert not nf[0] and same_bits(res.out[2], sc(nf[2])) and same_bits(res.out[3], sc(nf[3]))
    p = int((data["coarse"][1] - 1) / 8 + 1)
    for avg in (-3.0, 50.0):
        hf, hi, hs = g.specific_fft_snr_fix_avg(data["r_raw0"][0::64], (p - 5, p + 5), 16, 10, avg)
        res = both("specific_fft_snr_fix_avg", [col(data["r_raw0"][0::64]), row([p - 5, p + 5]), 16.0, 10.0, avg], [np.array([[hf]])],
                   nlhs=3, printed="")
        assert same_bits(res.out[2], sc(hs)) and (not hf or same_bits(res.out[1], sc(hi)))


# ---- the chain functions ------------------------------------------------------------------------------------------------------
def test_FCCH_coarse_position(g, data):
    pos, snr = g.FCCH_coarse_position(data["r_raw0"][0::64], 8)
    rep = g.last_call_report()
    both("FCCH_coarse_position", [col(data["r_raw0"][0::64]), 8.0], [row(pos), row(snr)], printed=rep)
    both("FCCH_coarse_position", [row(data["r_raw0"][0::64]), 8.0], [row(pos), row(snr)], printed=rep)       # s as a row
    parity.assert_positions(pos, data["orc0"]["coarse_pos"], "coarse position")                               # ... and the oracle
    assert np.allclose(snr, data["orc0"]["coarse_snr"], rtol=0, atol=parity.SNR_ATOL)
    assert g.FCCH_coarse_position(data["r_noise"][0::64], 8) == (-1.0, -1.0)                                  # the reference's -1, -1
    both("FCCH_coarse_position", [col(data["r_noise"][0::64]), 8.0], [sc(-1.0), sc(-1.0)], printed=g.last_call_report())


def test_FCCH_fine_correction(g, data):
    for name, base in (("r_raw0", data["coarse"]), ("r_cut", g.FCCH_coarse_position(data["r_cut"][0::64], 8)[0])):
        fp, r1, sp, cp = g.FCCH_fine_correction(data[name], base, OV, FC)
        rep = g.last_call_report()
        both("FCCH_fine_correction", [col(data[name]), row(base), float(OV), FC], [row(fp), stream(r1), sc(sp), sc(cp)], printed=rep)
    fp, r1, sp, cp = g.FCCH_fine_correction(data["r_raw0"], data["coarse"][:3], OV, FC)                       # :12 exit: -1, -1, inf, inf
    assert r1 == -1.0
    both("FCCH_fine_correction", [col(data["r_raw0"]), col(data["coarse"][:3]), float(OV), FC], [sc(-1.0), sc(-1.0), sc(sp), sc(cp)],
         printed=g.last_call_report())


def test_SCH_corr_rate_correction(g, data):
    ts = data["ts"]
    pi, r2, sp = g.SCH_corr_rate_correction(data["r1"], data["fcch_pos"], ts, OV)
    both("SCH_corr_rate_correction", [col(data["r1"]), row(data["fcch_pos"]), col(ts), float(OV)], [pi, stream(r2), sc(sp)],
         printed=g.last_call_report())
    parity.assert_positions(pi, data["orc0"]["pos_info"], "pos_info")                                         # ... and the oracle
    # the cut: the :84 exit with -ones(3K, 2); and r = -1, FCCH_pos = -1 from a failed fine stage: [-1 -1]
    cpos, _ = g.FCCH_coarse_position(data["r_cut"][0::64], 8)
    fp, r1, _, _ = g.FCCH_fine_correction(data["r_cut"], cpos, OV, FC)
    pi, r2, sp = g.SCH_corr_rate_correction(r1, fp, ts, OV)
    rep = g.last_call_report()
    assert pi.shape == (15, 2) and np.all(pi == -1) and r2 == -1.0
    both("SCH_corr_rate_correction", [stream(r1), row(fp), row(ts), float(OV)], [pi, sc(-1.0), sc(sp)], printed=rep)
    pi, r2, sp = g.SCH_corr_rate_correction(-1.0, -1.0, ts, OV)
    both("SCH_corr_rate_correction", [sc(-1.0), sc(-1.0), col(ts), float(OV)], [np.array([[-1.0, -1.0]]), sc(-1.0), sc(sp)],
         printed=g.last_call_report())


def test_carrier_correct_post_SCH(g, data):
    r3, cp = g.carrier_correct_post_SCH(data["r2"], data["pos_info"], OV, FC)
    both("carrier_correct_post_SCH", [col(data["r2"]), data["pos_info"], float(OV), FC], [stream(r3), sc(cp)], printed=g.last_call_report())
    for m1 in (np.array([[-1.0, -1.0]]), -np.ones((15, 2)), sc(-1.0)):                                         # every sentinel shape
        r3, cp = g.carrier_correct_post_SCH(-1.0, m1 if m1.shape[1] == 2 else np.array([[-1.0, -1.0]]), OV, FC)
        both("carrier_correct_post_SCH", [sc(-1.0), m1, float(OV), FC], [sc(-1.0), sc(cp)], printed=g.last_call_report())


def test_total_ppm_calculation(g):
    for v in ([34.78, -1.08], [12.5, np.inf]):
        both("total_ppm_calculation", [row(v)], [sc(g.total_ppm_calculation(v))], printed="")
        both("total_ppm_calculation", [col(v)], [sc(g.total_ppm_calculation(v))], printed="")
    both("total_ppm_calculation", [row([np.inf, np.inf])], [sc(np.inf)], printed="total PPM calculation: No valid PPM input!\n")


# ---- the follow-ups on the calibrated stream ------------------------------------------------------------------------------------
def test_FCCH_demod(g, data):
    d = g.FCCH_demod(data["r3"], data["pos_info"], OV, FC)
    both("FCCH_demod", [col(data["r3"]), data["pos_info"], float(OV), FC],
         [row(d["freq"]), row(d["snr"]), row(d["max_idx"]), sc(d["carrier_ppm"])], printed=g.last_call_report())
    assert g.FCCH_demod(-1.0, np.array([[-1.0, -1.0]]), OV, FC) is None
    e = np.zeros((1, 0))
    both("FCCH_demod", [sc(-1.0), sc(-1.0), float(OV), FC], [e, e, e, sc(np.nan)], printed=g.last_call_report())
    both("FCCH_demod", [col(data["r3"]), data["pos_info"], float(OV), FC], [], nlhs=0)


def test_BCCH_demod(g, data):
    tpl = g.synth.normal_training_sequences(OV)
    d = g.BCCH_demod(data["r3"], data["pos_info"], tpl, OV, FC)
    assert d["idx"] == bcch_decode_ref.CHAIN_TSC + 1                                                           # what was planted
    both("BCCH_demod", [col(data["r3"]), data["pos_info"], tpl, float(OV), FC],
         [sc(d["idx"]), stream(d["r"]), sc(d["carrier_ppm"]), np.asfortranarray(d["corr_val"])], printed=g.last_call_report())
    few = data["pos_info"][:7]                                                                                 # :14: fewer than four BCCH rows
    d = g.BCCH_demod(data["r3"], few, tpl, OV, FC)
    assert d["status"] == 11
    both("BCCH_demod", [col(data["r3"]), few, tpl, float(OV), FC], [sc(-1.0), sc(-1.0), sc(-1.0), np.zeros((0, 0))], printed=g.last_call_report())
    assert g.BCCH_demod(-1.0, np.array([[-1.0, -1.0]]), tpl, OV, FC) is None                                   # :9
    both("BCCH_demod", [sc(-1.0), sc(-1.0), tpl, float(OV), FC], [sc(-1.0), sc(-1.0), sc(-1.0), np.zeros((0, 0))], printed=g.last_call_report())


def test_SCH_decode(g, data):
    d = g.SCH_decode(data["r3"], data["pos_info"], data["ts"], OV)
    both("SCH_decode", [col(data["r3"]), data["pos_info"], row(data["ts"]), float(OV)],
         [sc(d["bsic"]), sc(d["fn_anchor"]), sc(d["pos_anchor"]), row(d["fn"]), row(d["ok"])], printed=g.last_call_report())
    assert g.SCH_decode(-1.0, np.array([[-1.0, -1.0]]), data["ts"], OV) is None
    e = np.zeros((1, 0))
    both("SCH_decode", [sc(-1.0), -np.ones((15, 2)), col(data["ts"]), float(OV)], [sc(-1.0), sc(-1.0), sc(-1.0), e, e], printed=g.last_call_report())


def test_BCCH_decode(g, data):
    d = g.BCCH_decode(data["r3"], data["pos_info"], bcch_decode_ref.CHAIN_TSC, OV)
    si = d["si"]
    res = both("BCCH_decode", [col(data["r3"]), data["pos_info"], float(bcch_decode_ref.CHAIN_TSC), float(OV)],
               [sc(si["cell_id"]), row([si["mcc"], si["mnc"], si["lac"]]), sc(si["si_type"] if d["status"] == 0 else -1),
                d["octets"].astype(np.float64), row(d["ok"])], printed=g.last_call_report())
    # ... and what was planted, on the gateway's own octet matrix
    ok = np.nonzero(res.out[4][0] == 1.0)[0]
    assert d["status"] == 0 and len(ok) >= 1 and res.out[3].shape == (d["num_blocks"], 23)
    for i in ok:
        assert bcch_decode_ref.planted_octets(data["truth0"], res.out[3][i].astype(np.uint8))
    assert res.out[1].tolist() == [[262.0, 2.0, float(0x1200)]] and res.out[2][0, 0] in (3.0, 4.0)
    assert g.BCCH_decode(-1.0, np.array([[-1.0, -1.0]]), 5, OV) is None
    both("BCCH_decode", [sc(-1.0), sc(-1.0), 5.0, float(OV)], [sc(-1.0), row([-1, -1, -1]), sc(-1.0), np.zeros((0, 23)), np.zeros((1, 0))],
         printed=g.last_call_report())


def test_CW_check_and_IQ_imbalance(g, data):
    s = g.raw2iq(data["cut"][:2 * 777])
    res = both("CW_check", [col(s)], [col(g.CW_check(s))], nlhs=2, printed="")
    assert abs(res.out[1][0, 0] - np.angle(np.mean(s[1:] / s[:-1]))) < 1e-12
    both("CW_check", [row(s.real)], [col(g.CW_check(s.real + 0j))])
    q = g.IQ_imbalance(s)
    both("IQ_imbalance", [col(s)], [sc(q[16]), sc(q[18]), sc(q[19]), row(q)], printed=g.last_call_report())
    both("IQ_imbalance", [row(s)], [sc(q[16]), sc(q[18]), sc(q[19]), row(q)])


def test_pair_coherence(g, data):
    a, pi = data["r3"], data["pos_info"]
    b = np.roll(a, 3) * np.exp(0.4j)
    for extra, kw in (([], {}), ([2.0], dict(lag0=2)), ([2.0, 6.0], dict(lag0=2, max_lag=6)), ([2.0, 6.0, 0.9], dict(lag0=2, max_lag=6, min_coherence=0.9))):
        d = g.pair_coherence(a, b, pi, OV, **kw)
        r = d["row"]
        both("pair_coherence", [col(a), row(b), pi, float(OV)] + extra, [sc(r[6]), sc(r[9]), sc(r[11]), sc(r[13]), sc(r[7]), row(r)],
             printed=g.last_call_report())
    assert g.pair_coherence(-1.0, -1.0, np.array([[-1.0, -1.0]]), OV) is None
    res = both("pair_coherence", [sc(-1.0), sc(-1.0), sc(-1.0), float(OV)], [], nlhs=6)
    assert res.out[5][0, 0] == 10.0 and np.isnan(res.out[4][0, 0])


def test_pair_align(g, data):
    s = data["r3"][:5001]
    p = np.array([2.25, 30.0, 120.0, 0.5, 1000.0, 1.0])
    for extra, n in (([], 5001), ([3000.0], 3000), ([6000.0], 6000)):                                          # out_len absent, shorter, longer
        out, info = g.pair_align(s, OV, p, n)
        vec = row([info[k] for k in g.ALIGN_INFO_FIELDS])
        both("pair_align", [col(s), float(OV), row(p)] + extra, [col(out), vec], printed=g.last_call_report())
        want = pair_align_ref.pair_align(s, len(s), OV, p, n)                                                  # ... and the restatement
        assert vec.tolist() == [[float(want["status"]), float(want["first_valid"]), float(want["end_valid"]), float(want["num_valid"])]]
    out, info = g.pair_align(s.real + 0j, OV, p)
    both("pair_align", [row(s.real), float(OV), col(p)], [col(out)])                                           # a real row s, params a column


# ---- the fused targets ----------------------------------------------------------------------------------------------------------
def test_gsmcal_calibrate(g, data, ctx):
    raw = np.stack([data["full3"], data["cut"], data["noise"]])                                                # calibrates | -ones(15,2) | [-1 -1]
    s = np.asfortranarray(raw.T)
    for freq, fpy in ((FC, FC), (row([FC, FC + 2e5, FC - 2e5]), np.array([FC, FC + 2e5, FC - 2e5]))):
        out = g.calibrate_batch(raw, data["coef"], data["ts"], fpy)
        det = g.last_batch_details(3, ctx=ctx)
        assert [p.shape for p in out["pos_info"]] == [(14, 2), (15, 2), (1, 2)] and out["table"][:, 9].tolist() == [0.0, 8.0, 1.0]
        both("gsmcal_calibrate", [s, row(data["coef"]), col(data["ts"]), freq], [out["table"], out["pos_info"]], printed="")
        for i in range(3):                                                                                      # ... and the oracle
            orc = o.calibrate_stream(raw[i], data["coef"], data["ts"], float(np.broadcast_to(fpy, (3,))[i]))
            parity.compare_stream(orc, out["table"][i], det, i, out["pos_info"][i])


def test_scanners(g, data):
    n = 40001
    raw = np.stack([data["full3"][:2 * n], data["cut"][:2 * n], data["noise"][:2 * n]])
    s = np.asfortranarray(raw.T)
    big = np.asfortranarray(np.stack([data["full3"], data["cut"], data["noise"]]).T)
    out = g.fcch_scan_batch(np.ascontiguousarray(big.T), data["coef"])
    both("gsmcal_fcch_scan", [big, row(data["coef"])], [row(out["snr"]), row(out["num_hit"])], printed="")
    for dec in (1, 64):
        both("gsmcal_band_power", [s, col(data["coef"]), float(dec)], [row(g.band_power_batch(raw, data["coef"], dec))], printed="")
    w = np.array([[0.1, np.nan, -0.3], [np.nan, 0.2, 0.25], [0.05, -0.15, np.nan]])                          # J = 3 x D = 3, a NaN slot per column
    both("gsmcal_subband_power", [s, row(data["coef"]), w], [np.asfortranarray(g.subband_power_batch(raw, data["coef"], w.T).T)], printed="")
    both("gsmcal_subband_power", [s, row(data["coef"]), w, 4.0], [np.asfortranarray(g.subband_power_batch(raw, data["coef"], w.T, 4).T)])


# ---- the chain as a driver runs it: gateway output into gateway input ---------------------------------------------------------
def once(target, mode, *args, nlhs):
    x = mg.gateway(target, mode, "lib")
    res = x.call(*args, nlhs=nlhs)
    x.run_atexit()                                                  # one gateway context at a time
    assert res.err is None and res.failures == "", (target, res.err, res.failures)
    return res.out[:nlhs]


@pytest.mark.parametrize("mode", mg.MODES)
def test_chain_through_the_gateways_ends_on_calibrate_batch(g, data, ctx, mode):
    """gsm_sync_demod.m:107-124 with every function a gateway call: raw2iq, filter(coef,1,.) (a MATLAB builtin, here the library's
    filter), r(1:64:end), FCCH_coarse_position ... carrier_correct_post_SCH, total_ppm_calculation, then FCCH_demod and BCCH_demod
    on what came out -- for the capture that calibrates, the cut (-ones(15,2), r = -1 handed on) and the noise (position -1 handed
    on).  The table it ends on is calibrate_batch's for the same bytes, within the bounds of parity.compare_stream."""
    raw = np.stack([data["full3"], data["cut"], data["noise"]])
    out = g.calibrate_batch(raw, data["coef"], data["ts"], FC)
    tpl = g.synth.normal_training_sequences(OV)
    for i in range(3):
        b, = once("raw2iq", mode, raw[i].reshape(-1, 1), nlhs=1)
        r = col(g.filter(data["coef"], b[:, 0]))
        pos, snr = once("FCCH_coarse_position", mode, r[0::64], 8.0, nlhs=2)
        fp, r1, sp1, cp1 = once("FCCH_fine_correction", mode, r, pos, float(OV), FC, nlhs=4)
        pi, r2, sp2 = once("SCH_corr_rate_correction", mode, r1, fp, col(data["ts"]), float(OV), nlhs=3)
        r3, cp2 = once("carrier_correct_post_SCH", mode, r2, pi, float(OV), FC, nlhs=2)
        ts_, = once("total_ppm_calculation", mode, np.hstack([sp1, sp2]), nlhs=1)
        tc_, = once("total_ppm_calculation", mode, np.hstack([cp1, cp2]), nlhs=1)
        t = out["table"][i]
        for got, want, what in ((sp1, t[0], "sampling_ppm(1)"), (sp2, t[1], "sampling_ppm(2)"), (cp1, t[2], "carrier_ppm(1)"),
                                (cp2, t[3], "carrier_ppm(2)"), (ts_, t[4], "total sampling ppm"), (tc_, t[5], "total carrier ppm")):
            parity.assert_ppm(got[0, 0], want, what)
        assert pi.shape == out["pos_info"][i].shape
        parity.assert_positions(pi, out["pos_info"][i], "pos_info")
        assert (fp.shape[1] if fp[0, 0] != -1 else 1) == t[6] and pi.shape[0] == t[7] and pi[0, 0] == t[8]
        fd = once("FCCH_demod", mode, r3, pi, float(OV), FC, nlhs=4)
        idx, rb, cpb, cv = once("BCCH_demod", mode, r3, pi, tpl, float(OV), FC, nlhs=4)
        if t[9] == 0:
            assert r3.shape[1] == 1 and r3.shape[0] > 1
            assert fd[0].shape[1] >= 1 and idx[0, 0] == bcch_decode_ref.CHAIN_TSC + 1 and cv.shape == (8, 4)
        else:
            assert same_bits(r3, sc(-1.0)) and np.all(pi == -1)
            assert fd[0].shape == (1, 0) and np.isnan(fd[3][0, 0]) and idx[0, 0] == -1 and cv.shape == (0, 0)


@pytest.mark.parametrize("mode", mg.MODES)
def test_chain_at_4x_through_chn_filter_8x_4x(g, data, mode):
    """raw2iq -> chn_filter_8x_4x -> FCCH_coarse_position -> FCCH_fine_correction -> SCH_corr_rate_correction ->
    carrier_correct_post_SCH at oversampling_ratio 4, gateway output into gateway input, against the oracle's functions called the
    same way (positions identical, ppm within parity's bounds).  calibrate_batch filters the 8x stream with the driver's own taps
    and keeps 8x, so this chain has no table of the batch to end on; the 8x chain above has."""
    num = o.load_num(os.path.join(HERE, "golden", "gsm_chn_filter_8x_num.txt"))
    raw = data["raw0"]
    b, = once("raw2iq", mode, raw.reshape(-1, 1), nlhs=1)
    assert np.array_equal(b[:, 0], o.raw2iq(raw.astype(np.float64)))
    r, = once("chn_filter_8x_4x", mode, b, nlhs=1)
    want_r = o.chn_filter_8x_4x(b[:, 0], num)
    assert r.shape == (len(want_r), 1) and np.max(np.abs(r[:, 0] - want_r)) < 1e-13 * max(1.0, np.max(np.abs(want_r)))
    ts4 = np.ascontiguousarray(data["ts"][0::2])
    pos, snr = once("FCCH_coarse_position", mode, r[0::32], 8.0, nlhs=2)
    o_pos, _ = o.FCCH_coarse_position(want_r[0::32], 8)
    parity.assert_positions(pos[0], o_pos, "coarse position")
    fp, r1, sp1, cp1 = once("FCCH_fine_correction", mode, r, pos, 4.0, FC, nlhs=4)
    o_fp, o_r1, o_sp1, o_cp1 = o.FCCH_fine_correction(want_r, o_pos, 4, FC)
    parity.assert_positions(fp[0], o_fp, "FCCH_pos")
    parity.assert_ppm(sp1[0, 0], o_sp1, "sampling_ppm(1)")
    parity.assert_ppm(cp1[0, 0], o_cp1, "carrier_ppm(1)")
    pi, r2, sp2 = once("SCH_corr_rate_correction", mode, r1, fp, row(ts4), 4.0, nlhs=3)
    o_pi, o_r2, o_sp2 = o.SCH_corr_rate_correction(o_r1, o_fp, ts4, 4)
    parity.assert_positions(pi, o_pi, "pos_info")
    parity.assert_ppm(sp2[0, 0], o_sp2, "sampling_ppm(2)")
    r3, cp2 = once("carrier_correct_post_SCH", mode, r2, pi, 4.0, FC, nlhs=2)
    o_r3, o_cp2 = o.carrier_correct_post_SCH(o_r2, o_pi, 4, FC)
    parity.assert_ppm(cp2[0, 0], o_cp2, "carrier_ppm(2)")
    assert isinstance(o_r3, np.ndarray) and r3.shape == (len(o_r3), 1)
    assert np.max(np.abs(r3[:, 0] - o_r3)) <= 2e-8 * np.max(np.abs(o_r3))                     # tests/test_gpu_parity.py's stream bound
