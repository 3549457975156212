"""GPU tests (-m gpu) of the per-function API across decimation ratios, window lengths, oversampling ratios and front-end
shapes (tests/geometry_cases.py; tests/test_geometry_cpu.py proves the premises with both oracles): everything through
gsmcal as a caller of the .m functions would, against the live oracle.

What runs here and nowhere else in the suite: k_coarse_snr<false> / k_coarse_scan_gen (window_snr_generic, the whole-block
hop walk on its own spectra) at fft_len 2..64; k_coarse_scan_lat behind decimation ratios 5, 6, 7; k_fine_cert<0, 0>,
k_fine_openall, k_fine_chunk, k_fine_verify, k_fft_burst<1> + k_fine_search, k_burst_tone<., 0, 0> and k_window_sch<0, 0, 0> at
1, 3, 5, 6, 12, 16 and 30 samples per symbol; the demodulator kernels at 1, 2, 3, 12, 16 and 33; k_fir_decim_raw, k_dc_sum and
k_fir_arr at every alignment, length and decimation of the front-end triples.

Bars (none tuned on the library): positions, flags, indices and shapes exact; SNRs parity.SNR_ATOL; ppm parity.assert_ppm;
streams 2e-8 of their peak; front end 2 ntaps 2^-53 sum|coef| max|x| (geometry_cases.fe_bound); the demodulator's bars are
those of test_gpu_parity.py / test_gpu_fcch_demod.py.  Limits come from the host's own sizing formulas, restated below.
fft_len = 3 is not compared with the oracle (geometry_cases' docstring)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import fcch_demod_ref as ref
import geometry_cases as gc
import parity
from oracle import gsmcal_oracle as o

pytestmark = pytest.mark.gpu

FC = gc.FC
STREAM_RTOL = 2e-8
HZ_TOL = 1e-6 * 1e-6 * FC            # test_gpu_fcch_demod.py: 1e-6 ppm of the carrier, in Hz
LDS_LIMIT = 159 * 1024               # what every launch with dynamic LDS is held to (host_plan.h, abi_calls.h)
E_ARG, E_INDEX, E_UNSUPPORTED, S_POST_NO_POS = -1, -5, -6, 10
ROUTE_OV = 8                         # the drivers' ratio: here only for the route (k_fine_cert<8, 47>) and as the chain's yardstick


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


def context_under(g, env):
    """a context created under `env` (the switches are read when a context is created), per-kernel profile on"""
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        cx = g.Context(0)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    cx.profile_enable()
    return cx


@pytest.fixture(scope="module")
def pcx(g):
    """one context with the per-kernel profile on, for the route assertions of the coarse stage"""
    cx = context_under(g, {})
    yield cx
    cx.close()


def launched(cx):
    """kernel name -> launches since the last profile_reset (names seen before it stay listed with 0: left out)"""
    return {k: v[1] for k, v in cx.profile_get().items() if v[1]}


def count(names, part):
    return sum(n for k, n in names.items() if part in k)


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def cbuf(s):
    return np.ascontiguousarray(np.asarray(s, dtype=np.complex128).ravel())


def stream_close(a, b, what):
    assert isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape, (what, np.shape(a), np.shape(b))
    scale = np.max(np.abs(b))
    err = np.max(np.abs(a - b))
    print(f"   {what}: max abs err / peak {err / scale:.3e}")
    assert err <= STREAM_RTOL * scale, f"{what}: max abs err {err} at scale {scale}"


def snr_close(a, b):
    return a == b or (math.isnan(a) and math.isnan(b)) or abs(a - b) <= parity.SNR_ATOL


# ---- coarse stage ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def captures():
    return gc.coarse_captures()


@pytest.mark.parametrize("dr", gc.COARSE_DRS)
def test_FCCH_coarse_position_at_other_decimation_ratios(g, pcx, captures, dr):
    """Both captures and the carrier without a BCCH at every ratio: positions exact, SNRs 1e-8 dB, the sentinel where the oracle
    returns it; one sample short of s(1:n_first) is MATLAB's index error; and the route: the 16-point scan for dr 5, 6, 7, the
    any-length one (k_coarse_snr<false> in front of it) everywhere else."""
    geo = gc.coarse_geometry(dr)
    for name, r8 in captures.items():
        s = gc.coarse_cut(r8, dr)
        want_p, want_s = o.FCCH_coarse_position(s, dr)
        pcx.profile_reset()
        got_p, got_s = g.FCCH_coarse_position(s, dr, ctx=pcx)
        names = launched(pcx)
        print(dr, name, "oracle", want_p, "kernels", sorted(names.items()))
        if np.ndim(want_p) == 0:
            assert (got_p, got_s) == (-1.0, -1.0) == (want_p, want_s), (dr, name, got_p)
        else:
            parity.assert_positions(got_p, want_p, f"position (dr {dr}, {name})")
            assert np.allclose(got_s, want_s, rtol=0, atol=parity.SNR_ATOL), (dr, name, got_s, want_s)
        if geo["fft_len"] == 16:
            assert names.get("k_coarse_scan_lat") == 1 and names.get("k_coarse_snr<true>") == 1 and count(names, "k_coarse_s") == 2, names
        else:
            assert names.get("k_coarse_scan_gen") == 1 and names.get("k_coarse_snr<false>") == 1 and count(names, "k_coarse_s") == 2, names
    s = gc.coarse_cut(captures["dongle0"], dr)
    with pytest.raises(g.GsmcalError, match="GSMCAL_E_INDEX"):
        g.FCCH_coarse_position(s[: geo["n_first"] - 1], dr)
    got = g.FCCH_coarse_position(s[: geo["n_first"]], dr)                  # ... and exactly n_first samples are enough
    want = o.FCCH_coarse_position(s[: geo["n_first"]], dr)
    parity.assert_positions(got[0], want[0], f"position on n_first samples (dr {dr})")


def test_coarse_ratios_cover_both_routes():
    assert [dr for dr in gc.COARSE_DRS if gc.coarse_geometry(dr)["fft_len"] == 16] == [5, 6, 7]


@pytest.fixture(scope="module")
def det():
    s = gc.det_stream()
    return s, {f: gc.window_snrs(s, f) for f in gc.DET_FFT_LENS}


@pytest.mark.parametrize("fft_len", gc.DET_FFT_LENS)
def test_move_fft_snr_runtime_avg_grid(g, pcx, det, fft_len):
    s, _ = det
    for f, mv_len, th, n in gc.move_cases():
        if f != fft_len:
            continue
        x = s if n is None else s[:n]
        pcx.profile_reset()
        got = g.move_fft_snr_runtime_avg(x, mv_len, fft_len, th, ctx=pcx)
        names = launched(pcx)
        assert count(names, "k_coarse_scan_lat" if fft_len == 16 else "k_coarse_scan_gen") == 1 and count(names, "k_coarse_scan") == 1, names
        nwin = len(x) - (fft_len - 1)
        if fft_len in gc.UNCOMPARED_FFT_LENS:
            assert got[1] == -1 or 1 <= got[1] <= nwin, (mv_len, th, n, got)     # rounding-defined: a clean return is all
            assert got[0] == (got[1] != -1)
            continue
        want = o.move_fft_snr_runtime_avg(x, mv_len, fft_len, th)
        assert got[:2] == want[:2] and snr_close(got[2], want[2]) and snr_close(got[3], want[3]), (fft_len, mv_len, th, n, got, want)


@pytest.mark.parametrize("fft_len", gc.DET_FFT_LENS)
def test_specific_fft_snr_fix_avg_cases(g, pcx, det, fft_len):
    """first / last window of the set, a miss, and the window-by-window bound behaviour of specific_fft_snr_fix_avg.m:10-11 at the
    end of s: a set that ends on the last window that fits is served; one past it is the index error unless a window before hits"""
    s, snrs = det
    nwin = len(snrs[fft_len])
    for name, (tset, th, avg) in gc.specific_cases(snrs[fft_len], fft_len).items():
        if fft_len in gc.UNCOMPARED_FFT_LENS:
            try:
                got = g.specific_fft_snr_fix_avg(s, tset, fft_len, th, avg)
            except g.GsmcalError as e:
                assert "GSMCAL_E_INDEX" in str(e) and tset[1] > nwin, (name, str(e))
                continue
            assert got[1] == -1 or tset[0] <= got[1] <= min(tset[1], nwin), (name, got)
            continue
        try:
            want = o.specific_fft_snr_fix_avg(s, tset, fft_len, th, avg)
        except o.MatlabIndexError:
            with pytest.raises(g.GsmcalError, match="GSMCAL_E_INDEX"):
                g.specific_fft_snr_fix_avg(s, tset, fft_len, th, avg)
            continue
        pcx.profile_reset()
        got = g.specific_fft_snr_fix_avg(s, tset, fft_len, th, avg, ctx=pcx)
        names = launched(pcx)
        assert names == {("k_coarse_scan_lat" if fft_len == 16 else "k_coarse_scan_gen"): 1}, names     # (it computes its own windows)
        assert got[:2] == want[:2] and snr_close(got[2], want[2]), (fft_len, name, got, want)


# ---- chain, function by function ------------------------------------------------------------------------------------------------
PATHS = {"default": {}, "no_certificate": {"GSMCAL_CERT": "0"}, "no_prescreen": {"GSMCAL_PRESCREEN": "0"}}


def carve_lds(length, level, to_lds):
    """kernels_frontend.h gather_carve for an array source (no taps, no padded FIR input): buf0 | buf1 | raw ushorts | rotator"""
    bufn = length + 40 if (level >= 1 or to_lds) else 0
    span = length + 8 + 24
    off_raw = bufn * 16 + (bufn if (level >= 2 or to_lds) else 0) * 16
    total = (off_raw + ((span + 7) & ~7) * 2 + 15) & ~15
    return max(total, (off_raw + (1 + 72 + 32) * 16 + 15) & ~15) if level >= 2 else total


def chain_lds(ov, len_ts):
    """host_plan.h api_chain_lds: the dynamic LDS of every launch of the three per-function stages, kernel by kernel"""
    nfft, nstep, sch = 148 * ov, 128 * ov, 11 * ov + 1
    wlen, n2 = nstep + nfft, 4 * ov
    burst_scratch = (40 + n2) * 16 + max((16 + nfft // 16 + 2) * 16, 2 * 56 * 8)
    fused = lambda length, level, scratch: (carve_lds(length, level, True) + scratch + 15) & ~15
    return {"k_fine_chunk": (nfft + 64 + 37 * (n2 + 1) + 40 + n2) * 16 + 64 * 8,                 # fk_lds_bytes
            "k_fine_verify": (wlen * 16 + 512 * (4 + 16) + 15) & ~15,                              # vlds
            "k_fft_burst": (nfft + 37 * (n2 + 1) + 40 + n2) * 16,                                  # fft_lds
            "k_fine_search": (nstep + 64) * 16,
            "k_gather": carve_lds(wlen, 0, False),
            "k_burst_tone<1>": fused(nfft, 1, burst_scratch), "k_burst_tone<0>": fused(nfft, 0, burst_scratch),
            "k_window_sch": fused(sch - 1 + len_ts, 0, (len_ts + sch * 4) * 16 + sch * 8)}


def certificate_fits(ov):
    """host_plan.h run_fine's cert_ok for an array source: 8 threads per 64-shift chunk in at most 512, and kernels_detect.h
    fc_lds_bytes -- the padded window, the level-1 partials or E(t), the twiddle planes or the fp32 sums -- within 159 KiB"""
    nfft, nstep = 148 * ov, 128 * ov
    wlen, b = nstep + nfft, math.gcd(64, nfft)
    xp = lambda p: p + (p >> 7)
    r1, e1 = 8 * (wlen // b) * 16, (nstep + 2) * 8
    r2, e2 = 8 * (b + 2 + nfft // b) * 16, 2 * (xp(nstep + 2) + 1) * 4 + 16 * 8
    clds = (xp(wlen) * 16 + max(r1, e1) + max(r2, e2) + 15) & ~15
    return max(256, (nstep // 64 * 8 + 63) // 64 * 64) <= 512 and clds <= LDS_LIMIT and nfft >= 16


CHAIN_MAX_OV = max(ov for ov in range(1, 128) if max(chain_lds(ov, 64 * ov).values()) <= LDS_LIMIT)
CHAIN_CASES = [(name, ov) for name in ("plain", "ppm") for ov in gc.OVS] + [("plain", ROUTE_OV), ("plain", CHAIN_MAX_OV)]


@pytest.fixture(scope="module")
def chain_inputs():
    """(capture, ov) -> (stream, training sequence, oracle chain), computed once"""
    bases = gc.ov_base_streams()
    cache = {}

    def get(name, ov):
        if (name, ov) not in cache:
            r = bases[name] if ov == 8 else gc.resample(bases[name], ov)
            ts = gc.training_sequence(ov)
            cache[(name, ov)] = (r, ts, gc.oracle_chain(o, r, ov, ts))
        return cache[(name, ov)]
    return get


@pytest.fixture(scope="module")
def path_contexts(g):
    cxs = {k: context_under(g, env) for k, env in PATHS.items()}
    yield cxs
    for cx in cxs.values():
        cx.close()


def gpu_chain(g, r, ov, ts, cx):
    res = {}
    res["coarse_pos"], res["coarse_snr"] = g.FCCH_coarse_position(r[0::8 * ov], 8, ctx=cx)
    cx.profile_reset()
    res["fcch_pos"], res["r1"], res["sp1"], res["cp1"] = g.FCCH_fine_correction(r, res["coarse_pos"], ov, FC, ctx=cx)
    res["fine_kernels"] = launched(cx)
    det = g.last_batch_details(1, ctx=cx)
    res["fine_first"] = det["fine_first"][0, :det["counts"][0, 1]].copy()
    cx.profile_reset()
    res["pos_info"], res["r2"], res["sp2"] = g.SCH_corr_rate_correction(res["r1"], res["fcch_pos"], ts, ov, ctx=cx)
    res["r3"], res["cp2"] = g.carrier_correct_post_SCH(res["r2"], res["pos_info"], ov, FC, ctx=cx)
    res["tail_kernels"] = launched(cx)
    return res


@pytest.mark.parametrize("name,ov", CHAIN_CASES, ids=[f"{n}-{v}x" for n, v in CHAIN_CASES])
def test_chain_function_by_function_at_other_oversampling_ratios(g, chain_inputs, path_contexts, name, ov):
    """gsm_sync_demod.m:117-120 call by call at 1, 3, 5, 6, 12 and 16 samples per symbol (and 8, the yardstick), on the default
    path, without the certificate (k_fine_openall: every chunk swept) and without the prescreen (k_fft_burst<1> + k_fine_search:
    the 37 x N2 FFT and the plain fp64 search): against the oracle on every path, first-round positions identical across the
    three, and the kernels each path is there for did run."""
    r, ts, want = chain_inputs(name, ov)
    assert want["exit"] == gc.CHAIN_EXIT[name].get(ov, 0)           # (8x, the yardstick, completes)
    first = {}
    for path, cx in path_contexts.items():
        got = gpu_chain(g, r, ov, ts, cx)
        fk, tk = got["fine_kernels"], got["tail_kernels"]
        print(name, ov, path, "fine:", sorted(fk.items()), "tail:", sorted(tk.items()))
        what = f"{name} {ov}x {path}: "
        parity.assert_positions(got["coarse_pos"], want["coarse_pos"], what + "coarse position")
        parity.assert_positions(got["fine_first"], want["info"][1]["first_round_pos"], what + "first-round FCCH_pos")
        first[path] = got["fine_first"]
        parity.assert_positions(got["fcch_pos"], want["fcch_pos"], what + "FCCH_pos")
        parity.assert_ppm(got["sp1"], want["sp1"], what + "sampling_ppm(1)")
        parity.assert_ppm(got["cp1"], want["cp1"], what + "carrier_ppm(1)")
        stream_close(got["r1"], want["r1"], what + "r of FCCH_fine_correction")
        assert got["pos_info"].shape == want["pos_info"].shape, (what, got["pos_info"].shape, want["pos_info"].shape)
        parity.assert_positions(got["pos_info"], want["pos_info"], what + "pos_info")
        parity.assert_ppm(got["sp2"], want["sp2"], what + "sampling_ppm(2)")
        parity.assert_ppm(got["cp2"], want["cp2"], what + "carrier_ppm(2)")
        if want["exit"] == 0:
            stream_close(got["r2"], want["r2"], what + "r of SCH_corr_rate_correction")
            stream_close(got["r3"], want["r3"], what + "r of carrier_correct_post_SCH")
        else:
            # the SCH stage's edge exit (SCH_corr_rate_correction.m:59-63): pos_info = [-1 -1]; carrier_correct_post_SCH then
            # returns r = -1, inf (:10-13)
            assert want["exit"] == o.S_SCH_EDGE and got["pos_info"].shape == (1, 2) and np.all(got["pos_info"] == -1)
            if not isinstance(want["r2"], np.ndarray):
                assert got["r2"] == -1.0
            assert got["r3"] == -1.0 and want["r3"] == -1.0 and math.isinf(got["cp2"])
        # the route (host_plan.h run_fine / run_sch / run_post): arrays handed in through the API take the any-geometry burst and
        # SCH kernels at every ov; the certificate is <8, 47> at 8x (it reads finished windows: no taps in it) and <0, 0> elsewhere
        cert = "(k_fine_cert<8, 47>)" if ov == 8 else "(k_fine_cert<0, 0>)"
        if path == "default" and not certificate_fits(ov):       # no room for the certificate's window and tables: every chunk is swept
            assert fk.get("k_fine_openall") == 1 and count(fk, "k_fine_cert") == 0, fk
        elif path == "default":
            assert fk.get(cert) == 1 and count(fk, "k_fine_cert") == 1 and count(fk, "k_fine_openall") == 0, fk
            assert count(fk, "k_fine_chunk") == 1 and count(fk, "k_fine_verify") == 1 and count(fk, "k_fine_search") == 0, fk
        elif path == "no_certificate":
            assert fk.get("k_fine_openall") == 1 and count(fk, "k_fine_cert") == 0, fk
            assert count(fk, "k_fine_chunk") == 1 and count(fk, "k_fine_verify") == 1 and count(fk, "k_fine_search") == 0, fk
        else:
            assert fk.get("k_fft_burst<1>") == 1 and fk.get("k_fine_search") == 1, fk
            assert count(fk, "k_fine_cert") + count(fk, "k_fine_openall") + count(fk, "k_fine_chunk") == 0, fk
        assert fk.get("(k_burst_tone<1, 0, 0>)") == 1 and count(fk, "k_burst_tone") == 1, fk
        assert tk.get("(k_window_sch<0, 0, 0>)") == 1 and count(tk, "k_window_sch") == 1, tk
        assert count(tk, "k_post_chain") == 0 and count(tk, "8, 47>") + count(tk, "8, 512, 47>") == 0, tk
        if want["exit"] == 0:
            assert tk.get("(k_burst_tone<0, 0, 0>)") == 1 and count(tk, "k_burst_tone") == 1, tk
    assert np.array_equal(first["default"], first["no_certificate"]) and np.array_equal(first["default"], first["no_prescreen"])


def test_the_sampling_error_capture_makes_both_stages_resample(chain_inputs):
    for ov in gc.OVS:
        want = chain_inputs("ppm", ov)[2]
        if want["exit"] == 0:
            assert abs(want["sp1"]) > 100.0 and want["sp2"] != 0.0 and math.isfinite(want["sp2"]), (ov, want["sp1"], want["sp2"])


# ---- SCH_equalise and FCCH_demod --------------------------------------------------------------------------------------------
def sch_equalise_lds(ov):
    """abi_calls.h gsmcal_SCH_equalise / kernels_demod.h dm_lds_bytes: three L-point buffers and the 97 x (N2 + 1) matrix"""
    L = 194 * ov
    return (3 * L + 97 * (L // 97 + 1)) * 16


SCH_EQ_MAX_OV = max(ov for ov in range(1, 64) if sch_equalise_lds(ov) <= LDS_LIMIT)


@pytest.fixture(scope="module")
def demod_inputs(chain_inputs):
    """ov -> (corrected stream, pos_info, training sequence) of the oracle chain on the plain capture; 2x like the existing
    tests make it: the 8x stream decimated"""
    cache = {}

    def get(ov):
        if ov not in cache:
            if ov == 2:
                r8, ts8, _ = chain_inputs("plain", 8)
                r, ts = np.ascontiguousarray(r8[0::4]), np.ascontiguousarray(ts8[0::4])
                want = gc.oracle_chain(o, r, 2, ts)
            else:
                r, ts, want = chain_inputs("plain", ov)
            cache[ov] = (want["r3"], want["pos_info"], ts)
        return cache[ov]
    return get


def test_sch_equalise_limit_is_twelve():
    assert SCH_EQ_MAX_OV == 12 and sch_equalise_lds(12) <= LDS_LIMIT < sch_equalise_lds(13)


@pytest.mark.parametrize("ov", (1, 2, 3, SCH_EQ_MAX_OV))
def test_SCH_equalise_at_other_oversampling_ratios(g, demod_inputs, ov):
    r, pi, ts = demod_inputs(ov)
    want = o.SCH_equalise(r, pi, ts, ov)
    got = g.SCH_equalise(r, pi, ts, ov)
    if ov == 1:                                                   # pos_info is the sentinel: SCH_demod.m:8-11
        assert np.all(pi == -1) and want is None and got is None
        return
    assert got.shape == want.shape == (int(np.sum(pi[:, 1] == 1)), 194 * ov) and got.shape[0] >= 4
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print(f"SCH_equalise {ov}x: max abs err / peak {err:.3e}")
    assert err <= 1e-10
    with pytest.raises(g.GsmcalError, match="GSMCAL_E_INDEX"):    # s(sp:ep) past the stream
        g.SCH_equalise(r[: int(pi[pi[:, 1] == 1, 0][-1]) + 10 * ov], pi, ts, ov)


@pytest.mark.parametrize("ov", (SCH_EQ_MAX_OV + 1, 16))
def test_SCH_equalise_refuses_what_its_lds_cannot_hold(g, ctx, demod_inputs, ov):
    """3 x 194 ov + 97 x (2 ov + 1) complex doubles pass 159 KiB at ov = 13: GSMCAL_E_UNSUPPORTED, nothing written"""
    r, pi, ts = demod_inputs(16)
    assert sch_equalise_lds(ov) > LDS_LIMIT
    s, t = cbuf(r), cbuf(ts)
    pic = np.ascontiguousarray(pi.T)
    nsch = int(np.sum(pi[:, 1] == 1))
    out = np.full((nsch, 194 * ov, 2), np.nan)
    nb, lf = C.c_int(-7), C.c_int(-7)
    rc = ctx.lib.gsmcal_SCH_equalise(ctx.h, dp(s), len(s), dp(pic), len(pi), len(pi), dp(t), len(t), ov, dp(out), nsch, C.byref(nb), C.byref(lf))
    assert rc == E_UNSUPPORTED and np.all(np.isnan(out)) and nb.value == 0


def demod_compare(got, want, tol):
    print("max_idx", got["max_idx"].tolist(), "|dfreq| max", np.max(np.abs(got["freq"] - want["freq"]), initial=0.0),
          "|dsnr| max", np.nanmax(np.abs(got["snr"] - want["snr"]), initial=0.0), "noise_ratio min", np.min(np.abs(want["noise_ratio"]), initial=np.inf))
    assert np.all(np.abs(want["noise_ratio"]) >= 1e-3), want["noise_ratio"]
    assert np.array_equal(got["max_idx"], want["max_idx"])
    assert got["freq"].shape == want["freq"].shape and np.all(np.abs(got["freq"] - want["freq"]) <= tol)
    assert abs(got["mean_freq"] - want["mean_freq"]) <= tol
    assert abs(got["carrier_ppm"] - want["carrier_ppm"]) <= 1e-6
    nan = np.isnan(want["snr"])
    assert np.array_equal(np.isnan(got["snr"]), nan) and np.all(np.abs(got["snr"][~nan] - want["snr"][~nan]) <= 1e-6)


@pytest.mark.parametrize("ov", gc.DEMOD_OVS)
def test_FCCH_demod_at_other_oversampling_ratios(g, demod_inputs, ov):
    r, pi, _ = demod_inputs(ov)
    want = ref.fcch_demod(r, pi, ov, FC)
    got = g.FCCH_demod(r, pi, ov, FC)
    if ov == 1:                                                   # FCCH_demod.m:8 on the sentinel
        assert want is None and got is None
        return
    assert len(want["freq"]) == int(np.sum(pi[:, 1] == 0)) >= 5
    demod_compare(got, want, HZ_TOL)


# ---- front end ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fe():
    filt = gc.fe_filters()
    raws = {n: gc.fe_raw(n) for n in gc.FE_NS}
    iq = {n: o.raw2iq(raw.T.astype(np.float64)) for n, raw in raws.items()}
    return filt, raws, iq


@pytest.mark.parametrize("n", gc.FE_NS)
def test_raw2iq_bit_exact_at_every_length(g, fe, n):
    _, raws, iq = fe
    got = g.raw2iq(raws[n].T)
    assert got.shape == (n, gc.FE_STREAMS) and np.array_equal(got, iq[n])
    assert np.array_equal(g.raw2iq(raws[n].T.astype(np.float64)), iq[n])


@pytest.mark.parametrize("n,decim,name", gc.FE_TRIPLES, ids=[f"n{n}-decim{d}-{f}" for n, d, f in gc.FE_TRIPLES])
def test_front_end_filter_and_decimation(g, fe, n, decim, name):
    filt, raws, iq = fe
    coef = filt[name]
    want = o.matlab_filter(coef, iq[n])[0::decim]
    bound = gc.fe_bound(coef, iq[n])
    nd = -(-n // decim)
    got = g.frontend_batch(raws[n], coef, decim)
    assert got.shape == (gc.FE_STREAMS, nd) and want.shape == (nd, gc.FE_STREAMS)
    err = np.max(np.abs(got.T - want))
    got2 = g.filter(coef, g.raw2iq(raws[n].T), decim)
    assert got2.shape == (nd, gc.FE_STREAMS)
    err2 = np.max(np.abs(got2 - want))
    print(f"n {n} decim {decim} {name}: frontend_batch err {err:.3e}, filter err {err2:.3e}, bound {bound:.3e}")
    assert err <= bound and err2 <= bound


# ---- limits -------------------------------------------------------------------------------------------------------------------------
def coarse_scan_lds(cx, nwin, mv_len):
    """cs_carve().launch (kernels_detect.h): the scan's own part (gsmcal_coarse_scan_lds_fixed: state copy, twiddles, hop buffers), then
    nwin + mv_len + 128 SNRs"""
    return cx.lib.gsmcal_coarse_scan_lds_fixed() + (nwin + mv_len + 128) * 8


def fir_decim_raw_lds(ntaps, decim):
    """host_plan.h fir_decim_raw: the taps, then the block's raw span as ushorts with 16 bytes of padding per 64 samples"""
    span = 256 * decim + ntaps + 24
    return ((ntaps * 8 + 15) & ~15) + (span + span // 8 + 16) * 2


def raw_move(cx, s, mv_len, fft_len, th):
    s = cbuf(s)
    hf, out = C.c_int(-7), [C.c_double(math.nan) for _ in range(3)]
    rc = cx.lib.gsmcal_move_fft_snr_runtime_avg(cx.h, dp(s), len(s), mv_len, fft_len, th, C.byref(hf), *[C.byref(v) for v in out])
    return rc, hf.value, [v.value for v in out]


def test_window_lengths_outside_2_to_64_are_refused(g, ctx, det, captures):
    s, _ = det
    rc, hf, out = raw_move(ctx, s, 10, 65, 10.0)
    assert rc == E_UNSUPPORTED and hf == -7 and all(math.isnan(v) for v in out)
    ts = (C.c_double * 2)(100.0, 110.0)
    hf, hi, hs = C.c_int(-7), C.c_double(math.nan), C.c_double(math.nan)
    sb = cbuf(s)
    rc = ctx.lib.gsmcal_specific_fft_snr_fix_avg(ctx.h, dp(sb), len(sb), ts, 65, 10.0, 0.0, C.byref(hf), C.byref(hi), C.byref(hs))
    assert rc == E_UNSUPPORTED and hf.value == -7 and math.isnan(hi.value) and math.isnan(hs.value)
    # a window of fewer than two samples handed in directly is an argument out of its range: GSMCAL_E_ARG, nothing written
    for f in (1, 0, -3):
        rc, hf, out = raw_move(ctx, s, 10, f, 10.0)
        assert rc == E_ARG and hf == -7 and all(math.isnan(v) for v in out), (f, rc)
        hf, hi, hs = C.c_int(-7), C.c_double(math.nan), C.c_double(math.nan)
        rc = ctx.lib.gsmcal_specific_fft_snr_fix_avg(ctx.h, dp(sb), len(sb), ts, f, 10.0, 0.0, C.byref(hf), C.byref(hi), C.byref(hs))
        assert rc == E_ARG and hf.value == -7 and math.isnan(hi.value) and math.isnan(hs.value), (f, rc)
    # FCCH_coarse_position: dr = 1 asks for 128-point windows, dr >= 75 for windows of one sample; 2 .. 74 are served (above)
    assert gc.coarse_geometry(1)["fft_len"] == 128 and gc.coarse_geometry(75)["fft_len"] == 1 and gc.coarse_geometry(74)["fft_len"] == 2
    for dr, r8 in ((1, captures["dongle0"][: 8 * 40000]), (75, captures["dongle0"]), (148, captures["dongle0"]), (149, captures["dongle0"]),
                   (1000, captures["dongle0"])):
        x = cbuf(gc.coarse_cut(r8, dr))
        assert len(x) >= gc.coarse_geometry(dr)["n_first"]
        pos, snr = np.full(24, np.nan), np.full(24, np.nan)
        cnt = C.c_int(-7)
        rc = ctx.lib.gsmcal_FCCH_coarse_position(ctx.h, dp(x), len(x), dr, dp(pos), dp(snr), 24, C.byref(cnt))
        assert rc == E_UNSUPPORTED and cnt.value == -7 and np.all(np.isnan(pos)) and np.all(np.isnan(snr)), (dr, rc)


def test_coarse_scan_lds_limit(g, ctx, captures):
    """the scan keeps len + mv_len + 128 SNRs in LDS behind its fixed part: the longest stream that fits is served and agrees
    with the oracle, one more sample is GSMCAL_E_UNSUPPORTED with nothing written"""
    assert 4096 < ctx.lib.gsmcal_coarse_scan_lds_fixed() < 32768
    s = np.ascontiguousarray(captures["dongle0"][0::32])
    for fft_len, mv_len, th in ((4, 40, 10.0), (8, 5000, 10.0)):
        n_max = max(n for n in range(1000, len(s)) if coarse_scan_lds(ctx, n, mv_len) <= LDS_LIMIT)
        assert coarse_scan_lds(ctx, n_max, mv_len) <= LDS_LIMIT < coarse_scan_lds(ctx, n_max + 1, mv_len) and n_max + 1 < len(s)
        want = o.move_fft_snr_runtime_avg(s[:n_max], mv_len, fft_len, th)
        assert gc.move_margin(gc.window_snrs(s[:n_max], fft_len), mv_len, th)[2] > gc.MARGIN_DB
        got = g.move_fft_snr_runtime_avg(s[:n_max], mv_len, fft_len, th)
        print("coarse scan LDS: longest stream", n_max, "mv_len", mv_len, want)
        assert got[:2] == want[:2] and snr_close(got[2], want[2]) and snr_close(got[3], want[3]), (got, want)
        rc, hf, out = raw_move(ctx, s[:n_max + 1], mv_len, fft_len, th)
        assert rc == E_UNSUPPORTED and hf == -7 and all(math.isnan(v) for v in out)


@pytest.mark.parametrize("name", ["one", "two", "ramp300"])
def test_front_end_decimation_limit(g, ctx, fe, name):
    """k_fir_decim_raw stages 256 decim + ntaps samples per block: the largest decim whose span fits 159 KiB is served and
    agrees with the oracle over more than one block, the next one is GSMCAL_E_UNSUPPORTED with nothing written"""
    coef = fe[0][name]
    ntaps = len(coef)
    d_max = max(d for d in range(1, 400) if fir_decim_raw_lds(ntaps, d) <= LDS_LIMIT)
    assert fir_decim_raw_lds(ntaps, d_max) <= LDS_LIMIT < fir_decim_raw_lds(ntaps, d_max + 1) and 270 < d_max < 290
    n = 257 * d_max + 3                                           # 258 outputs: two blocks, the first one full
    raw = np.random.default_rng(d_max).integers(0, 256, size=(2, 2 * n), dtype=np.uint8)
    x = o.raw2iq(raw.T.astype(np.float64))
    want = o.matlab_filter(coef, x)[0::d_max]
    got = g.frontend_batch(raw, coef, d_max)
    assert got.shape == (2, 258)
    err = np.max(np.abs(got.T - want))
    print(f"{name}: largest decim {d_max}, err {err:.3e}, bound {gc.fe_bound(coef, x):.3e}")
    assert err <= gc.fe_bound(coef, x)
    out = np.full((2, -(-n // (d_max + 1)), 2), np.nan)
    c = np.ascontiguousarray(coef)
    rc = ctx.lib.gsmcal_frontend_batch(ctx.h, raw.ctypes.data_as(C.POINTER(C.c_uint8)), 2, n, dp(c), ntaps, d_max + 1, dp(out))
    assert rc == E_UNSUPPORTED and np.all(np.isnan(out))
    # gsmcal_filter has no staging and no such limit
    got2 = g.filter(coef, x, d_max + 1)
    assert np.max(np.abs(got2 - o.matlab_filter(coef, x)[0::d_max + 1])) <= gc.fe_bound(coef, x)


def test_the_certificate_serves_every_ratio_but_the_largest():
    assert [ov for ov in gc.OVS + (ROUTE_OV, CHAIN_MAX_OV) if not certificate_fits(ov)] == [CHAIN_MAX_OV]
    print("certificate fits up to", max(ov for ov in range(1, 64) if certificate_fits(ov)))


def test_chain_ratio_limit_is_thirty():
    lds = chain_lds(CHAIN_MAX_OV + 1, 64 * (CHAIN_MAX_OV + 1))
    print(CHAIN_MAX_OV, chain_lds(CHAIN_MAX_OV, 64 * CHAIN_MAX_OV), lds)
    assert CHAIN_MAX_OV == gc.CHAIN_MAX_OV == 30 and max(lds, key=lds.get).startswith("k_burst_tone")
    assert all(v <= LDS_LIMIT for k, v in lds.items() if not k.startswith("k_burst_tone"))      # the chunk sweep follows at 34
    assert (128 * 127 + 63) // 64 <= 255 < (128 * 128 + 63) // 64                                 # the guard behind it: 255 chunks


@pytest.mark.parametrize("ov", (CHAIN_MAX_OV + 1, 34, 128))
def test_chain_refuses_ratios_its_kernels_cannot_hold(g, ctx, chain_inputs, ov):
    """The chain's three functions share one range: the largest ratio whose launches all fit 159 KiB (chain_lds) runs against the
    oracle on three paths in test_chain_function_by_function_at_other_oversampling_ratios; the next one, the ratio at which the
    chunk sweep stops fitting and the one that passes 255 chunks are GSMCAL_E_UNSUPPORTED on the host, nothing written."""
    assert max(chain_lds(ov, 64 * ov).values()) > LDS_LIMIT
    r, ts, want = chain_inputs("plain", CHAIN_MAX_OV)
    s, t = cbuf(r[:400000]), cbuf(gc.training_sequence(CHAIN_MAX_OV))
    bp = np.ascontiguousarray(want["coarse_pos"][:5])
    pos, rr = np.full(24, np.nan), np.full((len(s), 2), np.nan)
    npos, lr, sp, cp = C.c_int(-7), C.c_long(-7), C.c_double(math.nan), C.c_double(math.nan)
    rc = ctx.lib.gsmcal_FCCH_fine_correction(ctx.h, dp(s), len(s), dp(bp), len(bp), ov, FC, dp(pos), 24, C.byref(npos), dp(rr), len(s),
                                             C.byref(lr), C.byref(sp), C.byref(cp))
    assert rc == E_UNSUPPORTED and npos.value == -7 and lr.value == -7 and np.all(np.isnan(pos)) and np.all(np.isnan(rr))
    assert math.isnan(sp.value) and math.isnan(cp.value)
    fp = np.ascontiguousarray(want["fcch_pos"])
    pi = np.full((2, 144), np.nan)
    nrows, lr, sp = C.c_int(-7), C.c_long(-7), C.c_double(math.nan)
    rc = ctx.lib.gsmcal_SCH_corr_rate_correction(ctx.h, dp(s), len(s), dp(fp), len(fp), dp(t), len(t), ov, dp(pi), 144, C.byref(nrows),
                                                 dp(rr), len(s), C.byref(lr), C.byref(sp))
    assert rc == E_UNSUPPORTED and nrows.value == -7 and lr.value == -7 and np.all(np.isnan(pi)) and np.all(np.isnan(rr)) and math.isnan(sp.value)
    pic = np.ascontiguousarray(want["pos_info"].T)
    lr, cp = C.c_long(-7), C.c_double(math.nan)
    rc = ctx.lib.gsmcal_carrier_correct_post_SCH(ctx.h, dp(s), len(s), dp(pic), pic.shape[1], pic.shape[1], ov, FC, dp(rr), len(s),
                                                 C.byref(lr), C.byref(cp))
    assert rc == E_UNSUPPORTED and lr.value == -7 and np.all(np.isnan(rr)) and math.isnan(cp.value)


def fcch_demod_lds(ov):
    """kernels_demod.h fd_lds_bytes: the window, the 37 x (N2 + 1) matrix and the two twiddle tables"""
    nfft = 148 * ov
    return (nfft + 37 * (nfft // 37 + 1) + 40 + nfft // 37) * 16


FCCH_DEMOD_MAX_OV = max(ov for ov in range(1, 257) if fcch_demod_lds(ov) <= LDS_LIMIT)


def test_FCCH_demod_ratio_limit(g, ctx):
    """33x, the largest ratio whose window fits, on tones (the bar of test_gpu_fcch_demod.py's tone test: 1e-6 of the sampling rate);
    34x is GSMCAL_E_UNSUPPORTED with nothing written"""
    assert FCCH_DEMOD_MAX_OV == 33 and fcch_demod_lds(33) <= LDS_LIMIT < fcch_demod_lds(34)
    ov = FCCH_DEMOD_MAX_OV
    for k in (37, -30):
        s, pos = ref.tone_windows(ov, k)
        want = ref.fcch_demod(s, pos, ov, FC)
        got = g.FCCH_demod(s, pos, ov, FC)
        assert np.all(want["max_idx"] == k) and np.all(np.isfinite(want["snr"]))
        tol = 1e-6 * ref.SYMBOL_RATE * ov
        assert np.all(np.abs(want["noise_ratio"]) >= 1e-3) and np.array_equal(got["max_idx"], want["max_idx"])
        assert np.all(np.abs(got["freq"] - want["freq"]) <= tol) and abs(got["mean_freq"] - want["mean_freq"]) <= tol
        assert abs(got["carrier_ppm"] - want["carrier_ppm"]) <= 1e6 * tol / FC and np.all(np.abs(got["snr"] - want["snr"]) <= 1e-6)
    ov = FCCH_DEMOD_MAX_OV + 1
    s, pos = ref.tone_windows(ov, 37)
    sb, pic = cbuf(s), np.ascontiguousarray(pos.T)
    freq, snr, idx = (np.full(3, np.nan) for _ in range(3))
    nb, mf, cp = C.c_int(-7), C.c_double(math.nan), C.c_double(math.nan)
    rc = ctx.lib.gsmcal_FCCH_demod(ctx.h, dp(sb), len(sb), dp(pic), 3, 3, ov, FC, dp(freq), dp(snr), dp(idx), 3, C.byref(nb), C.byref(mf), C.byref(cp))
    assert rc == E_UNSUPPORTED and nb.value == 0 and all(np.all(np.isnan(a)) for a in (freq, snr, idx)) and math.isnan(mf.value)
