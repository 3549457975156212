"""CPU tests of the multi-channel diversity scanner (multi_rtl_sdr_diversity_scanner_another_bak.m): the frequency plan of
:64-81, the two restatements the GPU tests compare against (tests/subband_ref.py), the record of :225-231, the sign convention,
and the C ABI / MEX surface of gsmcal_subband_power_batch.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import subband_ref as ref

import gsmcal.dist  # noqa: F401  (gsmcal does not import its multi-GPU layer by itself)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gsmcal_subband_power_batch", "gsmcal_subband_power_batch_dev")
FS = ref.FS


def _plan_literal(start, stop, step, fs):
    """:64-81 statement by statement (1-based find() turned into 0-based indices)."""
    def colon(a, d, b):
        out, k = [], 0
        while a + k * d <= b + 1e-6:
            out.append(a + k * d)
            k += 1
        return out
    freq = colon(start, step, stop)                                              # :64
    real_freq_step = fs / 4                                                      # :65
    real_freq = colon(start, real_freq_step, stop)                               # :66
    if real_freq[-1] + (real_freq_step / 2) < freq[-1]:                          # :67
        real_freq = real_freq + [real_freq[-1] + real_freq_step]                 # :68
    info = []
    for i in range(len(real_freq)):                                              # :73
        freq_start = real_freq[i] - (real_freq_step / 2)                         # :75
        freq_end = real_freq[i] + (real_freq_step / 2)                           # :76
        freq_set = [k for k, f in enumerate(freq) if f > freq_start and f <= freq_end]     # :77
        info.append((real_freq[i], freq_set, [freq[k] - real_freq[i] for k in freq_set]))  # :74,78-80
    return freq, info


@pytest.mark.parametrize("start, stop, step, nfreq, counts, slots", [
    (935e6, 942e6, 0.1e6, 71, [3, 5, 5, 5, 6, 5, 5, 5, 5, 5, 5, 5, 6, 5, 1], 7),
    (935e6, 937e6, 0.05e6, 41, [6, 10, 10, 10, 5], 12),
    (1176.45e6, 1177.5e6, 0.1e6, 11, [3, 5, 3], None),
    (935e6, 935e6, 0.1e6, 1, [1], None),
    (935e6, 960e6, 0.1e6, 251, None, 7),
    (935e6, 960e6, 0.05e6, 501, None, 12)])
def test_plan_matches_the_literal_loop(gsmcal_mod, start, stop, step, nfreq, counts, slots):
    plan = gsmcal_mod.dist.multichannel_frequency_plan(start, stop, step, FS)
    freq, info = _plan_literal(start, stop, step, FS)
    assert len(plan["freq"]) == nfreq == len(freq) and np.array_equal(plan["freq"], np.array(freq))
    assert len(plan["real_freq"]) == len(info)
    got_counts = [len(k) for k in plan["freq_set"]]
    if counts is not None:
        assert got_counts == counts
    else:
        assert len(plan["real_freq"]) == 50 and sum(got_counts) == nfreq        # 50 captures instead of 251 (501) tunings
    for c, (centre, fset, rel) in enumerate(info):
        assert plan["real_freq"][c] == centre
        assert plan["freq_set"][c].tolist() == fset
        assert np.array_equal(plan["relative_sub_freq_set"][c], np.array(rel))
    # every grid point exactly once, in order: idx of :186-210 runs 1..length(freq) capture by capture
    assert np.concatenate(plan["freq_set"]).tolist() == list(range(nfreq))
    if slots is not None:
        assert int(np.ceil((FS / 4) / step)) + 1 == slots and max(got_counts) <= slots          # :71


def test_plan_tie_at_plus_a_quarter_step_goes_to_the_lower_capture(gsmcal_mod):
    """935-942 MHz at 100 kHz: capture 12 (941.144 MHz) ends with relative offset +256 000 Hz exactly -- the <= of :77 keeps
    941.4 MHz there, the strict > keeps it out of capture 13."""
    plan = gsmcal_mod.dist.multichannel_frequency_plan(935e6, 942e6, 0.1e6, FS)
    assert plan["real_freq"][12] == 941.144e6
    assert plan["relative_sub_freq_set"][12][-1] == 256000.0 and plan["freq"][plan["freq_set"][12][-1]] == 941.4e6
    assert plan["relative_sub_freq_set"][13][0] == -156000.0
    with pytest.raises(ValueError):
        gsmcal_mod.dist.multichannel_frequency_plan(935e6, 934e6, 0.1e6, FS)


@pytest.mark.parametrize("ntaps, decim, n, w", [(32, 1, 97, 0.3), (64, 1, 200, -1.7), (7, 3, 40, 3.0), (1, 1, 33, 0.5),
                                                (12, 50, 9, -0.2), (33, 7, 120, 40.0)])
def test_literal_matches_its_per_sample_loop_and_the_exact_form(ntaps, decim, n, w):
    rng = np.random.default_rng(ntaps * 1000 + n)
    a = rng.integers(0, 256, 2 * n).astype(np.uint8)
    coef = rng.standard_normal(ntaps)
    lit = ref.literal(a, coef, w, decim)
    assert abs(ref.loop(a, list(coef), w, decim) - lit) <= 1e-12 * lit
    assert abs(ref.exact(a, coef, w, decim) - lit) <= 1e-12 * lit
    c = np.full(2 * n, 77, dtype=np.uint8)
    assert ref.literal(c, coef, w, decim) == 0.0 and ref.loop(c, list(coef), w, decim) == 0.0 and ref.exact(c, coef, w, decim) == 0.0


def _agree(raw, coef, w, decim, rows=None, tol=1e-11):
    lit = ref.table(ref.literal, raw, coef, w, decim, rows)
    ex = ref.table(ref.exact, raw, coef, w, decim, rows)
    assert np.array_equal(np.isnan(lit), np.isnan(ex))
    worst = 0.0
    for a, b in zip(lit.ravel(), ex.ravel()):
        if np.isnan(b):
            continue
        if b == 0.0:
            assert a == 0.0
        else:
            worst = max(worst, abs(a - b) / b)
    assert worst <= tol, worst
    return worst


@pytest.mark.parametrize("name", ref.CASES + ("defaults", "large_dc", "many"))
def test_literal_and_exact_agree_on_every_gpu_input(gsmcal_mod, name):
    """The reference's own rounding (the n*w product of :196, n up to 4e5) against the form the kernel computes, on every input
    of tests/test_gpu_subband.py: within 1e-11 everywhere, so the GPU tests compare against `literal` at 1e-10 throughout.
    Largest figures seen: 4.6e-12 ("phases": w = 40 at n = 30 001), 6.8e-13 ("128taps/16"), 6.5e-13 ("defaults", n = 409 600)."""
    sf = gsmcal_mod.dist.spectrum_filter
    if name == "many":
        _agree(*ref.many(sf), rows=ref.MANY_ROWS)
    elif name in ("defaults", "large_dc"):
        _agree(*getattr(ref, name)(sf))
    else:
        _agree(*ref.case(name, sf))


def test_mirror_states_the_sign_convention():
    """With c = I + jQ a carrier at RF centre + f sits at +f; exp(+1i*n*w) (:195-196 as written, w = 2*pi*f/fs) moves it to 2f and
    brings centre - f to 0 Hz.  Stated without a GPU: +w on a capture equals -w on the capture with Q negated (its mirror
    image about the centre) -- exactly, DC and all."""
    rng = np.random.default_rng(5)
    n = 3000
    k = np.arange(n)
    f = 150e3
    i = 127.5 + 40 * np.cos(2 * np.pi * f / FS * k) + rng.standard_normal(n)
    q = 127.5 + 40 * np.sin(2 * np.pi * f / FS * k) + rng.standard_normal(n)
    a = np.empty(2 * n, dtype=np.uint8)
    a[0::2], a[1::2] = np.clip(np.rint(i), 0, 255), np.clip(np.rint(q), 0, 255)
    b = a.copy()
    b[1::2] = 255 - a[1::2]                                                      # Q negated about mid-scale: conj after raw2iq's DC removal
    import gsmcal
    coef = gsmcal.dist.spectrum_filter(FS, 100e3, 0.2)[1]
    w = 2 * np.pi * f / FS
    up, down = ref.literal(a, coef, +w), ref.literal(a, coef, -w)
    assert abs(ref.literal(b, coef, -w) - up) <= 1e-12 * up and abs(ref.literal(b, coef, +w) - down) <= 1e-12 * down
    assert down > 1e3 * up                                                       # the carrier at +f is found with -w (shift_sign = -1)


def test_record_fields_shapes_and_name(gsmcal_mod):
    rng = np.random.default_rng(3)
    ps = rng.random((4, 251))
    rec = gsmcal_mod.dist.multichannel_spectrum_record(ps, 935e6, 960e6, 0.1e6, 4, 12.5, 0.2, FS)
    # save(filename, 'power_spectrum', 'power_spectrum_combine', 'start_freq', 'end_freq', 'freq_step', 'observe_time', 'RBW',
    #      'gain', 'sample_rate', 'coef')   :231
    assert set(rec) == {"power_spectrum", "power_spectrum_combine", "start_freq", "end_freq", "freq_step", "observe_time",
                        "RBW", "gain", "sample_rate", "coef", "filename"}
    assert rec["power_spectrum"].shape == (4, 251) and rec["power_spectrum_combine"].shape == (251,)
    assert np.array_equal(rec["power_spectrum_combine"], np.mean(ps, axis=0))   # :227, linear
    assert rec["filename"] == "scan_935000000_960000000_gain12.5_4dongles.mat"  # :230
    assert (rec["RBW"], rec["observe_time"], rec["sample_rate"], len(rec["coef"])) == (0.1e6, 0.2, FS, 32)
    assert np.array_equal(rec["coef"], gsmcal_mod.dist.spectrum_filter(FS, 0.1e6, 0.2)[1])
    with pytest.raises(ValueError):
        gsmcal_mod.dist.multichannel_spectrum_record(rng.random((4, 250)), 935e6, 960e6, 0.1e6, 4, 0, 0.2, FS)


def test_header_exports_and_prototypes(gsmcal_mod):
    txt = open(os.path.join(ROOT, "include", "gsmcal.h")).read()
    assert int(re.search(r"#define GSMCAL_MAX_SUBBANDS (\d+)", txt).group(1)) == gsmcal_mod.MAX_SUBBANDS == 16
    src = open(os.path.join(ROOT, "multi-rtl-sdr-calibration_amd", "csrc", "abi_calls.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in gsmcal_mod.SIGNATURES
        assert hasattr(gsmcal_mod.load(), name)
        # ctx, raw, d, n, coef, ntaps, decim, phase_rotate, nsub, power
        res, args = gsmcal_mod.SIGNATURES[name]
        assert res is C.c_int and len(args) == 10
        assert [args[i] for i in (2, 3, 5, 6, 8)] == [C.c_int, C.c_long, C.c_int, C.c_int, C.c_int]
        assert args[7] is gsmcal_mod._lib.c_double_p                            # phase_rotate: host doubles in both forms
    for fn in ("subband_power_batch", "subband_power_batch_dev", "multichannel_spectrum_scan"):
        assert callable(getattr(gsmcal_mod, fn))


def test_null_context_and_bad_arguments_are_refused(gsmcal_mod):
    """GSMCAL_E_ARG before anything touches a device: a NULL context with good and with every kind of bad argument."""
    lib = gsmcal_mod.load()
    raw = np.zeros((2, 64), dtype=np.uint8)
    coef = np.ones(4)
    w = np.zeros((2, 3))
    out = np.zeros((2, 3))
    dp = C.POINTER(C.c_double)
    rp, cp, wp, op = raw.ctypes.data_as(C.POINTER(C.c_uint8)), coef.ctypes.data_as(dp), w.ctypes.data_as(dp), out.ctypes.data_as(dp)
    rv, ov = C.c_void_p(raw.ctypes.data), C.c_void_p(out.ctypes.data)
    E_ARG = -1
    assert lib.gsmcal_subband_power_batch(None, rp, 2, 32, cp, 4, 1, wp, 3, op) == E_ARG
    assert lib.gsmcal_subband_power_batch_dev(None, rv, 2, 32, cp, 4, 1, wp, 3, ov) == E_ARG
    for d, n, nt, dec, ns in ((0, 32, 4, 1, 3), (-1, 32, 4, 1, 3), (2, 0, 4, 1, 3), (2, 32, 0, 1, 3), (2, 32, 129, 1, 3),
                              (2, 32, 4, 0, 3), (2, 32, 4, 1, 0), (2, 32, 4, 1, 17)):
        assert lib.gsmcal_subband_power_batch(None, rp, d, n, cp, nt, dec, wp, ns, op) == E_ARG
        assert lib.gsmcal_subband_power_batch_dev(None, rv, d, n, cp, nt, dec, wp, ns, ov) == E_ARG
    for args in ((None, 2, 32, cp, 4, 1, wp, 3, op), (rp, 2, 32, None, 4, 1, wp, 3, op), (rp, 2, 32, cp, 4, 1, None, 3, op),
                 (rp, 2, 32, cp, 4, 1, wp, 3, None)):
        assert lib.gsmcal_subband_power_batch(None, *args) == E_ARG
    w[1, 2] = np.inf
    assert lib.gsmcal_subband_power_batch(None, rp, 2, 32, cp, 4, 1, wp, 3, op) == E_ARG
    assert lib.gsmcal_subband_power_batch_dev(None, rv, 2, 32, cp, 4, 1, wp, 3, ov) == E_ARG


def test_scan_refuses_more_points_per_capture_than_slots(gsmcal_mod):
    """10 kHz steps put 52 grid points into a capture: more than GSMCAL_MAX_SUBBANDS, refused before any GPU work."""
    n = gsmcal_mod.dist.spectrum_filter(FS, 10e3, 0.001)[3]
    plan = gsmcal_mod.dist.multichannel_frequency_plan(935e6, 936e6, 10e3, FS)
    assert max(len(k) for k in plan["freq_set"]) > gsmcal_mod.MAX_SUBBANDS
    r = np.zeros((2 * n, 1, len(plan["real_freq"])), dtype=np.uint8)
    with pytest.raises(ValueError, match="grid points"):
        gsmcal_mod.multichannel_spectrum_scan(r, 935e6, 936e6, 10e3, observe_time=0.001, sample_rate=FS, ctx=object())
    with pytest.raises(ValueError):
        gsmcal_mod.multichannel_spectrum_scan(r, 935e6, 936e6, 10e3, observe_time=0.001, sample_rate=FS, shift_sign=0, ctx=object())


@pytest.mark.parametrize("api", ["interleaved", "split"])
def test_mex_subband_power_target_compiles_against_the_abi(api):
    """The gsmcal_subband_power MEX target through the same gcc -fsyntax-only check as the other targets (test_abi_cpu.py)."""
    r = subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-std=c99", "-DGSMCAL_FN_gsmcal_subband_power"] +
                       (["-DGSMCAL_STUB_SPLIT"] if api == "split" else []) +
                       ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mex_stub"),
                        os.path.join(ROOT, "mex", "gsmcal_mex.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(ROOT, "mex", "gsmcal_mex.c")).read()
    assert re.search(r"for f in [^;]*\bgsmcal_subband_power\b[^;]*; do", src)   # in the build loop of the header comment
    assert "gsmcal_subband_power" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
