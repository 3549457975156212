"""mex/gsmcal_mex.c, run: every one of its 22 targets, in both complex-storage modes, is built against a working mxArray stand-in
(tests/mex_stub/mxstub.c) and a recording fake of the ABI (tests/mex_stub/fake_gsmcal.c) and called through tests/mex_gateway.py.
What is held here is the marshalling between a MATLAB caller and the library: arguments decided before the ABI is touched, status
codes turned into errors or sentinels, lengths / leading dimensions / defaults as passed, class, shape and orientation of every
output -- the fake fills each output with an index pattern (output j, element k: 1000*(j+1) + k, imaginary part its negative),
so a value shows where column-major storage puts it.  No GPU is needed."""
import numpy as np
import pytest

import mex_gateway as mg

MAX_HITS, MAX_POS_ROWS = 24, 144
S_NO_FCCH, S_POST_NO_POS, S_POST_FEW_BCCH, S_ALL_INF, S_BCCH_NO_DECODE = 1, 10, 11, 12, 15
FC = 957.4e6


def pat(j, n):
    return 1000.0 * (j + 1) + np.arange(n, dtype=np.float64)


def patc(j, n):
    return pat(j, n) - 1j * pat(j, n)


def F(v, m, n):
    return np.asarray(v).reshape((m, n), order="F")


def col(v):
    return np.asarray(v).reshape(-1, 1)


def row(v):
    return np.asarray(v).reshape(1, -1)


def cvec(n, seed):
    """n distinct complex samples whose real and imaginary parts cannot be confused"""
    k = np.arange(n, dtype=np.float64)
    return (seed + k) + 1j * (100.0 * seed + 0.5 + k)


S9, S8 = col(cvec(9, 1)), col(cvec(8, 2))
S73 = F(cvec(21, 3), 7, 3)
U83 = F((np.arange(24) * 7 + 3) % 256, 8, 3).astype(np.uint8)
POS = np.array([[11.0, 0], [12, 1], [13, 2], [14, 2], [15, 2]])              # 5 x 2
TS6 = row(cvec(6, 4))
TPL = F(cvec(32, 5), 4, 8)                                                     # 4 x 8 templates
COEF = row([0.25, 0.5, 1.0, 0.5, 0.25])
PARAMS = row([1.5, -2.0, 30.0, 0.25, 4.0, 1.0])
PHI = np.array([[0.1, 0.2, np.nan], [np.nan, 0.4, 0.5]])                      # 2 x 3


def cell_expect(count=3):
    pi = pat(1, 3 * 2 * MAX_POS_ROWS)
    cells = []
    for i in range(3):
        r = count + i
        cells.append(np.stack([pi[i * 288:i * 288 + r], pi[i * 288 + 144:i * 288 + 144 + r]], axis=1))
    return cells


def table_expect(count=3):
    t = pat(0, 30).reshape(3, 10)
    t[:, 7] = count + np.arange(3)
    return t


SCH_ROW, SI_ROW, PAIR_ROW = pat(3, 176), pat(4, 172), pat(5, 736)

# target -> args of a valid call, the ABI function it must reach, what the fake must have seen (scalars as text, the inputs it
# hashed in order) and every output at the default preset (status 0, count 3, len_r 5), nlhs = all of them
SPECS = {
    "raw2iq": dict(args=[U83], fn="raw2iq_u8", seen=dict(rows_2n="8", d="3"), hashed=[U83], out=[F(patc(0, 12), 4, 3)], says=False),
    "chn_filter_8x_4x": dict(args=[S73], fn="chn_filter_8x_4x", seen=dict(n="7", d="3", num="0", ntaps="0"), hashed=[S73],
                             out=[F(patc(0, 12), 4, 3)], says=False),
    "chn_filter_4x": dict(args=[S73], fn="chn_filter_4x", seen=dict(n="7", d="3", num="0", ntaps="0"), hashed=[S73],
                          out=[F(patc(0, 21), 7, 3)], says=False),
    "move_fft_snr_runtime_avg": dict(args=[S9, 4.0, 16.0, 10.5], fn="move_fft_snr_runtime_avg",
                                     seen=dict(len="9", mv_len="4", fft_len="16", th="10.5"), hashed=[S9],
                                     out=[np.array([[True]]), F([2000.0], 1, 1), F([3000.0], 1, 1), F([4000.0], 1, 1)], says=False),
    "specific_fft_snr_fix_avg": dict(args=[S9, row([3.0, 5.0]), 16.0, 10.5, 2.25], fn="specific_fft_snr_fix_avg",
                                     seen=dict(len="9", fft_len="16", th="10.5", avg_snr="2.25"), hashed=[S9, [3.0, 5.0]],
                                     out=[np.array([[True]]), F([2000.0], 1, 1), F([3000.0], 1, 1)], says=False),
    "FCCH_coarse_position": dict(args=[S9, 8.0], fn="FCCH_coarse_position", seen=dict(len="9", decimation_ratio="8", cap="24"),
                                 hashed=[S9], out=[row(pat(0, 3)), row(pat(1, 3))], says=True),
    "FCCH_fine_correction": dict(args=[S9, row([5.0, 6, 7, 8]), 4.0, FC], fn="FCCH_fine_correction",
                                 seen=dict(len="9", num_base="4", ov="4", carrier_freq="957400000", cap_pos="24", r="1", cap_r="9"),
                                 hashed=[S9, [5.0, 6, 7, 8]], out=[row(pat(0, 3)), col(patc(1, 5)), F([3000.0], 1, 1), F([4000.0], 1, 1)],
                                 says=True),
    "SCH_corr_rate_correction": dict(args=[S9, row([1.0, 2, 3]), TS6, 4.0], fn="SCH_corr_rate_correction",
                                     seen=dict(s="1", len="9", num_fcch="3", len_ts="6", ov="4", cap_rows="144", r="1", cap_r="9"),
                                     hashed=[S9, [1.0, 2, 3], TS6],
                                     out=[np.stack([pat(0, 3), pat(1, 3)], axis=1), col(patc(2, 5)), F([4000.0], 1, 1)], says=True),
    "carrier_correct_post_SCH": dict(args=[S9, POS, 4.0, FC], fn="carrier_correct_post_SCH",
                                     seen=dict(s="1", len="9", rows="5", ld="5", ov="4", carrier_freq="957400000", r="1", cap_r="9"),
                                     hashed=[S9, POS], out=[col(patc(0, 5)), F([2000.0], 1, 1)], says=True),
    "FCCH_demod": dict(args=[S9, POS, 4.0, FC], fn="FCCH_demod",
                       seen=dict(s="1", len="9", rows="5", ld="5", ov="4", carrier_freq="957400000", cap="24"), hashed=[S9, POS],
                       out=[row(pat(0, 3)), row(pat(1, 3)), row(pat(2, 3)), F([5000.0], 1, 1)], says=True),
    "BCCH_demod": dict(args=[S9, POS, TPL, 4.0, FC], fn="BCCH_demod",
                       seen=dict(s="1", len="9", rows="5", ld="5", len_ts="4", ov="4", carrier_freq="957400000", r="1", cap_r="9",
                                 table_row="0"), hashed=[S9, POS, TPL],
                       out=[F([3.0], 1, 1), col(patc(1, 5)), F([3000.0], 1, 1), F(patc(3, 32), 8, 4)], says=True),
    "SCH_decode": dict(args=[S9, POS, TS6, 4.0], fn="SCH_decode",
                       seen=dict(s="1", len="9", rows="5", ld="5", len_ts="6", ov="4", soft="0", u="0"), hashed=[S9, POS, TS6],
                       out=[F([1000.0], 1, 1), F([2000.0], 1, 1), F([3000.0], 1, 1), row(SCH_ROW[8 + 2 * MAX_HITS:][:3]), row(SCH_ROW[8:11])],
                       says=True),
    "BCCH_decode": dict(args=[S9, POS, 2.0, 4.0], fn="BCCH_decode",
                        seen=dict(s="1", len="9", rows="5", ld="5", tsc="2", ov="4", soft="0"), hashed=[S9, POS],
                        out=[F([1000.0], 1, 1), row([2000.0, 2001, 2002]), F([3.0], 1, 1),
                             (np.arange(3 * 23) % 251).reshape(3, 23).astype(np.float64), row(SI_ROW[4:7])], says=True),
    "CW_check": dict(args=[S9], fn="CW_check", seen=dict(len="9"), hashed=[S9], out=[col(pat(0, 8)), F([2000.0], 1, 1)], says=False),
    "IQ_imbalance": dict(args=[S9], fn="IQ_imbalance", seen=dict(len="9"), hashed=[S9],
                         out=[F([4016.0], 1, 1), F([4018.0], 1, 1), F([4019.0], 1, 1), row(pat(3, 22))], says=True),
    "pair_coherence": dict(args=[S9, S8, POS, 4.0], fn="pair_coherence",
                           seen=dict(s_a="1", len_a="9", s_b="1", len_b="8", rows="5", ld="5", ov="4", lag0="0", max_lag="0",
                                     min_coherence="0.5", corr="0"), hashed=[S9, S8, POS],
                           out=[F([PAIR_ROW[k]], 1, 1) for k in (6, 9, 11, 13, 7)] + [row(PAIR_ROW)], says=True),
    "pair_align": dict(args=[S9, 4.0, PARAMS], fn="pair_align", seen=dict(s="1", len="9", ov="4", out_len="9"), hashed=[S9, PARAMS],
                       out=[col(patc(0, 9)), row(pat(1, 4))], says=True),
    "total_ppm_calculation": dict(args=[row([1.5, 2.5, np.inf])], fn="total_ppm_calculation", seen=dict(n="3"), hashed=[[1.5, 2.5, np.inf]],
                                  out=[F([1000.0], 1, 1)], says=False, no_ctx=True),
    "gsmcal_calibrate": dict(args=[U83, COEF, TS6, row([9.0e8, 9.1e8, 9.2e8])], fn="calibrate_batch",
                             seen=dict(d="3", n="4", ntaps="5", len_ts="6", r_correct="0", r_len="0"),
                             hashed=[U83, COEF, TS6, [9.0e8, 9.1e8, 9.2e8]],
                             out=[table_expect(), {"shape": (1, 3), "cells": cell_expect()}], says=False),
    "gsmcal_fcch_scan": dict(args=[U83, COEF], fn="fcch_scan_batch", seen=dict(d="3", n="4", ntaps="5", positions="0", pos_snr="0", counts="0"),
                             hashed=[U83, COEF], out=[row(pat(0, 3)), row(pat(1, 3))], says=False),
    "gsmcal_band_power": dict(args=[U83, COEF, 2.0], fn="band_power_batch", seen=dict(d="3", n="4", ntaps="5", decim="2"), hashed=[U83, COEF],
                              out=[row(pat(0, 3))], says=False),
    "gsmcal_subband_power": dict(args=[U83, COEF, PHI], fn="subband_power_batch", seen=dict(d="3", n="4", ntaps="5", decim="1", nsub="2"),
                                 hashed=[U83, COEF, PHI], out=[F(pat(0, 6), 2, 3)], says=False),
}
# optional trailing arguments: what a valid call may leave out
MIN_NRHS = {t: len(s["args"]) for t, s in SPECS.items()}
USES_POS_INFO = {"carrier_correct_post_SCH": 1, "FCCH_demod": 1, "BCCH_demod": 1, "SCH_decode": 1, "BCCH_decode": 1, "pair_coherence": 2}
BOTH = [(t, m) for t in mg.TARGETS for m in mg.MODES]


def test_every_target_has_a_spec():
    src = open(mg.SOURCE).read()
    assert sorted(SPECS) == sorted(mg.TARGETS) and len(mg.TARGETS) == 22
    assert src.count("defined(GSMCAL_FN_") == 22
    for t in mg.TARGETS:
        assert "defined(GSMCAL_FN_%s)" % t in src


def same(a, b):
    """class, complexity, shape and every value (NaN equal to NaN)"""
    if isinstance(b, dict):
        return isinstance(a, dict) and a["shape"] == b["shape"] and len(a["cells"]) == len(b["cells"]) and \
            all(same(x, y) for x, y in zip(a["cells"], b["cells"]))
    b = np.asarray(b)
    return isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=not a.dtype == np.bool_)


def clean(g, res, calls=1):
    """what holds after every call"""
    assert res.failures == "", res.failures
    assert g.calls() == calls, g.log()


def good_call(g, spec, args=None, nlhs=None, **preset):
    g.preset(**preset)
    res = g.call(*(spec["args"] if args is None else args), nlhs=len(spec["out"]) if nlhs is None else nlhs)
    assert res.err is None, res.err
    clean(g, res)
    return res, g.log()[0]


@pytest.mark.parametrize("target,mode", BOTH)
def test_valid_call_passes_and_returns_what_the_header_says(target, mode):
    g, spec = mg.gateway(target, mode), SPECS[target]
    res, rec = good_call(g, spec)
    assert rec["fn"] == spec["fn"]
    for k, v in spec["seen"].items():
        assert rec[k] == v, (k, rec)
    if not spec.get("no_ctx"):
        assert rec["ctx"] == "1" and g.created() == 1
    assert rec["hash"] == mg.fnv(*spec["hashed"]), "the ABI did not read the inputs in their order and layout"
    n_out = len(spec["out"])
    assert res.set_mask == [True] * n_out + [False] * (mg.MAX_OUT - n_out)
    for i, want in enumerate(spec["out"]):
        assert same(res.out[i], want), (i, res.out[i], want)
    assert res.printed == ("report of %s: 100%% fake\n" % spec["fn"] if spec["says"] else "")


@pytest.mark.parametrize("target", mg.TARGETS)
def test_storage_modes_pass_and_return_the_same(target):
    spec = SPECS[target]
    a, ra = good_call(mg.gateway(target, "interleaved"), spec)
    b, rb = good_call(mg.gateway(target, "split"), spec)
    assert ra == rb
    assert all(same(x, y) if x is not None else y is None for x, y in zip(a.out, b.out)) and a.printed == b.printed


@pytest.mark.parametrize("target,mode", BOTH)
def test_only_the_outputs_asked_for_are_set(target, mode):
    g, spec = mg.gateway(target, mode), SPECS[target]
    for nlhs in range(len(spec["out"]) + 1):
        res, _ = good_call(g, spec, nlhs=nlhs)
        k = max(nlhs, 1) if target != "FCCH_demod" else nlhs      # FCCH_demod.m returns nothing: nlhs = 0 sets nothing
        assert res.set_mask == [True] * k + [False] * (mg.MAX_OUT - k), (nlhs, res.set_mask)
        for i in range(k):
            assert same(res.out[i], spec["out"][i])
    g.preset()
    res = g.call(*spec["args"], nlhs=len(spec["out"]) + 1)        # more outputs than the function has
    assert res.err and res.err[0] == "gsmcal:args" and g.calls() == 0


def refused(g, args, nlhs=1, ident="gsmcal:"):
    """the call ends in a gsmcal: error before the ABI is touched; no context is made for it"""
    before = g.created()
    g.preset()
    res = g.call(*args, nlhs=nlhs)
    assert res.err is not None, "accepted: %s" % (g.log(),)
    assert res.err[0].startswith(ident), res.err
    assert g.calls() == 0 and g.created() == before, g.log()
    assert res.failures == "" and res.set_mask == [False] * mg.MAX_OUT and res.printed == ""
    return res.err


@pytest.mark.parametrize("target,mode", BOTH)
def test_too_few_arguments_are_refused(target, mode):
    g, spec = mg.gateway(target, mode), SPECS[target]
    for k in range(MIN_NRHS[target]):
        err = refused(g, spec["args"][:k])
        assert "usage:" in err[1] and target.replace("gsmcal_", "") in err[1]
    most = {"pair_coherence": 7, "pair_align": 4, "gsmcal_subband_power": 4}.get(target, MIN_NRHS[target])
    refused(g, spec["args"] + [1.0] * (most + 1 - MIN_NRHS[target]))         # and one too many


@pytest.mark.parametrize("target,mode", BOTH)
def test_an_argument_of_another_class_is_refused(target, mode):
    """no typed accessor is taken of an array of another class: logical anywhere, uint8 where doubles are expected (raw2iq takes
    both), doubles where the raw bytes are expected, complex where a real table is expected"""
    g, spec = mg.gateway(target, mode), SPECS[target]
    for i, a in enumerate(spec["args"]):
        a = np.atleast_2d(np.asarray(a))
        refused(g, spec["args"][:i] + [np.ones(a.shape, dtype=bool)] + spec["args"][i + 1:])
        if a.dtype == np.uint8:
            other = a.astype(np.float64) if target != "raw2iq" else None
        else:
            other = np.ones(a.shape, dtype=np.uint8)
        if other is not None:
            refused(g, spec["args"][:i] + [other] + spec["args"][i + 1:])
        if not np.iscomplexobj(a) and a.dtype != np.uint8:
            refused(g, spec["args"][:i] + [np.nan_to_num(a) + 1j] + spec["args"][i + 1:])
    g.run_atexit()
    assert g.created() == g.destroyed()


@pytest.mark.parametrize("mode", mg.MODES)
def test_class_checks_also_hold_without_mxIsDouble(mode):
    """built without MATLAB_MEX_FILE, as the -fsyntax-only checks see the gateway against the reduced mex.h, the class is read off
    the typed accessors: the same refusals, the same valid call"""
    for target in ("raw2iq", "chn_filter_4x", "carrier_correct_post_SCH", "pair_align", "total_ppm_calculation", "gsmcal_calibrate"):
        g, spec = mg.Gateway(target, mode, defines=()), SPECS[target]
        res, rec = good_call(g, spec)
        assert rec["hash"] == mg.fnv(*spec["hashed"]) and all(same(res.out[i], w) for i, w in enumerate(spec["out"]))
        for i, a in enumerate(spec["args"]):
            a = np.atleast_2d(np.asarray(a))
            refused(g, spec["args"][:i] + [np.ones(a.shape, dtype=bool)] + spec["args"][i + 1:])
            if a.dtype != np.uint8:
                refused(g, spec["args"][:i] + [np.ones(a.shape, dtype=np.uint8)] + spec["args"][i + 1:])
                if not np.iscomplexobj(a):
                    refused(g, spec["args"][:i] + [np.nan_to_num(a) + 1j] + spec["args"][i + 1:])
            elif target != "raw2iq":
                refused(g, spec["args"][:i] + [a.astype(np.float64)] + spec["args"][i + 1:])


@pytest.mark.parametrize("mode", mg.MODES)
@pytest.mark.parametrize("target", sorted(USES_POS_INFO))
def test_pos_info_must_have_two_columns(target, mode):
    g, spec, i = mg.gateway(target, mode), SPECS[target], USES_POS_INFO[target]
    for bad in (POS[:, :1], np.hstack([POS, POS[:, :1]]), POS[:0], row([-1.0, -1.0, -1.0]), F([7.0], 1, 1), POS.T):
        refused(g, spec["args"][:i] + [bad] + spec["args"][i + 1:])
    # the scalar -1 that the .m files' `pos_info==-1` accepts arrives as the [-1 -1] the ABI reads two columns of
    for m1 in (F([-1.0], 1, 1), row([-1.0, -1.0])):
        _, rec = good_call(g, spec, args=spec["args"][:i] + [m1] + spec["args"][i + 1:])
        assert rec["rows"] == "1" and rec["ld"] == "1"
        assert rec["hash"] == mg.fnv(*[h if h is not POS else [-1.0, -1.0] for h in spec["hashed"]])
    # rows and ld are the matrix's own, whatever its height
    for r in (1, 2, 7):
        p = np.stack([np.arange(r) + 20.0, np.arange(r) % 3.0], axis=1)
        _, rec = good_call(g, spec, args=spec["args"][:i] + [p] + spec["args"][i + 1:])
        assert rec["rows"] == str(r) and rec["ld"] == str(r)
        assert rec["hash"] == mg.fnv(*[h if h is not POS else p for h in spec["hashed"]])


@pytest.mark.parametrize("mode", mg.MODES)
def test_shapes_the_targets_rely_on_are_checked(mode):
    def swap(target, i, bad):
        a = SPECS[target]["args"]
        refused(mg.gateway(target, mode), a[:i] + [bad] + a[i + 1:])
    swap("specific_fft_snr_fix_avg", 1, F([3.0], 1, 1))                       # target_set with fewer than two elements
    swap("specific_fft_snr_fix_avg", 1, np.zeros((0, 0)))
    swap("BCCH_demod", 2, TPL[:, :7])                                         # templates without eight columns
    swap("BCCH_demod", 2, TPL.T)
    swap("pair_align", 2, PARAMS[:, :5])                                      # params without six elements
    swap("pair_align", 2, row(np.arange(7.0)))
    swap("gsmcal_calibrate", 3, row([9.0e8, 9.1e8]))                          # freq of a length that is neither 1 nor D
    swap("gsmcal_calibrate", 3, row([9.0e8] * 4))
    swap("gsmcal_calibrate", 3, np.zeros((0, 0)))
    swap("gsmcal_subband_power", 2, PHI[:, :2])                               # phase_rotate with a column count other than D
    swap("gsmcal_subband_power", 2, PHI.T)
    swap("CW_check", 0, F([1.0 + 1j], 1, 1))                                  # fewer than two samples
    swap("raw2iq", 0, U83.astype(np.float64) + 1j)                            # complex bytes
    a = SPECS["pair_align"]["args"]
    refused(mg.gateway("pair_align", mode), a + [0.0])                        # out_len below 1
    for t in mg.TARGETS:                                                      # a scalar argument given as a vector
        a = SPECS[t]["args"]
        for i, x in enumerate(a):
            if isinstance(x, float):
                refused(mg.gateway(t, mode), a[:i] + [row([x, x])] + a[i + 1:])


@pytest.mark.parametrize("target,mode", BOTH)
def test_negative_status_becomes_an_error_with_name_code_and_text(target, mode):
    g, spec = mg.gateway(target, mode), SPECS[target]
    g.preset(status=-4)
    res = g.call(*spec["args"], nlhs=len(spec["out"]))
    assert res.err is not None and res.err[0] == "gsmcal:error"
    assert res.err[1] == "%s failed (-4): the fake's last error" % target
    assert res.set_mask == [False] * mg.MAX_OUT and res.failures == "" and g.calls() == 1
    assert res.printed == ""
    g.preset()
    res = g.call(*spec["args"], nlhs=1)                                       # nothing of the failed call is left behind
    assert res.err is None and res.failures == ""


@pytest.mark.parametrize("mode", mg.MODES)
def test_context_creation_failure_is_gsmcal_nodevice(mode):
    g = mg.Gateway("CW_check", mode)
    g.preset(create_rc=-3)
    res = g.call(S9)
    assert res.err and res.err[0] == "gsmcal:nodevice" and g.calls() == 0 and g.num_hooks() == 0 and res.failures == ""
    g.preset()
    assert g.call(S9).err is None and g.created() == 1 and g.num_hooks() == 1


# ---- positive status: the sentinel outputs of the .m files -------------------------------------------------------------------
M1 = F([-1.0], 1, 1)


@pytest.mark.parametrize("mode", mg.MODES)
def test_sentinels_of_the_chain(mode):
    g = mg.gateway("FCCH_coarse_position", mode)                               # FCCH_coarse_position.m:27-30: position = snr = -1
    res, _ = good_call(g, SPECS["FCCH_coarse_position"], status=S_NO_FCCH)
    assert same(res.out[0], M1) and same(res.out[1], M1)

    g, spec = mg.gateway("FCCH_fine_correction", mode), SPECS["FCCH_fine_correction"]
    res, _ = good_call(g, spec, status=4, count=1, len_r=-1)                   # r = -1: a real 1 x 1
    assert same(res.out[1], M1) and res.out[0].shape == (1, 1)
    res, _ = good_call(g, spec, status=0, count=24, len_r=9)                   # every position, the whole stream
    assert same(res.out[0], row(pat(0, 24))) and same(res.out[1], col(patc(1, 9)))

    g, spec = mg.gateway("SCH_corr_rate_correction", mode), SPECS["SCH_corr_rate_correction"]
    for count in (1, 2, MAX_POS_ROWS):                                         # pos_info at the row count the ABI reported
        res, _ = good_call(g, spec, status=7 if count == 1 else 0, count=count, len_r=-1)
        assert same(res.out[0], np.stack([pat(0, count), pat(1, count)], axis=1)) and same(res.out[1], M1)
    # r = -1 upstream: a 1 x 1 s is handed on as "no stream"
    _, rec = good_call(g, spec, args=[M1] + spec["args"][1:], status=2, count=1, len_r=-1)
    assert rec["s"] == "0" and rec["len"] == "0" and rec["r"] == "0" and rec["cap_r"] == "0"

    g, spec = mg.gateway("carrier_correct_post_SCH", mode), SPECS["carrier_correct_post_SCH"]
    res, rec = good_call(g, spec, args=[M1, M1] + spec["args"][2:], status=S_POST_NO_POS, len_r=-1)
    assert same(res.out[0], M1) and rec["s"] == "0" and rec["rows"] == "1"


@pytest.mark.parametrize("mode", mg.MODES)
def test_sentinels_of_the_follow_ups(mode):
    g, spec = mg.gateway("BCCH_demod", mode), SPECS["BCCH_demod"]
    for st in (S_POST_NO_POS, S_POST_FEW_BCCH):                                # BCCH_demod.m:9, :14: -1, -1, -1 and no corr_val
        res, _ = good_call(g, spec, status=st)
        assert same(res.out[0], M1) and same(res.out[1], M1) and same(res.out[2], M1)
        assert same(res.out[3], np.zeros((0, 0)))
    res, _ = good_call(g, spec, status=13, count=-1)                           # :103: idx = -1, r and corr_val valid
    assert same(res.out[0], M1) and same(res.out[1], col(patc(1, 5))) and same(res.out[3], F(patc(3, 32), 8, 4))

    g, spec = mg.gateway("FCCH_demod", mode), SPECS["FCCH_demod"]
    res, _ = good_call(g, spec, status=S_POST_NO_POS)                          # FCCH_demod.m:8: empty rows, carrier_ppm NaN
    assert all(same(res.out[i], np.zeros((1, 0))) for i in range(3)) and same(res.out[3], F([np.nan], 1, 1))
    res, _ = good_call(g, spec, count=MAX_HITS)
    assert same(res.out[2], row(pat(2, MAX_HITS)))

    g, spec = mg.gateway("BCCH_decode", mode), SPECS["BCCH_decode"]
    for st in (S_POST_NO_POS, S_BCCH_NO_DECODE):                               # si_type = -1 whenever no block decoded
        res, _ = good_call(g, spec, status=st, count=0)
        assert same(res.out[2], M1) and same(res.out[3], np.zeros((0, 23))) and same(res.out[4], np.zeros((1, 0)))
    res, _ = good_call(g, spec, count=MAX_HITS + 5)                            # a count beyond the capacity is clipped to it
    assert res.out[3].shape == (MAX_HITS, 23) and same(res.out[3], (np.arange(MAX_HITS * 23) % 251).reshape(MAX_HITS, 23).astype(float))

    g, spec = mg.gateway("SCH_decode", mode), SPECS["SCH_decode"]
    res, _ = good_call(g, spec, status=14, count=0)
    assert same(res.out[3], np.zeros((1, 0))) and same(res.out[4], np.zeros((1, 0)))

    g, spec = mg.gateway("total_ppm_calculation", mode), SPECS["total_ppm_calculation"]
    res, _ = good_call(g, spec, status=S_ALL_INF)                              # total_ppm_calculation.m:8
    assert res.printed == "total PPM calculation: No valid PPM input!\n" and g.created() == 0

    g, spec = mg.gateway("move_fft_snr_runtime_avg", mode), SPECS["move_fft_snr_runtime_avg"]
    res, _ = good_call(g, spec, count=0)
    assert same(res.out[0], np.array([[False]]))

    g, spec = mg.gateway("gsmcal_calibrate", mode), SPECS["gsmcal_calibrate"]
    res, _ = good_call(g, spec, count=1)                                       # the [-1 -1] sentinel has one row: 1 x 2 cells
    assert same(res.out[1], {"shape": (1, 3), "cells": cell_expect(1)}) and same(res.out[0], table_expect(1))
    res, _ = good_call(g, spec, count=MAX_POS_ROWS - 2)
    assert same(res.out[1], {"shape": (1, 3), "cells": cell_expect(MAX_POS_ROWS - 2)})


# ---- what was passed ---------------------------------------------------------------------------------------------------------
VECTOR_ARGS = [("move_fft_snr_runtime_avg", 0, "len"), ("specific_fft_snr_fix_avg", 0, "len"), ("FCCH_coarse_position", 0, "len"),
               ("FCCH_fine_correction", 0, "len"), ("FCCH_fine_correction", 1, "num_base"), ("SCH_corr_rate_correction", 0, "len"),
               ("SCH_corr_rate_correction", 1, "num_fcch"), ("SCH_corr_rate_correction", 2, "len_ts"), ("carrier_correct_post_SCH", 0, "len"),
               ("FCCH_demod", 0, "len"), ("BCCH_demod", 0, "len"), ("SCH_decode", 0, "len"), ("SCH_decode", 2, "len_ts"),
               ("BCCH_decode", 0, "len"), ("CW_check", 0, "len"), ("IQ_imbalance", 0, "len"), ("pair_coherence", 0, "len_a"),
               ("pair_coherence", 1, "len_b"), ("pair_align", 0, "len"), ("total_ppm_calculation", 0, "n"), ("gsmcal_calibrate", 1, "ntaps"),
               ("gsmcal_calibrate", 2, "len_ts"), ("gsmcal_fcch_scan", 1, "ntaps"), ("gsmcal_band_power", 1, "ntaps"),
               ("gsmcal_subband_power", 1, "ntaps")]


@pytest.mark.parametrize("mode", mg.MODES)
def test_vector_lengths_are_numel_for_rows_and_columns(mode):
    for target, i, key in VECTOR_ARGS:
        g, spec = mg.gateway(target, mode), SPECS[target]
        v = np.asarray(spec["args"][i])
        recs = []
        for shaped in (v.reshape(1, -1), v.reshape(-1, 1)):
            _, rec = good_call(g, spec, args=spec["args"][:i] + [shaped] + spec["args"][i + 1:])
            assert rec[key] == str(v.size), (target, key, rec)
            recs.append(rec)
        assert recs[0] == recs[1], target                                      # and the same elements in the same order


@pytest.mark.parametrize("mode", mg.MODES)
def test_a_real_stream_arrives_with_zero_imaginary_parts(mode):
    re = np.arange(9.0) + 1.0
    for target in ("chn_filter_4x", "move_fft_snr_runtime_avg", "FCCH_coarse_position", "carrier_correct_post_SCH", "CW_check",
                   "IQ_imbalance", "pair_align", "SCH_corr_rate_correction"):
        g, spec = mg.gateway(target, mode), SPECS[target]
        _, rec = good_call(g, spec, args=[col(re)] + spec["args"][1:])
        assert rec["hash"] == mg.fnv(col(re) + 0j, *spec["hashed"][1:]), target
    g, spec = mg.gateway("SCH_corr_rate_correction", mode), SPECS["SCH_corr_rate_correction"]      # a real template too
    _, rec = good_call(g, spec, args=spec["args"][:2] + [row(re[:6])] + spec["args"][3:])
    assert rec["hash"] == mg.fnv(S9, [1.0, 2, 3], re[:6] + 0j)


@pytest.mark.parametrize("mode", mg.MODES)
def test_optional_arguments_and_their_defaults(mode):
    g, spec = mg.gateway("pair_coherence", mode), SPECS["pair_coherence"]
    want = [("0", "0", "0.5"), ("-3", "0", "0.5"), ("-3", "12", "0.5"), ("-3", "12", "0.75")]
    for k, extra in enumerate(([], [-3.0], [-3.0, 12.0], [-3.0, 12.0, 0.75])):
        _, rec = good_call(g, spec, args=spec["args"] + extra)
        assert (rec["lag0"], rec["max_lag"], rec["min_coherence"]) == want[k]
    g, spec = mg.gateway("pair_align", mode), SPECS["pair_align"]
    for extra, n in (([], 9), ([4.0], 4), ([13.0], 13), ([9.0], 9)):           # out_len: absent = numel(s), shorter, longer
        res, rec = good_call(g, spec, args=spec["args"] + extra)
        assert rec["out_len"] == str(n) and rec["len"] == "9" and same(res.out[0], col(patc(0, n)))
    _, rec = good_call(g, spec, args=[row(S9)] + spec["args"][1:])             # a row s: numel again
    assert rec["out_len"] == "9"
    g, spec = mg.gateway("gsmcal_subband_power", mode), SPECS["gsmcal_subband_power"]
    for extra, d in (([], "1"), ([4.0], "4")):
        _, rec = good_call(g, spec, args=spec["args"] + extra)
        assert rec["decim"] == d
    g, spec = mg.gateway("gsmcal_calibrate", mode), SPECS["gsmcal_calibrate"]  # a scalar freq is every dongle's
    _, rec = good_call(g, spec, args=spec["args"][:3] + [9.3e8])
    assert rec["hash"] == mg.fnv(U83, COEF, TS6, [9.3e8] * 3)
    _, rec = good_call(g, spec, args=spec["args"][:3] + [col([9.0e8, 9.1e8, 9.2e8])])
    assert rec["hash"] == mg.fnv(*spec["hashed"])


@pytest.mark.parametrize("mode", mg.MODES)
def test_raw_bytes_rows_and_columns(mode):
    """rows_2n / 2 for odd and even row counts, d the column count, the bytes column by column; raw2iq as doubles too"""
    for rows, d in ((8, 3), (9, 2), (2, 1), (7, 4)):
        u = F((np.arange(rows * d) * 5 + 1) % 256, rows, d).astype(np.uint8)
        for target in ("gsmcal_calibrate", "gsmcal_fcch_scan", "gsmcal_band_power", "gsmcal_subband_power"):
            g, spec = mg.gateway(target, mode), SPECS[target]
            args = [u] + spec["args"][1:]
            hashed = [u[:rows // 2 * 2]] + spec["hashed"][1:]
            if target == "gsmcal_calibrate":
                args[3], hashed[3] = 9.0e8, [9.0e8] * d
            if target == "gsmcal_subband_power":
                args[2] = hashed[2] = np.arange(2.0 * d).reshape(2, d)
            g.preset()
            res = g.call(*args, nlhs=1)
            assert res.err is None and res.failures == ""
            rec = g.log()[0]
            assert rec["n"] == str(rows // 2) and rec["d"] == str(d)
            assert rec["hash"] == mg.fnv(*hashed), target                      # an odd row count: every column without its last byte
        g, spec = mg.gateway("raw2iq", mode), SPECS["raw2iq"]
        for a, fn in ((u, "raw2iq_u8"), (u.astype(np.float64), "raw2iq")):     # uint8 goes to the byte entry point, doubles stay
            res, rec = good_call(g, spec, args=[a])
            assert rec["fn"] == fn and rec["rows_2n"] == str(rows) and rec["d"] == str(d) and rec["hash"] == mg.fnv(a)
            assert same(res.out[0], F(patc(0, rows // 2 * d), rows // 2, d))
    for n in (1, 6, 7):                                                        # chn_filter_8x_4x: ceil(n / 2) rows
        s = F(cvec(2 * n, 6), n, 2)
        res, rec = good_call(mg.gateway("chn_filter_8x_4x", mode), SPECS["chn_filter_8x_4x"], args=[s])
        assert rec["n"] == str(n) and rec["d"] == "2" and res.out[0].shape == ((n + 1) // 2, 2)


# ---- the context, its exit hook and say() --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", mg.MODES)
def test_context_is_made_once_and_the_exit_hook_destroys_it_once(mode):
    g, spec = mg.Gateway("FCCH_demod", mode), SPECS["FCCH_demod"]
    assert g.created() == 0 and g.num_hooks() == 0
    for _ in range(3):
        good_call(g, spec)
    assert g.created() == 1 and g.destroyed() == 0 and g.num_hooks() == 1
    assert g.run_atexit() == 1 and g.destroyed() == 1
    assert g.run_atexit() == 0 and g.destroyed() == 1
    good_call(g, spec)                                                         # loaded again: a new context, a new hook
    assert g.created() == 2 and g.num_hooks() == 1
    assert g.run_atexit() == 1 and g.destroyed() == 2


def test_objects_in_one_process_do_not_share_stub_or_context():
    a, b = mg.Gateway("CW_check", "interleaved"), mg.Gateway("CW_check", "split")
    good_call(a, SPECS["CW_check"])
    assert (a.created(), b.created(), a.calls(), b.calls(), a.num_hooks(), b.num_hooks()) == (1, 0, 1, 0, 1, 0)
    good_call(b, SPECS["CW_check"])
    assert a.run_atexit() == 1 and (a.destroyed(), b.destroyed()) == (1, 0) and b.run_atexit() == 1 and b.destroyed() == 1


@pytest.mark.parametrize("mode", mg.MODES)
def test_quiet_switch_silences_the_report(mode, monkeypatch):
    g, spec = mg.gateway("SCH_decode", mode), SPECS["SCH_decode"]
    monkeypatch.setenv("GSMCAL_QUIET", "1")
    res, _ = good_call(g, spec)
    assert res.printed == ""
    monkeypatch.setenv("GSMCAL_QUIET", "0")
    res, _ = good_call(g, spec)
    assert res.printed == "report of SCH_decode: 100% fake\n"


@pytest.mark.parametrize("mode", mg.MODES)
def test_memory_the_gateway_leaves_is_released_and_counted(mode):
    res, _ = good_call(mg.gateway("chn_filter_4x", mode), SPECS["chn_filter_4x"])
    assert res.released == (1 if mode == "split" else 0)                       # the split copy of s: MATLAB frees it at the end of the call


# ---- the stand-in itself: it must notice what it is there to notice ---------------------------------------------------------
BAD_GATEWAY = r'''
#include <string.h>
#include "mex.h"
#if MX_HAS_INTERLEAVED_COMPLEX
#define REAL_PTR(a) mxGetDoubles(a)
#else
#define REAL_PTR(a) mxGetPr(a)
#endif
void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    int what = (int)mxGetScalar(prhs[0]);
    double* p = (double*)mxMalloc(4 * sizeof(double));
    (void)nlhs; (void)nrhs;
    plhs[0] = mxCreateDoubleMatrix(2, 2, mxREAL);
    if (what == 1) REAL_PTR(plhs[0])[4] = 1.0;                  /* one past an output */
    if (what == 2) p[4] = 1.0;                                  /* one past an mxMalloc block */
    if (what == 3) { mxFree(p); mxFree(p); return; }            /* freed twice */
    if (what == 4) mxFree(REAL_PTR(plhs[0]));                   /* not an mxMalloc block */
    if (what == 5) REAL_PTR(prhs[0])[1] = 1.0;                  /* one past an input */
    if (what == 6) plhs[0] = mxCreateDoubleScalar(REAL_PTR(prhs[1]) == NULL ? 1.0 : 0.0);    /* doubles of a uint8 array */
    if (what == 7) { mexPrintf("a %d%%\n", 7); mexErrMsgIdAndTxt("bad:id", "text %d", 7); }
    if (what == 8) plhs[0] = mxCreateDoubleScalar(REAL_PTR(plhs[0])[3] + p[0] * 0.0 == 0.0 ? 1.0 : 0.0);   /* zero-filled */
}
'''


@pytest.mark.parametrize("mode", mg.MODES)
def test_the_stand_in_notices_what_it_is_there_for(mode, tmp_path):
    src = tmp_path / "bad.c"
    src.write_text(BAD_GATEWAY)
    g = mg.Gateway("none", mode, source=str(src))
    one = F([1.0], 1, 1)
    res = g.call(0.0)
    assert res.err is None and res.failures == "" and res.released == 1 and same(res.out[0], np.zeros((2, 2)))
    for what, word in ((1, "guard words"), (2, "guard words"), (3, "mxFree"), (4, "mxFree"), (5, "guard words")):
        res = g.call(float(what))
        assert word in res.failures, (what, res.failures)
    assert same(g.call(6.0, np.ones((2, 2), dtype=np.uint8)).out[0], one)
    # of a complex one: mxGetDoubles has none, mxGetPr is its real part
    assert same(g.call(6.0, np.ones((2, 2)) + 1j).out[0], one if mode == "interleaved" else F([0.0], 1, 1))
    assert same(g.call(6.0, np.ones((2, 2))).out[0], F([0.0], 1, 1))
    live = g.h.mxh_live_blocks()
    res = g.call(7.0)
    assert res.err == ("bad:id", "text 7") and res.printed == "a 7%\n" and res.set_mask == [False] * mg.MAX_OUT
    assert g.h.mxh_live_blocks() == live - 2 and res.failures == ""           # nothing of the call survives; the old output went
    assert same(g.call(8.0).out[0], one)


def test_a_missing_compiler_is_an_error_not_a_skip(monkeypatch):
    monkeypatch.setenv("PATH", "/nonexistent")
    monkeypatch.setenv("ROCM_PATH", "/nonexistent")
    with pytest.raises(RuntimeError, match="no C compiler"):
        mg.compiler()
