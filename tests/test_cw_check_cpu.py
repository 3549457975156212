"""CPU tests of the CW sample-loss check (CW_check.m:6-8): the boundary -- header, library exports, constants, generator, MEX
target -- and, for every input tests/test_gpu_cw_check.py hands to the GPU, the margins that make its comparisons honest:
identical indices and 1e-10 rad on values only mean something where no decision of the restatement hangs on its own last bits.

Checked with thr = 0.2: min |s| >= 5.8 (58 for the captures with amp 60 and up), distance of angle(q) to pi >= 0.149, threshold
margin >= 0.153, |mean q| >= 0.99, numpy against longdouble <= 3.8e-16, lead of the maximum >= 1.4e-3 ("clean").  A seed or a
case that breaks a bound below gets another input, never another bound."""
import os
import re
import subprocess

import numpy as np
import pytest

import cw_check_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("gsmcal_CW_check", "gsmcal_cw_check_batch", "gsmcal_cw_check_batch_dev")


@pytest.mark.parametrize("name", sorted(ref.ALL))
def test_margins_of_every_gpu_input(name):
    m = ref.margins(name)
    print(name, {k: v for k, v in m.items() if k != "events"}, "events:", len(m["events"]))
    assert m["min_abs_s"] > 0.0
    assert m["dist_pi"] >= 1e-3                    # no ulp can flip a branch of atan2
    assert m["thr_margin"] >= 1e-3                 # ... nor an exceed
    assert m["abs_mean_q"] >= 0.5                  # the summation-order bound on phase_rotate (test_gpu_cw_check.py) needs this
    assert m["numpy_vs_longdouble"] <= 1e-12
    assert m["events"] == sorted(ref.planted(name))   # the events are exactly the planted drops
    assert m["lead"] >= 1e-3                       # ... nor the index of the maximum


def test_case_table_is_the_documented_one():
    c = ref.CASES
    assert c["clean"]["n"] == c["drops"]["n"] == 409600 and c["small"]["n"] == c["dense"]["n"] == 4099 and c["tiny"]["n"] == 3
    assert c["drops"]["drops"] == ((8191, 3), (100000, 1), (300001, 5), (409598, 2))
    assert c["small"]["drops"] == ((0, 2), (255, 1), (256, 4), (4097, 3))
    assert len(c["dense"]["drops"]) == 67 and all(k == 1 for _, k in c["dense"]["drops"])
    assert len(c["dense"]["drops"]) > ref.gsmcal.CW_MAX_EVENTS                 # overflows the event list
    assert [v["n"] for k, v in ref.SHAPES.items() if k != "n3"] == [ref.TILE + 1, ref.TILE, ref.TILE + 2, 2 * ref.TILE + 2]
    for v in ref.SHAPES.values():                                              # a drop at n = 1 and one at the last ratio
        assert not v["drops"] or [p for p, _ in v["drops"]] == [0, v["n"] - 2]
    _, r, _ = ref.reference("small")
    assert np.abs(r).max() > np.pi                                            # one spike is unwrapped: 4.09 rad


def test_one_ratio_and_longdouble_form_agree_on_the_pair():
    r, pr = ref.numpy_form(ref.S_N2)
    rl, prl = ref.longdouble_form(ref.S_N2)
    assert r.shape == (1,) and r[0] == 0.0 and abs(rl[0]) <= 1e-18 and abs(pr - float(prl)) <= 1e-15
    assert np.pi - abs(pr) >= 1e-3 and np.abs(ref.S_N2).min() > 0


def test_summary_restatement():
    r = np.array([0.1, -0.5, 0.3, 0.5, -0.2, 0.21])
    s = ref.summary(r, 0.2)
    assert s == {"count": 4, "max_abs": 0.5, "max_n": 2, "events": [(2, -0.5), (3, 0.3), (4, 0.5), (6, 0.21)]}   # -0.2 is not > 0.2


def test_make_cw_is_seeded_and_places_the_spike(gsmcal_mod):
    mk = gsmcal_mod.synth.make_cw
    a, b = mk(1000, seed=5), mk(1000, seed=5)
    assert a.dtype == np.uint8 and a.shape == (2000,) and np.array_equal(a, b)
    assert not np.array_equal(a, mk(1000, seed=6))
    n = 62832                                                                  # 100 cycles of the 0.01 rad/sample tone: its mean is ~0, raw2iq removes the DC only
    d = mk(n, step=0.01, noise=0.0, drops=[(400, 17)], seed=5)
    assert np.array_equal(d[:2 * 401], mk(n, step=0.01, noise=0.0, seed=5)[:2 * 401])  # nothing changes up to and including output 400
    from oracle import gsmcal_oracle as o
    r, _ = ref.numpy_form(o.raw2iq(d))
    assert int(np.argmax(np.abs(r))) + 1 == 401 and abs(r[400] - 0.17) < 0.02   # 17 samples of 0.01 rad: a 0.17 rad spike at n = pos + 1
    # (0.02: rounding to bytes moves a sample of modulus 100 by at most 0.5*sqrt(2)/100 = 0.0071 rad, a ratio by twice that)
    with pytest.raises(ValueError):
        mk(10, drops=[(9, 1)])


def test_header_declares_and_library_exports_the_entry_points(gsmcal_mod):
    txt = open(os.path.join(ROOT, "include", "gsmcal.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = gsmcal_mod.load()
    for s in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % s, code), s + " is not declared in include/gsmcal.h"
        assert hasattr(lib, s) and s in gsmcal_mod.SIGNATURES
    for f in ("CW_check", "cw_check_batch", "cw_check_batch_dev", "cw_rows"):
        assert callable(getattr(gsmcal_mod, f))
    assert callable(gsmcal_mod.ingest.check_sample_loss)


def test_constants_match_the_header(gsmcal_mod):
    txt = open(os.path.join(ROOT, "include", "gsmcal.h")).read()

    def define(name):
        return re.search(r"#define %s (.+?)\s*(?:/\*|$)" % name, txt, flags=re.M).group(1)
    assert int(define("GSMCAL_CW_MAX_EVENTS")) == gsmcal_mod.CW_MAX_EVENTS == 16
    assert define("GSMCAL_CW_COLS") == "(5 + 2 * GSMCAL_CW_MAX_EVENTS)" and gsmcal_mod.CW_COLS == 5 + 2 * gsmcal_mod.CW_MAX_EVENTS == 37
    assert int(define("GSMCAL_CW_TILE")) == gsmcal_mod.CW_TILE
    assert (int(define("GSMCAL_CW_OK")), int(define("GSMCAL_CW_SHORT")), int(define("GSMCAL_CW_ZERO"))) == \
        (gsmcal_mod.CW_OK, gsmcal_mod.CW_SHORT, gsmcal_mod.CW_ZERO) == (0, 1, 2)


def test_cw_rows_names_the_columns(gsmcal_mod):
    t = np.full((2, gsmcal_mod.CW_COLS), np.nan)
    t[0, :9] = [0.7, 2, 2.1, 8192, 0, 8192, 2.1, 100001, 0.7]
    t[1, :5] = [np.nan, 0, np.nan, np.nan, 2]
    rows = gsmcal_mod.cw_rows(t)
    assert rows[0] == {"phase_rotate": 0.7, "count": 2, "max_abs": 2.1, "max_n": 8192, "status": 0,
                       "events": [(8192, 2.1), (100001, 0.7)]}
    assert rows[1]["status"] == 2 and rows[1]["count"] == 0 and rows[1]["max_n"] is None and rows[1]["events"] == []
    assert np.isnan(rows[1]["phase_rotate"]) and np.isnan(rows[1]["max_abs"])


@pytest.mark.parametrize("api", ["interleaved", "split"])
def test_mex_cw_check_target_compiles_against_the_abi(api):
    """The CW_check target of mex/gsmcal_mex.c through `gcc -fsyntax-only` against the declaration-only mex.h (tests/mex_stub),
    once per MEX complex-storage API, as tests/test_abi_cpu.py does for the other targets."""
    src = open(os.path.join(ROOT, "mex", "gsmcal_mex.c")).read()
    assert "defined(GSMCAL_FN_CW_check)" in src
    r = subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-std=c99", "-DGSMCAL_FN_CW_check"] +
                       (["-DGSMCAL_STUB_SPLIT"] if api == "split" else []) +
                       ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mex_stub"),
                        os.path.join(ROOT, "mex", "gsmcal_mex.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
