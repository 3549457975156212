"""CPU tests of pair_coherence: the numpy restatement of the definition (tests/pair_coherence_ref.py) against a brute-force loop,
against the values planted in the designed pair, and on three oracle-calibrated dongles of one transmission against what was
planted and what the chain left; the constants of the Python layer against the header; the MEX target.

Bars on the calibrated triple (measured with the restatement when the definition was fixed, margins about 3x): every evaluated
burst coherent to >= 0.9; delay0 within 0.15 samples of the planted difference (0.05 measured); rel_carrier_hz within 6 Hz of
what the chain left (2.1); rel_sampling_ppm within 0.1 (0.03); (b, a) against (a, b): -delay0 within 0.02, -carrier within 0.5 Hz;
the top-two gap of y >= 1e-6 (1.3e-4 measured) and the parabola's curvature >= 1e-4."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import pair_coherence_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_against_a_brute_force_loop_on_the_designed_pair():
    ov, M, lag0 = 2, 3, 10
    r, r_len, pi, _ = ref.designed_streams(ov)
    want = ref.pair_coherence(r, r_len, pi, ov, 0, 1, lag0, M)
    a, b = r
    L, Ls = 148 * ov, 37 * ov
    bursts = [int(p) - 1 for p, t in zip(pi[0, 0], pi[0, 1]) if t in (1.0, 2.0)]
    assert len(bursts) == 3 and want["evaluated"][:3].all() and not want["evaluated"][3:].any()
    for j, p in enumerate(bursts):
        y = np.zeros(2 * M + 1)
        for m in range(-M, M + 1):
            for k in range(4):
                av = a[p + k * Ls: p + (k + 1) * Ls]
                bv = b[p + lag0 + m + k * Ls: p + lag0 + m + (k + 1) * Ls]
                c = np.vdot(av, bv)                                  # sum b conj(a)
                assert abs(c - want["corr"][j, m + M, k]) <= 1e-12 * Ls
                assert abs(np.vdot(bv, bv).real - want["eb"][j, m + M, k]) <= 1e-12 * Ls
                y[m + M] += abs(c) ** 2
            assert abs(np.vdot(a[p: p + L], a[p: p + L]).real - want["ea"][j].sum()) <= 1e-12 * L
        ms = int(np.argmax(y)) - M
        assert ms == want["mstar"][j] == 1                           # D = 11.25 against lag0 = 10
        d = lag0 + ms + 0.5 * (y[ms + M - 1] - y[ms + M + 1]) / (y[ms + M - 1] - 2 * y[ms + M] + y[ms + M + 1])
        assert abs(d - want["row"][ref.col("delay") + j]) <= 1e-12
    assert np.isnan(want["corr"][3:]).all()


@pytest.mark.parametrize("ov", [2, 4, 8])
def test_designed_pair_returns_what_was_planted(ov):
    """a: unit modulus with noise in its phase; b: a shifted by 11.25 samples through a phase ramp in the FFT domain, turned by a
    planted phase and frequency, light noise; the table: an FCCH row, which is ignored, and three type-1 / type-2 rows.  ov 2 and
    M 3 is the case of record; 4 and 8 run the same design at the other ratios the GPU tests use."""
    M = 3
    r, r_len, pi, plant = ref.designed_streams(ov)
    want = ref.pair_coherence(r, r_len, pi, ov, 0, 1, 11, M)
    row, c, bound = want["row"], ref.col, ref.designed_bounds(ov, plant)
    assert ref.ties_ok(want), (want["gap"][:3], want["curvature"][:3], want["coh_margin"][:3])
    assert row[0] == 0 and row[1:5].tolist() == [3, 3, 3, 2] and row[c("lag0")] == 11 and row[c("max_lag")] == M
    assert np.array_equal(row[c("pos"): c("pos") + 3], pi[0, 0, 1:4])               # the FCCH row is not among them
    assert np.isnan(row[c("pos") + 3: c("pos") + ref.MAX_PAIR_BURSTS]).all()
    err = {"delay": row[c("delay"): c("delay") + 3] - plant["delay"], "freq": row[c("freq"): c("freq") + 3] - plant["freq"],
           "phase": ref.wrap(row[c("phase"): c("phase") + 3] - plant["phase"])}
    print("ov", ov, {k: (np.abs(v).max(), bound[k]) for k, v in err.items()})
    for k, v in err.items():
        assert np.all(np.abs(v) <= bound[k]), (k, v, bound[k])
    pair = {"delay0": row[c("delay0")] - plant["delay"], "phase0": float(ref.wrap(row[c("phase0")] - plant["phase"][0])),
            "rel_carrier_hz": row[c("rel_carrier_hz")] - plant["freq"], "rel_sampling_ppm": row[c("rel_sampling_ppm")]}
    print("   ", pair, "coherence", row[c("coherence"): c("coherence") + 3])
    assert abs(pair["delay0"]) <= bound["delay"] and abs(pair["phase0"]) <= bound["phase"]
    assert abs(pair["rel_carrier_hz"]) <= bound["rel_carrier_hz"] and abs(pair["rel_sampling_ppm"]) <= bound["rel_sampling_ppm"]
    assert abs(row[c("burst_carrier_hz")] - plant["freq"]) <= bound["freq"]
    assert np.all(row[c("coherence"): c("coherence") + 3] >= 0.95) and np.all(row[c("coherence"): c("coherence") + 3] <= 1.0)
    assert row[c("delay_rms")] <= bound["delay"] and row[c("phase_rms")] <= bound["phase"]
    assert row[c("min_coherence_seen")] <= row[c("mean_coherence")] <= 1.0


def test_restatement_exits():
    ov = 2
    r, r_len, pi, _ = ref.designed_streams(ov)
    c = ref.col
    row = ref.pair_coherence(r, r_len, pi, ov, 0, 1, 11 + 5, 3)["row"]              # lag0 off by M + 2: every maximum at the edge
    assert row[0] == ref.S_PAIR_FEW and row[1:5].tolist() == [3, 3, 0, 0] and row[c("edge"): c("edge") + 3].tolist() == [1, 1, 1]
    assert np.isnan(row[c("delay0"): c("max_lag")]).all() and np.isnan(row[c("delay"): c("delay") + 3]).all()
    assert ref.pair_coherence(r, np.array([len(r[0]), -1]), pi, ov, 0, 1, 11, 3)["row"][0] == ref.S_POST_NO_POS
    assert ref.pair_coherence(r, r_len, pi, ov, 1, 0, -11, 3)["row"][0] == ref.S_POST_NO_POS      # b's table is all -1
    many = ref.raw_table([(201.0 + 10 * i, 1.0 + (i & 1)) for i in range(121)])
    row = ref.pair_coherence(r, r_len, np.stack([many, pi[1]]), ov, 0, 1, 11, 3)["row"]
    assert row[0] == ref.E_CAPACITY and row[1] == 121
    same = ref.pair_coherence(*ref.periodic_self_stream(ov), ov, 0, 0, 0, 3)["row"]     # a stream against itself
    assert same[0] == 0 and same[3] == 3 and np.all(np.abs(same[c("coherence"): c("coherence") + 3] - 1) <= 1e-12)
    assert np.all(np.abs(same[c("delay"): c("delay") + 3]) <= 1e-8) and np.all(np.abs(same[c("phase"): c("phase") + 3]) <= 1e-9)
    assert np.all(np.abs(same[c("freq"): c("freq") + 3]) <= 1e-6) and abs(same[c("delay0")]) <= 1e-8 and abs(same[c("phase0")]) <= 1e-9


@functools.lru_cache(maxsize=None)
def oracle_triple():
    import gsmcal
    from oracle import gsmcal_oracle as o
    s = gsmcal.synth
    coef, ts = s.fir1(46, 200e3 / s.FS), s.sch_training_sequence()
    made = [s.make_stream(**ref.triple_stream_args(i)) for i in range(3)]
    outs = [o.calibrate_stream(raw, coef, ts, ref.FC, keep_r=True) for raw, _ in made]
    assert [x["status"] for x in outs] == [0, 0, 0]
    stride = max(x["r_len"] for x in outs)
    r = np.zeros((3, stride), dtype=np.complex128)
    pi = -np.ones((3, 2, ref.MAX_POS_ROWS))
    for i, x in enumerate(outs):
        r[i, :x["r_len"]] = x["r_correct"]
        pi[i, :, :len(x["pos_info"])] = x["pos_info"].T
    return (r, np.array([x["r_len"] for x in outs], dtype=np.int64), pi, [t for _, t in made],
            [x["total_sampling_ppm"] for x in outs], [x["total_carrier_ppm"] for x in outs])


def test_oracle_calibrated_triple_against_the_planted_delay_and_what_the_chain_left():
    r, r_len, pi, truth, tot_s, tot_c = oracle_triple()
    c = ref.col
    for a, b in ref.TRIPLE_PAIRS:
        planted = ref.triple_planted_delay(a, b)
        lag0 = int(ref.matlab_round(planted))
        fwd = ref.pair_coherence(r, r_len, pi, 8, a, b, lag0)
        bwd = ref.pair_coherence(r, r_len, pi, 8, b, a, -lag0)
        left_hz, left_ppm = ref.triple_left_by_the_chain(truth, tot_s, tot_c, a, b)
        f, g = fwd["row"], bwd["row"]
        ev = fwd["evaluated"]
        coh = f[c("coherence"): c("coherence") + ref.MAX_PAIR_BURSTS][ev]
        print(f"pair {a}->{b}: bursts {int(f[1])} eval {int(f[2])} used {int(f[3])} adjacent {int(f[4])} coherence {coh.min():.4f}..{coh.max():.4f} "
              f"delay0 {f[c('delay0')]:.4f} planted {planted} carrier {f[c('rel_carrier_hz')]:.3f} left {left_hz:.3f} "
              f"ppm {f[c('rel_sampling_ppm')]:.4f} left {left_ppm:.4f} gap min {np.min(fwd['gap'][ev]):.3g} curvature min {np.nanmin(fwd['curvature'][ev]):.3g} "
              f"reverse: delay0 {g[c('delay0')]:.4f} carrier {g[c('rel_carrier_hz')]:.3f}")
        assert f[0] == 0 and g[0] == 0 and f[2] >= 16 and not fwd["edge"].any()
        assert np.all(coh >= 0.9)
        assert abs(f[c("delay0")] - planted) <= 0.15
        assert abs(f[c("rel_carrier_hz")] - left_hz) <= 6.0
        assert abs(f[c("rel_sampling_ppm")] - left_ppm) <= 0.1
        assert abs(g[c("delay0")] + f[c("delay0")]) <= 0.02 and abs(g[c("rel_carrier_hz")] + f[c("rel_carrier_hz")]) <= 0.5
        assert np.all(fwd["gap"][ev] >= 1e-6) and np.all(fwd["curvature"][ev] >= 1e-4)


def test_python_constants_equal_the_headers(gsmcal_mod):
    txt = open(os.path.join(ROOT, "include", "gsmcal.h")).read()

    def macro(name):
        m = re.search(r"#define %s\s+(\(.*?\)|\S+)\s" % name, txt)
        expr = m.group(1)
        for _ in range(4):
            expr = re.sub(r"GSMCAL_[A-Z_0-9]+", lambda q: "(%s)" % macro_text(q.group(0)), expr)
        return int(eval(expr, {"__builtins__": {}}))                    # integers, + * and parentheses only

    def macro_text(name):
        return re.search(r"#define %s\s+(\(.*?\)|\S+)\s" % name, txt).group(1)

    assert macro("GSMCAL_MAX_PAIR_BURSTS") == gsmcal_mod.MAX_PAIR_BURSTS == ref.MAX_PAIR_BURSTS == 120
    assert macro("GSMCAL_PAIR_COLS") == gsmcal_mod.PAIR_COLS == ref.PAIR_COLS == 736
    assert int(re.search(r"GSMCAL_S_PAIR_FEW = (\d+)", txt).group(1)) == gsmcal_mod.S_PAIR_FEW == ref.S_PAIR_FEW
    assert gsmcal_mod.S_PAIR_FEW == 1 + int(re.search(r"GSMCAL_S_BCCH_NO_DECODE = (\d+)", txt).group(1))     # the next free value
    for i, name in enumerate(gsmcal_mod.PAIR_FIELDS):
        assert macro("GSMCAL_P_" + name.upper()) == i == ref.HEAD.index(name)
    for name, short in zip(gsmcal_mod.PAIR_BURST_FIELDS, ("POS", "DELAY", "PHASE", "FREQ", "COH", "EDGE")):
        assert macro("GSMCAL_P_" + short) == ref.col(name)
    t = gsmcal_mod.pair_rows(np.arange(2 * ref.PAIR_COLS, dtype=np.float64))
    assert t["max_lag"].tolist() == [15.0, 15.0 + ref.PAIR_COLS] and t["edge"].shape == (2, 120) and t["edge"][0, 0] == ref.col("edge")
    for sym in ("gsmcal_pair_coherence", "gsmcal_pair_coherence_batch", "gsmcal_pair_coherence_batch_dev"):
        assert sym in gsmcal_mod.SIGNATURES and hasattr(gsmcal_mod.load(), sym)


def test_pair_lag0_rounds_the_alignment_difference_and_refuses_nan(gsmcal_mod):
    rows = {"status": np.array([0.0, 0.0, 14.0]), "fn_anchor": np.array([100.0, 101.0, -1.0]),
            "pos_anchor": np.array([5000.0, 15003.5, -1.0])}
    assert gsmcal_mod.pair_lag0(rows, [(0, 1), (1, 0)], 8).tolist() == [4, -4]          # 3.5 rounds away from zero
    with pytest.raises(ValueError):
        gsmcal_mod.pair_lag0(rows, [(0, 2)], 8)


@pytest.mark.parametrize("api", ["interleaved", "split"])
def test_pair_coherence_mex_target_compiles_against_the_abi(api):
    """The pair_coherence target of mex/gsmcal_mex.c through `gcc -fsyntax-only` against the declaration-only mex.h (tests/mex_stub),
    once per MEX complex-storage API, as tests/test_abi_cpu.py does for the other targets."""
    src = open(os.path.join(ROOT, "mex", "gsmcal_mex.c")).read()
    assert "defined(GSMCAL_FN_pair_coherence)" in src
    r = subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-std=c99", "-DGSMCAL_FN_pair_coherence"] +
                       (["-DGSMCAL_STUB_SPLIT"] if api == "split" else []) +
                       ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mex_stub"),
                        os.path.join(ROOT, "mex", "gsmcal_mex.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
