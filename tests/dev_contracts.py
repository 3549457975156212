"""The registry of the device entry points (`gsmcal_*_batch_dev`) and what include/gsmcal.h promises for each of them: which
elements of which buffer a call may read, which it writes, which it leaves alone -- and, per entry, small designed inputs
("variants") that differ in exactly the things the context's caches key on.  tests/test_dev_contracts_cpu.py keeps this table
honest without a GPU (every exported _dev symbol is here, every cache of csrc/host_plan.h / csrc/abi_calls.h has a colliding
pair of variants, every variant passes its family's margins on the restatement); tests/test_gpu_dev_contracts.py drives it on
the GPU (anchor against the restatement, reads and writes inside the declared extents, call history, two contexts).

Plain module: numpy, the package's host code and the restatements only.  No torch here; `run` gets device addresses.

One entry per entry point.  Of an entry:
  name, family, symbol   `symbol` is the exported C name
  caches                 members of gsmcal_ctx (csrc/host_plan.h) whose content decides whether the call uploads again
  shared                 device buffers of the context it shares with other entries
  variants               name -> why it is there; `refused`: the variant whose argument error the header lists under "decided before
                         anything is enqueued" (or the entry's own rule), with its code
  pairs                  cache -> (variant A, variant A'): the same sizes with other contents in that cache
  smallest               the smallest shape at which the kernel has a partial last tile, more than one tile, more than one stream
  build(variant)         -> Case: host arguments, device inputs (array, live mask), outputs (shape, dtype, written, alone)
  run(g, ctx, case, ptr) calls the _dev form of api.py on the addresses ptr[name]; allocates nothing
  check(case, outs, g, extra)   the family's fp64 restatement under the family's own bound: the compare functions and bounds
                         are imported from the family's test module / *_ref.py, none is restated here
  margins(case)          the margins the family's tests demand of the restatement before they compare (CPU only)
  cached(case)           cache -> the host array the library keeps for it (what the CPU test compares between the two variants)

Masks: `live` marks the elements of an input the header lets the call read (everything else is poisoned in the reads test);
`written` the elements of an output the header says are written, `alone` those it says are left alone; what is in neither is
unspecified and nothing is asserted about it (DESIGN.md section 22 lists those elements)."""
import functools
import math

import numpy as np

BAND = 4096                                   # guard band either side of every slot, bytes
NAN_PAYLOAD = 0x7FF8DEADBEEF0001              # the poison of doubles: a quiet NaN whose payload no arithmetic produces
_PATTERN = {8: 0xC0DEC0DEC0DEC0DE, 4: 0xC0DEC0DE, 1: 0xA5}      # the prefill of outputs, by the size of the base type: as a double
#                                               -31 500.0138...: finite, not NaN, not an integer; as int64 / int32 a large negative
#                                               number no length or count equals; as a byte 0xA5, which no output byte of a
#                                               variant here equals (asserted when the anchors are made)
FC = 957.4e6
S_POST_NO_POS = 10


def base_dtype(dtype):
    dtype = np.dtype(dtype)
    return np.dtype(np.float64) if dtype == np.complex128 else dtype


def pattern(shape, dtype):
    """an array of `shape` and `dtype` holding the prefill pattern in every element"""
    b = base_dtype(dtype)
    word = np.array([_PATTERN[b.itemsize]], dtype={8: np.uint64, 4: np.uint32, 1: np.uint8}[b.itemsize])
    flat = np.tile(word.view(np.uint8), int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize // b.itemsize)
    return flat.view(dtype).reshape(shape).copy()


def pattern_bytes(nbytes):
    """the 8-byte pattern over `nbytes` bytes: what a guard band holds (every base type's pattern tiles it, but the byte's)"""
    return np.tile(np.array([_PATTERN[8]], dtype=np.uint64).view(np.uint8), (nbytes + 7) // 8)[:nbytes].copy()


def bits(a):
    """the bytes of an array: bit-for-bit comparison, NaN payloads included"""
    return np.ascontiguousarray(a).view(np.uint8).ravel()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


class In:
    def __init__(self, data, live=None):
        self.data = np.ascontiguousarray(data)
        self.live = np.ones(self.data.shape, bool) if live is None else np.broadcast_to(live, self.data.shape).copy()


class Out:
    def __init__(self, shape, dtype, written=True, alone=False):
        self.shape, self.dtype = tuple(int(v) for v in shape), np.dtype(dtype)
        self.written = np.broadcast_to(written, self.shape).copy()
        self.alone = np.broadcast_to(alone, self.shape).copy()
        assert not np.any(self.written & self.alone)


class Case:
    def __init__(self, entry, variant, host, ins, outs, refused=None):
        self.entry, self.variant, self.host, self.ins, self.refused = entry, variant, host, ins, refused
        self.outs = outs
        if refused is not None:                                # a refused call writes nothing
            self.outs = {k: Out(o.shape, o.dtype, False, True) for k, o in outs.items()}

    @property
    def key(self):
        return (self.entry, self.variant)


class Entry:
    def __init__(self, name, family, symbol, caches, shared, variants, refused, pairs, smallest, build, run, check, margins, cached):
        self.name, self.family, self.symbol, self.caches, self.shared = name, family, symbol, tuple(caches), tuple(shared)
        self.variants, self.refused, self.pairs, self.smallest = dict(variants), refused, dict(pairs), smallest
        self.variants[refused] = "refused: " + REFUSALS[name]
        self._build, self.run, self.check, self.margins, self.cached = build, run, check, margins, cached

    def build(self, variant):
        return _build_cached(self.name, variant)

    def good(self):
        return [v for v in self.variants if v != self.refused]


@functools.lru_cache(maxsize=None)
def _build_cached(name, variant):
    e = REGISTRY[name]
    case = e._build(variant)
    assert case.key == (name, variant) and (case.refused is not None) == (variant == e.refused)
    for i in case.ins.values():
        i.data.setflags(write=False)
    return case


class _Answers:
    """stands in for the package where a family's check function asks it for the result: `check(g, raw, ...)` of
    tests/test_gpu_spectrum.py and tests/test_gpu_subband.py call g.band_power_batch / g.subband_power_batch themselves and then
    compare with their own bound; handing them the device form's answer keeps the bound where it is"""

    def __init__(self, got):
        self.got = got

    def band_power_batch(self, *a, **k):
        return self.got

    def subband_power_batch(self, *a, **k):
        return self.got


def _synth():
    import gsmcal
    return gsmcal.synth


def _fir1(n, f):
    s = _synth()
    return s.fir1(n, f / s.FS)


# ================================================================ the raw-byte families =========================================
def _raw_run(fn_name, args):
    def run(g, ctx, case, ptr):
        h = case.host
        getattr(g, fn_name)(ptr["raw"], h["d"], h["n"], *args(h, ptr), ctx=ctx)
    return run


def _raw_case(entry, variant, raw, host, outs, refused=None):
    d, two_n = raw.shape
    host = dict(host, d=d, n=host.get("n", two_n // 2))
    return Case(entry, variant, host, {"raw": In(raw)}, outs, refused)


# ---- frontend_batch_dev --------------------------------------------------------------------------------------------------------
def _frontend_build(v):
    import geometry_cases as gc
    filt = gc.fe_filters()
    n, decim, coef = {"a": (4099, 7, filt["fir47"]), "a2": (4099, 7, _fir1(46, 150e3)), "big": (65541, 64, filt["fir47"]),
                      "small": (257, 2, filt["two"]), "refused": (4099, 300, filt["fir47"])}[v]
    raw = gc.fe_raw(n)
    nd = -(-n // decim)
    return _raw_case("frontend", v, raw, {"coef": coef, "decim": decim}, {"out": Out((len(raw), nd), np.complex128)},
                     "-6" if v == "refused" else None)


def _frontend_check(case, outs, g, extra=None):
    import geometry_cases as gc
    from oracle import gsmcal_oracle as o
    raw, coef, decim = case.ins["raw"].data, case.host["coef"], case.host["decim"]
    iq = o.raw2iq(raw.T.astype(np.float64))
    want = o.matlab_filter(coef, iq)[0::decim]
    err, bound = np.max(np.abs(outs["out"].T - want)), gc.fe_bound(coef, iq)
    assert err <= bound, (case.key, err, bound)


# ---- band_power_batch_dev ------------------------------------------------------------------------------------------------------
def _band_build(v):
    import subband_ref
    from gsmcal import dist
    fs = subband_ref.FS
    sf = dist.spectrum_filter
    rng = np.random.default_rng(64)
    d, n, coef, decim = {"a": (3, 30001, sf(fs, 50e3, 0.1)[1], 20), "a2": (3, 30001, rng.standard_normal(64), 20),
                         "big": (4, 65541, sf(fs, 10e3, 0.1)[1], 102), "small": (2, 77, sf(fs, 10e3, 0.1)[1], 102),
                         "refused": (2, 77, np.ones(1025), 1)}[v]
    raw = subband_ref.tone_captures(d, n, 7)
    return _raw_case("band_power", v, raw, {"coef": np.asarray(coef, dtype=np.float64), "decim": decim}, {"power": Out((d,), np.float64)},
                     "-1" if v == "refused" else None)


def _band_check(case, outs, g, extra=None):
    from test_gpu_spectrum import check
    check(_Answers(outs["power"]), case.ins["raw"].data, case.host["coef"], case.host["decim"], None)


# ---- subband_power_batch_dev ---------------------------------------------------------------------------------------------------
def _subband_build(v):
    import subband_ref as ref
    from gsmcal import dist
    sf = dist.spectrum_filter
    name = {"big": "128taps/16", "small": "n4097"}.get(v, "ragged")
    raw, coef, w, decim = ref.case(name, sf)
    w = np.array(w)
    if v == "a2":                                   # other phases in the same slots: other tap rows, the same index table
        w = w + 0.01
    elif v == "a3":                                 # the same phases in other slots: the same tap rows, another index table
        w[0], w[1] = w[0][::-1].copy(), w[0].copy()
    elif v == "coef2":
        coef = np.random.default_rng(32).standard_normal(32)
    elif v == "small":
        raw, w = raw[:2], w[:2, :1]
    elif v == "refused":
        w[1, 1] = np.inf
    return _raw_case("subband_power", v, raw, {"coef": coef, "decim": decim, "w": w}, {"power": Out(w.shape, np.float64)},
                     "-1" if v == "refused" else None)


def _subband_check(case, outs, g, extra=None):
    from test_gpu_subband import check
    h = case.host
    check(_Answers(outs["power"]), None, case.ins["raw"].data, h["coef"], h["w"], h["decim"])


def _subband_cached(case):
    w = case.host["w"]
    fin = w[~np.isnan(w)]
    order = list(dict.fromkeys(fin.tolist()))
    idx = np.array([order.index(x) if x == x else -1 for x in w.ravel()], dtype=np.int32)
    uniq = np.array(order)
    return {"h_sb_coef": case.host["coef"], "h_sb_w": uniq, "h_sb_rows": np.outer(uniq, case.host["coef"]), "h_sb_idx": idx}


# ---- cw_check_batch_dev --------------------------------------------------------------------------------------------------------
_CW = {"a": (("small", "dense"), True, 0), "a2": (("dense", "small"), True, 0), "no_r": (("small", "dense"), False, 0),
       "wide": (("small", "dense"), True, 5), "big": (("clean", "drops"), True, 0), "small": (("tile_minus_1",), True, 0),
       "refused": (("small", "dense"), True, 0)}


def _cw_build(v):
    import cw_check_ref as ref
    names, with_r, pad = _CW[v]
    raw = np.stack([ref.raw(k) for k in names])
    d, n = len(raw), raw.shape[1] // 2
    stride = n - 1 + pad
    outs = {"summary": Out((d, 5 + 2 * 16), np.float64)}
    if with_r:
        col = np.arange(stride)[None, :] < n - 1
        outs["r"] = Out((d, stride), np.float64, col, ~col)                      # "N-1 written per row, the padding left alone"
    return _raw_case("cw_check", v, raw, {"thr": 0.0 if v == "refused" else ref.THR, "names": names, "r_stride": stride}, outs,
                     "-1" if v == "refused" else None)


def _cw_run(g, ctx, case, ptr):
    h = case.host
    g.cw_check_batch_dev(ptr["raw"], h["d"], h["n"], h["thr"], ptr["summary"], ptr.get("r"), h["r_stride"], ctx=ctx)


def _cw_check(case, outs, g, extra=None):
    from test_gpu_cw_check import check_row
    n = case.host["n"]
    for i, name in enumerate(case.host["names"]):
        check_row(g, outs["summary"][i], outs["r"][i, :n - 1] if "r" in outs else None, name)


def _cw_margins(case):
    import cw_check_ref as ref
    for name in case.host["names"]:                                             # tests/test_cw_check_cpu.py::test_margins_of_every_gpu_input
        m = ref.margins(name)
        assert m["min_abs_s"] > 0.0 and m["dist_pi"] >= 1e-3 and m["thr_margin"] >= 1e-3 and m["abs_mean_q"] >= 0.5, (name, m)
        assert m["numpy_vs_longdouble"] <= 1e-12 and m["events"] == sorted(ref.planted(name)) and m["lead"] >= 1e-3, (name, m)


# ---- iq_imbalance_batch_dev ----------------------------------------------------------------------------------------------------
def _iq_build(v):
    import gsmcal
    tile = gsmcal.IQ_TILE
    d, n, seed = {"a": (3, tile + 1, 0), "a2": (3, tile + 1, 1), "big": (3, 2 * tile + 5, 0), "small": (2, 9, 0), "refused": (2, 9, 0)}[v]
    raw = np.random.default_rng(1000 * n + d + seed).integers(0, 256, size=(d, 2 * n), dtype=np.uint8)
    return _raw_case("iq_imbalance", v, raw, {"odd": v == "refused"}, {"table": Out((d, gsmcal.IQ_COLS), np.float64)},
                     "-1" if v == "refused" else None)


def _iq_run(g, ctx, case, ptr):
    h = case.host
    g.iq_imbalance_batch_dev(ptr["raw"] + (1 if h["odd"] else 0), h["d"], h["n"], ptr["table"], ctx=ctx)


def _iq_check(case, outs, g, extra=None):
    import iq_imbalance_ref as ref
    from test_gpu_iq_imbalance import check_rows
    check_rows(outs["table"], ref.raw_table(case.ins["raw"].data), case.key)


# ---- the captures of the chain: fcch_scan_batch_dev and calibrate_batch_dev -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_captures(frames):
    """(raw (3, 2N), names): the planted captures of dongles 0 and 3 of tests/impaired.py at `frames` frames (62: the shortest that
    calibrates there, its "plain62"), and bytes of noise alone, which the chain leaves at its first exit with r_len = -1"""
    import impaired as im
    s = _synth()
    raws = [s.make_stream(num_frames=frames, **im.planted_args(b))[0] for b in ("d0", "d3")]
    rng = np.random.Generator(np.random.Philox(key=[62, frames]))
    raws.append(np.clip(np.rint(127.5 + 20.0 * rng.standard_normal(len(raws[0]))), 0, 255).astype(np.uint8))
    raw = np.stack(raws)
    raw.setflags(write=False)
    return raw, ("d0", "d3", "noise")


def _chain_raw(v):
    frames, rows = {"big": (72, (0, 1, 2)), "small": (62, (0,))}.get(v, (62, (0, 1, 2)))
    raw = chain_captures(frames)[0][list(rows)]
    return raw[:, : 2 * 22 * 10000] if v == "refused_short" else raw


@functools.lru_cache(maxsize=None)
def scan_oracle(v, taps):
    from oracle import gsmcal_oracle as o
    return [o.scan_capture(r, _scan_coef(taps)) for r in _chain_raw(v)]


def _scan_coef(taps):
    return _fir1(30, 200e3) if taps == "fir31" else _fir1(30, 170e3)


def _scan_build(v):
    import gsmcal
    raw = _chain_raw("refused_short" if v == "refused" else v)
    d, H = len(raw), gsmcal.MAX_HITS
    taps = "other31" if v == "a2" else "fir31"
    outs = {"snr_numhit": Out((d, 2), np.float64), "counts": Out((d,), np.int32)}
    if v != "refused":
        cnt = np.array([0 if s["coarse_pos"][0] == -1.0 else len(s["coarse_pos"]) for s in scan_oracle(v, taps)])
        listed = np.arange(H)[None, :] < cnt[:, None]                           # the header names [D][MAX_HITS] and says no more: the
        outs["positions"] = Out((d, H), np.float64, listed)                      # slots behind a capture's count are unspecified
        outs["pos_snr"] = Out((d, H), np.float64, listed)
    else:
        outs["positions"], outs["pos_snr"] = Out((d, H), np.float64), Out((d, H), np.float64)
    return _raw_case("fcch_scan", v, raw, {"coef": _scan_coef(taps), "taps": taps}, outs, "-5" if v == "refused" else None)


def _scan_run(g, ctx, case, ptr):
    h = case.host
    g.fcch_scan_batch_dev(ptr["raw"], h["d"], h["n"], h["coef"], ptr["snr_numhit"], ptr["positions"], ptr["pos_snr"], ptr["counts"], ctx=ctx)


def _scan_check(case, outs, g, extra=None):
    import parity
    from test_gpu_impaired import snr_same
    for i, live in enumerate(scan_oracle(case.variant, case.host["taps"])):    # tests/test_gpu_impaired.py::test_scanner_against_the_oracle
        n = int(outs["counts"][i])
        assert live["num_hit"] == outs["snr_numhit"][i, 1], (case.key, i, live["num_hit"], outs["snr_numhit"][i])
        assert snr_same(outs["snr_numhit"][i, 0], live["snr"]), (case.key, i, outs["snr_numhit"][i, 0], live["snr"])
        if live["coarse_pos"][0] == -1.0:
            assert n == 0, (case.key, i)
        else:
            parity.assert_positions(outs["positions"][i, :n], live["coarse_pos"], f"scan positions {case.key} {i}")
            assert snr_same(outs["pos_snr"][i, :n], live["coarse_snr"]), (case.key, i)


def _scan_margins(case):
    st = [s["coarse_pos"][0] != -1.0 for s in scan_oracle(case.variant, case.host["taps"])]
    assert st[0] and (len(st) < 3 or not st[2]), (case.key, st)                  # a capture with hits and, in a batch of three, one without


_CAL = {"r": {}, "coef2": {"coef": "other47"}, "ts2": {"ts": "tapered"}, "cf2": {"fc": FC + 40e6}, "no_r": {"with_r": False}, "big": {},
        "small": {}, "refused": {"coef": "none"}}


def _cal_args(v):
    s = _synth()
    kw = _CAL[v]
    coef = {"fir47": _fir1(46, 200e3), "other47": _fir1(46, 185e3), "none": np.zeros(0)}[kw.get("coef", "fir47")]
    ts = s.sch_training_sequence()
    if kw.get("ts") == "tapered":             # (a template turned by a constant phase gives the same bits: the search takes magnitudes)
        ts = ts * np.linspace(0.7, 1.3, len(ts))
    return coef, ts, kw.get("fc", FC), kw.get("with_r", True)


@functools.lru_cache(maxsize=None)
def cal_oracle(v):
    """the oracle's answer per stream of a calibrate variant, the corrected stream included"""
    from oracle import gsmcal_oracle as o
    coef, ts, fc, _ = _cal_args(v)
    return [o.calibrate_stream(r, coef, ts, fc, keep_r=True) for r in _chain_raw(v)]


def _cal_build(v):
    import gsmcal
    raw = _chain_raw(v)
    d, n = len(raw), raw.shape[1] // 2
    coef, ts, fc, with_r = _cal_args(v)
    outs = {"table": Out((d, gsmcal.TABLE_COLS), np.float64), "pos_info": Out((d, 2, gsmcal.MAX_POS_ROWS), np.float64),
            "r_len": Out((d,), np.int64)}
    if with_r:
        rl = np.ones(d, np.int64) if v == "refused" else np.array([o["r_len"] for o in cal_oracle(v)])
        # the header: r_correct [D][N] with r_len [D].  Written: the r_len samples of a stream that has one; it is silent about the
        # samples behind r_len and about the row of a stream with r_len = -1: unspecified
        outs["r_correct"] = Out((d, n), np.complex128, np.arange(n)[None, :] < rl[:, None])
    return _raw_case("calibrate", v, raw, {"coef": coef, "ts": ts, "fc": fc}, outs, "-1" if v == "refused" else None)


def _cal_run(g, ctx, case, ptr):
    h = case.host
    g.calibrate_batch_dev(ptr["raw"], h["d"], h["n"], h["coef"], h["ts"], h["fc"], ptr["table"], ptr["pos_info"], ptr.get("r_correct"),
                          ptr["r_len"], ctx=ctx)


def cal_as_out(outs):
    """the device outputs as the dict g.calibrate_batch returns (tests/test_gpu_exit_paths.py as_out); what still holds the prefill
    pattern in r_correct becomes NaN, the prefill check_against_oracle expects where nothing may be written"""
    table, p = outs["table"], outs["pos_info"]
    rows = []
    for i in range(len(table)):
        k = int(table[i, 7])
        rows.append(-np.ones((k, 2)) if table[i, 8] == -1.0 else p[i, :, :k].T.copy())
    r = None
    if "r_correct" in outs:
        r = outs["r_correct"].copy()
        untouched = np.all(r.view(np.uint64).reshape(r.shape + (2,)) == np.uint64(_PATTERN[8]), axis=-1)
        r[untouched] = np.nan
    return {"table": table, "pos_info": rows, "pos_info_raw": p, "r_len": outs["r_len"], "r_correct": r}


def _cal_check(case, outs, g, extra=None):
    import parity
    from test_gpu_exit_paths import check_against_oracle
    orcs = cal_oracle(case.variant)
    out = cal_as_out(outs)
    cases = [{"name": f"{case.variant}/{i}", "orc": o, "status": o["status"]} for i, o in enumerate(orcs)]
    if out["r_correct"] is not None and extra is not None:
        check_against_oracle(cases, out, extra["det"])
    else:                                                                        # without r_correct (or without the details): the rows
        for i, o in enumerate(orcs):
            if extra is not None:
                parity.compare_stream(o, out["table"][i], extra["det"], i, out["pos_info"][i])
            assert out["table"][i, 9] == o["status"] and out["r_len"][i] == o["r_len"], (case.key, i)
    p = outs["pos_info"]                                                         # "pos_info [D][2][MAX_POS_ROWS] with -1 padding"
    for i in range(len(p)):
        k = int(outs["table"][i, 7])
        assert np.all(p[i, :, k:] == -1.0), (case.key, i, "the padding of pos_info")


def _cal_margins(case):
    st = [o["status"] for o in cal_oracle(case.variant)]
    assert st[0] == 0 and (len(st) < 3 or (st[1] == 0 and st[2] != 0)), (case.key, st)     # the batch calibrates; the noise leaves early
    assert all((o["r_len"] > 0) == (o["status"] in (0, 11)) for o in cal_oracle(case.variant))


# ================================================================ the follow-up families ========================================
# All six take (r [D][stride], r_len [D], pos_info [D][2][MAX_POS_ROWS]).  A batch here is: the family's own designed streams,
# each its own length, in rows 13 samples longer than the longest; behind r_len a row holds plausible samples (seeded noise at the
# streams' level), and the last row is a stream with r_len = -1 and the table of stream 0 -- samples and a table that nothing may
# use.  The calibrated batches ("cal8", "cal4") are the three streams of the calibrate entry as ONE calibrate_batch call
# returned them (the GPU session's, passed in through `use_calibrated`; without a GPU the oracle's), decimated by two for "cal4".
_CALIBRATED = {}


def use_calibrated(r=None, r_len=None, pos_info=None):
    """hand the registry the session's calibrate_batch outputs (8x); the cal* variants are built from them from then on (no
    arguments: back to the oracle's).  What lies behind r_len -- and the row of a stream without one -- is set to 1 + 1j: the
    library's staging buffer returns whatever it held there"""
    _CALIBRATED.clear()
    if r is not None:
        r, r_len = np.array(r, dtype=np.complex128), np.asarray(r_len, dtype=np.int64).copy()
        r[np.arange(r.shape[1])[None, :] >= r_len[:, None]] = 1.0 + 1.0j
        _CALIBRATED[8] = (r, r_len, np.ascontiguousarray(pos_info, dtype=np.float64))
    _build_cached.cache_clear()
    _calibrated.cache_clear()


def followup_case(name, tag, r, r_len, pos_info):
    """the cal8 case of a follow-up entry on another calibrated batch (what a calibrate call with other arguments returned)"""
    e = REGISTRY[name]
    keep = dict(_CALIBRATED)
    try:
        use_calibrated(r, r_len, pos_info)
        case = e._build("cal8")
    finally:
        _CALIBRATED.clear()
        _CALIBRATED.update(keep)
        _build_cached.cache_clear()
        _calibrated.cache_clear()
    case.variant = tag
    return case


def oracle_calibrated():
    """the oracle's r, r_len and pos_info of the calibrate entry's "r" variant in the batch form's layout"""
    import gsmcal
    orcs = cal_oracle("r")
    n = _chain_raw("r").shape[1] // 2
    r = np.zeros((len(orcs), n), dtype=np.complex128)
    rl = np.array([o["r_len"] for o in orcs], dtype=np.int64)
    pi = -np.ones((len(orcs), 2, gsmcal.MAX_POS_ROWS))
    for i, o in enumerate(orcs):
        if o["r_len"] > 0:
            r[i, :o["r_len"]] = o["r_correct"]
        p = np.atleast_2d(o["pos_info"])
        pi[i, :, :len(p)] = p.T
    return r, rl, pi


@functools.lru_cache(maxsize=None)
def _calibrated(ov):
    if ov == 8:
        return _CALIBRATED[8] if 8 in _CALIBRATED else oracle_calibrated()
    r, rl, pi = _calibrated(2 * ov)
    pi2 = pi.copy()                                                              # bcch_decode_ref.decimate_by_2 on the batch layout
    used = pi[:, 1, :] != -1.0
    pi2[:, 0, :][used] = (np.floor((pi[:, 0, :] - 1) / 2) + 1)[used]
    return np.ascontiguousarray(r[:, ::2]), np.where(rl > 0, (rl + 1) // 2, rl), pi2


def _table(pos):
    import pair_coherence_ref as pc
    return pc.raw_table(np.asarray(pos, dtype=np.float64).reshape(-1, 2))


def _batch(streams, seed):
    """[(s, pos)] -> r, r_len, pos_info, live as described above"""
    rng = np.random.Generator(np.random.Philox(key=[2200, seed]))
    lens = [len(s) for s, _ in streams]
    stride, d = max(lens) + 13, len(streams) + 1
    level = float(np.sqrt(np.mean(np.abs(streams[0][0]) ** 2)))
    r = level * (rng.standard_normal((d, stride)) + 1j * rng.standard_normal((d, stride))) / math.sqrt(2.0)
    live = np.zeros((d, stride), bool)
    for i, (s, _) in enumerate(streams):
        r[i, :len(s)], live[i, :len(s)] = s, True
    r_len = np.array(lens + [-1], dtype=np.int64)
    pi = np.stack([_table(p) for _, p in streams] + [_table(streams[0][1])])
    return r, r_len, pi, live


def _post_ins(r, r_len, pi, live):
    return {"r": In(r, live), "r_len": In(r_len), "pos_info": In(pi)}


def _post_ov(v):
    digits = [c for c in v if c.isdigit()]
    return int(digits[0]) if digits else 8


def _post_streams(case):
    """(i, s, pos rows) of every stream of a follow-up case that has samples and a table"""
    r, rl, pi = (case.ins[k].data for k in ("r", "r_len", "pos_info"))
    for i in range(len(r)):
        if rl[i] > 0 and not np.all(pi[i] == -1.0):
            k = int(np.max(np.nonzero(np.any(pi[i] != -1.0, axis=0))[0])) + 1
            yield i, np.ascontiguousarray(r[i, :min(int(rl[i]), r.shape[1])]), pi[i, :, :k].T.copy()


def _post_build(entry, v, designed, host, outs_of, refused_code=None, seed=0):
    """designed(ov) -> [(s, pos)]; host(ov, d, v) -> the host arguments; outs_of(d, stride, r_len, host) -> the outputs"""
    ov = _post_ov(v)
    if v.startswith("cal"):
        r, r_len, pi = _calibrated(ov)
        live = np.arange(r.shape[1])[None, :] < r_len[:, None]
    else:
        r, r_len, pi, live = _batch(designed(ov), 10 * seed + ov)
    d, stride = r.shape
    h = dict(host(ov, d, v), ov=ov, d=d, stride=stride)
    return Case(entry, v, h, _post_ins(r, r_len, pi, live), outs_of(d, stride, r_len, h), refused_code if v == "refused" else None)


def _dead(case):
    r, rl, pi = (case.ins[k].data for k in ("r", "r_len", "pos_info"))
    return [i for i in range(len(r)) if rl[i] <= 0 or np.all(pi[i] == -1.0)]


_POST_VARIANTS = {"ov8": "the designed streams at 8x", "ov2": "at 2x: a smaller problem, another twiddle table", "ov4": "at 4x",
                  "cal8": "the calibrated batch: a larger problem", "cal4": "the calibrated batch decimated by two"}


# ---- fcch_demod_batch_dev ------------------------------------------------------------------------------------------------------
def _fd_designed(ov):
    import bcch_demod_ref as bd
    import pair_coherence_ref as pc
    a, _, pos, _ = pc.designed_pair(ov)
    return [bd.designed_stream(_synth(), ov, [2, 2, 2, 2], nf=2, seed=1), (a, np.array(pos))]


def _fd_host(ov, d, v):
    cf = FC + 1e6 * np.arange(d)
    return {"cf": cf + 35e6 if v == "ov8b" else cf, "ov_arg": 40 if v == "refused" else ov}


def _fd_build(v):
    import gsmcal
    return _post_build("fcch_demod", v, _fd_designed, _fd_host, lambda d, stride, rl, h: {"out": Out((d, gsmcal.DEMOD_COLS), np.float64)}, "-6")


def _fd_run(g, ctx, case, ptr):
    h = case.host
    g.fcch_demod_batch_dev(ptr["r"], h["stride"], ptr["r_len"], ptr["pos_info"], h["d"], h["ov_arg"], h["cf"], ptr["out"], ctx=ctx)


def _fd_want(case):
    import fcch_demod_ref as ref
    return {i: ref.fcch_demod(s, pos, case.host["ov"], case.host["cf"][i]) for i, s, pos in _post_streams(case)}


def _fd_compare(got, want, fc):
    """tests/test_gpu_fcch_demod.py compare() holds carrier_ppm to 1e-6 ppm of ITS carrier; a stream with another carrier is compared
    through the frequency (the same bound in Hz) and the definition carrier_ppm = 1e6 (mean_freq - symbol_rate/4) / carrier"""
    import test_gpu_fcch_demod as t
    scale = fc / t.FC
    t.compare(dict(got, carrier_ppm=got["carrier_ppm"] * scale), dict(want, carrier_ppm=want["carrier_ppm"] * scale))


def _fd_check(case, outs, g, extra=None):
    from test_gpu_fcch_demod import check_sentinel_row
    t = g.demod_rows(outs["out"])
    want = _fd_want(case)
    for i in _dead(case):
        check_sentinel_row(outs["out"][i])
    for i, w in want.items():
        k = int(t["num_fcch"][i])
        got = {"freq": t["freq"][i, :k], "snr": t["snr"][i, :k], "max_idx": t["max_idx"][i, :k].astype(np.int64),
               "mean_freq": float(t["mean_freq"][i]), "carrier_ppm": float(t["carrier_ppm"][i])}
        assert t["status"][i] == 0.0 and np.all(np.isnan(outs["out"][i, 4 + k:28])), (case.key, i)
        _fd_compare(got, w, case.host["cf"][i])


def _fd_margins(case):
    want = _fd_want(case)
    assert len(want) >= 2 and sum(len(w["freq"]) for w in want.values()) >= 3
    for i, w in want.items():
        _fd_compare(w, w, case.host["cf"][i])


# ---- bcch_demod_batch_dev ------------------------------------------------------------------------------------------------------
def _bc_designed(ov):
    import bcch_demod_ref as bd
    return [bd.designed_stream(_synth(), ov, [3, 3, 3, 3, 3], nf=1), bd.designed_stream(_synth(), ov, [1, 6, 1, 1], nf=2, seed=2)]


def _bc_host(ov, d, v):
    nts = _synth().normal_training_sequences(ov)
    cf = FC + 1e6 * np.arange(d)
    return {"cf": cf, "nts": nts * np.exp(0.4j) if v == "ov8b" else nts, "bare": v == "ov8c", "short_ts": v == "refused"}


def _bc_outs(d, stride, r_len, h):
    import gsmcal
    outs = {"out": Out((d, gsmcal.BCCH_COLS), np.float64)}
    if not h["bare"]:
        outs["corr"] = Out((d, gsmcal.MAX_BCCH, 8), np.complex128)
        # "r_out [D][stride] complex with r_len_out [D]: the rotated stream and its length, -1 wherever the reference leaves r = -1
        # (the _dev form leaves those rows of r_out untouched)".  The samples behind a stream's length: unspecified
        has = r_len > 0
        col = np.arange(stride)[None, :] < np.minimum(r_len, stride)[:, None]
        outs["r_out"] = Out((d, stride), np.complex128, col & has[:, None], np.broadcast_to(~has[:, None], (d, stride)))
        outs["r_len_out"] = Out((d,), np.int64)
    return outs


def _bc_build(v):
    return _post_build("bcch_demod", v, _bc_designed, _bc_host, _bc_outs, "-1", seed=1)


def _bc_run(g, ctx, case, ptr):
    h = case.host
    nts = h["nts"][:-1] if h["short_ts"] else h["nts"]
    g.bcch_demod_batch_dev(ptr["r"], h["stride"], ptr["r_len"], ptr["pos_info"], h["d"], h["ov"], nts, h["cf"], ptr["out"],
                           d_corr=ptr.get("corr"), d_r_out=ptr.get("r_out"), d_r_len_out=ptr.get("r_len_out"), ctx=ctx)


def _bc_want(case):
    import bcch_demod_ref as ref
    h = case.host
    return {i: ref.bcch_demod(s, pos, h["nts"], h["ov"], h["cf"][i]) for i, s, pos in _post_streams(case)}


def _bc_compare(got, want, s, pos, ov, fc):
    import test_gpu_bcch_demod as t
    scale = fc / t.FC                                                            # (as _fd_compare: carrier_ppm at the module's carrier)
    t.compare(dict(got, carrier_ppm=got["carrier_ppm"] * scale), dict(want, carrier_ppm=want["carrier_ppm"] * scale), s, pos, ov)


def _bc_check(case, outs, g, extra=None):
    from test_gpu_bcch_demod import check_no_pos_row
    h = case.host
    if h["bare"]:                                                                # without the optional outputs: the rows of the full call, which
        full = extra["anchor"](("bcch_demod", "ov8"))                            # is itself held to the restatement
        assert same_bits(outs["out"], full["out"]), case.key
        return
    t = g.bcch_rows(outs["out"])
    rl = case.ins["r_len"].data
    for i in _dead(case):
        check_no_pos_row(outs["out"][i])
        assert outs["r_len_out"][i] == -1 and np.all(np.isnan(outs["corr"][i])), (case.key, i)
    streams = {i: (s, pos) for i, s, pos in _post_streams(case)}
    for i, w in _bc_want(case).items():
        k = int(t["num_bcch"][i])
        s, pos = streams[i]
        assert w["status"] in (0, 13) and outs["r_len_out"][i] == rl[i], (case.key, i, w["status"])
        got = {"status": int(t["status"][i]), "idx": int(t["tsc_idx"][i]), "num_bcch": k, "num_agree": t["num_agree"][i],
               "mean_fo": float(t["mean_fo"][i]), "carrier_ppm": float(t["carrier_ppm"][i]), "corr_val": outs["corr"][i, :4].T,
               "r": outs["r_out"][i, :int(rl[i])]}
        for f in ("max_idx", "peak", "runner_up", "phase"):
            got[f] = t[f][i, :k]
        _bc_compare(got, w, s, pos, h["ov"], h["cf"][i])


def _bc_margins(case):
    streams = {i: (s, pos) for i, s, pos in _post_streams(case)}
    want = _bc_want(case)
    assert len(want) >= 2
    if not case.variant.startswith("cal"):
        assert sorted(w["status"] for w in want.values()) == [0, 13], [w["status"] for w in want.values()]
    for i, w in want.items():
        assert w["status"] in (0, 13)
        _bc_compare(dict(w, corr_val=w["corr_val"][:, :4]), w, *streams[i], case.host["ov"], case.host["cf"][i])


# ---- sch_decode_batch_dev ------------------------------------------------------------------------------------------------------
_SCH_FRAMES = (0, 10, 20)                     # the first three bursts of the designed five-burst stream of tests/sch_decode_ref.py


def _sd_designed(ov):
    import sch_decode_ref as ref
    s = _synth()
    fns = [ref.DESIGNED_FN0 + f for f in _SCH_FRAMES]
    clean = [s.sch_encode(ref.DESIGNED_BSIC, fn) for fn in fns]
    hurt = [c.copy() for c in clean]
    hurt[1][20:34] ^= 1                                                          # "flipped": the CRC of burst 1 fails
    return [ref.designed_stream(ov, clean, _SCH_FRAMES, seed=0), ref.designed_stream(ov, hurt, _SCH_FRAMES, seed=1)]


def _sd_host(ov, d, v):
    return {"ts": np.zeros(64 * ov + (1 if v == "refused" else 0), dtype=np.complex128)}


def _sd_outs(d, stride, r_len, h):
    import gsmcal
    return {"out": Out((d, gsmcal.SCH_COLS), np.float64), "soft": Out((d, gsmcal.MAX_HITS, 148), np.float64),
            "u": Out((d, gsmcal.MAX_HITS, 39), np.uint8)}


def _sd_build(v):
    return _post_build("sch_decode", v, _sd_designed, _sd_host, _sd_outs, "-1", seed=2)


def _sd_run(g, ctx, case, ptr):
    h = case.host
    g.sch_decode_batch_dev(ptr["r"], h["stride"], ptr["r_len"], ptr["pos_info"], h["d"], h["ov"], h["ts"], ptr["out"], d_soft=ptr["soft"],
                           d_u=ptr["u"], ctx=ctx)


def _sd_want(case):
    import sch_decode_ref as ref
    return {i: (ref.sch_decode(s, pos, case.host["ov"]), s, pos) for i, s, pos in _post_streams(case)}


def _sd_check(case, outs, g, extra=None):
    from test_gpu_sch_decode import check_no_pos_row, compare
    t = g.sch_rows(outs["out"])
    for i in _dead(case):
        check_no_pos_row(outs["out"][i])
        assert np.all(outs["u"][i] == 255) and np.all(np.isnan(outs["soft"][i])), (case.key, i)
    for i, (w, s, pos) in _sd_want(case).items():
        k = int(t["num_sch"][i])
        got = {"status": int(t["status"][i]), "bsic": int(t["bsic"][i]), "fn_anchor": int(t["fn_anchor"][i]), "pos_anchor": int(t["pos_anchor"][i]),
               "num_sch": k, "num_ok": int(t["num_ok"][i]), "num_consistent": int(t["num_consistent"][i]), "mean_slope": float(t["mean_slope"][i]),
               "u": outs["u"][i, :k], "soft": outs["soft"][i, :k]}
        for f in ("ok", "bsic_b", "fn", "ts_err", "corrected", "slope", "amp"):
            got[f] = t[f][i, :k]
        compare(got, w, s, pos, case.host["ov"])
        assert np.all(outs["u"][i, k:] == 255) and np.all(np.isnan(outs["soft"][i, k:])), (case.key, i, "the unused slots")


def _sd_margins(case):
    from test_gpu_sch_decode import compare
    want = _sd_want(case)
    assert len(want) >= 2
    for i, (w, s, pos) in want.items():
        compare(w, w, s, pos, case.host["ov"])
    if not case.variant.startswith("cal"):
        assert [w["status"] for w, _, _ in want.values()] == [0, 0] and [w["num_ok"] for w, _, _ in want.values()] == [3, 2]


# ---- bcch_decode_batch_dev -----------------------------------------------------------------------------------------------------
def _bd_designed(ov):
    import bcch_decode_ref as ref
    return [ref.designed_case(ov, k)[:2] for k in ("clean", "flipped")]


def _bd_host(ov, d, v):
    import bcch_decode_ref as ref
    import impaired as im
    if v.startswith("cal"):
        tsc = [im.PLANTED["d0"][1], im.PLANTED["d3"][1], 0][:d]
    else:
        tsc = [ref.DESIGNED_TSC] * d
    tsc = np.array(tsc, dtype=np.int32)
    if v == "ov8b":
        tsc[0] = (tsc[0] + 1) % 8                                                # the wrong code for stream 0: nothing passes the Fire code there
    if v == "refused":
        tsc[1] = 8
    return {"tsc": tsc}


def _bd_outs(d, stride, r_len, h):
    import gsmcal
    return {"out": Out((d, gsmcal.SI_COLS), np.float64), "octets": Out((d, gsmcal.MAX_HITS, 23), np.uint8),
            "soft": Out((d, gsmcal.MAX_HITS, 456), np.float64)}


def _bd_build(v):
    return _post_build("bcch_decode", v, _bd_designed, _bd_host, _bd_outs, "-1", seed=3)


def _bd_run(g, ctx, case, ptr):
    h = case.host
    g.bcch_decode_batch_dev(ptr["r"], h["stride"], ptr["r_len"], ptr["pos_info"], h["d"], h["ov"], h["tsc"], ptr["out"], ptr["octets"],
                            d_soft=ptr["soft"], ctx=ctx)


def _bd_want(case):
    import bcch_decode_ref as ref
    return {i: (ref.bcch_decode(s, pos, int(case.host["tsc"][i]), case.host["ov"]), s, pos) for i, s, pos in _post_streams(case)}


def _bd_check(case, outs, g, extra=None):
    from test_gpu_bcch_decode import check_no_pos, compare
    t = g.si_rows(outs["out"])
    for i in _dead(case):
        check_no_pos({"table": outs["out"], "octets": outs["octets"]}, i)
        assert np.all(np.isnan(outs["soft"][i])), (case.key, i)
    for i, (w, s, pos) in _bd_want(case).items():
        k = int(t["num_blocks"][i])
        got = {"status": int(t["status"][i]), "num_blocks": k, "num_ok": int(t["num_ok"][i]), "first_ok": int(t["first_ok"][i]),
               "octets": outs["octets"][i, :k], "soft": outs["soft"][i, :k]}
        for f in g.SI_BLOCK_FIELDS:
            got[f] = t[f][i, :k]
        compare(got, w, s, pos, case.host["ov"])
        assert np.all(outs["octets"][i, k:] == 0) and np.all(np.isnan(outs["soft"][i, k:])), (case.key, i, "the unused slots")


def _bd_margins(case):
    from test_gpu_bcch_decode import compare
    want = _bd_want(case)
    assert len(want) >= 2
    for i, (w, s, pos) in want.items():
        compare(w, w, s, pos, case.host["ov"])
    if case.variant in ("ov8", "ov4", "ov2"):
        assert [w["status"] for w, _, _ in want.values()] == [0, 15]
    if case.variant.startswith("cal"):
        assert all(w["status"] == 0 for w, _, _ in want.values())


# ---- pair_coherence_batch_dev --------------------------------------------------------------------------------------------------
def _pc_designed(ov):
    import pair_coherence_ref as pc
    a, b, pos, _ = pc.designed_pair(ov)
    return [(a, np.array(pos)), (b, np.array(pos)), (a[::-1].copy(), np.array(pos))]     # stream 2: samples no pair names


def _pc_host(ov, d, v):
    # (0, 1): the designed pair; (0, 3): b is the stream with r_len = -1; the maximum one lag off the centre (lag0 10, D = 11.25)
    pairs, lag0 = [(0, 1), (0, 3)], [10, 10]
    if v == "ov8b":
        pairs, lag0 = [(0, 1), (1, 0)], [10, -12]
    if v == "refused":
        pairs = [(0, 1), (0, d)]
    return {"pairs": np.array(pairs, dtype=np.int32), "lag0": np.array(lag0, dtype=np.int32), "M": 3}


def _pc_outs(d, stride, r_len, h):
    import gsmcal
    p = len(h["pairs"])
    return {"out": Out((p, gsmcal.PAIR_COLS), np.float64), "corr": Out((p, gsmcal.MAX_PAIR_BURSTS, 2 * h["M"] + 1, 4), np.complex128)}


def _pc_build(v):
    case = _post_build("pair_coherence", v, _pc_designed, _pc_host, _pc_outs, "-1", seed=4)
    named = np.zeros(case.host["d"], bool)
    if v != "refused":
        named[case.host["pairs"].ravel()] = True
    case.ins["r"].live &= named[:, None]                                         # "streams no pair names"
    return case


def _pc_run(g, ctx, case, ptr):
    h = case.host
    g.pair_coherence_batch_dev(ptr["r"], h["stride"], ptr["r_len"], ptr["pos_info"], h["d"], h["ov"], h["pairs"], h["lag0"], ptr["out"],
                               max_lag=h["M"], d_corr=ptr["corr"], ctx=ctx)


def _pc_want(case):
    import pair_coherence_ref as pc
    h = case.host
    r, rl, pi = (case.ins[k].data for k in ("r", "r_len", "pos_info"))
    return [pc.pair_coherence(r, rl, pi, h["ov"], int(a), int(b), int(l), h["M"]) for (a, b), l in zip(h["pairs"], h["lag0"])]


def _pc_check(case, outs, g, extra=None):
    from test_gpu_pair_coherence import compare
    for q, w in enumerate(_pc_want(case)):
        compare(outs["out"][q], outs["corr"][q], w, f"{case.key} pair {q}")
        assert outs["out"][q, 0] == w["row"][0]


def _pc_margins(case):
    import pair_coherence_ref as pc
    want = _pc_want(case)
    assert all(pc.ties_ok(w) for w in want)
    assert want[0]["row"][0] == 0 and want[0]["used"].sum() == 3 and np.all(want[0]["mstar"][:3] == 1)
    assert want[1]["row"][0] == (0 if case.variant == "ov8b" else S_POST_NO_POS)


# ---- pair_align_batch_dev ------------------------------------------------------------------------------------------------------
def _pa_host(ov, d, v):
    import pair_align_ref as ref
    n = 3750 * ov
    rows = np.array([list(ref.ref_row(0.5)), [11.2503717, 1000.0, 300.0, 0.7, 0.0, 0.2], [-25.6, 3.7, 40.0, 0.1, 1000.0, 0.25],
                     [3.4, -0.9, 3000.0, 1.3, 333.0, 0.1]])
    members = [0, 1, 1, 3]                                                       # stream 3 has r_len = -1: status 10, left out of the sum
    if v == "ov8b":
        members, rows = [1, 0, 1, 3], rows[[0, 2, 1, 3]] + np.array([0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    if v == "refused":
        rows[1, 1] = 1000.5
    form = {"ov8c": "aligned", "ov8d": "combined"}.get(v, "both")
    return {"members": np.array(members, dtype=np.int32), "params": rows, "out_len": n - 7, "form": form}


def _pa_outs(d, stride, r_len, h):
    import gsmcal
    G, n = len(h["members"]), h["out_len"]
    outs = {"info": Out((G + 1, gsmcal.ALIGN_INFO_COLS), np.float64)}
    if h["form"] in ("both", "aligned"):
        outs["aligned"] = Out((G, n), np.complex128)
    if h["form"] in ("both", "combined"):
        outs["combined"] = Out((n,), np.complex128)
    return outs


def _pa_build(v):
    case = _post_build("pair_align", v, _pc_designed, _pa_host, _pa_outs, "-1", seed=4)
    named = np.zeros(case.host["d"], bool)
    named[case.host["members"]] = True
    case.ins["r"].live &= named[:, None]                                         # "streams no member names"
    return case


def _pa_run(g, ctx, case, ptr):
    h = case.host
    g.pair_align_batch_dev(ptr["r"], h["stride"], ptr["r_len"], h["d"], h["ov"], h["members"], h["params"], h["out_len"], ptr["info"],
                           d_aligned=ptr.get("aligned"), d_combined=ptr.get("combined"), ctx=ctx)


def _pa_want(case):
    import pair_align_ref as ref
    h = case.host
    return ref.pair_align_batch(case.ins["r"].data, case.ins["r_len"].data, h["ov"], h["members"], h["params"], h["out_len"])


def _pa_check(case, outs, g, extra=None):
    from test_gpu_pair_align import compare
    compare({k: outs[k] for k in ("info", "aligned", "combined") if k in outs}, _pa_want(case), str(case.key))


def _pa_margins(case):
    import pair_align_ref as ref
    want = _pa_want(case)
    assert ref.no_x_near_an_integer(want["x"][~want["exact"]]), case.key
    assert want["info"][:, 0].tolist() == [0.0, 0.0, 0.0, 10.0, 3.0], want["info"][:, 0]
    assert np.all(want["info"][:3, 3] > case.host["out_len"] - 200)


# ================================================================ the array family ===============================================
@functools.lru_cache(maxsize=None)
def array_data():
    """the `data` fixture of tests/test_gpu_array.py with 6 rows instead of 70: random rows of different power, 3 chunks + 200 long"""
    import gsmcal
    chunk = gsmcal.COV_CHUNK
    stride, d = 3 * chunk + 200, 6
    rng = np.random.Generator(np.random.Philox(key=[21, 70]))
    x = rng.standard_normal((d, stride)) + 1j * rng.standard_normal((d, stride))
    x *= np.exp(rng.uniform(-3.0, 3.0, (d, 1)))
    x.setflags(write=False)
    return x, stride, chunk


def _cov_build(v):
    x, stride, chunk = array_data()
    rows, wins = {"a": ([4, 1, 3, 4], [(0, 0), (37, 64), (stride - chunk + 1, chunk - 1), (5, chunk + 1)]),
                  "a2": ([1, 4, 4, 3], [(3, 0), (37, 65), (stride - chunk, chunk), (5, chunk + 1)]),
                  "big": ([5, 0, 2, 1, 5], [(0, 1), (1, 63), (37, 64), (stride - 65, 65), (0, chunk), (37, chunk + 1), (193, 3 * chunk + 7),
                                            (0, stride), (stride, 0)]),
                  "small": ([2], [(100, 300)]),
                  "refused": ([4, 1, 3, 4], [(0, 0), (37, 64), (stride - chunk + 2, chunk - 1), (5, chunk + 1)])}[v]
    rows, wins = np.array(rows, dtype=np.int32), np.array(wins, dtype=np.int64)
    live = np.zeros(x.shape, bool)
    for s, ln in wins:
        live[np.unique(rows), s:s + ln] = True                                   # "samples outside every covariance window"; rows nothing names
    G, W = len(rows), len(wins)
    return Case("array_covariance", v, {"rows": rows, "windows": wins, "stride": stride, "d": len(x)}, {"x": In(x, live)},
                {"cov": Out((W, G, G), np.complex128)}, "-1" if v == "refused" else None)


def _cov_run(g, ctx, case, ptr):
    h = case.host
    g.array_covariance_dev(ptr["x"], h["stride"], h["d"], h["rows"], h["windows"], ptr["cov"], ctx=ctx)


def _cov_check(case, outs, g, extra=None):
    from test_gpu_array import check_cov
    check_cov(outs["cov"], case.ins["x"].data, case.host["rows"], case.host["windows"], str(case.key))


def _comb_build(v):
    from test_gpu_array import weights_for
    x, stride, chunk = array_data()
    B = {"b1": 1, "b3": 3, "b3w": 3, "b3r": 3, "b16": 16, "big": 16, "small": 1, "refused": 3}[v]
    rows = {"b3r": [1, 4, 4, 3], "big": [5, 0, 2, 1, 5], "small": [2]}.get(v, [4, 1, 3, 4])
    out_len = {"big": stride, "small": 1, "refused": stride + 1}.get(v, 257)
    w = weights_for(len(rows), 16, 7 if v == "b3w" else len(rows))[:B]
    rows = np.array(rows, dtype=np.int32)
    live = np.zeros(x.shape, bool)
    live[np.unique(rows), :out_len] = True                                       # "samples at n >= out_len"; rows nothing names
    return Case("array_combine", v, {"rows": rows, "weights": w, "out_len": out_len, "stride": stride, "d": len(x)}, {"x": In(x, live)},
                {"out": Out((B, min(out_len, stride)), np.complex128)}, "-1" if v == "refused" else None)


def _comb_run(g, ctx, case, ptr):
    h = case.host
    g.array_combine_dev(ptr["x"], h["stride"], h["d"], h["rows"], h["weights"], h["out_len"], ptr["out"], ctx=ctx)


def _comb_check(case, outs, g, extra=None):
    import array_ref as ref
    h = case.host                                                                # tests/test_gpu_array.py::test_combine_against_the_restatement
    x = case.ins["x"].data
    want, bound = ref.array_combine(x, h["rows"], h["weights"], h["out_len"]), ref.combine_bound(x, h["rows"], h["weights"], h["out_len"])
    assert outs["out"].shape == want.shape and np.all(np.abs(outs["out"] - want) <= bound), case.key


def _nothing(case):
    pass


def _host_cached(**names):
    return lambda case: {cache: np.asarray(case.host[key]) for cache, key in names.items()}


def _pc_cached(case):
    return {"h_pc_pairs": np.concatenate([case.host["pairs"], case.host["lag0"][:, None]], axis=1)}


# the refused variant of every entry: the rule of include/gsmcal.h it breaks, and the code the call answers
REFUSALS = {
    "frontend": "decim 300 with 47 taps: more raw samples than a workgroup can stage (GSMCAL_E_UNSUPPORTED, nothing written)",
    "band_power": "1 025 taps (1 <= ntaps <= 1024, anything else GSMCAL_E_ARG)",
    "subband_power": "an infinite phase_rotate (GSMCAL_E_ARG, decided before anything is enqueued)",
    "cw_check": "thr = 0 (thr must be finite and > 0: GSMCAL_E_ARG, decided before anything is enqueued)",
    "iq_imbalance": "raw at an odd address (raw 2-byte aligned in the _dev form, anything else GSMCAL_E_ARG)",
    "fcch_scan": "22 frames: fewer than the 23 FCCH_coarse_position.m:25 indexes (GSMCAL_E_INDEX instead of reading out of bounds)",
    "calibrate": "no taps (ntaps < 1: GSMCAL_E_ARG)",
    "fcch_demod": "oversampling_ratio 40 (GSMCAL_E_UNSUPPORTED from 34 on)",
    "bcch_demod": "templates of 26*ov - 1 samples (any other len_ts: GSMCAL_E_ARG)",
    "sch_decode": "a template of 64*ov + 1 samples (len_ts != 64*ov: GSMCAL_E_ARG)",
    "bcch_decode": "a training sequence code of 8 (each 0..7, anything else GSMCAL_E_ARG)",
    "pair_coherence": "a pair that names stream D (each in [0, D), anything else GSMCAL_E_ARG, decided before anything is enqueued)",
    "pair_align": "|slope_ppm| = 1000.5 (decided before anything is enqueued: GSMCAL_E_ARG)",
    "array_covariance": "a window with start + len = stride + 1 (decided before anything is enqueued: GSMCAL_E_ARG)",
    "array_combine": "out_len = stride + 1 (1 <= out_len <= stride: GSMCAL_E_ARG)",
}
_RAW_V = {"a": "the smallest shape", "a2": "the same sizes with other contents", "big": "a larger problem", "small": "a smaller problem"}
_ARGS = {
    "frontend": lambda h, p: (h["coef"], h["decim"], p["out"]),
    "band_power": lambda h, p: (h["coef"], h["decim"], p["power"]),
    "subband_power": lambda h, p: (h["coef"], h["w"], p["power"], h["decim"]),
}

ENTRIES = [
    Entry("frontend", "front end", "gsmcal_frontend_batch_dev", ["h_coef"], ["coef", "state"], _RAW_V, "refused", {"h_coef": ("a", "a2")},
          "3 streams x 4 099 samples, decim 7: 586 outputs = two blocks of 256 and a partial one",
          _frontend_build, _raw_run("frontend_batch_dev", _ARGS["frontend"]), _frontend_check, _nothing, _host_cached(h_coef="coef")),
    Entry("band_power", "band power", "gsmcal_band_power_batch_dev", ["h_bp_coef"], ["bp_state", "bp_part"], _RAW_V, "refused",
          {"h_bp_coef": ("a", "a2")}, "3 captures x 30 001 samples, 64 taps, decim 20: 1 501 kept rows, several blocks, the last partial",
          _band_build, _raw_run("band_power_batch_dev", _ARGS["band_power"]), _band_check, _nothing, _host_cached(h_bp_coef="coef")),
    Entry("subband_power", "band power", "gsmcal_subband_power_batch_dev", ["h_sb_coef", "h_sb_w", "h_sb_rows", "h_sb_idx"],
          ["sb_state", "sb_part", "sb_taps"], dict(_RAW_V, a3="the same phases in other slots", coef2="the same phases, other taps"), "refused",
          {"h_sb_coef": ("a", "coef2"), "h_sb_w": ("a", "a2"), "h_sb_rows": ("a", "a2"), "h_sb_idx": ("a", "a3")},
          "4 captures x 30 001 samples, 32 taps, 7 slots with NaN slots and an all-NaN capture (the family's \"ragged\" case)",
          _subband_build, _raw_run("subband_power_batch_dev", _ARGS["subband_power"]), _subband_check, _nothing, _subband_cached),
    Entry("cw_check", "CW check", "gsmcal_cw_check_batch_dev", [], ["cw_part"],
          dict(_RAW_V, no_r="without d_r", wide="r_stride = N - 1 + 5: padding behind every row of r"), "refused", {},
          "2 captures x 4 099 samples: 4 098 ratios = two tiles of 2 048 and two ratios", _cw_build, _cw_run, _cw_check, _cw_margins,
          lambda case: {}),
    Entry("iq_imbalance", "I/Q check", "gsmcal_iq_imbalance_batch_dev", [], ["iq_part"], _RAW_V, "refused", {},
          "3 captures x 16 385 samples: one tile of 16 384 and one sample", _iq_build, _iq_run, _iq_check, _nothing, lambda case: {}),
    Entry("fcch_scan", "chain", "gsmcal_fcch_scan_batch_dev", ["h_coef"], ["coef", "csum_head", "lanes", "g_scan"], _RAW_V, "refused",
          {"h_coef": ("a", "a2")}, "3 captures x 620 000 samples (62 frames: a capture must hold 23 frames, and these calibrate)",
          _scan_build, _scan_run, _scan_check, _scan_margins, _host_cached(h_coef="coef")),
    Entry("calibrate", "chain", "gsmcal_calibrate_batch_dev", ["h_coef", "h_ts", "h_cf"], ["coef", "ts", "cf", "csum_head", "lanes", "g_calib"],
          {"r": "with r_correct: the 62-frame captures of dongles 0 and 3 and one of noise", "coef2": "other taps", "ts2": "another template",
           "cf2": "another carrier", "no_r": "without r_correct", "big": "72 frames", "small": "one stream"}, "refused",
          {"h_coef": ("r", "coef2"), "h_ts": ("r", "ts2"), "h_cf": ("r", "cf2")},
          "3 streams x 620 000 samples: the shortest capture that calibrates here, a stream that leaves at the first exit beside two that do not",
          _cal_build, _cal_run, _cal_check, _cal_margins, lambda case: {"h_coef": case.host["coef"], "h_ts": case.host["ts"],
                                                                        "h_cf": np.broadcast_to(np.float64(case.host["fc"]), (case.host["d"],))}),
    Entry("fcch_demod", "demod", "gsmcal_fcch_demod_batch_dev", ["h_fd_cf", "fd_tw_n"], ["fd_in", "fd_len", "fd_pos", "fd_tw", "fd_part", "fd_cf"],
          dict(_POST_VARIANTS, ov8b="the same sizes, other carrier frequencies"), "refused", {"h_fd_cf": ("ov8", "ov8b"), "fd_tw_n": ("ov8", "ov4")},
          "3 streams at 2x, 7 513 samples a row: three bursts in two streams beside one with r_len = -1", _fd_build, _fd_run, _fd_check,
          _fd_margins, lambda case: {"h_fd_cf": case.host["cf"], "fd_tw_n": np.array([148 * case.host["ov"]])}),
    Entry("bcch_demod", "demod", "gsmcal_bcch_demod_batch_dev", ["h_fd_cf", "fd_tw_n", "h_bc_ts"],
          ["fd_in", "fd_len", "fd_pos", "fd_tw", "fd_part", "fd_cf", "bc_corr", "bc_flag"],
          dict(_POST_VARIANTS, ov8b="the same sizes, other templates", ov8c="without corr and r_out"), "refused",
          {"h_bc_ts": ("ov8", "ov8b"), "fd_tw_n": ("ov8", "ov2")},
          "3 streams at 2x: six and six bursts (one stream's codes agree, the other's do not) beside one with r_len = -1", _bc_build, _bc_run,
          _bc_check, _bc_margins, lambda case: {"h_bc_ts": case.host["nts"], "h_fd_cf": case.host["cf"], "fd_tw_n": np.array([148 * case.host["ov"]])}),
    Entry("sch_decode", "demod", "gsmcal_sch_decode_batch_dev", [], ["fd_in", "fd_len", "fd_pos", "sd_part"], _POST_VARIANTS, "refused", {},
          "3 streams at 2x, three bursts each; the streams end with the last burst's symbol 144", _sd_build, _sd_run, _sd_check, _sd_margins,
          lambda case: {}),
    Entry("bcch_decode", "demod", "gsmcal_bcch_decode_batch_dev", ["h_bd_tsc"], ["fd_in", "fd_len", "fd_pos", "bd_tsc"],
          dict(_POST_VARIANTS, ov8b="the same sizes, another code for stream 0"), "refused", {"h_bd_tsc": ("ov8", "ov8b")},
          "3 streams at 2x, one block each (one decodes, one does not); the streams end at the last burst's symbol 144", _bd_build, _bd_run,
          _bd_check, _bd_margins, _host_cached(h_bd_tsc="tsc")),
    Entry("pair_coherence", "pair", "gsmcal_pair_coherence_batch_dev", ["h_pc_pairs"], ["fd_in", "fd_len", "fd_pos", "pc_pairs"],
          {"ov8": "the designed pair at 8x", "ov2": "at 2x", "ov4": "at 4x", "ov8b": "the same sizes, other pairs and lags"}, "refused",
          {"h_pc_pairs": ("ov8", "ov8b")}, "4 streams at 2x, two pairs (one names the stream with r_len = -1), three bursts, M = 3",
          _pc_build, _pc_run, _pc_check, _pc_margins, _pc_cached),
    Entry("pair_align", "pair", "gsmcal_pair_align_batch_dev", ["h_pa_members", "h_pa_params"], ["fd_in", "fd_len", "pa_members", "pa_params"],
          {"ov8": "aligned and combined at 8x", "ov2": "at 2x", "ov4": "at 4x", "ov8b": "the same sizes, other members and rows",
           "ov8c": "aligned only", "ov8d": "combined only"}, "refused", {"h_pa_members": ("ov8", "ov8b"), "h_pa_params": ("ov8", "ov8b")},
          "4 members of 4 streams at 2x, out_len 7 493: no multiple of the tile", _pa_build, _pa_run, _pa_check, _pa_margins,
          _host_cached(h_pa_members="members", h_pa_params="params")),
    Entry("array_covariance", "array", "gsmcal_array_covariance_batch_dev", ["h_ac_rows", "h_ac_win"], ["ac_rows", "ac_win", "ac_part"], _RAW_V,
          "refused", {"h_ac_rows": ("a", "a2"), "h_ac_win": ("a", "a2")},
          "4 rows of 6 streams (one named twice, two unnamed), 4 windows: empty, 64 at an odd start, chunk - 1 ending at stride, chunk + 1",
          _cov_build, _cov_run, _cov_check, _nothing, _host_cached(h_ac_rows="rows", h_ac_win="windows")),
    Entry("array_combine", "array", "gsmcal_array_combine_batch_dev", ["h_ac_rows", "h_ac_w"], ["ac_rows", "ac_w"],
          {"b1": "one beam", "b3": "three beams", "b16": "sixteen beams", "b3w": "three beams, other weights", "b3r": "three beams, other rows",
           "big": "16 beams of 5 rows over the whole stride", "small": "one sample"}, "refused", {"h_ac_rows": ("b3", "b3r"), "h_ac_w": ("b3", "b3w")},
          "4 rows of 6 streams, out_len 257 = a tile of 256 and one sample; B = 1, 3, 16: the three template instances", _comb_build, _comb_run,
          _comb_check, _nothing, _host_cached(h_ac_rows="rows", h_ac_w="weights")),
]
REGISTRY = {e.name: e for e in ENTRIES}

# exported gsmcal_*_dev symbols that are no entry: a name and the reason, nothing else
NOT_AN_ENTRY = {"gsmcal_synth_expand_dev": "a test tool (synthetic captures for benchmarks), no part of the reference's path"}
# caches of the context no _dev entry point can move, with the reason; tests/test_dev_contracts_cpu.py checks the reason against the code
HOST_ONLY_CACHES = {
    "tw_sch_n": ("gsmcal_SCH_equalise",), "h_iq_par": ("gsmcal_iq_correct",),
    "tw_n": ("ensure_twiddles",),             # keyed by Geom(ov).nfft; every _dev entry point runs at ov = 8, only the per-function host
}                                             # forms (gsmcal_FCCH_fine_correction, ...) ask for another length
# the buffers several families share, and the entries that meet on them
SHARED = {"fd_in": ("fcch_demod", "bcch_demod", "sch_decode", "bcch_decode", "pair_coherence", "pair_align"),
          "fd_tw": ("fcch_demod", "bcch_demod"), "ac_rows": ("array_covariance", "array_combine"), "coef": ("frontend", "fcch_scan", "calibrate")}


def all_keys(refused=True):
    return [(e.name, v) for e in ENTRIES for v in e.variants if refused or v != e.refused]


def case_of(key):
    return REGISTRY[key[0]].build(key[1])
