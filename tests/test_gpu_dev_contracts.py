"""GPU tests (-m gpu) of what include/gsmcal.h promises for every device entry point, uniformly and across families, driven by the
registry of tests/dev_contracts.py:

  a. anchor      every variant once on a fresh context, held to its family's fp64 restatement under the family's own bound (the
                 compare functions of the family's test module; no tolerance is stated in this file).  Every later comparison is
                 bit for bit against these anchored outputs, NaN payloads included.
  b. reads       every input inside a larger allocation, everything the header does not call an input poisoned (a NaN with a
                 payload for doubles; 0x00 and 0xFF in two runs for bytes): the outputs are the anchor's bits.
  c. writes      every output in a slot of its own between guard bands of 4 KiB, slot and bands prefilled with a fixed pattern: the
                 bands keep it, what the header says is written differs from it, what it says is left alone keeps it -- on a
                 refused call everything.
  d. history     one context on a torch stream, no synchronisation between calls, one at the end: A, A', A per cache; grow, shrink,
                 grow per shared buffer, alternating the families that share it; refused calls between good ones; calibrate and the
                 follow-ups on its outputs, one and three deep; set_params and back; graph replay through more keys than slots;
                 and a seeded schedule of 150 calls over all variants.
  e. contexts    the schedule split over two contexts on two torch streams, call by call.

Every GPU run here places its buffers the same way (guard bands, pattern prefill), so b, d and e check the bands and the elements
left alone as well."""
import numpy as np
import pytest

import dev_contracts as dc

pytestmark = pytest.mark.gpu

BAND = dc.BAND
RAW_ENTRIES = ("frontend", "band_power", "subband_power", "cw_check", "iq_imbalance", "fcch_scan", "calibrate")
FOLLOW_UPS = ("fcch_demod", "bcch_demod", "sch_decode", "bcch_decode")
FD_FAMILIES = dc.SHARED["fd_in"]
ADD_ONS = (("band_power", "a"), ("cw_check", "a"), ("fcch_demod", "ov8"), ("sch_decode", "ov2"), ("array_covariance", "a"),
           ("pair_align", "ov2"), ("iq_imbalance", "a"), ("subband_power", "small"))      # the families that take no thresholds
_ANCHORS = {}


@pytest.fixture(scope="module")
def g(gsmcal_mod):
    return gsmcal_mod


@pytest.fixture(scope="module", autouse=True)
def calibrated(g):
    """the r, r_len, pos_info triple of the follow-up families' calibrated variants: ONE calibrate_batch call on a context of its own"""
    raw = dc.case_of(("calibrate", "r"))
    own = g.Context(0)
    try:
        out = g.calibrate_batch(raw.ins["raw"].data, raw.host["coef"], raw.host["ts"], raw.host["fc"], want_r=True, ctx=own)
    finally:
        own.close()
    dc.use_calibrated(out["r_correct"], out["r_len"], out["pos_info_raw"])
    yield out
    dc.use_calibrated()


# ---- placement: inputs and outputs inside larger allocations ---------------------------------------------------------------------
def _poison_bytes(dtype, nbytes, byte):
    if dc.base_dtype(dtype).kind == "f":
        return np.tile(np.array([dc.NAN_PAYLOAD], dtype=np.uint64).view(np.uint8), (nbytes + 7) // 8)[:nbytes]
    return np.full(nbytes, byte, dtype=np.uint8)


def place_input(inp, poison=None):
    """-> (tensor, address of the data): [band][data][band]; with `poison` (a byte value) the bands and every element that is not
    live hold the poison"""
    import torch
    data = inp.data
    if poison is not None and not inp.live.all():
        data = data.copy()
        flat = data.view(np.uint8).reshape(data.shape + (data.dtype.itemsize,))
        bad = _poison_bytes(data.dtype, data.dtype.itemsize, poison)
        flat[~inp.live] = bad
    band = np.zeros(BAND, dtype=np.uint8) if poison is None else _poison_bytes(data.dtype, BAND, poison)
    host = np.concatenate([band, dc.bits(data), band])
    t = torch.from_numpy(host).to("cuda:0")
    return t, t.data_ptr() + BAND


def place_output(out):
    """-> (tensor, address): [band][slot][band], all of it holding the prefill pattern"""
    import torch
    body = dc.bits(dc.pattern(out.shape, out.dtype))
    host = np.concatenate([dc.pattern_bytes(BAND), body, dc.pattern_bytes(BAND)])
    t = torch.from_numpy(host).to("cuda:0")
    return t, t.data_ptr() + BAND


class Call:
    """one call of a schedule: its case, the addresses it runs on and the slots of its outputs"""

    def __init__(self, case, ins, outs=None):
        self.case, self.ins = case, ins
        self.slots = {name: place_output(o) for name, o in case.outs.items()} if outs is None else outs

    def ptr(self):
        p = {name: a for name, (_, a) in self.ins.items()}
        p.update({name: a for name, (_, a) in self.slots.items()})
        return p

    def run(self, g, ctx):
        e = dc.REGISTRY[self.case.entry]
        if self.case.refused is None:
            e.run(g, ctx, self.case, self.ptr())
        else:
            with pytest.raises(g.GsmcalError, match=f"failed with {self.case.refused} "):
                e.run(g, ctx, self.case, self.ptr())

    def read(self):
        """-> ({name: array}, [complaints about the guard bands])"""
        outs, bad = {}, []
        for name, o in self.case.outs.items():
            raw = self.slots[name][0].cpu().numpy()
            n = int(np.prod(o.shape, dtype=np.int64)) * o.dtype.itemsize
            for side, band in (("in front of", raw[:BAND]), ("behind", raw[BAND + n:])):
                if not np.array_equal(band, dc.pattern_bytes(BAND)):
                    bad.append(f"{self.case.key} {name}: {int(np.sum(band != dc.pattern_bytes(BAND)))} bytes of the guard band {side} the slot were written")
            outs[name] = raw[BAND:BAND + n].view(o.dtype).reshape(o.shape).copy()
        return outs, bad


def upload(case, poison=None):
    return {name: place_input(i, poison) for name, i in case.ins.items()}


def differs(a, b):
    """elementwise: do the bits of a and b differ?"""
    size = a.dtype.itemsize
    return np.any(dc.bits(a).reshape(a.shape + (size,)) != dc.bits(b).reshape(b.shape + (size,)), axis=-1)


def complaints(case, outs, anchor=None):
    """what a call's outputs break of the contract: elements left alone that changed, elements written that still hold the
    pattern (without an anchor) or differ from the anchor's bits (with one)"""
    bad = []
    for name, o in case.outs.items():
        pat = dc.pattern(o.shape, o.dtype)
        moved = differs(outs[name], pat)
        if np.any(moved & o.alone):
            bad.append(f"{case.key} {name}: {int(np.sum(moved & o.alone))} elements the header says are left alone were written, first at "
                       f"{tuple(int(v[0]) for v in np.nonzero(moved & o.alone))}")
        if anchor is None:
            if np.any(~moved & o.written):
                bad.append(f"{case.key} {name}: {int(np.sum(~moved & o.written))} elements the header says are written hold the prefill, first at "
                           f"{tuple(int(v[0]) for v in np.nonzero(~moved & o.written))}")
        else:
            off = differs(outs[name], anchor[name]) & o.written
            if np.any(off):
                at = tuple(int(v[0]) for v in np.nonzero(off))
                bad.append(f"{case.key} {name}: {int(np.sum(off))} of {int(np.sum(o.written))} written elements differ from the anchor's bits, first at {at}: "
                           f"{outs[name][at]!r} for {anchor[name][at]!r}")
    return bad


def fresh_context(g, **kw):
    import torch
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    return g.Context(0, stream=st.cuda_stream, **kw), st


def anchor(g, key):
    """the outputs of one variant on a fresh context (made once): {"outs", "bands", "det"}"""
    import torch
    if key not in _ANCHORS:
        case = dc.case_of(key)
        call = Call(case, upload(case))
        torch.cuda.synchronize()
        ctx = g.Context(0)
        try:
            call.run(g, ctx)
            ctx.sync()
            det = g.last_batch_details(case.host["d"], ctx=ctx) if case.entry == "calibrate" and case.refused is None else None
        finally:
            ctx.close()
        outs, bands = call.read()
        _ANCHORS[key] = {"outs": outs, "bands": bands, "det": det}
    return _ANCHORS[key]


def play(g, ctx, steps, uploads=None):
    """steps: keys, cases or callables, enqueued one behind the other with no synchronisation; one at the end.  -> complaints.
    Every call writes into slots of its own; inputs are uploaded once per case before the first call."""
    import torch
    uploads = {} if uploads is None else uploads
    calls = []
    for s in steps:
        if callable(s):
            calls.append(s)
            continue
        case = dc.case_of(s) if isinstance(s, tuple) else s
        if case.key not in uploads:
            uploads[case.key] = upload(case)
        calls.append(Call(case, uploads[case.key]))
    torch.cuda.synchronize()
    for c in calls:
        if callable(c):
            c()
        else:
            c.run(g, ctx)
    ctx.sync()
    return collect(g, calls)


def collect(g, calls, anchors=None):
    bad = []
    for k, c in enumerate(calls):
        if callable(c):
            continue
        outs, bands = c.read()
        ref = (anchors or {}).get(c.case.key) or anchor(g, c.case.key)["outs"]
        bad += [f"call {k}: {m}" for m in bands + complaints(c.case, outs, ref)]
    return bad


def on_stream(g, steps, env=None, depth=1, monkeypatch=None):
    import torch
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)                      # (read when a context is created, as tests/test_gpu_params.py sets them)
    ctx, st = fresh_context(g)
    try:
        with torch.cuda.stream(st):
            if depth > 1:
                ctx.set_pipeline_depth(depth)
            return play(g, ctx, steps)
    finally:
        ctx.close()


def report(bad, steps):
    names = [s if isinstance(s, tuple) else getattr(s, "key", getattr(s, "__name__", "?")) for s in steps]
    assert not bad, "\n".join(bad[:40]) + f"\n({len(bad)} complaints) schedule: {names}"


# ---- a. anchor ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", dc.all_keys(), ids=lambda k: "-".join(k))
def test_a_anchor_against_the_restatement(g, key):
    case = dc.case_of(key)
    a = anchor(g, key)
    if case.refused is None:
        extra = {"det": a["det"], "anchor": lambda k: anchor(g, k)["outs"]}
        dc.REGISTRY[key[0]].check(case, a["outs"], g, extra)


def test_a_the_calibrated_triple_is_what_the_device_form_returns(g, calibrated):
    a = anchor(g, ("calibrate", "r"))["outs"]
    rl = calibrated["r_len"]
    assert np.array_equal(a["r_len"], rl) and dc.same_bits(a["pos_info"], calibrated["pos_info_raw"]) and dc.same_bits(a["table"], calibrated["table"])
    for i, n in enumerate(rl):
        assert n < 0 or dc.same_bits(a["r_correct"][i, :n], calibrated["r_correct"][i, :n]), i


# ---- c. writes (on the anchor's own run: its slots are placed like every other run's) ------------------------------------------
@pytest.mark.parametrize("key", dc.all_keys(), ids=lambda k: "-".join(k))
def test_c_writes_stay_inside_the_declared_extent(g, key):
    case = dc.case_of(key)
    a = anchor(g, key)
    bad = a["bands"] + complaints(case, a["outs"])
    assert not bad, "\n".join(bad)
    if case.refused is not None:
        assert all(not differs(a["outs"][n], dc.pattern(o.shape, o.dtype)).any() for n, o in case.outs.items())


# ---- b. reads -------------------------------------------------------------------------------------------------------------------
def _poisons(key):
    return (0x00, 0xFF) if key[0] in RAW_ENTRIES else (0xFF,)


@pytest.mark.parametrize("key", dc.all_keys(refused=False), ids=lambda k: "-".join(k))
def test_b_reads_stay_inside_the_declared_extent(g, key):
    import torch
    case = dc.case_of(key)
    for poison in _poisons(key):
        call = Call(case, upload(case, poison))
        torch.cuda.synchronize()
        ctx = g.Context(0)
        try:
            call.run(g, ctx)
            ctx.sync()
        finally:
            ctx.close()
        outs, bands = call.read()
        bad = bands + complaints(case, outs, anchor(g, key)["outs"])
        assert not bad, f"surroundings at {poison:#04x} / NaN:\n" + "\n".join(bad)


def run_hurt(g, key, name, at):
    """the variant with one LIVE sample of input `name` replaced by the NaN poison -> (case, outputs)"""
    import torch
    case = dc.case_of(key)
    inp = case.ins[name]
    assert inp.live[at]
    hurt = inp.data.copy()
    hurt[at] = np.array([dc.NAN_PAYLOAD], dtype=np.uint64).view(np.float64)[0]
    ins = upload(case)
    ins[name] = place_input(dc.In(hurt, inp.live))
    call = Call(case, ins)
    torch.cuda.synchronize()
    ctx = g.Context(0)
    try:
        call.run(g, ctx)
        ctx.sync()
    finally:
        ctx.close()
    outs, bands = call.read()
    assert not bands, bands
    return case, outs


def test_b_the_poison_bites(g):
    """the same placement with a LIVE sample poisoned, in the two families whose contract is that NaN propagates ("nothing is
    screened"): the NaN arrives in the outputs, so a read behind the declared extent would show there as well"""
    for key, where in ((("array_combine", "b3"), lambda c: (int(c.host["rows"][0]), 5)),
                       (("array_covariance", "a"), lambda c: (int(c.host["rows"][1]), 40))):
        case, outs = run_hurt(g, key, "x", where(dc.case_of(key)))
        assert complaints(case, outs, anchor(g, key)["outs"]), key


# ---- d. call history ------------------------------------------------------------------------------------------------------------
CACHE_PAIRS = [(e.name, cache) for e in dc.ENTRIES for cache in e.pairs]


@pytest.mark.parametrize("name,cache", CACHE_PAIRS, ids=lambda v: v)
def test_d_cache_a_other_a(g, name, cache):
    """A, A', A: the same sizes with other contents in one cache, then back"""
    a, b = dc.REGISTRY[name].pairs[cache]
    ca, oa, ob = dc.case_of((name, a)), anchor(g, (name, a))["outs"], anchor(g, (name, b))["outs"]
    assert any(np.any(differs(oa[k], ob[k]) & o.written) for k, o in ca.outs.items() if k in ob and oa[k].shape == ob[k].shape), \
        "the two variants give the same bits: a stale cache would not show"
    steps = [(name, a), (name, b), (name, a), (name, b)]
    report(on_stream(g, steps), steps)


def fd_round_robin():
    return [(fam, f"ov{ov}") for ov in (8, 2, 4, 8) for fam in FD_FAMILIES]


def test_d_six_families_on_the_fd_buffers(g):
    """fd_in / fd_len / fd_pos (the host forms' staging) and fd_tw, fd_part, fd_cf: all six families at 8x, 2x, 4x, 8x"""
    steps = fd_round_robin()
    report(on_stream(g, steps), steps)


def test_d_twiddles_shared_by_every_oversampling_ratio(g):
    steps = [("fcch_demod", "ov8"), ("bcch_demod", "ov2"), ("fcch_demod", "ov4"), ("bcch_demod", "ov8"), ("fcch_demod", "ov2"),
             ("bcch_demod", "ov4"), ("bcch_demod", "cal8"), ("fcch_demod", "cal4"), ("fcch_demod", "ov8b"), ("bcch_demod", "ov8")]
    report(on_stream(g, steps), steps)


def test_d_combine_instances_and_covariance_on_ac_rows(g):
    steps = [("array_combine", "b1"), ("array_covariance", "a"), ("array_combine", "b3"), ("array_covariance", "big"),
             ("array_combine", "b16"), ("array_covariance", "small"), ("array_combine", "big"), ("array_covariance", "a2"),
             ("array_combine", "b3r"), ("array_covariance", "a"), ("array_combine", "small"), ("array_combine", "b3w"), ("array_combine", "b3")]
    report(on_stream(g, steps), steps)


def test_d_taps_shared_by_front_end_scanner_and_chain(g):
    """h_coef / coef / csum_head: the front end with the chain's own taps and with others, the scanner's 31 taps, between calibrate calls"""
    steps = [("calibrate", "r"), ("frontend", "a2"), ("calibrate", "r"), ("fcch_scan", "a"), ("frontend", "a"), ("calibrate", "coef2"),
             ("fcch_scan", "a2"), ("calibrate", "no_r"), ("frontend", "big"), ("fcch_scan", "a"), ("calibrate", "r")]
    report(on_stream(g, steps), steps)


@pytest.mark.parametrize("e", dc.ENTRIES, ids=lambda e: e.name)
def test_d_grow_shrink_grow(g, e):
    big = "big" if "big" in e.variants else ("cal8" if "cal8" in e.variants else "ov8")
    small = "small" if "small" in e.variants else "ov2"
    steps = [(e.name, big), (e.name, small), (e.name, big), (e.name, e.good()[0]), (e.name, small)]
    report(on_stream(g, steps), steps)


@pytest.mark.parametrize("e", dc.ENTRIES, ids=lambda e: e.name)
def test_d_refused_calls_between_good_ones(g, e):
    """the refusal raises, writes nothing, and the next good call still matches"""
    good = e.good()
    steps = [(e.name, good[0]), (e.name, e.refused), (e.name, good[1]), (e.name, e.refused), (e.name, good[0])]
    report(on_stream(g, steps), steps)


def followups_on(g, tag, cal_call, anchors):
    """the follow-up families reading the output slots of a calibrate call; their anchors: the same inputs brought back to the
    host, run on a fresh context and held to the restatement"""
    calls = []
    for name in FOLLOW_UPS:
        a = anchors[tag]
        case = dc.followup_case(name, f"{tag}-cal8", a["r_correct"], a["r_len"], a["pos_info"])
        ins = {"r": cal_call.slots["r_correct"], "r_len": cal_call.slots["r_len"], "pos_info": cal_call.slots["pos_info"]}
        calls.append(Call(case, ins))
    return calls


@pytest.fixture(scope="module")
def followup_anchors(g):
    """(entry, tag) -> anchored outputs of the follow-ups on what calibrate r and calibrate coef2 return"""
    import torch
    cal = {tag: anchor(g, ("calibrate", tag))["outs"] for tag in ("r", "coef2")}
    out = {}
    for tag, a in cal.items():
        for name in FOLLOW_UPS:
            case = dc.followup_case(name, f"{tag}-cal8", a["r_correct"], a["r_len"], a["pos_info"])
            call = Call(case, upload(case))
            torch.cuda.synchronize()
            ctx = g.Context(0)
            try:
                call.run(g, ctx)
                ctx.sync()
            finally:
                ctx.close()
            outs, bands = call.read()
            assert not bands + complaints(case, outs), (name, tag)
            dc.REGISTRY[name].check(case, outs, g, None)
            out[case.key] = outs
    return cal, out


@pytest.mark.parametrize("depth", [1, 3])
def test_d_calibrate_then_the_follow_ups_on_its_outputs(g, followup_anchors, depth):
    """calibrate (with r_correct) -> each follow-up on its outputs -> calibrate with other taps -> the follow-ups again; at depth 3
    both calibrate calls are in flight before the first follow-up"""
    import torch
    cal, anchors = followup_anchors
    ctx, st = fresh_context(g)
    try:
        with torch.cuda.stream(st):
            ctx.set_pipeline_depth(depth)
            c1, c2 = (Call(dc.case_of(("calibrate", t)), upload(dc.case_of(("calibrate", t)))) for t in ("r", "coef2"))
            f1, f2 = followups_on(g, "r", c1, cal), followups_on(g, "coef2", c2, cal)
            order = [c1, c2] + f1 + f2 if depth > 1 else [c1] + f1 + [c2] + f2
            order = order + [c1] + f2[::-1]                  # ... and once more into the same buffers, the follow-ups the other way round
            torch.cuda.synchronize()
            for c in order:
                c.run(g, ctx)
            ctx.sync()
        bad = collect(g, order, anchors)
    finally:
        ctx.close()
    assert not bad, "\n".join(bad[:40])


def test_d_set_params_and_back_with_add_on_calls_between(g):
    import torch
    ctx, st = fresh_context(g)
    add_ons = list(ADD_ONS)

    def other():
        ctx.set_params(fine_max_ppm=4110.0, sch_max_ppm=390.0, coarse_th_db=9.0, scan_tol=40.0)     # (tests/test_gpu_params.py STALE_PARAMS)

    def back():
        ctx.set_params(fine_max_ppm=4000.0, sch_max_ppm=400.0, coarse_th_db=10.0, scan_tol=50.0)

    steps = [("calibrate", "r"), ("fcch_scan", "a"), other] + add_ons + [back] + add_ons[::-1] + [("calibrate", "r"), ("fcch_scan", "a")]
    try:
        with torch.cuda.stream(st):
            bad = play(g, ctx, steps)
    finally:
        ctx.close()
    report(bad, steps)


def test_d_graph_replay_through_more_keys_than_slots(g, monkeypatch):
    """GSMCAL_GRAPH=2: a key comes three times (eager, capture and replay, replay); five distinct keys pass through the slots; then
    the first key again -- the same buffers -- with an add-on call that grows one of its own buffers in between"""
    import torch
    monkeypatch.setenv("GSMCAL_GRAPH", "2")
    ctx, st = fresh_context(g)
    try:
        with torch.cuda.stream(st):
            keys = [("calibrate", t) for t in ("r", "coef2", "ts2", "cf2", "no_r")]
            firsts = {k: Call(dc.case_of(k), upload(dc.case_of(k))) for k in keys}
            order = []
            for k in keys:
                order += [firsts[k]] * 3
            small, big = (Call(dc.case_of(("band_power", v)), upload(dc.case_of(("band_power", v)))) for v in ("small", "big"))
            order += [small, firsts[keys[0]], big, firsts[keys[0]], firsts[keys[1]], firsts[keys[0]]]
            torch.cuda.synchronize()
            for c in order:
                c.run(g, ctx)
            ctx.sync()
        bad = collect(g, order)
    finally:
        ctx.close()
    assert not bad, "\n".join(bad[:40])


SEED = 20261021
HEAVY = {("cw_check", "big"): 0.25, ("calibrate", "big"): 0.25, ("fcch_scan", "big"): 0.25}


def schedule(seed=SEED, calls=150):
    rng = np.random.Generator(np.random.Philox(key=[seed, 150]))
    keys = dc.all_keys()
    w = np.array([HEAVY.get(k, 1.0) for k in keys])
    return [keys[i] for i in rng.choice(len(keys), size=calls, p=w / w.sum())]


def test_d_seeded_schedule_over_all_variants(g):
    steps = schedule()
    assert len({k for k in steps}) >= 60 and sum(dc.case_of(k).refused is not None for k in steps) >= 8
    bad = on_stream(g, steps)
    assert not bad, "\n".join(bad[:40]) + f"\nseed {SEED}; the schedule, call by call (a failing call's predecessors are the diagnosis):\n" + \
        "\n".join(f"{i}: {k}" for i, k in enumerate(steps))


# ---- e. two contexts ------------------------------------------------------------------------------------------------------------
def test_e_two_contexts_interleaved_call_by_call(g):
    """the schedule dealt to two contexts on two torch streams from one host thread: nothing lives in a static they share"""
    import torch
    steps = schedule(SEED + 1, 120)
    pair = [fresh_context(g), fresh_context(g)]
    try:
        uploads, calls = {}, []
        for k in steps:
            case = dc.case_of(k)
            if k not in uploads:
                uploads[k] = upload(case)
            calls.append(Call(case, uploads[k]))
        torch.cuda.synchronize()
        for i, c in enumerate(calls):
            ctx, st = pair[i & 1]
            with torch.cuda.stream(st):
                c.run(g, ctx)
        for ctx, _ in pair:
            ctx.sync()
        bad = collect(g, calls)
    finally:
        for ctx, _ in pair:
            ctx.close()
    assert not bad, "\n".join(bad[:40]) + f"\nseed {SEED + 1}; the schedule (even calls: context 0, odd: context 1):\n" + \
        "\n".join(f"{i}: {k}" for i, k in enumerate(steps))
