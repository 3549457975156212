"""Keeps tests/dev_contracts.py honest without a GPU: every exported gsmcal_*_dev symbol of include/gsmcal.h is an entry of the
registry (or on its short allow-list), every cache of the context -- the host vectors csrc/abi_calls.h hands to upload_if_changed /
upload_cached / upload_host_copy, and the lengths tw_n, tw_sch_n, fd_tw_n -- is named by an entry with two variants of the same
sizes that differ in it (a cache added later without such a pair turns this file red), every variant passes on its restatement the
margins its family's own tests demand before they compare, and the refused variants break the rule they say they break."""
import os
import re

import numpy as np
import pytest

import dev_contracts as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-rtl-sdr-calibration_amd", "csrc")
UPLOAD = re.compile(r"\bupload_(?:if_changed|cached|host_copy)\s*\(\s*c\s*,\s*c->\w+\s*,\s*c->(\w+)")
LENGTH = re.compile(r"\bc->(tw_n|tw_sch_n|fd_tw_n)\s*=[^=]")
FUNC = re.compile(r"^(?:static\s+|inline\s+)*(?:[\w:<>]+[\s\*&]+)+(\w+)\s*\([^;]*$")


def read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def exported_dev_symbols(header):
    return sorted(set(re.findall(r"\b(gsmcal_\w+_dev)\s*\(", header)))


def caches_in(text):
    """cache name -> the functions it is written in (the last definition at column 0 above the line)"""
    found, fn = {}, None
    for line in text.splitlines():
        m = FUNC.match(line)
        if m and not line.startswith((" ", "\t", "#", "//")):
            fn = m.group(1)
        for rx in (UPLOAD, LENGTH):
            for name in rx.findall(line):
                if "(gsmcal_ctx* c, DevBuf& b" not in line:
                    found.setdefault(name, set()).add(fn)
    return found


def context_caches():
    found = {}
    for name in ("host_plan.h", "abi_calls.h"):
        for k, v in caches_in(read(CSRC, name)).items():
            found.setdefault(k, set()).update(v)
    return found


def test_every_exported_dev_symbol_is_an_entry():
    syms = exported_dev_symbols(read(ROOT, "include", "gsmcal.h"))
    assert len(syms) == 16, syms
    entries = {e.symbol for e in dc.ENTRIES}
    assert len(entries) == len(dc.ENTRIES) == 15
    missing = [s for s in syms if s not in entries and s not in dc.NOT_AN_ENTRY]
    assert not missing, f"exported _dev symbols without an entry in tests/dev_contracts.py: {missing}"
    assert set(dc.NOT_AN_ENTRY) <= {"gsmcal_synth_expand_dev"} and all(len(r) > 10 for r in dc.NOT_AN_ENTRY.values())
    assert entries <= set(syms), entries - set(syms)
    import gsmcal
    assert all(s in gsmcal.SIGNATURES for s in entries)


def test_the_parser_finds_the_caches_the_issue_names():
    found = context_caches()
    for name in ("h_coef", "h_ts", "h_cf", "h_bp_coef", "h_fd_cf", "h_bc_ts", "h_sb_idx", "h_sb_rows", "h_iq_par", "h_bd_tsc", "h_pc_pairs",
                 "h_pa_members", "h_pa_params", "h_ac_rows", "h_ac_win", "h_ac_w", "tw_n", "tw_sch_n", "fd_tw_n"):
        assert name in found, (name, sorted(found))
    members = read(CSRC, "host_plan.h")
    for name in found:                                                      # ... and they are members of gsmcal_ctx
        assert re.search(r"\b%s\b" % name, members), name
    # a cache added to a copy of the source is found, and is then without a pair
    more = caches_in(read(CSRC, "abi_calls.h") + "\nint gsmcal_new_batch_dev(gsmcal_ctx* c) {\n"
                     '    RET_IF(upload_if_changed(c, c->nw_tab, c->h_nw_tab, tab, n, "new table"));\n}\n')
    assert more["h_nw_tab"] == {"gsmcal_new_batch_dev"} and uncovered(set(more)) == ["h_nw_tab"]


def uncovered(caches):
    named = {c for e in dc.ENTRIES for c in e.pairs}
    return sorted(c for c in caches if c not in named and c not in dc.HOST_ONLY_CACHES)


def test_every_cache_has_two_variants_that_differ_in_it():
    found = context_caches()
    assert uncovered(set(found)) == [], "caches of the context no entry of tests/dev_contracts.py covers with a colliding pair"
    # h_sb_coef and h_sb_w are compared by hand in gsmcal_subband_power_batch_dev (they key h_sb_rows): named by the entry all the same
    for e in dc.ENTRIES:
        assert set(e.pairs) <= set(e.caches), (e.name, e.pairs, e.caches)
        assert all(c in found or c in ("h_sb_coef", "h_sb_w") for c in e.caches), (e.name, e.caches)
        for cache, (va, vb) in e.pairs.items():
            a, b = e.build(va), e.build(vb)
            ca, cb = e.cached(a)[cache], e.cached(b)[cache]
            assert not np.array_equal(ca, cb), (e.name, cache, "the two variants hold the same content")
            if cache != "fd_tw_n":                                          # a content cache: the same size, or the size alone tells them apart
                assert np.shape(ca) == np.shape(cb), (e.name, cache, np.shape(ca), np.shape(cb))
                assert {k: i.data.shape for k, i in a.ins.items()} == {k: i.data.shape for k, i in b.ins.items()}, (e.name, cache)
    # what no _dev entry point can move: the only functions that write it are host-only forms no _dev function calls
    text = read(CSRC, "abi_calls.h") + read(CSRC, "host_plan.h")
    for cache, writers in dc.HOST_ONLY_CACHES.items():
        assert found[cache] == set(writers), (cache, found[cache])
    dev_bodies = "".join(re.findall(r"^int gsmcal_\w+_dev\(.*?^}", text, flags=re.S | re.M))
    assert "gsmcal_SCH_equalise(" not in dev_bodies and "gsmcal_iq_correct(" not in dev_bodies
    assert len(re.findall(r"ensure_twiddles\(c, g\.nfft\)", dev_bodies)) == 1 and "const int ov = 8" in dev_bodies      # calibrate: Geom(8) alone


def test_shared_buffers_are_members_and_their_entries_name_them():
    members = read(CSRC, "host_plan.h")
    for buf, names in dc.SHARED.items():
        assert re.search(r"\b%s\b" % buf, members), buf
        assert len(names) >= 2 and all(buf in dc.REGISTRY[n].shared for n in names), (buf, names)
    for e in dc.ENTRIES:
        assert len(e.good()) >= 2 and e.refused in e.variants and e.smallest, e.name


@pytest.mark.parametrize("key", dc.all_keys(refused=False), ids=lambda k: "-".join(k))
def test_margins_of_every_variant(key):
    """the family's own preconditions on the restatement: a case that fails one fails here, none is dropped"""
    e = dc.REGISTRY[key[0]]
    case = e.build(key[1])
    e.margins(case)
    for name, o in case.outs.items():
        assert not np.any(o.written & o.alone), (key, name)
    for name, i in case.ins.items():
        assert i.live.shape == i.data.shape, (key, name)


def test_the_variants_the_issue_lists_are_there():
    v = {e.name: set(e.variants) for e in dc.ENTRIES}
    assert {"no_r", "wide"} <= v["cw_check"] and {"r", "no_r"} <= v["calibrate"] and {"ov8", "ov8c"} <= v["bcch_demod"]
    assert {"ov8", "ov8c", "ov8d"} <= v["pair_align"] and {"b1", "b3", "b16"} <= v["array_combine"]
    for name in ("fcch_demod", "bcch_demod", "sch_decode", "bcch_decode", "pair_coherence", "pair_align"):
        assert {"ov8", "ov4", "ov2"} <= v[name], name
    assert dc.case_of(("cw_check", "wide")).host["r_stride"] > dc.case_of(("cw_check", "wide")).host["n"] - 1
    assert [dc.case_of(("array_combine", k)).host["weights"].shape[0] for k in ("b1", "b3", "b16")] == [1, 3, 16]
    assert {dc.case_of(("pair_align", k)).host["form"] for k in ("ov8", "ov8c", "ov8d")} == {"both", "aligned", "combined"}


@pytest.mark.parametrize("e", dc.ENTRIES, ids=lambda e: e.name)
def test_refused_variants_break_the_rule_they_name(e):
    """a CPU-side reading of the rule each refusal is taken from (include/gsmcal.h)"""
    import gsmcal
    case = e.build(e.refused)
    h = case.host
    assert case.refused in ("-1", "-5", "-6") and all(np.all(o.alone) and not np.any(o.written) for o in case.outs.values())
    good = e.build(e.good()[0]).host
    if e.name == "frontend":
        # fir_decim_raw stages 256*decim + ntaps raw samples of 4 bytes: "1 .. 281 for 47 taps"
        assert h["decim"] > 281 and len(h["coef"]) == 47 and good["decim"] <= 281
    elif e.name == "band_power":
        assert len(h["coef"]) > 1024 >= len(good["coef"])
    elif e.name == "subband_power":
        assert np.isinf(h["w"]).any() and not np.isinf(good["w"]).any()
    elif e.name == "cw_check":
        assert not h["thr"] > 0 and good["thr"] > 0
    elif e.name == "iq_imbalance":
        assert h["odd"] and not good["odd"]
    elif e.name == "fcch_scan":
        assert -(-h["n"] // 64) < int(np.ceil(23 * 1250 / 8)) <= -(-good["n"] // 64)
    elif e.name == "calibrate":
        assert len(h["coef"]) < 1 <= len(good["coef"])
    elif e.name == "fcch_demod":
        assert h["ov_arg"] >= 34 > good["ov_arg"]
    elif e.name == "bcch_demod":
        assert h["short_ts"] and not good["short_ts"] and len(h["nts"]) == 26 * h["ov"]
    elif e.name == "sch_decode":
        assert len(h["ts"]) != 64 * h["ov"] and len(good["ts"]) == 64 * good["ov"]
    elif e.name == "bcch_decode":
        assert not np.all((h["tsc"] >= 0) & (h["tsc"] <= 7)) and np.all((good["tsc"] >= 0) & (good["tsc"] <= 7))
    elif e.name == "pair_coherence":
        assert h["pairs"].max() >= h["d"] and good["pairs"].max() < good["d"] and good["pairs"].min() >= 0
    elif e.name == "pair_align":
        assert np.abs(h["params"][:, 1]).max() > 1000 >= np.abs(good["params"][:, 1]).max()
    elif e.name == "array_covariance":
        assert (h["windows"].sum(axis=1) > h["stride"]).any() and not (good["windows"].sum(axis=1) > good["stride"]).any()
    elif e.name == "array_combine":
        assert h["out_len"] > h["stride"] >= good["out_len"] and h["weights"].shape[0] <= gsmcal.MAX_BEAMS
    else:
        raise AssertionError(f"no reading of the rule for {e.name}")


def test_patterns_and_poison():
    p = dc.pattern((3, 2), np.complex128)
    assert p.dtype == np.complex128 and not np.isnan(p.view(np.float64)).any() and np.all(p.view(np.uint64) == 0xC0DEC0DEC0DEC0DE)
    assert np.all(dc.pattern((5,), np.uint8) == 0xA5) and np.all(dc.pattern((2,), np.int32).view(np.uint32) == 0xC0DEC0DE)
    assert np.all(dc.pattern_bytes(16).view(np.uint64) == 0xC0DEC0DEC0DEC0DE) and len(dc.pattern_bytes(13)) == 13
    nan = np.array([dc.NAN_PAYLOAD], dtype=np.uint64).view(np.float64)
    assert np.isnan(nan[0]) and dc.same_bits(nan, nan.copy()) and not dc.same_bits(nan, np.array([np.nan]))
