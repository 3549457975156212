#!/usr/bin/env python3
"""Multi-channel band scanner sweeps on one GPU (gsmcal_subband_power_batch_dev) -> profiles/subband_bench.json and one JSON line.

Workloads (multi_rtl_sdr_diversity_scanner_another_bak.m's plan, 2.048 MS/s, observe_time 0.2 s = 409 600 samples per capture,
4 dongles): GSM-900 935-960 MHz at 100 kHz (50 captures per dongle = 200 captures, 32 taps, 251 points per dongle, up to 6 per
capture) at decimation 1 (the script) and 10, and the same sweep at 50 kHz (64 taps, 501 points, up to 11 per capture).  For the
same grids the finished scanners' way: gsmcal_band_power_batch_dev with one capture per point (1004 / 2004 captures) at the
scanners' own decimation and at decimation 1.  And the yardstick of DESIGN.md 10, row "1 MHz 32/1" (2004 x 204 800 samples,
k_band_power<32> at decimation 1), measured again in the same session.

Per workload: ms per sweep from device events after warm-up (median and min-max over --repeats timed loops of --steps sweeps),
and the time per (sample x tap x sub-band) -- per (sample x tap) for the band-power rows.  Input: seeded random bytes in distinct
device buffers that together exceed 512 MB, rotated call by call, so no sweep starts with its bytes in the 256 MiB Infinity Cache.

    python tools/subband_bench.py [--steps 10] [--warmup 3] [--repeats 5] [--only sub100k_d1,...] [--no-check] [--out profiles/subband_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS, OBS, DONGLES = 2.048e6, 0.2, 4
START, STOP = 935e6, 960e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-check", action="store_true", help="skip the comparison of one capture with the restatements")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subband_bench.json"))
    args = ap.parse_args()

    import torch
    import gsmcal
    import gsmcal.dist
    import subband_ref as ref

    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    ctx = gsmcal.Context(0, stream=stream.cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261018)

    def timed(fn):
        for i in range(args.warmup):
            fn(i)
        torch.cuda.synchronize()
        ms = []
        for r in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for i in range(args.steps):
                fn(args.warmup + r * args.steps + i)
            e1.record(stream)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.steps)
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    def buffers(d, n):
        nbytes = d * 2 * n
        nbuf = max(2, -(-512_000_000 // nbytes) + 1)
        return [torch.randint(0, 256, (d, 2 * n), dtype=torch.uint8, device=dev, generator=gen) for _ in range(nbuf)], nbytes

    rec = {"tool": "subband_bench", "gpu": torch.cuda.get_device_name(0), "lib": os.path.relpath(gsmcal.lib_path(), ROOT),
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "dongles": DONGLES,
           "cache": "seeded random bytes, distinct buffers rotated per call, > 512 MB in rotation", "workloads": {}}
    only = set(args.only.split(",")) if args.only else None

    def want(name):
        return only is None or name in only

    for step, tag in ((100e3, "100k"), (50e3, "50k")):
        _, coef, sdecim, n = gsmcal.dist.spectrum_filter(FS, step, OBS)
        plan = gsmcal.dist.multichannel_frequency_plan(START, STOP, step, FS)
        ncap, nsub = len(plan["real_freq"]), max(len(k) for k in plan["freq_set"])
        w1 = np.full((ncap, nsub), np.nan)
        for c, rel in enumerate(plan["relative_sub_freq_set"]):
            w1[c, :len(rel)] = -rel * 2 * np.pi / FS
        w = np.tile(w1, (DONGLES, 1))
        d = DONGLES * ncap
        units = int(np.sum(~np.isnan(w)))
        for decim in (1, 10):
            name = "sub%s_d%d" % (tag, decim)
            if not want(name) or (tag == "50k" and decim != 1):
                continue
            bufs, nbytes = buffers(d, n)
            out = torch.empty((d, nsub), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()

            def sweep(i):
                gsmcal.subband_power_batch_dev(bufs[i % len(bufs)].data_ptr(), d, n, coef, w, out.data_ptr(), decim=decim, ctx=ctx)

            med, lo, hi = timed(sweep)
            sweep(0)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            a = bufs[0][d // 3].cpu().numpy()
            dev_lit = dev_ex = 0.0
            for j in range(nsub):
                if not args.no_check and not np.isnan(w[d // 3, j]):
                    lit, ex = ref.literal(a, coef, w[d // 3, j], decim), ref.exact(a, coef, w[d // 3, j], decim)
                    dev_lit = max(dev_lit, abs(got[d // 3, j] - lit) / lit)
                    dev_ex = max(dev_ex, abs(got[d // 3, j] - ex) / ex)
            nd = -(-n // decim)
            work = float(units) * nd * len(coef)
            rec["workloads"][name] = {
                "captures": d, "samples": n, "ntaps": len(coef), "decim": decim, "slots": nsub, "points": units,
                "distinct_phases": int(len(np.unique(w[~np.isnan(w)]))), "ms_per_sweep": round(med, 4), "ms_min": round(lo, 4),
                "ms_max": round(hi, 4), "raw_bytes": nbytes, "sample_tap_subband": work,
                "ps_per_sample_tap_subband": round(med * 1e-3 / work * 1e12, 5),
                "max_rel_dev_from_literal_checked": None if args.no_check else dev_lit,
                "max_rel_dev_from_exact_checked": None if args.no_check else dev_ex}
            del bufs, out
            torch.cuda.empty_cache()
        # the finished scanners' way: one capture per grid point
        dp = DONGLES * len(plan["freq"])
        for decim in (sdecim, 1):
            name = "bandpower%s_d%d" % (tag, decim)
            if not want(name):
                continue
            bufs, nbytes = buffers(dp, n)
            out = torch.empty(dp, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()

            def bsweep(i):
                gsmcal.band_power_batch_dev(bufs[i % len(bufs)].data_ptr(), dp, n, coef, decim, out.data_ptr(), ctx=ctx)

            med, lo, hi = timed(bsweep)
            work = float(dp) * (-(-n // decim)) * len(coef)
            rec["workloads"][name] = {"captures": dp, "samples": n, "ntaps": len(coef), "decim": decim, "ms_per_sweep": round(med, 4),
                                      "ms_min": round(lo, 4), "ms_max": round(hi, 4), "raw_bytes": nbytes,
                                      "ps_per_sample_tap": round(med * 1e-3 / work * 1e12, 5)}
            del bufs, out
            torch.cuda.empty_cache()
    if want("yardstick_32_1"):
        _, coef, decim, _ = gsmcal.dist.spectrum_filter(FS, 1e6, 0.1)
        d, n = 2004, 204800
        bufs, nbytes = buffers(d, n)
        out = torch.empty(d, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def ysweep(i):
            gsmcal.band_power_batch_dev(bufs[i % len(bufs)].data_ptr(), d, n, coef, decim, out.data_ptr(), ctx=ctx)

        med, lo, hi = timed(ysweep)
        work = float(d) * n * len(coef)
        rec["workloads"]["yardstick_32_1"] = {"captures": d, "samples": n, "ntaps": len(coef), "decim": decim, "ms_per_sweep": round(med, 4),
                                              "ms_min": round(lo, 4), "ms_max": round(hi, 4), "raw_bytes": nbytes,
                                              "ps_per_sample_tap": round(med * 1e-3 / work * 1e12, 5),
                                              "design_10_row_ms": 2.895, "design_10_row_ps_per_sample_tap": round(2.895e-3 / work * 1e12, 5)}
        y = rec["workloads"]["yardstick_32_1"]["ps_per_sample_tap"]
        for k, v in rec["workloads"].items():
            if "ps_per_sample_tap_subband" in v:
                v["ratio_to_yardstick"] = round(v["ps_per_sample_tap_subband"] / y, 3)
    line = json.dumps(rec)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
