#!/usr/bin/env python3
"""row_coherence on device-resident apply_calibration rows (gsmcal_row_coherence_batch_resident) -> one JSON line, and
profiles/row_coherence_bench.json.

Workload: 64 rows of 1 020 000 samples written by apply_calibration_resident from synth.make_wideband captures of ONE transmission.
Evaluating 96 tones exactly at 64 x 1 020 000 sample times costs minutes of host time, so `--distinct` (default 8) dongles are
generated, each with its own clock error, carrier error, start and noise, and row i is capture i mod distinct corrected with a
delay and a phase of its own: every row differs from every other, and what the kernels do does not depend on the content.  W = 64
windows of 4 096 samples, M = 16; two pair lists: the 63 pairs against row 0, and all 4 032 ordered pairs.
The yardstick is pair_coherence_batch_dev on tools/pair_coherence_bench.py's inputs -- 64 calibrated GSM streams, 63
pairs, ov 8, M 16 --, timed before and after in the same process, the lower median counts.  Device events, warm-up calls, then
`repeats` timings of `calls` back-to-back calls each.  Recorded per call: fp64 FMAs over the evaluated work, (2M+1) 4Ls 6 + 2 4Ls per
evaluated (pair, window) (4 for c and 2 for Eb per lag and sample, 2 for Ea), per second and as a fraction of the vector fp64 rate;
the condition of DESIGN 24 is that the rate at 63 pairs is not below the yardstick's rate (same count per evaluated burst, L = 148 ov).

    python tools/row_coherence_bench.py [--calls 20] [--repeats 7] [--warmup 5] [--distinct 8] [--out profiles/row_coherence_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FC = 957.4e6
N = 1_020_000
D = 64
OV = 8
W, WIN, M = 64, 4096, 16
FS, TUNED = 2.048e6, 433.92e6
PEAK_FMA_PER_S = 39.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--no-yardstick", action="store_true", help="skip the GSM streams and pair_coherence_batch_dev")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "row_coherence_bench.json"))
    args = ap.parse_args()

    import torch
    import gsmcal

    synth = gsmcal.synth
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    ctx = gsmcal.Context(0, stream=stream.cuda_stream)

    def timed(call):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.calls):
                call()
            e1.record(stream)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.calls)
        return {"ms_per_call_median": round(statistics.median(ms), 5), "ms_per_call_min": round(min(ms), 5), "ms_per_call_max": round(max(ms), 5)}

    # ---- the rows: apply_calibration_resident of make_wideband captures ----
    k = max(1, min(args.distinct, D))
    rng = np.random.Generator(np.random.Philox(key=[24, 64]))
    planted = [(float(rng.uniform(-80, 80)), float(rng.uniform(-40, 40)), float(rng.uniform(0, 20)), float(rng.uniform(0, 6.28))) for _ in range(k)]
    caps = np.stack([synth.make_wideband(dongle=i, n=N, sample_rate=FS, tuned_freq=TUNED, e_ppm=e, c_ppm=c, start=st, phase=ph, tx_key=3)[0]
                     for i, (e, c, st, ph) in enumerate(planted)])
    params = np.zeros((D, gsmcal.APPLY_PARAMS))
    for i in range(D):
        e, c, _, _ = planted[i % k]
        params[i] = (0.37 * (i // k), e + 0.5, 1e-6 * (c - 0.4) * TUNED * (1 + 1e-6 * e), 0.1 * i, 0.0, 1.0, 127.4, 127.6, 1.0, 0.0)
    d_caps = torch.from_numpy(caps).to(dev)
    d_raw = d_caps[torch.arange(D, device=dev) % k].contiguous()
    x = torch.empty((D, N), dtype=torch.complex128, device=dev)
    info = torch.zeros((D, gsmcal.APPLY_INFO_COLS), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    gsmcal.apply_calibration_resident(d_raw.data_ptr(), D, N, params, FS, N, N, x.data_ptr(), info.data_ptr(), ctx=ctx)
    ctx.sync()
    valid = gsmcal.valid_of(info.cpu().numpy())
    del d_raw, d_caps
    starts = [4000 + 15000 * j for j in range(W)]
    lists = {"pairs_63": [(0, b) for b in range(1, D)], "pairs_4032": [(a, b) for a in range(D) for b in range(D) if a != b]}
    Ls = WIN // 4
    fma_per_window = (2 * M + 1) * 4 * Ls * 6 + 2 * 4 * Ls
    rec = {"tool": "row_coherence_bench", "gpu": torch.cuda.get_device_name(0), "lib": os.path.relpath(gsmcal.lib_path(), ROOT), "rows": D,
           "samples_per_row": N, "distinct_captures": k, "windows": W, "win_len": WIN, "max_lag": M, "sample_rate": FS,
           "calls_per_timing": args.calls, "repeats": args.repeats, "warmup_calls": args.warmup,
           "timing": "device events around `calls` back-to-back calls, all calls in one session",
           "grid": {"k_row_xcorr": [W, "pairs"], "threads": 256, "k_row_finish": ["pairs"]},
           "fp64_fma_per_pair_window": fma_per_window, "vector_fp64_peak_fma_per_s": PEAK_FMA_PER_S, "workloads": {}}
    outs, calls = {}, {}
    for name, pairs in lists.items():
        outs[name] = torch.zeros((len(pairs), gsmcal.ROW_COLS), dtype=torch.float64, device=dev)

        def call(pairs=pairs, out=outs[name]):
            gsmcal.row_coherence_resident(x.data_ptr(), N, D, pairs, starts, WIN, FS, out.data_ptr(), lag0=0, max_lag=M, valid=valid, ctx=ctx)
        calls[name] = call

    # ---- the yardstick: pair_coherence_batch_dev on DESIGN 19's bench inputs ----
    yard = None
    if not args.no_yardstick:
        coef, ts = synth.fir1(46, 200e3 / synth.FS), synth.sch_training_sequence()
        frac = [7000.0 + 3.37 * i for i in range(D)]
        base = np.stack([synth.make_stream(dongle=i, tx_key=7, start_frame=4, bsic=52, fn0=51 * 300 + 4, frac_start=frac[i])[0] for i in range(D)])
        raw = torch.from_numpy(base).to(dev)
        table = torch.zeros((D, gsmcal.TABLE_COLS), dtype=torch.float64, device=dev)
        pos = torch.zeros((D, 2, gsmcal.MAX_POS_ROWS), dtype=torch.float64, device=dev)
        r = torch.empty((D, N), dtype=torch.complex128, device=dev)
        rlen = torch.zeros(D, dtype=torch.int64, device=dev)
        out_s = torch.zeros((D, gsmcal.SCH_COLS), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        gsmcal.calibrate_batch_dev(raw.data_ptr(), D, N, coef, ts, FC, table.data_ptr(), pos.data_ptr(), r.data_ptr(), rlen.data_ptr(), ctx=ctx)
        gsmcal.sch_decode_batch_dev(r.data_ptr(), N, rlen.data_ptr(), pos.data_ptr(), D, OV, ts, out_s.data_ptr(), ctx=ctx)
        ctx.sync()
        sch = gsmcal.sch_rows(out_s.cpu().numpy())
        align = gsmcal.sch_alignment(sch, OV)
        p63 = np.array(lists["pairs_63"], dtype=np.int32)
        diff = align[p63[:, 1]] - align[p63[:, 0]]
        lg = np.zeros(len(p63), dtype=np.int32)
        if (~np.isnan(diff)).any():
            lg[~np.isnan(diff)] = gsmcal.pair_lag0(sch, p63[~np.isnan(diff)], OV)
        out_p = torch.zeros((len(p63), gsmcal.PAIR_COLS), dtype=torch.float64, device=dev)

        def pair():
            gsmcal.pair_coherence_batch_dev(r.data_ptr(), N, rlen.data_ptr(), pos.data_ptr(), D, OV, p63, lg, out_p.data_ptr(), ctx=ctx)
        t_y = timed(pair)
    times = {name: timed(calls[name]) for name in lists}
    if not args.no_yardstick:
        t_y2 = timed(pair)
        bursts = int(np.sum(gsmcal.pair_rows(out_p.cpu().numpy())["num_eval"]))
        L = 148 * OV
        fma_y = bursts * ((2 * M + 1) * L * 6 + 2 * L)
        ms_y = min(t_y["ms_per_call_median"], t_y2["ms_per_call_median"])
        yard = fma_y / (ms_y * 1e-3)
        rec["yardstick"] = {"call": "pair_coherence_batch_dev, 63 pairs, ov 8, M 16", "before": t_y, "after": t_y2, "ms": ms_y, "bursts_evaluated": bursts,
                            "fp64_fma_per_call": fma_y, "fp64_fma_per_s": round(yard, 1), "fraction_of_vector_fp64_rate": round(yard / PEAK_FMA_PER_S, 5),
                            "workgroups_launched": len(p63) * gsmcal.MAX_PAIR_BURSTS}
    for name, pairs in lists.items():
        rows = gsmcal.row_rows(outs[name].cpu().numpy())
        windows = int(np.sum(rows["num_eval"]))
        ms = times[name]["ms_per_call_median"]
        rate = windows * fma_per_window / (ms * 1e-3)
        w = {"pairs": len(pairs), "pairs_status_0": int(np.sum(rows["status"] == 0)), "windows_evaluated": windows, "windows_used": int(np.sum(rows["num_used"])),
             "k_row_xcorr_workgroups_launched": len(pairs) * W, "row_coherence_batch_resident": times[name],
             "fp64_fma_per_call": windows * fma_per_window, "fp64_fma_per_s": round(rate, 1), "fraction_of_vector_fp64_rate": round(rate / PEAK_FMA_PER_S, 5)}
        if yard:
            w["fma_rate_over_yardstick"] = round(rate / yard, 4)
        rec["workloads"][name] = w
    if yard:
        rec["condition_rate_at_63_pairs_not_below_yardstick"] = bool(rec["workloads"]["pairs_63"]["fma_rate_over_yardstick"] >= 1.0)
    # the first row of the 63-pair table against a call of its own
    one = torch.zeros((1, gsmcal.ROW_COLS), dtype=torch.float64, device=dev)
    gsmcal.row_coherence_resident(x.data_ptr(), N, D, [lists["pairs_63"][0]], starts, WIN, FS, one.data_ptr(), lag0=0, max_lag=M, valid=valid, ctx=ctx)
    ctx.sync()
    rec["first_row_equals_a_call_of_its_own"] = bool(np.array_equal(one.cpu().numpy()[0].view(np.uint64), outs["pairs_63"].cpu().numpy()[0].view(np.uint64)))
    ctx.close()
    line = json.dumps(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
