#!/usr/bin/env python3
"""BCCH_demod on device-resident corrected streams (gsmcal_bcch_demod_batch_dev) -> one JSON line, and profiles/bcch_demod_bench.json.

Workloads: D = 64 and D = 1 024 streams of 1 020 000 samples, as tools/fcch_demod_bench.py: a calibrate_batch_dev call writes
r_correct, r_len and both pos_info tables into device buffers (raw bytes: eight seeded synthetic dongles, training sequence code =
dongle, expanded on the device into D distinct captures); the timed calls run on exactly those buffers.  In one session, per
workload, two calls are timed the same way -- device events, warm-up calls, then `repeats` timings of `calls` back-to-back calls
each; median, min and max over the repeats:
    fcch_demod_batch_dev    the kernel pair the new call contains (k_fcch_demod + its finish kernel): the yardstick
    bcch_demod_batch_dev    k_fcch_demod + k_bcch_corr + k_bcch_finish (table only: no correlations, no r)
`added_ms` = the BCCH median minus the FCCH median is what the feature adds; it must not exceed the FCCH median (the correlator
reads 26/148 of the samples the FCCH kernel reads and has no transform).  Row 0 is checked bit for bit against the single-stream
gsmcal_BCCH_demod.

    python tools/bcch_demod_bench.py [--streams 64,1024] [--calls 50] [--repeats 7] [--warmup 5] [--out profiles/bcch_demod_bench.json]
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
NBASE = 8
GRID_X = 8                 # BC_GRID_X of csrc/kernels_demod.h: workgroups of k_bcch_corr per stream


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="64,1024")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bcch_demod_bench.json"))
    args = ap.parse_args()

    import torch
    import gsmcal

    synth = gsmcal.synth
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    ctx = gsmcal.Context(0, stream=stream.cuda_stream)
    coef = synth.fir1(46, 200e3 / synth.FS)
    ts = synth.sch_training_sequence()
    nts = synth.normal_training_sequences(8)
    base = np.stack([synth.make_stream(dongle=d, tsc=d)[0] for d in range(NBASE)])
    assert base.shape == (NBASE, 2 * N)
    d_base = torch.from_numpy(base).to(dev)
    rec = {"tool": "bcch_demod_bench", "gpu": torch.cuda.get_device_name(0), "lib": os.path.relpath(gsmcal.lib_path(), ROOT),
           "samples_per_stream": N, "oversampling_ratio": 8, "calls_per_timing": args.calls, "repeats": args.repeats,
           "warmup_calls": args.warmup, "timing": "device events around `calls` back-to-back calls, both calls in one session",
           "grid": {"k_bcch_corr": [GRID_X, "streams"], "threads": 256},
           "note": "the captures are circular shifts (+-1 LSB) of eight base captures: each has a seam where the 51-multiframe jumps, the "
                   "chain rejects most of them and BCCH positions interpolated across the seam are not burst starts, so "
                   "rows_with_the_planted_code describes the input, not the kernels (DESIGN.md section 15)",
           "workloads": {}}

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
        return {"ms_per_call_median": round(statistics.median(ms), 5), "ms_per_call_min": round(min(ms), 5),
                "ms_per_call_max": round(max(ms), 5)}

    for D in (int(v) for v in args.streams.split(",")):
        raw = torch.empty((D, 2 * N), dtype=torch.uint8, device=dev)
        table = torch.zeros((D, gsmcal.TABLE_COLS), dtype=torch.float64, device=dev)
        pos = torch.zeros((D, 2, gsmcal.MAX_POS_ROWS), dtype=torch.float64, device=dev)
        r = torch.empty((D, N), dtype=torch.complex128, device=dev)
        rlen = torch.zeros(D, dtype=torch.int64, device=dev)
        out_f = torch.zeros((D, gsmcal.DEMOD_COLS), dtype=torch.float64, device=dev)
        out_b = torch.zeros((D, gsmcal.BCCH_COLS), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        gsmcal.synth_expand_dev(d_base.data_ptr(), NBASE, N, raw.data_ptr(), D, ctx=ctx)
        gsmcal.calibrate_batch_dev(raw.data_ptr(), D, N, coef, ts, FC, table.data_ptr(), pos.data_ptr(), r.data_ptr(), rlen.data_ptr(),
                                   ctx=ctx)
        ctx.sync()

        def fcch():
            gsmcal.fcch_demod_batch_dev(r.data_ptr(), N, rlen.data_ptr(), pos.data_ptr(), D, 8, FC, out_f.data_ptr(), ctx=ctx)

        def bcch():
            gsmcal.bcch_demod_batch_dev(r.data_ptr(), N, rlen.data_ptr(), pos.data_ptr(), D, 8, nts, FC, out_b.data_ptr(), ctx=ctx)

        t_f, t_b, t_f2 = timed(fcch), timed(bcch), timed(fcch)
        rows = gsmcal.bcch_rows(out_b.cpu().numpy())
        ok = (rows["status"] == 0) | (rows["status"] == 13)
        bursts = int(np.sum(rows["num_bcch"][ok]))
        planted = (np.arange(D) % NBASE) + 1.0                      # capture u expands base capture u mod NBASE
        L = int(rlen[0].item())
        same = None
        if L > 0:
            k = int(table[0, 7].item())
            one = gsmcal.BCCH_demod(r[0, :L].cpu().numpy(), pos[0, :, :k].cpu().numpy().T, nts, 8, FC, ctx=ctx, want_r=False)
            same = bool(np.array_equal(one["row"].view(np.uint64), out_b[0].cpu().numpy().view(np.uint64)))
        yard = min(t_f["ms_per_call_median"], t_f2["ms_per_call_median"])
        added = round(t_b["ms_per_call_median"] - yard, 5)
        rec["workloads"][f"streams_{D}"] = {
            "streams": D, "rows_evaluated": int(np.sum(ok)), "rows_status_0": int(np.sum(rows["status"] == 0)),
            "rows_with_the_planted_code": int(np.sum(rows["tsc_idx"][ok] == planted[ok])), "bcch_bursts": bursts,
            "k_bcch_corr_workgroups_launched": D * GRID_X,
            "fcch_demod_batch_dev": t_f, "bcch_demod_batch_dev": t_b, "fcch_demod_batch_dev_again": t_f2,
            "yardstick_ms": yard, "added_ms": added, "added_over_yardstick": round(added / yard, 4),
            "added_within_yardstick": bool(added <= yard),
            "peak_over_runner_up_min": float(np.nanmin(rows["peak"][ok] / rows["runner_up"][ok])) if np.any(ok) else None,
            "row0_equals_single_stream_call": same}
        del raw, table, pos, r, rlen, out_f, out_b
        torch.cuda.empty_cache()
    ctx.close()
    line = json.dumps(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
