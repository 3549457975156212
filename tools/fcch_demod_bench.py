#!/usr/bin/env python3
"""FCCH_demod on device-resident corrected streams (gsmcal_fcch_demod_batch_dev) -> one JSON line.

Workloads: D = 64 and D = 1 024 streams of 1 020 000 samples.  A calibrate_batch_dev call writes r_correct, r_len and both
pos_info tables into device buffers (raw bytes: eight seeded synthetic dongles expanded on the device into D distinct
captures, as bench.py does); the timed call is fcch_demod_batch_dev on exactly those buffers.  Per workload: ms per call from
device events -- warm-up calls, then `repeats` timings of `calls` back-to-back calls each; median, min and max over the
repeats -- the bursts and rows behind the figure, and row 0 checked bit for bit against the single-stream gsmcal_FCCH_demod.

A last section runs a few 64-stream calibrate calls with the four-launch tail (a context created under GSMCAL_FUSE_POST=0), so
that a `rocprofv3 --kernel-trace --stats` run of this tool holds k_burst_tone<1, 8, 47> -- the burst stage of the chain, same
1 184-point window and 37 x 32 transform -- next to k_fcch_demod in one session's trace.

    python tools/fcch_demod_bench.py [--streams 64,1024] [--calls 50] [--repeats 7] [--warmup 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="64,1024")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--yardstick-calls", type=int, default=8)
    args = ap.parse_args()

    import torch
    import gsmcal

    synth = gsmcal.synth
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    ctx = gsmcal.Context(0, stream=stream.cuda_stream)
    coef = synth.fir1(46, 200e3 / synth.FS)
    ts = synth.sch_training_sequence()
    base = np.stack([synth.make_stream(dongle=d)[0] for d in range(NBASE)])
    assert base.shape == (NBASE, 2 * N)
    d_base = torch.from_numpy(base).to(dev)
    rec = {"tool": "fcch_demod_bench", "gpu": torch.cuda.get_device_name(0), "lib": os.path.relpath(gsmcal.lib_path(), ROOT),
           "samples_per_stream": N, "oversampling_ratio": 8, "calls_per_timing": args.calls, "repeats": args.repeats,
           "warmup_calls": args.warmup, "timing": "device events around `calls` back-to-back fcch_demod_batch_dev calls",
           "workloads": {}}
    for D in (int(v) for v in args.streams.split(",")):
        raw = torch.empty((D, 2 * N), dtype=torch.uint8, device=dev)
        table = torch.zeros((D, gsmcal.TABLE_COLS), dtype=torch.float64, device=dev)
        pos = torch.zeros((D, 2, gsmcal.MAX_POS_ROWS), dtype=torch.float64, device=dev)
        r = torch.empty((D, N), dtype=torch.complex128, device=dev)
        rlen = torch.zeros(D, dtype=torch.int64, device=dev)
        out = torch.zeros((D, gsmcal.DEMOD_COLS), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        gsmcal.synth_expand_dev(d_base.data_ptr(), NBASE, N, raw.data_ptr(), D, ctx=ctx)
        gsmcal.calibrate_batch_dev(raw.data_ptr(), D, N, coef, ts, FC, table.data_ptr(), pos.data_ptr(), r.data_ptr(), rlen.data_ptr(),
                                   ctx=ctx)
        ctx.sync()

        def call():
            gsmcal.fcch_demod_batch_dev(r.data_ptr(), N, rlen.data_ptr(), pos.data_ptr(), D, 8, FC, out.data_ptr(), ctx=ctx)

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
        rows = gsmcal.demod_rows(out.cpu().numpy())
        ok = rows["status"] == 0
        bursts = int(np.sum(rows["num_fcch"][ok]))
        # row 0 against the single-stream call
        L = int(rlen[0].item())
        same = None
        if L > 0 and ok[0]:
            k = int(table[0, 7].item())
            one = gsmcal.FCCH_demod(r[0, :L].cpu().numpy(), pos[0, :, :k].cpu().numpy().T, 8, FC, ctx=ctx)
            nb = len(one["freq"])
            same = bool(np.array_equal(one["freq"], rows["freq"][0, :nb]) and np.array_equal(one["snr"], rows["snr"][0, :nb], equal_nan=True)
                        and np.array_equal(one["max_idx"], rows["max_idx"][0, :nb]) and one["carrier_ppm"] == rows["carrier_ppm"][0])
        med = statistics.median(ms)
        rec["workloads"][f"streams_{D}"] = {
            "streams": D, "rows_status_0": int(np.sum(ok)), "bursts": bursts, "workgroups_launched": D * gsmcal.MAX_HITS,
            "ms_per_call_median": round(med, 5), "ms_per_call_min": round(min(ms), 5), "ms_per_call_max": round(max(ms), 5),
            "us_per_burst_at_median": round(1e3 * med / max(bursts, 1), 4),
            "residual_carrier_ppm_abs_max": float(np.max(np.abs(rows["carrier_ppm"][ok]))) if np.any(ok) else None,
            "snr_db_min_max": [float(np.nanmin(rows["snr"][ok])), float(np.nanmax(rows["snr"][ok]))] if np.any(ok) else None,
            "row0_equals_single_stream_call": same}
        del raw, table, pos, r, rlen, out
        torch.cuda.empty_cache()

    # the yardstick's kernels for a kernel trace of this session: the four-launch tail at 64 streams
    if args.yardstick_calls > 0:
        os.environ["GSMCAL_FUSE_POST"] = "0"
        c4 = gsmcal.Context(0, stream=stream.cuda_stream)
        del os.environ["GSMCAL_FUSE_POST"]
        D = 64
        raw = torch.empty((D, 2 * N), dtype=torch.uint8, device=dev)
        table = torch.zeros((D, gsmcal.TABLE_COLS), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        gsmcal.synth_expand_dev(d_base.data_ptr(), NBASE, N, raw.data_ptr(), D, ctx=c4)
        for _ in range(args.yardstick_calls):
            gsmcal.calibrate_batch_dev(raw.data_ptr(), D, N, coef, ts, FC, table.data_ptr(), ctx=c4)
        c4.sync()
        rec["yardstick"] = {"calls": args.yardstick_calls, "streams": D, "tail": "four launches (GSMCAL_FUSE_POST=0)",
                            "rows_status_0": int(torch.sum(table[:, 9] == 0).item()),
                            "bursts_per_call": int(torch.sum(table[:, 6][table[:, 9] == 0]).item())}
        c4.close()
    ctx.close()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
