#!/usr/bin/env python3
"""SCH_decode on device-resident corrected streams (gsmcal_sch_decode_batch_dev) -> one JSON line, and profiles/sch_decode_bench.json.

Workloads: D = 64 and D = 1 024 streams of 1 020 000 samples, as tools/bcch_demod_bench.py: a calibrate_batch_dev call writes
r_correct, r_len and both pos_info tables into device buffers (raw bytes: eight seeded synthetic dongles with a planted SCH payload,
bsic = 8*dongle + 5 and fn0 = 51*(1000*dongle + 7) + start_frame, expanded on the device into D distinct captures); the timed calls
run on exactly those buffers.  In one session, per workload, two calls are timed the same way -- device events, warm-up calls, then
`repeats` timings of `calls` back-to-back calls each; median, min and max over the repeats:
    fcch_demod_batch_dev    the yardstick, timed before and after; the lower median counts
    sch_decode_batch_dev    k_sch_decode + k_sch_finish (table only: no soft values, no decoded words)
The new call reads an eighth or less of the samples the yardstick reads and has no transform; its 39 dependent trellis steps are
latency, not work: its median should not exceed the yardstick's (`within_yardstick`).  Row 0 is checked bit for bit against the
single-stream gsmcal_SCH_decode.

    python tools/sch_decode_bench.py [--streams 64,1024] [--calls 50] [--repeats 7] [--warmup 5] [--out profiles/sch_decode_bench.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sch_decode_bench.json"))
    args = ap.parse_args()

    import torch
    import gsmcal

    synth = gsmcal.synth
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    ctx = gsmcal.Context(0, stream=stream.cuda_stream)
    coef = synth.fir1(46, 200e3 / synth.FS)
    ts = synth.sch_training_sequence()
    made = []
    for d in range(NBASE):
        sf = synth.make_stream(dongle=d, num_frames=1)[1]["start_frame"]
        made.append(synth.make_stream(dongle=d, bsic=8 * d + 5, fn0=51 * (1000 * d + 7) + sf))
    base = np.stack([m[0] for m in made])
    assert base.shape == (NBASE, 2 * N)
    d_base = torch.from_numpy(base).to(dev)
    rec = {"tool": "sch_decode_bench", "gpu": torch.cuda.get_device_name(0), "lib": os.path.relpath(gsmcal.lib_path(), ROOT),
           "samples_per_stream": N, "oversampling_ratio": 8, "calls_per_timing": args.calls, "repeats": args.repeats,
           "warmup_calls": args.warmup, "timing": "device events around `calls` back-to-back calls, both calls in one session",
           "grid": {"k_sch_decode": [gsmcal.MAX_HITS, "streams"], "threads": 64, "k_sch_finish": ["streams"]},
           "note": "the captures are circular shifts (+-1 LSB) of eight base captures: each has a seam where the 51-multiframe and the "
                   "frame number jump, the chain rejects most of them and SCH positions interpolated across the seam are not burst "
                   "starts, so the rows_* counts describe the input, not the kernels (DESIGN.md sections 15 and 16)",
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
        out_s = torch.zeros((D, gsmcal.SCH_COLS), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        gsmcal.synth_expand_dev(d_base.data_ptr(), NBASE, N, raw.data_ptr(), D, ctx=ctx)
        gsmcal.calibrate_batch_dev(raw.data_ptr(), D, N, coef, ts, FC, table.data_ptr(), pos.data_ptr(), r.data_ptr(), rlen.data_ptr(),
                                   ctx=ctx)
        ctx.sync()

        def fcch():
            gsmcal.fcch_demod_batch_dev(r.data_ptr(), N, rlen.data_ptr(), pos.data_ptr(), D, 8, FC, out_f.data_ptr(), ctx=ctx)

        def sch():
            gsmcal.sch_decode_batch_dev(r.data_ptr(), N, rlen.data_ptr(), pos.data_ptr(), D, 8, ts, out_s.data_ptr(), ctx=ctx)

        t_f, t_s, t_f2 = timed(fcch), timed(sch), timed(fcch)
        rows = gsmcal.sch_rows(out_s.cpu().numpy())
        ev = (rows["status"] == 0) | (rows["status"] == 14)
        good = rows["status"] == 0
        planted = 8.0 * (np.arange(D) % NBASE) + 5.0                # capture u expands base capture u mod NBASE
        L = int(rlen[0].item())
        same = None
        if L > 0:
            k = int(table[0, 7].item())
            one = gsmcal.SCH_decode(r[0, :L].cpu().numpy(), pos[0, :, :k].cpu().numpy().T, ts, 8, ctx=ctx)
            same = bool(np.array_equal(one["row"].view(np.uint64), out_s[0].cpu().numpy().view(np.uint64)))
        yard = min(t_f["ms_per_call_median"], t_f2["ms_per_call_median"])
        rec["workloads"][f"streams_{D}"] = {
            "streams": D, "rows_evaluated": int(np.sum(ev)), "rows_status_0": int(np.sum(good)),
            "rows_with_the_planted_bsic": int(np.sum(rows["bsic"][good] == planted[good])),
            "rows_with_every_ok_burst_consistent": int(np.sum(good & (rows["num_consistent"] == rows["num_ok"]))),
            "sch_bursts": int(np.sum(rows["num_sch"][ev])), "sch_bursts_ok": int(np.sum(rows["num_ok"][ev])),
            "k_sch_decode_waves_launched": D * gsmcal.MAX_HITS,
            "fcch_demod_batch_dev": t_f, "sch_decode_batch_dev": t_s, "fcch_demod_batch_dev_again": t_f2,
            "yardstick_ms": yard, "sch_over_yardstick": round(t_s["ms_per_call_median"] / yard, 4),
            "within_yardstick": bool(t_s["ms_per_call_median"] <= yard),
            "row0_equals_single_stream_call": same}
        del raw, table, pos, r, rlen, out_f, out_s
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
