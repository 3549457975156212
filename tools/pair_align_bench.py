#!/usr/bin/env python3
"""pair_align on device-resident corrected streams (gsmcal_pair_align_batch_dev) -> one JSON line, and
profiles/pair_align_bench.json.

Workload: the 64 dongles of tools/pair_coherence_bench.py (one transmission, every dongle its own clocks, carrier offset, noise and
start instant; 1 020 000 samples each), calibrated by one calibrate_batch_dev call into device buffers; SCH_decode gives the frame
alignment, pair_coherence_batch_dev the 63 rows against stream 0, pair_align_params the parameter rows.  All 64 are then aligned
onto stream 0 and combined with equal weights (a dongle that did not pass the chain's gates, or whose pair row has a status other
than 0, is skipped: its row is written as zeros, it is not read).  Three calls at ov 8, timed the same way in one session -- device
events, warm-up calls, then `repeats` timings of `calls` back-to-back calls each; median, min and max over the repeats:
    sum_only      combined written, aligned not:   reads 16 B per sample per used member, writes 16 B per sample
    aligned_only  aligned written, combined not:   reads 16 B per sample per used member, writes 16 B per sample per member
    both          both written
The yardstick of each is a device-to-device copy that reads + writes the same number of bytes, timed before and after the three
calls; the lower median counts.  Recorded: bytes per second of the call and of the copy, their ratio, and the output samples per
second per used member.  No rate is set as a bar: nobody had measured this kernel.  The first used member's aligned row is checked
bit for bit against the single call.

    python tools/pair_align_bench.py [--calls 10] [--repeats 7] [--warmup 3] [--out profiles/pair_align_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_align_bench.json"))
    args = ap.parse_args()

    import torch
    import gsmcal

    synth = gsmcal.synth
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    ctx = gsmcal.Context(0, stream=stream.cuda_stream)
    coef = synth.fir1(46, 200e3 / synth.FS)
    ts = synth.sch_training_sequence()
    frac = [7000.0 + 3.37 * i for i in range(D)]
    base = np.stack([synth.make_stream(dongle=i, tx_key=7, start_frame=4, bsic=52, fn0=51 * 300 + 4, frac_start=frac[i])[0] for i in range(D)])
    assert base.shape == (D, 2 * N)
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
    del raw
    sch = gsmcal.sch_rows(out_s.cpu().numpy())
    align = gsmcal.sch_alignment(sch, OV)
    pairs = np.array([(0, b) for b in range(1, D)], dtype=np.int32)
    ok = ~np.isnan(align[pairs[:, 1]] - align[pairs[:, 0]])
    lag0 = np.zeros(len(pairs), dtype=np.int32)                   # (0 where a stream has no alignment: such a pair measures nothing)
    if ok.any():
        lag0[ok] = gsmcal.pair_lag0(sch, pairs[ok], OV)
    out_p = torch.zeros((len(pairs), gsmcal.PAIR_COLS), dtype=torch.float64, device=dev)
    gsmcal.pair_coherence_batch_dev(r.data_ptr(), N, rlen.data_ptr(), pos.data_ptr(), D, OV, pairs, lag0, out_p.data_ptr(), ctx=ctx)
    ctx.sync()
    pair_table = out_p.cpu().numpy()
    members = np.arange(D, dtype=np.int32)
    params = np.vstack([[0.0, 0.0, 0.0, 0.0, 0.0, 1.0 / D], gsmcal.pair_align_params(pair_table, OV, 1.0 / D)])

    aligned = torch.empty((D, N), dtype=torch.complex128, device=dev)
    combined = torch.empty(N, dtype=torch.complex128, device=dev)
    info = torch.zeros((D + 1, gsmcal.ALIGN_INFO_COLS), dtype=torch.float64, device=dev)

    def call(al, cb):
        gsmcal.pair_align_batch_dev(r.data_ptr(), N, rlen.data_ptr(), D, OV, members, params, N, info.data_ptr(),
                                    d_aligned=aligned.data_ptr() if al else None, d_combined=combined.data_ptr() if cb else None, ctx=ctx)

    call(True, True)
    ctx.sync()
    t = gsmcal.align_rows(info.cpu().numpy())
    used = int(t["members_used"])
    valid = int(np.sum(t["num_valid"]))

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.calls):
                fn()
            e1.record(stream)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.calls)
        return {"ms_per_call_median": round(statistics.median(ms), 5), "ms_per_call_min": round(min(ms), 5), "ms_per_call_max": round(max(ms), 5)}

    # bytes read + written per call: every used member's valid samples are read once (16 B; the 15 neighbours of a sample come from
    # LDS), every output sample that is asked for is written once
    shapes = {"sum_only": (False, True, 16 * valid + 16 * N),
              "aligned_only": (True, False, 16 * valid + 16 * N * D),
              "both": (True, True, 16 * valid + 16 * N * D + 16 * N)}
    dst = torch.empty(max(b for _, _, b in shapes.values()) // 16 + 1, dtype=torch.float64, device=dev)
    src = torch.rand_like(dst)

    def copy_of(nbytes):
        k = nbytes // 16                                           # doubles per direction: the copy reads 8 k bytes and writes 8 k
        return lambda: dst[:k].copy_(src[:k])

    rec = {"tool": "pair_align_bench", "gpu": torch.cuda.get_device_name(0), "lib": os.path.relpath(gsmcal.lib_path(), ROOT),
           "streams": D, "samples_per_stream": N, "oversampling_ratio": OV, "out_len": N, "calls_per_timing": args.calls,
           "repeats": args.repeats, "warmup_calls": args.warmup,
           "timing": "device events around `calls` back-to-back calls, all calls in one session",
           "streams_calibrated": int(np.sum(table[:, 9].cpu().numpy() == 0)), "pair_rows_status_0": int(np.sum(pair_table[:, 0] == 0)),
           "members": D, "members_used": used, "members_status_no_pos": int(np.sum(t["status"] == 10)),
           "members_status_skipped": int(np.sum(t["status"] == gsmcal.S_ALIGN_SKIPPED)), "valid_samples_of_used_members": valid,
           "combined_interval": [int(t["combined_first"]), int(t["combined_end"])],
           "grid": {"k_pair_align": ["ceil(out_len / 256) tiles", "1 with the sum, members without"], "threads": 256, "k_pair_align_info": [1]},
           "resources": {"k_pair_align": {"vgpr": 99, "sgpr": 106, "scratch_bytes": 0, "lds_static_bytes": 4480, "waves_per_simd": 4},
                         "k_pair_align_info": {"vgpr": 28, "sgpr": 26, "scratch_bytes": 0, "lds_static_bytes": 0},
                         "from": "tools/resource_usage.sh on these sources"},
           "workloads": {}}
    before = {k: timed(copy_of(b)) for k, (_, _, b) in shapes.items()}
    times = {k: timed(lambda al=al, cb=cb: call(al, cb)) for k, (al, cb, _) in shapes.items()}
    after = {k: timed(copy_of(b)) for k, (_, _, b) in shapes.items()}
    for k, (al, cb, nbytes) in shapes.items():
        yard = min(before[k]["ms_per_call_median"], after[k]["ms_per_call_median"])
        ms = times[k]["ms_per_call_median"]
        rec["workloads"][k] = {"aligned_written": al, "combined_written": cb, "bytes_read_plus_written": nbytes,
                               "pair_align_batch_dev": times[k], "copy_before": before[k], "copy_after": after[k], "yardstick_ms": yard,
                               "bytes_per_s": round(nbytes / (ms * 1e-3), 1), "copy_bytes_per_s": round(nbytes / (yard * 1e-3), 1),
                               "call_over_copy": round(ms / yard, 3),
                               "valid_output_samples_per_s": round(valid / (ms * 1e-3), 1)}
    # the first used member past the reference against the single call
    call(True, True)
    ctx.sync()
    first = [g for g in range(1, D) if t["status"][g] == 0]
    same = None
    if first:
        g = first[0]
        one, _ = gsmcal.pair_align(r[g, :int(rlen[g].item())].cpu().numpy(), OV, params[g], N, ctx=ctx)
        same = bool(np.array_equal(one.view(np.float64).view(np.uint64), aligned[g].cpu().numpy().view(np.float64).view(np.uint64)))
    rec["first_used_member_equals_single_call"] = same
    ctx.close()
    line = json.dumps(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
