#!/usr/bin/env python3
"""pair_coherence on device-resident corrected streams (gsmcal_pair_coherence_batch_dev) -> one JSON line, and
profiles/pair_coherence_bench.json.

Workload: 64 dongles on ONE transmission (synth.make_stream with the same tx_key, start_frame, bsic and fn0 and a frac_start of
its own each: every dongle its own clocks, carrier offset and noise), 1 020 000 samples each, calibrated by one calibrate_batch_dev
call into device buffers; SCH_decode on them gives the frame alignment and pair_lag0 the expected offset of every pair.  Two pair
lists at ov 8 and the default max_lag 16: the 63 pairs against stream 0, and all 4 032 ordered pairs.  In one session three calls
are timed the same way -- device events, warm-up calls, then `repeats` timings of `calls` back-to-back calls each; median, min and
max over the repeats:
    bcch_demod_batch_dev          on the same 64 streams: the yardstick, timed before and after; the lower median counts
    pair_coherence_batch_dev      k_pair_xcorr + k_pair_finish, 63 pairs
    pair_coherence_batch_dev      ... 4 032 pairs
Recorded: the ratio to the yardstick, the fp64 FMAs of the evaluated bursts -- per burst (2M+1) L 4 for c, (2M+1) L 2 for Eb and
2 L for Ea, L = 148 ov -- and the fraction of the vector fp64 rate (39.3 T FMA/s = 78.6 TFLOP/s) they amount to per second.  No bar
is set: nobody had measured this kernel.  The first row of the 63-pair table with status 0 is checked bit for bit against the
single call.  (Ten of the 64 seeded dongles do not pass the chain's own gates: their pairs come back GSMCAL_S_POST_NO_POS.)

    python tools/pair_coherence_bench.py [--calls 50] [--repeats 7] [--warmup 5] [--out profiles/pair_coherence_bench.json]
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
PEAK_FMA_PER_S = 39.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_coherence_bench.json"))
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
    frac = [7000.0 + 3.37 * i for i in range(D)]
    base = np.stack([synth.make_stream(dongle=i, tx_key=7, start_frame=4, bsic=52, fn0=51 * 300 + 4, frac_start=frac[i])[0] for i in range(D)])
    assert base.shape == (D, 2 * N)
    raw = torch.from_numpy(base).to(dev)
    table = torch.zeros((D, gsmcal.TABLE_COLS), dtype=torch.float64, device=dev)
    pos = torch.zeros((D, 2, gsmcal.MAX_POS_ROWS), dtype=torch.float64, device=dev)
    r = torch.empty((D, N), dtype=torch.complex128, device=dev)
    rlen = torch.zeros(D, dtype=torch.int64, device=dev)
    out_s = torch.zeros((D, gsmcal.SCH_COLS), dtype=torch.float64, device=dev)
    out_b = torch.zeros((D, gsmcal.BCCH_COLS), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    gsmcal.calibrate_batch_dev(raw.data_ptr(), D, N, coef, ts, FC, table.data_ptr(), pos.data_ptr(), r.data_ptr(), rlen.data_ptr(), ctx=ctx)
    gsmcal.sch_decode_batch_dev(r.data_ptr(), N, rlen.data_ptr(), pos.data_ptr(), D, OV, ts, out_s.data_ptr(), ctx=ctx)
    ctx.sync()
    sch = gsmcal.sch_rows(out_s.cpu().numpy())
    align = gsmcal.sch_alignment(sch, OV)
    aligned = ~np.isnan(align)

    def lags(pairs):
        """pair_lag0 where both streams have an alignment, 0 elsewhere (such a pair measures nothing; its row says so)"""
        diff = align[pairs[:, 1]] - align[pairs[:, 0]]
        ok = ~np.isnan(diff)
        out = np.zeros(len(pairs), dtype=np.int32)
        if ok.any():
            out[ok] = gsmcal.pair_lag0(sch, pairs[ok], OV)
        return out

    lists = {"pairs_63": np.array([(0, b) for b in range(1, D)], dtype=np.int32),
             "pairs_4032": np.array([(a, b) for a in range(D) for b in range(D) if a != b], dtype=np.int32)}
    M, L = 2 * OV, 148 * OV
    fma_per_burst = (2 * M + 1) * L * 6 + 2 * L
    rec = {"tool": "pair_coherence_bench", "gpu": torch.cuda.get_device_name(0), "lib": os.path.relpath(gsmcal.lib_path(), ROOT),
           "streams": D, "samples_per_stream": N, "oversampling_ratio": OV, "max_lag": M, "calls_per_timing": args.calls,
           "repeats": args.repeats, "warmup_calls": args.warmup,
           "timing": "device events around `calls` back-to-back calls, all calls in one session",
           "streams_calibrated": int(np.sum(table[:, 9].cpu().numpy() == 0)), "streams_with_sch_alignment": int(aligned.sum()),
           "grid": {"k_pair_xcorr": [gsmcal.MAX_PAIR_BURSTS, "pairs"], "threads": 256, "k_pair_finish": ["pairs"]},
           "resources": {"k_pair_xcorr": {"vgpr": 60, "sgpr": 50, "scratch_bytes": 0, "lds_static_bytes": 6272, "lds_dynamic_bytes": (2 * L + 2 * M) * 16},
                         "k_pair_finish": {"vgpr": 124, "sgpr": 60, "scratch_bytes": 0, "lds_static_bytes": 1920},
                         "from": "tools/resource_usage.sh on these sources"},
           "fp64_fma_per_pair_burst": {"c": (2 * M + 1) * L * 4, "energies": (2 * M + 1) * L * 2 + 2 * L, "total": fma_per_burst},
           "vector_fp64_peak_fma_per_s": PEAK_FMA_PER_S, "workloads": {}}

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

    def bcch():
        gsmcal.bcch_demod_batch_dev(r.data_ptr(), N, rlen.data_ptr(), pos.data_ptr(), D, OV, nts, FC, out_b.data_ptr(), ctx=ctx)

    outs, calls = {}, {}
    for name, pairs in lists.items():
        outs[name] = torch.zeros((len(pairs), gsmcal.PAIR_COLS), dtype=torch.float64, device=dev)
        lg = lags(pairs)

        def call(pairs=pairs, lg=lg, out=outs[name]):
            gsmcal.pair_coherence_batch_dev(r.data_ptr(), N, rlen.data_ptr(), pos.data_ptr(), D, OV, pairs, lg, out.data_ptr(), ctx=ctx)
        calls[name] = (call, pairs, lg)
    t_y = timed(bcch)
    times = {name: timed(calls[name][0]) for name in lists}
    t_y2 = timed(bcch)
    yard = min(t_y["ms_per_call_median"], t_y2["ms_per_call_median"])
    rec["bcch_demod_batch_dev"], rec["bcch_demod_batch_dev_again"], rec["yardstick_ms"] = t_y, t_y2, yard
    for name, (call, pairs, lg) in calls.items():
        rows = gsmcal.pair_rows(outs[name].cpu().numpy())
        good = rows["status"] == 0
        bursts = int(np.sum(rows["num_eval"]))
        ms = times[name]["ms_per_call_median"]
        fma_rate = bursts * fma_per_burst / (ms * 1e-3)
        w = {"pairs": len(pairs), "pairs_status_0": int(good.sum()), "pairs_status_few": int(np.sum(rows["status"] == gsmcal.S_PAIR_FEW)),
             "pairs_status_no_pos": int(np.sum(rows["status"] == 10)), "bursts_evaluated": bursts, "bursts_used": int(np.sum(rows["num_used"])),
             "k_pair_xcorr_workgroups_launched": len(pairs) * gsmcal.MAX_PAIR_BURSTS,
             "pair_coherence_batch_dev": times[name], "pair_over_yardstick": round(ms / yard, 4),
             "fp64_fma_per_call": bursts * fma_per_burst, "fp64_fma_per_s": round(fma_rate, 1),
             "fraction_of_vector_fp64_rate": round(fma_rate / PEAK_FMA_PER_S, 5)}
        if good.any():
            w["mean_coherence_median"] = round(float(np.median(rows["mean_coherence"][good])), 5)
            w["delay_rms_median"] = round(float(np.median(rows["delay_rms"][good])), 5)
            w["abs_rel_carrier_hz_median"] = round(float(np.median(np.abs(rows["rel_carrier_hz"][good]))), 3)
            w["abs_rel_sampling_ppm_median"] = round(float(np.median(np.abs(rows["rel_sampling_ppm"][good]))), 4)
        rec["workloads"][name] = w
    # the first row of the 63-pair table with status 0 against the single call
    _, pairs, lg = calls["pairs_63"]
    t63 = outs["pairs_63"].cpu().numpy()
    first = np.nonzero(t63[:, 0] == 0)[0]
    same = None
    if len(first):
        q = int(first[0])
        a, b = int(pairs[q, 0]), int(pairs[q, 1])
        la, lb, k = int(rlen[a].item()), int(rlen[b].item()), int(table[a, 7].item())
        one = gsmcal.pair_coherence(r[a, :la].cpu().numpy(), r[b, :lb].cpu().numpy(), pos[a, :, :k].cpu().numpy().T, OV, int(lg[q]), ctx=ctx)
        same = bool(one is not None and np.array_equal(one["row"].view(np.uint64), t63[q].view(np.uint64)))
    rec["first_good_row_equals_single_call"] = same
    ctx.close()
    line = json.dumps(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
