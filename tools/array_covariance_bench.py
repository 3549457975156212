#!/usr/bin/env python3
"""array_covariance and array_combine on device-resident aligned streams (gsmcal_array_covariance_batch_dev,
gsmcal_array_combine_batch_dev) -> one JSON line, and profiles/array_covariance_bench.json.

Workload: the 64 dongles of tools/pair_coherence_bench.py and tools/pair_align_bench.py (one transmission, every dongle its own
clocks, carrier offset, noise and start instant; 1 020 000 samples each), calibrated, measured against stream 0 and aligned onto
its time base by pair_align_batch_dev into a [64][N] device buffer.  The rows of the members with status 0 are then the input of
four cases at ov 8, all timed the same way in one process -- device events, warm-up calls, then `repeats` timings of `calls`
back-to-back calls each; median, min and max over the repeats:
    cov_whole     one window: the whole interval where every used member is valid
    cov_bursts    the windows of stream 0's SCH and BCCH bursts inside that interval (burst_windows)
    combine_1     one beam (the dominant eigenvector of cov_bursts' sum) over all N samples
    combine_16    sixteen beams
The yardstick of each case is a device-to-device copy that reads + writes the same number of bytes, timed before and after the
four cases; the lower median counts.  Recorded per case: the ratio call / copy, the fp64 multiply-add rate of the call as a fraction
of the rate tools/micro/clock_fp64.hip measured on this device (profiles/r06_clock_lds_microbench.txt: 73.0 TFLOP/s), and which of
the two the kernel sits against (the larger of: copy time / call time, flop time / call time; neither when both are below 0.1).
No rate is set as a bar: nobody had measured these kernels.  Every GPU step runs under a time limit of its own; a step that runs
into it ends the process at once (exit status 124) and nothing further is started.  A window of cov_bursts is checked bit for bit
against the same window alone.

    python tools/array_covariance_bench.py [--calls 10] [--repeats 7] [--warmup 3] [--out profiles/array_covariance_bench.json]
"""
import argparse
import contextlib
import json
import os
import signal
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FC = 957.4e6
N = 1_020_000
D = 64
OV = 8
FP64_FMA_FLOPS = 73.0e12        # profiles/r06_clock_lds_microbench.txt (tools/micro/clock_fp64.hip, the best of its three passes)


@contextlib.contextmanager
def limit(seconds, what):
    """the step's own time limit: the process ends here (status 124), nothing further is started on the GPU"""
    def bail(signum, frame):
        sys.stderr.write(f"array_covariance_bench: step '{what}' ran into its limit of {seconds} s\n")
        sys.stderr.flush()
        os._exit(124)
    old = signal.signal(signal.SIGALRM, bail)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-limit", type=int, default=120, help="seconds per GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "array_covariance_bench.json"))
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
    with limit(args.step_limit, "calibrate, SCH_decode, pair_coherence, pair_align"):
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
        lag0 = np.zeros(len(pairs), dtype=np.int32)
        if ok.any():
            lag0[ok] = gsmcal.pair_lag0(sch, pairs[ok], OV)
        out_p = torch.zeros((len(pairs), gsmcal.PAIR_COLS), dtype=torch.float64, device=dev)
        gsmcal.pair_coherence_batch_dev(r.data_ptr(), N, rlen.data_ptr(), pos.data_ptr(), D, OV, pairs, lag0, out_p.data_ptr(), ctx=ctx)
        ctx.sync()
        pair_table = out_p.cpu().numpy()
        members = np.arange(D, dtype=np.int32)
        params = np.vstack([[0.0, 0.0, 0.0, 0.0, 0.0, 1.0 / D], gsmcal.pair_align_params(pair_table, OV, 1.0 / D)])
        aligned = torch.empty((D, N), dtype=torch.complex128, device=dev)
        info = torch.zeros((D + 1, gsmcal.ALIGN_INFO_COLS), dtype=torch.float64, device=dev)
        gsmcal.pair_align_batch_dev(r.data_ptr(), N, rlen.data_ptr(), D, OV, members, params, N, info.data_ptr(), d_aligned=aligned.data_ptr(), ctx=ctx)
        ctx.sync()
        del r
    info_h = info.cpu().numpy()
    t = gsmcal.align_rows(info_h)
    rows = np.flatnonzero(t["status"] == 0).astype(np.int32)
    G = len(rows)
    first, end = int(t["combined_first"]), int(t["combined_end"])
    assert G >= 1 and rows[0] == 0 and end > first, "stream 0 did not pass the chain, or no interval is covered by every member"
    whole = np.array([[first, end - first]], dtype=np.int64)
    bursts = gsmcal.burst_windows(pos[0].cpu().numpy(), OV, info_h)
    assert len(bursts) >= 1, "no burst of stream 0 inside the combined interval"
    bursts = bursts[:gsmcal.MAX_COV_WINDOWS]

    cov_whole = torch.zeros((1, G, G), dtype=torch.complex128, device=dev)
    cov_bursts = torch.zeros((len(bursts), G, G), dtype=torch.complex128, device=dev)
    out = torch.empty((16, N), dtype=torch.complex128, device=dev)
    with limit(args.step_limit, "the weights"):
        gsmcal.array_covariance_dev(aligned.data_ptr(), N, D, rows, bursts, cov_bursts.data_ptr(), ctx=ctx)
        ctx.sync()
        cb = cov_bursts.cpu().numpy()
        w, winfo = gsmcal.combine_weights(cb.sum(axis=0), ref=0)
        gsmcal.array_covariance_dev(aligned.data_ptr(), N, D, rows, bursts[len(bursts) // 2:len(bursts) // 2 + 1], cov_whole.data_ptr(), ctx=ctx)
        ctx.sync()
        alone = cov_whole.cpu().numpy()[0]
        same = bool(np.array_equal(alone.view(np.float64).view(np.uint64), cb[len(bursts) // 2].view(np.float64).view(np.uint64)))
    rng = np.random.Generator(np.random.Philox(key=[21, 16]))
    w16 = np.vstack([w, rng.standard_normal((15, G)) + 1j * rng.standard_normal((15, G))]) if winfo["status"] == 0 else \
        rng.standard_normal((16, G)) + 1j * rng.standard_normal((16, G))

    def timed(fn, what):
        with limit(args.step_limit, what):
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

    nb = (G + 3) // 4
    per_sample = 8 * 16 * nb * (nb + 1) // 2                      # flops the kernel executes per sample: 4 x 4 blocks of the upper triangle, 4 FMAs an entry
    burst_samples = int(bursts[:, 1].sum())
    cases = {
        "cov_whole": (lambda: gsmcal.array_covariance_dev(aligned.data_ptr(), N, D, rows, whole, cov_whole.data_ptr(), ctx=ctx),
                      16 * G * (end - first) + 16 * G * G, per_sample * (end - first), {"windows": 1, "samples": end - first}),
        "cov_bursts": (lambda: gsmcal.array_covariance_dev(aligned.data_ptr(), N, D, rows, bursts, cov_bursts.data_ptr(), ctx=ctx),
                       16 * G * burst_samples + 16 * G * G * len(bursts), per_sample * burst_samples, {"windows": len(bursts), "samples": burst_samples}),
        "combine_1": (lambda: gsmcal.array_combine_dev(aligned.data_ptr(), N, D, rows, w16[:1], N, out.data_ptr(), ctx=ctx),
                      16 * G * N + 16 * N, 8 * G * N, {"beams": 1, "samples": N}),
        "combine_16": (lambda: gsmcal.array_combine_dev(aligned.data_ptr(), N, D, rows, w16, N, out.data_ptr(), ctx=ctx),
                       16 * G * N + 16 * 16 * N, 8 * G * 16 * N, {"beams": 16, "samples": N}),
    }
    dst = torch.empty(max(b for _, b, _, _ in cases.values()) // 16 + 1, dtype=torch.float64, device=dev)
    src = torch.rand_like(dst)

    def copy_of(nbytes):
        k = max(nbytes // 16, 1)                                   # doubles per direction: the copy reads 8 k bytes and writes 8 k
        return lambda: dst[:k].copy_(src[:k])

    rec = {"tool": "array_covariance_bench", "gpu": torch.cuda.get_device_name(0), "lib": os.path.relpath(gsmcal.lib_path(), ROOT),
           "streams": D, "samples_per_stream": N, "oversampling_ratio": OV, "calls_per_timing": args.calls, "repeats": args.repeats,
           "warmup_calls": args.warmup, "timing": "device events around `calls` back-to-back calls, all cases in one process",
           "rows_used": G, "combined_interval": [first, end], "cov_chunk": gsmcal.COV_CHUNK,
           "fp64_fma_flops_measured": FP64_FMA_FLOPS, "fp64_fma_flops_from": "profiles/r06_clock_lds_microbench.txt (tools/micro/clock_fp64.hip)",
           "weights_status": winfo["status"], "lambda_1_over_lambda_2": (winfo["lambda_1"] / winfo["lambda_2"]) if G > 1 else None,
           "burst_window_equals_the_window_alone": same, "cases": {}}
    before = {k: timed(copy_of(b), "copy before " + k) for k, (_, b, _, _) in cases.items()}
    times = {k: timed(fn, k) for k, (fn, _, _, _) in cases.items()}
    after = {k: timed(copy_of(b), "copy after " + k) for k, (_, b, _, _) in cases.items()}
    for k, (_, nbytes, flops, shape) in cases.items():
        yard = min(before[k]["ms_per_call_median"], after[k]["ms_per_call_median"])
        ms = times[k]["ms_per_call_median"]
        frac_copy, frac_fma = yard / ms, flops / FP64_FMA_FLOPS / (ms * 1e-3)
        rec["cases"][k] = dict(shape, bytes_read_plus_written=nbytes, flops_executed=flops, call=times[k], copy_before=before[k], copy_after=after[k],
                               yardstick_ms=yard, call_over_copy=round(ms / yard, 3), bytes_per_s=round(nbytes / (ms * 1e-3), 1),
                               flops_per_s=round(flops / (ms * 1e-3), 1), fraction_of_fp64_fma_rate=round(frac_fma, 4),
                               fraction_of_copy_rate=round(frac_copy, 4),
                               sits_against=("neither: too few workgroups, each a long run of dependent sums" if max(frac_fma, frac_copy) < 0.1 else
                                             "fp64 multiply-add rate" if frac_fma > frac_copy else "memory"))
    ctx.close()
    line = json.dumps(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
