#!/usr/bin/env python3
"""apply_calibration on device-resident raw captures (gsmcal_apply_calibration_batch_resident) -> one JSON line, and
profiles/apply_calibration_bench.json.

Workload: 64 captures of 1 020 000 samples of seeded random bytes, resident on the device, every capture with a parameter row of
its own (sampling clock error within +-80 ppm, carrier error within +-40 ppm of 433.92 MHz, a delay of a few samples, a DC and an
I/Q imbalance), corrected into 64 complex rows of 1 020 000 samples at 2.048 MHz.  The call reads 2 bytes and writes 16 per output
sample: 18 B / sample.
Beside it, in the same process and on the same device: gsmcal_pair_align_batch_dev writing the aligned rows only, 64 members of 64
complex streams of the same length with the same delays, drifts and carriers -- the same arithmetic per output sample on an input
eight times as wide.  apply_calibration must not be slower than it per valid output sample.
Timing: device events, warm-up calls, then `repeats` timings of `calls` back-to-back calls each, the two entry points taking turns;
median, min and max over the repeats.  The yardstick is a device-to-device copy that reads + writes the same number of bytes as
apply_calibration, timed before and after; the lower median counts.  No rate is set as a bar.  The first capture's row is checked
bit for bit against the host form.

    python tools/apply_calibration_bench.py [--calls 10] [--repeats 7] [--warmup 3] [--out profiles/apply_calibration_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 1_020_000
D = 64
FS = 2.048e6
F_T = 433.92e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--captures", type=int, default=D)
    ap.add_argument("--samples", type=int, default=N)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "apply_calibration_bench.json"))
    args = ap.parse_args()
    d, n = args.captures, args.samples

    import torch
    import gsmcal

    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    ctx = gsmcal.Context(0, stream=stream.cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20260101)
    raw = torch.randint(0, 256, (d, 2 * n), dtype=torch.uint8, device=dev, generator=gen)
    rng = np.random.Generator(np.random.Philox(key=[23, 64]))
    table = np.zeros((d, gsmcal.TABLE_COLS))
    table[:, 4], table[:, 5] = rng.uniform(-80.0, 80.0, d), rng.uniform(-40.0, 40.0, d)
    params = gsmcal.apply_params(table, F_T, delay=rng.uniform(-3.0, 3.0, d), phase=rng.uniform(-3.0, 3.0, d))
    params[:, 6], params[:, 7] = rng.uniform(126.5, 128.5, d), rng.uniform(126.5, 128.5, d)
    params[:, 8], params[:, 9] = rng.uniform(0.95, 1.05, d), np.sin(np.radians(rng.uniform(-3.0, 3.0, d)))
    out = torch.empty((d, n), dtype=torch.complex128, device=dev)
    info = torch.zeros((d, gsmcal.APPLY_INFO_COLS), dtype=torch.float64, device=dev)

    def apply():
        gsmcal.apply_calibration_resident(raw.data_ptr(), d, n, params, FS, n, n, out.data_ptr(), info.data_ptr(), ctx=ctx)

    apply()
    ctx.sync()
    t = gsmcal.apply_rows(info.cpu().numpy())
    valid = int(np.sum(t["num_valid"]))
    first_row = out[0].cpu().numpy()

    # the comparison: pair_align of as many members of as many complex streams, the aligned rows only
    r = torch.view_as_complex(torch.rand((d, n, 2), dtype=torch.float64, device=dev, generator=gen) * 255.0 - 127.5)
    rlen = torch.full((d,), n, dtype=torch.int64, device=dev)
    members = np.arange(d, dtype=np.int32)
    pa_params = np.column_stack([params[:, :5], np.full(d, 1.0 / d)])
    pa_info = torch.zeros((d + 1, gsmcal.ALIGN_INFO_COLS), dtype=torch.float64, device=dev)
    aligned = torch.empty((d, n), dtype=torch.complex128, device=dev)

    def align():
        gsmcal.pair_align_batch_dev(r.data_ptr(), n, rlen.data_ptr(), d, 8, members, pa_params, n, pa_info.data_ptr(),
                                    d_aligned=aligned.data_ptr(), ctx=ctx)

    align()
    ctx.sync()
    pa_valid = int(np.sum(gsmcal.align_rows(pa_info.cpu().numpy())["num_valid"]))

    def timed_once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.calls):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.calls

    def summary(ms):
        return {"ms_per_call_median": round(statistics.median(ms), 5), "ms_per_call_min": round(min(ms), 5), "ms_per_call_max": round(max(ms), 5)}

    def timed(*fns):
        """the functions taking turns: warm-up calls of each, then `repeats` rounds of one timing each"""
        for fn in fns:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = [[] for _ in fns]
        for _ in range(args.repeats):
            for i, fn in enumerate(fns):
                ms[i].append(timed_once(fn))
        return [summary(m) for m in ms]

    nbytes = 18 * d * n                                            # read 2 B + written 16 B per output sample
    k = nbytes // 2                                                # the copy reads k bytes and writes k
    src = torch.randint(0, 256, (k,), dtype=torch.uint8, device=dev, generator=gen)
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)

    before, = timed(copy)
    t_apply, t_align = timed(apply, align)
    after, = timed(copy)
    yard = min(before["ms_per_call_median"], after["ms_per_call_median"])
    ms, ms_pa = t_apply["ms_per_call_median"], t_align["ms_per_call_median"]
    per_apply, per_align = ms * 1e6 / valid, ms_pa * 1e6 / pa_valid        # ns per valid output sample
    one, _ = gsmcal.apply_calibration(raw[0:1].cpu().numpy(), params[0:1], FS, n, ctx=ctx)
    rec = {"tool": "apply_calibration_bench", "gpu": torch.cuda.get_device_name(0), "lib": os.path.relpath(gsmcal.lib_path(), ROOT),
           "captures": d, "samples_per_capture": n, "sample_rate": FS, "out_len": n, "calls_per_timing": args.calls, "repeats": args.repeats,
           "warmup_calls": args.warmup,
           "timing": "device events around `calls` back-to-back calls, apply_calibration and pair_align taking turns, all in one process",
           "captures_status_0": int(np.sum(t["status"] == 0)), "valid_output_samples": valid,
           "grid": {"k_apply_calibration": ["ceil(out_len / 256) tiles", "captures"], "threads": 256, "k_apply_info": ["ceil(captures / 64)"]},
           "resources": {"k_apply_calibration": {"vgpr": 60, "sgpr": 77, "scratch_bytes": 0, "lds_static_bytes": 4480, "waves_per_simd": 8},
                         "k_apply_info": {"vgpr": 24, "sgpr": 20, "scratch_bytes": 0, "lds_static_bytes": 0},
                         "from": "tools/resource_usage.sh on these sources"},
           "apply_calibration_batch_resident": t_apply, "bytes_read_plus_written": nbytes, "bytes_per_output_sample": 18,
           "bytes_per_s": round(nbytes / (ms * 1e-3), 1), "valid_output_samples_per_s": round(valid / (ms * 1e-3), 1),
           "copy_before": before, "copy_after": after, "yardstick_ms": yard, "copy_bytes_per_s": round(nbytes / (yard * 1e-3), 1),
           "call_over_copy": round(ms / yard, 3),
           "pair_align_batch_dev_aligned_only": dict(t_align, members=d, valid_output_samples=pa_valid,
                                                     bytes_read_plus_written=16 * pa_valid + 16 * d * n,
                                                     valid_output_samples_per_s=round(pa_valid / (ms_pa * 1e-3), 1)),
           "ns_per_valid_output_sample": {"apply_calibration": round(per_apply, 6), "pair_align": round(per_align, 6)},
           "apply_over_pair_align_per_valid_sample": round(per_apply / per_align, 4),
           "not_slower_than_pair_align": bool(per_apply <= per_align),
           "first_capture_equals_host_form": bool(np.array_equal(one[0].view(np.float64).view(np.uint64), first_row.view(np.float64).view(np.uint64)))}
    ctx.close()
    line = json.dumps(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
