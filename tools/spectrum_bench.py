#!/usr/bin/env python3
"""Band power-spectrum scanner sweeps on one GPU (gsmcal_band_power_batch_dev) -> one JSON line.

Workloads (diversity plan, 2.048 MS/s, 0.1 s per point = 204 800 samples per capture): GSM-900 at 50 kHz for 1 and 4 dongles
(501 and 2004 captures; 64 taps, decimation 20), and with 2004 captures 10 kHz (128 / 102), 200 kHz (32 / 5), 1 MHz (32 / 1)
and coef = [1] (scan_band_power_spectrum.m).  Per workload: ms per sweep from device events after warm-up, raw bytes, the
fraction of 8 TB/s with bytes counted once, fp64 FLOPs executed (an FMA counts 2) and the fraction of 78.6 TF, which bound
applies, the same sweep through gsmcal_frontend_batch_dev + a torch reduction in the same session, and the largest relative
deviation from the fp64 restatement over a checked subset.  Input: seeded random bytes in distinct device buffers that
together exceed 512 MB, rotated call by call, so no sweep starts with its bytes in the 256 MiB Infinity Cache.

    python tools/spectrum_bench.py [--steps 20] [--warmup 3] [--only div50k_4dongles]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, N = 2.048e6, 204800
HBM, FP64 = 8.0e12, 78.6e12


def restate(a, coef, decim):
    from oracle import gsmcal_oracle as o
    y = o.matlab_filter(np.asarray(coef, dtype=np.float64), o.raw2iq(np.asarray(a, dtype=np.float64)))
    return float(np.mean(np.abs(y[::decim]) ** 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-frontend", action="store_true", help="skip the frontend_batch_dev + reduction comparison")
    args = ap.parse_args()

    import torch
    import gsmcal
    import gsmcal.dist

    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    ctx = gsmcal.Context(0, stream=stream.cuda_stream)
    filt = {r: gsmcal.dist.spectrum_filter(FS, r, 0.1) for r in (50e3, 10e3, 200e3, 1e6)}
    work = [("div50k_1dongle", 501, filt[50e3][1], filt[50e3][2]),
            ("div50k_4dongles", 2004, filt[50e3][1], filt[50e3][2]),
            ("div10k", 2004, filt[10e3][1], filt[10e3][2]),
            ("div200k", 2004, filt[200e3][1], filt[200e3][2]),
            ("div1M", 2004, filt[1e6][1], filt[1e6][2]),
            ("coef1", 2004, np.array([1.0]), 1)]
    if args.only:
        work = [w for w in work if w[0] in args.only.split(",")]
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261016)
    rec = {"tool": "spectrum_bench", "gpu": torch.cuda.get_device_name(0), "lib": os.path.relpath(gsmcal.lib_path(), ROOT), "samples": N,
           "steps": args.steps, "warmup": args.warmup, "hbm_peak_tbs": HBM / 1e12, "fp64_peak_tf": FP64 / 1e12,
           "cache": "seeded random bytes, distinct buffers rotated per call, > 512 MB in rotation", "workloads": {}}
    worst = 0.0
    for name, d, coef, decim in work:
        nbytes = d * 2 * N
        nbuf = max(2, -(-512_000_000 // nbytes))
        bufs = [torch.randint(0, 256, (d, 2 * N), dtype=torch.uint8, device=dev, generator=gen) for _ in range(nbuf)]
        out = torch.empty(d, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def sweep(i):
            gsmcal.band_power_batch_dev(bufs[i % nbuf].data_ptr(), d, N, coef, decim, out.data_ptr(), ctx=ctx)

        def timed(fn):
            for i in range(args.warmup):
                fn(i)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for i in range(args.steps):
                fn(args.warmup + i)
            e1.record(stream)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.steps

        ms = timed(sweep)
        # correctness on a subset: the last sweep's buffer
        sweep(0)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        dev_max = 0.0
        for u in sorted({0, d // 3, d - 1}):
            ref = restate(bufs[0][u].cpu().numpy(), coef, decim)
            dev_max = max(dev_max, abs(got[u] - ref) / ref)
        worst = max(worst, dev_max)
        nd = -(-N // decim)
        nt = len(coef)
        sym = nt in (32, 64, 128) and np.array_equal(coef, coef[::-1])
        per_row = (nt // 2 if sym else nt) * 2 * 4 + 4            # per tap (pair) and component: exact DC FMA + FIR FMA; |y|^2
        flops = float(d) * nd * per_row
        t_mem, t_fp = nbytes / HBM, flops / FP64
        w = {"captures": d, "ntaps": nt, "decim": decim, "symmetric_path": bool(sym), "ms_per_sweep": round(ms, 4),
             "raw_bytes": nbytes, "frac_hbm_8tbs": round(t_mem / (ms * 1e-3), 4), "fp64_flops": flops,
             "frac_fp64_78_6tf": round(t_fp / (ms * 1e-3), 4), "bound": "memory" if t_mem >= t_fp else "fp64",
             "max_rel_dev_checked": dev_max}
        if not args.no_frontend:
            fo = torch.empty((d, nd), dtype=torch.complex128, device=dev)
            res = torch.empty(d, dtype=torch.float64, device=dev)

            def front(i):
                ctx.check(ctx.lib.gsmcal_frontend_batch_dev(ctx.h, gsmcal.api.C.c_void_p(bufs[i % nbuf].data_ptr()), d, N,
                                                            gsmcal.api._dp(np.ascontiguousarray(coef)), nt, decim,
                                                            gsmcal.api.C.c_void_p(fo.data_ptr())), "frontend_batch_dev")
                torch.mean(fo.real ** 2 + fo.imag ** 2, dim=1, out=res)

            w["frontend_plus_reduction_ms"] = round(timed(front), 4)
            del fo
        rec["workloads"][name] = w
        del bufs
        torch.cuda.empty_cache()
    rec["max_rel_dev_checked"] = worst
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
