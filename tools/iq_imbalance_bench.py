#!/usr/bin/env python3
"""I/Q imbalance and clipping check on one GPU (gsmcal_iq_imbalance_batch_dev) -> profiles/iq_imbalance_bench.json and one JSON line.

Workloads: D = 64 and D = 1 024 device-resident captures of 1 020 000 samples (the reference's capture length).  Per workload: ms
per call from device events after --warmup calls (median and min-max over --repeats timed loops of --steps back-to-back calls), and
the achieved bytes per second on ALGORITHMIC bytes (2 B/sample read once).  Input: seeded CW captures with a planted imbalance
(tone + noise + DC, made on the device), rotated call by call over four buffers as bench.py rotates its input.

The yardstick is gsmcal_cw_check_batch_dev, summary only (d_r = NULL), on the same buffers: it reads the same bytes twice and
divides.  It is timed before and after the new call in the same process, and its lower median counts.  The expectation is that the
new call's median is no higher; "expectation_met" says whether it was.

Every workload runs in a process of its own under `timeout -k 10`; the first one that fails ends the run and nothing further is
started.

    python tools/iq_imbalance_bench.py [--steps 50] [--warmup 5] [--repeats 7] [--only d64,d1024] [--out profiles/iq_imbalance_bench.json]
"""
import argparse
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 1020000
THR = 0.2
NBUF = 4
GAIN, PHASE_DEG = 1.05, 3.0
README_TBPS = (6.05, 6.16)                                      # what the project's streaming kernel reaches (README)
WORKLOADS = [("d64", 64), ("d1024", 1024)]


def cw_bytes(torch, d, n, gen, dev):
    """d seeded CW captures on the device: tone of 0.7 rad/sample, amplitude 100, Q = g (x_Q cos phi + x_I sin phi), noise 0.5,
    DC 127.4 / 127.6 -> (d, 2n) uint8"""
    out = torch.empty((d, 2 * n), dtype=torch.uint8, device=dev)
    t = torch.arange(n, dtype=torch.float32, device=dev)
    cs, sn = math.cos(math.radians(PHASE_DEG)), math.sin(math.radians(PHASE_DEG))
    for lo in range(0, d, 32):
        k = min(32, d - lo)
        ph = 0.7 * t[None, :] + 6.2831853 * torch.rand((k, 1), generator=gen, device=dev)
        xi, xq = 100.0 * torch.cos(ph), 100.0 * torch.sin(ph)
        x = torch.stack([xi + 127.4, GAIN * (xq * cs + xi * sn) + 127.6], dim=2)
        x = x + 0.5 * torch.randn(x.shape, generator=gen, device=dev)
        out[lo:lo + k] = torch.clamp(torch.floor(x + 0.5), 0, 255).to(torch.uint8).reshape(k, 2 * n)
    return out


def worker(args):
    import torch
    import gsmcal

    d = dict(WORKLOADS)[args.worker]
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    ctx = gsmcal.Context(0, stream=stream.cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261020)
    bufs = [cw_bytes(torch, d, N, gen, dev) for _ in range(NBUF)]
    table = torch.empty((d, gsmcal.IQ_COLS), dtype=torch.float64, device=dev)
    summ = torch.empty((d, gsmcal.CW_COLS), dtype=torch.float64, device=dev)

    def iq(i):
        gsmcal.iq_imbalance_batch_dev(bufs[i % NBUF].data_ptr(), d, N, table.data_ptr(), ctx=ctx)

    def yardstick(i):
        gsmcal.cw_check_batch_dev(bufs[i % NBUF].data_ptr(), d, N, THR, summ.data_ptr(), None, 0, ctx=ctx)

    def timed(call):
        for i in range(args.warmup):
            call(i)
        torch.cuda.synchronize()
        ms = []
        for rep in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for i in range(args.steps):
                call(args.warmup + rep * args.steps + i)
            e1.record(stream)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.steps)
        return {"ms_per_call": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}

    nbytes = d * 2 * N
    rec = {"captures": d, "samples": N, "raw_bytes": nbytes, "buffers_in_rotation": NBUF, "steps": args.steps, "repeats": args.repeats}
    rec["yardstick_before"] = timed(yardstick)
    rec["iq_imbalance"] = timed(iq)
    rec["yardstick_after"] = timed(yardstick)
    y = min(rec["yardstick_before"]["ms_per_call"], rec["yardstick_after"]["ms_per_call"])
    med = rec["iq_imbalance"]["ms_per_call"]
    rec["yardstick_ms_per_call"] = y
    rec["iq_imbalance"]["TB_per_s"] = round(nbytes / (med * 1e-3) / 1e12, 3)
    rec["iq_imbalance"]["share_of_readme_rate"] = round(nbytes / (med * 1e-3) / 1e12 / README_TBPS[0], 3)
    rec["yardstick_over_iq_imbalance"] = round(y / med, 2)
    rec["expectation_met"] = bool(med <= y)
    # what the call measured on the first capture of the last buffer it saw
    row = gsmcal.iq_rows(table[:1].cpu().numpy())[0]
    rec["first_capture"] = {k: row[k] for k in ("gain", "phase_deg", "irr_db", "level_dbfs", "clip_I", "clip_Q", "status")}
    rec["gpu"] = torch.cuda.get_device_name(0)
    with open(args.part, "w") as f:
        json.dump(rec, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", default="")
    ap.add_argument("--limit", type=int, default=240, help="seconds per workload (timeout -k 10)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iq_imbalance_bench.json"))
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--part", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    only = set(args.only.split(",")) if args.only else None
    rec = {"tool": "iq_imbalance_bench", "warmup": args.warmup, "planted": {"gain": GAIN, "phase_deg": PHASE_DEG},
           "yardstick": "gsmcal_cw_check_batch_dev, summary only, same buffers; the lower of the medians before and after",
           "readme_streaming_TB_per_s": list(README_TBPS), "workloads": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name, _ in WORKLOADS:
            if only is not None and name not in only:
                continue
            part = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker", name,
                   "--part", part, "--steps", str(args.steps), "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
            rc = subprocess.run(cmd, cwd=ROOT).returncode
            if rc != 0:
                print("[iq_imbalance_bench] %s ended with status %d: stopping here (nothing further is started)" % (name, rc), file=sys.stderr)
                return rc
            with open(part) as f:
                w = json.load(f)
            rec["gpu"] = w.pop("gpu")
            rec["workloads"][name] = w
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
