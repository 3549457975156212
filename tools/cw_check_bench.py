#!/usr/bin/env python3
"""CW sample-loss check on one GPU (gsmcal_cw_check_batch_dev) -> profiles/cw_check_bench.json and one JSON line.

Workloads: D = 2 (check_CW_samples_loss_tcp.m's own two dongles), D = 64 and D = 1 024 captures of 409 600 samples
(4*num_frame*fread_len/2), each summary only and with r written.  Per workload: ms per call from device events after warm-up
(median and min-max over --repeats timed loops of --steps calls), the share of 8 TB/s counted on ALGORITHMIC bytes (2 B/sample
read once, + 8 B/sample when r is written; the second pass's re-read is not counted) and the share of the fp64 vector rate
(78.6 TFLOP/s = 39.3e12 lane-instructions/s) counted on the fp64 instructions the two tile loops execute per ratio (FP64_INSTR:
counted in the gfx950 ISA; a division is ~12 of them, a ratio has three, the angle one more).  Input: seeded CW captures
(tone + noise + DC, made on the device) in distinct buffers that together exceed 512 MB, rotated call by call, so no call
starts with its bytes in the 256 MiB Infinity Cache.

For comparison, in the same session, the same result from what the library offered before: raw2iq (gsmcal_raw2iq_u8, host
pointers: 2 B/sample up, 16 B/sample back) + the torch expression of CW_check.m on the device -- timed for D = 2 and D = 64
(D = 1 024 would move 6.7 GB through the host per call: left out) -- and, as the most favourable form of that, raw2iq written
in torch on the device (16 B/sample to HBM) + the same expression, for every D.

Every workload runs in a process of its own under `timeout -k 10`; the first one that fails ends the run and nothing further
is started.

    python tools/cw_check_bench.py [--steps 10] [--warmup 3] [--repeats 5] [--only d64_summary,...] [--out profiles/cw_check_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 409600
THR = 0.2
HBM, FP64_LANE_RATE = 8.0e12, 78.6e12 / 2
FP64_INSTR = {"k_cw_ratio_sum": 52, "k_cw_residual": 110}      # fp64 VALU instructions per ratio in the tile loops (static count in the gfx950 ISA)
WORKLOADS = [("d2", 2), ("d64", 64), ("d1024", 1024)]
NAMES = [w + k for w, _ in WORKLOADS for k in ("_summary", "_with_r", "_torch_device")] + ["d2_raw2iq_torch", "d64_raw2iq_torch"]
LIMIT = {"d1024_torch_device": 300}


def cw_bytes(torch, d, n, gen, dev):
    """d seeded CW captures on the device: tone of 0.7 rad/sample, amplitude 100, noise 0.5, DC 127.4 / 127.6 -> (d, 2n) uint8"""
    out = torch.empty((d, 2 * n), dtype=torch.uint8, device=dev)
    t = torch.arange(n, dtype=torch.float32, device=dev)
    for lo in range(0, d, 64):
        k = min(64, d - lo)
        ph = 0.7 * t[None, :] + 6.2831853 * torch.rand((k, 1), generator=gen, device=dev)
        x = torch.stack([100.0 * torch.cos(ph) + 127.4, 100.0 * torch.sin(ph) + 127.6], dim=2)
        x = x + 0.5 * torch.randn(x.shape, generator=gen, device=dev)
        out[lo:lo + k] = torch.clamp(torch.floor(x + 0.5), 0, 255).to(torch.uint8).reshape(k, 2 * n)
    return out


def torch_cw(torch, s, thr):
    """CW_check.m:6-8 on a (D, N) complex tensor + the count a summary row holds"""
    q = s[:, 1:] / s[:, :-1]
    pr = torch.angle(q.mean(dim=1, keepdim=True))
    r = torch.angle(q) - pr
    return r, (r.abs() > thr).sum(dim=1)


def worker(args):
    import torch
    import gsmcal

    name = args.worker
    d = dict(WORKLOADS)[name.split("_")[0]]
    kind = name.split("_", 1)[1]
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    ctx = gsmcal.Context(0, stream=stream.cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261019)
    nbytes = d * 2 * N
    nbuf = max(2, -(-512_000_000 // nbytes) + 1)
    bufs = [cw_bytes(torch, d, N, gen, dev) for _ in range(nbuf)]
    steps, repeats = args.steps, args.repeats
    rec = {"captures": d, "samples": N, "raw_bytes": nbytes, "buffers_in_rotation": nbuf}
    if kind in ("summary", "with_r"):
        summ = torch.empty((d, gsmcal.CW_COLS), dtype=torch.float64, device=dev)
        r = torch.empty((d, N - 1), dtype=torch.float64, device=dev) if kind == "with_r" else None

        def call(i):
            gsmcal.cw_check_batch_dev(bufs[i % nbuf].data_ptr(), d, N, THR, summ.data_ptr(), r.data_ptr() if r is not None else None,
                                      N - 1, ctx=ctx)
        alg = d * N * (2 + (8 if r is not None else 0))
        rec["algorithmic_bytes"] = alg
        rec["fp64_lane_instructions"] = d * (N - 1) * sum(FP64_INSTR.values())
    elif kind == "torch_device":
        def call(i):
            x = bufs[i % nbuf].view(d, N, 2).to(torch.float64)
            m = x.sum(dim=1, keepdim=True) / N
            x = x - m
            torch_cw(torch, torch.complex(x[:, :, 0], x[:, :, 1]), THR)
    else:                                                       # raw2iq through the library (host pointers) + torch
        hosts = [b.cpu().numpy() for b in bufs[:2]]
        steps, repeats = 2, 3

        def call(i):
            s = gsmcal.raw2iq(hosts[i % 2].T, ctx=ctx)
            torch_cw(torch, torch.from_numpy(np.ascontiguousarray(s.T)).to(dev), THR)
    for i in range(args.warmup):
        call(i)
    torch.cuda.synchronize()
    ms = []
    for rep in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(steps):
            call(args.warmup + rep * steps + i)
        e1.record(stream)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    med = float(np.median(ms))
    rec.update({"ms_per_call": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "steps": steps, "repeats": repeats})
    if "algorithmic_bytes" in rec:
        rec["share_of_8TBps"] = round(rec["algorithmic_bytes"] / (med * 1e-3) / HBM, 4)
        rec["share_of_fp64_rate"] = round(rec["fp64_lane_instructions"] / (med * 1e-3) / FP64_LANE_RATE, 4)
        rec["bound_by"] = "fp64" if rec["share_of_fp64_rate"] > rec["share_of_8TBps"] else "bandwidth"
        # the same capture through the torch expression: how far apart the two are (reordered fp64 sums: last bits)
        call(0)
        torch.cuda.synchronize()
        x = bufs[0][:1].view(1, N, 2).to(torch.float64)
        x = x - x.sum(dim=1, keepdim=True) / N
        rt, cnt = torch_cw(torch, torch.complex(x[:, :, 0], x[:, :, 1]), THR)
        row = summ[0].cpu().numpy()
        rec["count_first_capture"] = [int(row[1]), int(cnt[0])]
        if r is not None:
            rec["max_abs_dev_from_torch_first_capture"] = float((r[0] - rt[0]).abs().max())
    rec["gpu"] = torch.cuda.get_device_name(0)
    with open(args.part, "w") as f:
        json.dump(rec, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--limit", type=int, default=180, help="seconds per workload (timeout -k 10)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cw_check_bench.json"))
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--part", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    only = set(args.only.split(",")) if args.only else None
    rec = {"tool": "cw_check_bench", "thr": THR, "warmup": args.warmup, "fp64_instructions_per_ratio": FP64_INSTR,
           "cache": "seeded CW captures, distinct buffers rotated per call, > 512 MB in rotation", "workloads": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name in NAMES:
            if only is not None and name not in only:
                continue
            part = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(LIMIT.get(name, args.limit)), sys.executable, os.path.abspath(__file__), "--worker", name,
                   "--part", part, "--steps", str(args.steps), "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
            rc = subprocess.run(cmd, cwd=ROOT).returncode
            if rc != 0:
                print("[cw_check_bench] %s ended with status %d: stopping here (nothing further is started)" % (name, rc), file=sys.stderr)
                return rc
            with open(part) as f:
                w = json.load(f)
            rec["gpu"] = w.pop("gpu")
            rec["workloads"][name] = w
    for w, _ in WORKLOADS:                                      # how the new path compares with the forms it replaces
        a = rec["workloads"].get(w + "_summary")
        for other in ("_torch_device", "_raw2iq_torch"):
            b = rec["workloads"].get(w + other)
            if a and b:
                a["speedup_over" + other] = round(b["ms_per_call"] / a["ms_per_call"], 2)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
