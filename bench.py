#!/usr/bin/env python3
"""bench.py -- IQ Msample/s through the FCCH+SCH calibration chain on MI355X.

One step = one pass of the whole per-dongle body of gsm_sync_demod.m:107-124 (raw2iq -> channel filter ->
FCCH_coarse_position -> FCCH_fine_correction -> SCH_corr_rate_correction -> carrier_correct_post_SCH ->
total_ppm_calculation) over D synthetic dongle streams per GPU that are already resident in HBM, ending with the
calibration table ON THE HOST (an asynchronous device-to-host copy of the 80 B/stream table inside the step) and, for
N > 1, one RCCL all-gather of that table across ranks.  Msample/s = complex input samples of all ranks / wall time
(SURVEY.md 8d).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--streams D] [--mode table|stream] [--scaling weak|strong]
                    [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times the K steps, writes the last step's outputs if
--dump-outputs is given and prints the line.  With --full the run (N = 1) also times, inside the same process, the other
BASELINE configurations as sub-results: config 2 (two streams), the same 64 streams with the corrected stream written
(18 B/sample) and the scanner path at 200 and 12 800 captures (configs 3 / 5 per GPU); it also checks rows against the
CPU oracle, times the variants of the headline loop, runs the kernel event passes and the CPU baselines, and reports
the rooflines.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("OMP_NUM_THREADS", "1")
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP64_VECTOR_PEAK_TFLOPS = 78.6   # MI355X vector fp64: 256 CUs x 4 SIMDs x 16 lanes x 2 flop x 2.4 GHz (dense; the matrix pipe has the same fp64 peak)
VALU_ISSUE_PEAK = 256 * 4 * 2.4e9 / 4.0    # wave-level VALU instructions per second: one per SIMD every 4 cycles, whatever the type


def _newest_profile(suffix):
    """profiles/rNN_<suffix> of the latest round that committed one"""
    import glob
    c = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_" + suffix)))
    return c[-1] if c else os.path.join(ROOT, "profiles", "r03_" + suffix)


PMC_FILE = _newest_profile("pmc_traffic.json")      # HBM bytes per launch from committed rocprofv3 --pmc passes
VALU_FILE = _newest_profile("valu_per_step.json")   # wave-level VALU instructions per step from committed SQ passes
STATS_FILE = PMC_FILE.replace("pmc_traffic.json", "kernel_stats.csv")                       # rocprofv3 --kernel-trace --stats of the headline loop
STATS_ISO_FILE = PMC_FILE.replace("pmc_traffic.json", "kernel_stats_one_call_at_a_time.csv")  # ... of the same loop fenced behind every step


def useful_flop_per_stream(n_samples, ntaps, n_windows=10, mode="table"):
    """Useful fp64 floating-point operations of ONE stream through the chain: the arithmetic the algorithm as implemented needs
    (a complex MAC = 8, a real-coefficient complex MAC = 4 flop), without address arithmetic, conversions, reductions' shuffles or
    anything re-computed for convenience.  Itemised so that DESIGN.md can be checked against it."""
    nd = (n_samples + 63) // 64
    f = {}
    f["front_fir_kept_rows"] = nd * ntaps * 4                                   # filter() at the rows r(1:64:end) only
    f["coarse_window_spectra"] = (3594 - 15) * (5 * 16 * 4 + 16 * 3 + 40)         # 16-point FFT + powers + SNR per moving-search window
    f["fine_window_build"] = n_windows * 2208 * ntaps * 4                       # filter() on the 2208 samples of each fine window
    f["fine_certificate"] = n_windows * (8 * 2208 * 8 + 16 * 8 * 37 * 8 + 8 * 1024 * 11 + 2208 * 6 + 1025 * 12)   # level-1 sums, anchors, slides, E(t), bounds
    per_burst = 1184 * 6 + 7 * 1184 * 8 + 1184 * 40                             # lerp, 7 candidate bins, unit-phasor step
    gate = 19 * 32 * 18 * 4 + 110 * 32 * 8 + 1184 * 16                          # rotation + 37 x 32 transform on the gate's 110 bins
    f["burst_estimates"] = n_windows * (2 * per_burst + gate + 1184 * 14)       # FCCH_fine_correction + carrier_correct_post_SCH bursts (+ the level-2/3 chain of the second)
    f["sch_correlation"] = n_windows * (600 * ntaps * 4 + 600 * 20 + 89 * 512 * 8)   # window through the chain + 89 x 512 complex MACs
    if mode == "stream":
        f["corrected_stream"] = n_samples * (ntaps * 4 + 2 * (6 + 8))           # filter() at every sample + two lerps + two derotations
    return f


def compute_roofline(regime, streams, n_samples, ntaps, seconds_per_step, mode="table"):
    """The compute side of the roofline for one regime of the chain: useful fp64 FLOP per step against the
    78.6 TFLOP/s vector peak, and VALU issue utilisation = wave-level VALU instructions per step (committed SQ pass) over
    what the 1024 SIMDs can issue in the measured step time."""
    items = useful_flop_per_stream(n_samples, ntaps, mode=mode)
    flop = float(sum(items.values())) * streams
    out = {"useful_fp64_flop": int(flop), "achieved_TFLOPs": round(flop / seconds_per_step / 1e12, 3),
           "peak_TFLOPs": FP64_VECTOR_PEAK_TFLOPS, "frac_of_78.6TF": round(flop / seconds_per_step / 1e12 / FP64_VECTOR_PEAK_TFLOPS, 4),
           "valu_issue_util": None}
    try:
        with open(VALU_FILE) as fh:
            vf = json.load(fh)
        v = vf.get(regime)
        ok, note = _profile_is_current(vf)
        if v and not ok:
            out["valu_source"] = note
        elif v:
            n = float(v["valu_wave_instr_per_step"])
            out["valu_wave_instr_per_step"] = int(n)
            out["valu_issue_util"] = round(n / VALU_ISSUE_PEAK / seconds_per_step, 4)
            out["valu_per_useful_flop_lane"] = round(n * 64 / flop, 3)
            out["valu_source"] = os.path.relpath(VALU_FILE, ROOT) + f" (committed rocprofv3 SQ pass of this configuration; {note}; not measured in this run)"
    except (OSError, ValueError, KeyError):
        pass
    return out


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prewarm-steps", type=int, default=256,
                    help="untimed steps before the --warmup steps (clock / power state of a GPU that idled during the host-side set-up); reported in the line")
    ap.add_argument("--streams", type=int, default=64,
                    help="dongle streams: per GPU with --scaling weak (default), in total with --scaling strong")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak: --streams per GPU (64/GPU: the driver's curve); strong: BASELINE config 4 as stated -- "
                         "--streams in total, sharded block-contiguously over the ranks (64 -> 8 per GPU on 8 GPUs)")
    ap.add_argument("--frames", type=int, default=102, help="TDMA frames per stream (gsm_sync_demod.m:23)")
    ap.add_argument("--distinct", type=int, default=64, help="distinct synthetic streams per GPU (tiled to --streams when fewer)")
    ap.add_argument("--mode", choices=["table", "stream"], default="table",
                    help="table: ppm table + pos_info only (2 B/sample); stream: also write r_correct (18 B/sample)")
    ap.add_argument("--workload", choices=["calib", "scan"], default="calib",
                    help="calib: full FCCH+SCH chain (headline); scan: scanner path of multi_rtl_sdr_gsm_FCCH_scanner.m "
                         "(front end + FCCH_coarse_position + acceptance; use --frames 64 --streams 200)")
    ap.add_argument("--pipeline-depth", type=int, default=4,
                    help="gsmcal_ctx_set_pipeline_depth for the headline loop: consecutive steps in flight inside ONE context, each the "
                         "same full chain on its own internal stream, workspace and output set (default 4 = the device's hardware queues; "
                         "the K steps are timed from the first launch to the host's fence behind the last).  1 = one step at a time: "
                         "reported beside the headline as ms_per_step_depth1")
    ap.add_argument("--raw-buffers", type=int, default=4,
                    help="device copies of the raw batch the headline loop takes in turn (4 x 130 MB > the 256 MB Infinity Cache: every "
                         "raw byte comes from HBM proper, SURVEY 8d); 1 = re-read one buffer (reported as ms_per_step_llc_resident)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="budget for the CPU-oracle baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--one-in-flight", action="store_true",
                    help="profiler passes: the headline loop's kernels (the depth it is set to) but the host fences behind every step, so that "
                         "rocprofv3's per-kernel averages are those of a kernel that has the GPU to itself (tools/profile.sh); marked in the line")
    ap.add_argument("--no-kernel-events", action="store_true", help="skip the untimed HIP-event passes (roofline kernel figure, breakdown)")
    ap.add_argument("--no-sub", action="store_true", help="skip the sub-results (config 2, stream mode, scanner path)")
    ap.add_argument("--cache-streams", default=None,
                    help="keep the generated synthetic streams in this .npy file and reuse them (profiling passes that rerun the "
                         "same command; generation is deterministic, the file only saves the host time)")
    ap.add_argument("--full", action="store_true",
                    help="also everything beyond the headline figure: the pre-warm-less figure, the depth-1 / sustained / one-buffer "
                         "variants, the oracle and all-gather checks, the kernel event passes, rooflines, sub-results and CPU "
                         "baselines (each still subject to --no-kernel-events / --no-sub / --no-cpu-baseline)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float64; a fixed "
                         "sample of r_correct in stream mode, and of the streams past 64 MB in all)")
    return ap.parse_args()


# ------------------------------------------------------------------------------------------------------------------
def _gen_one(job):
    dongle, frames, kw = job
    from gsmcal import synth
    return synth.make_stream(dongle=dongle, num_frames=frames, **kw)[0]


def gen_streams(jobs):
    """Synthetic captures for `jobs` = [(dongle, frames, kwargs)], one worker process per host core, at most 16 (0.5 s of
    NumPy per stream).  Called BEFORE this process touches the GPU: the workers are forked from a process without HIP state."""
    ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    world = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1"))))
    workers = max(1, min(ncpu // world, 16, len(jobs)))      # under torchrun every rank of the node generates at the same time
    if workers == 1:
        return [_gen_one(j) for j in jobs]
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(_gen_one, jobs, chunksize=1))


def mixed_kwargs(n, seed):
    """The widened distribution of tests/sweep_parity.py: every 5th stream at 5-15 dB, every 7th with up to +-300 ppm of
    sampling error, every 11th without a BCCH carrier, every 13th with up to +-60 ppm of carrier error."""
    rng = np.random.default_rng(seed)
    kws = []
    for i in range(n):
        kw = {}
        if i % 5 == 1:
            kw["snr_db"] = float(rng.uniform(5, 15))
        if i % 7 == 2:
            kw["sampling_ppm"] = float(rng.uniform(-300, 300))
        if i % 11 == 3:
            kw["bcch"] = False
        if i % 13 == 4:
            kw["carrier_ppm"] = float(rng.uniform(-60, 60))
        kws.append(kw)
    return kws


# ------------------------------------------------------------------------------------------------------------------
class Calib:
    """D streams resident in HBM + everything one calibration step needs."""

    def __init__(self, torch, gsmcal, dev, ctx, raw_t, N, mode, coef, ts, fc, zero_copy=True, nbuf=2, nraw=1):
        # zero_copy: the library's last kernel stores the table straight into pinned host memory (the C ABI takes any
        # device-accessible pointer for its outputs), so the step ends with the table on the host and no copy is queued;
        # off for the RCCL path, whose all-gather reads the table from device memory
        self.zero_copy = zero_copy
        self.torch, self.g, self.dev, self.ctx = torch, gsmcal, dev, ctx
        self.raw_t, self.N, self.D = raw_t, N, raw_t.shape[0]
        self.coef, self.ts = coef, ts
        self.cf = np.full(self.D, fc)
        D = self.D
        # nbuf output sets (table, pos_info, r_len): consecutive steps of a pipelined loop write distinct ones; nraw device copies
        # of the raw batch taken in turn (the headline: more bytes than the Infinity Cache holds)
        self.nbuf = nbuf
        self.table_t = [torch.zeros((D, gsmcal.TABLE_COLS), dtype=torch.float64, device=dev) for _ in range(nbuf)]
        self.pos_ts = [torch.zeros((D, 2, gsmcal.MAX_POS_ROWS), dtype=torch.float64, device=dev) for _ in range(nbuf)]
        self.rlen_ts = [torch.zeros((D,), dtype=torch.int64, device=dev) for _ in range(nbuf)]
        self.pos_t, self.rlen_t = self.pos_ts[0], self.rlen_ts[0]
        self.r_ts = [torch.empty((D, N, 2), dtype=torch.float64, device=dev) for _ in range(nbuf)] if mode == "stream" else None
        self.r_t = self.r_ts[0] if self.r_ts else None
        self.host_table = [torch.zeros((D, gsmcal.TABLE_COLS), dtype=torch.float64).pin_memory() for _ in range(nbuf)]
        self.raws = [raw_t] + [raw_t.clone() for _ in range(nraw - 1)]
        dp = gsmcal._lib.c_double_p
        self._p = (coef.ctypes.data_as(dp), ts.ctypes.data_as(dp), self.cf.ctypes.data_as(dp))

    def launch(self, b=0, d=None, r=0):
        """enqueue one calibration pass over the first d streams of raw buffer r into output set b"""
        ctx, lib = self.ctx, self.ctx.lib
        cp, tp, fp = self._p
        rc = lib.gsmcal_calibrate_batch_dev(ctx.h, C.c_void_p(self.raws[r].data_ptr()), self.D if d is None else d, self.N,
                                            cp, len(self.coef), tp, len(self.ts), fp,
                                            C.c_void_p((self.host_table[b] if self.zero_copy else self.table_t[b]).data_ptr()),
                                            C.c_void_p(self.pos_ts[b].data_ptr()),
                                            C.c_void_p(self.r_ts[b].data_ptr()) if self.r_ts is not None else None,
                                            C.c_void_p(self.rlen_ts[b].data_ptr()))
        ctx.check(rc, "gsmcal_calibrate_batch_dev")

    def to_host(self, b=0):
        """the step ends with the table on the host: already there (zero_copy), else an asynchronous copy on the same
        stream into the pinned destination"""
        if not self.zero_copy:
            self.host_table[b].copy_(self.table_t[b], non_blocking=True)

    def table(self, b=0):
        """the table of buffer b as a host tensor (after a synchronize)"""
        return self.host_table[b] if self.zero_copy else self.table_t[b].cpu()


SUB_PREWARM_S = 0.06       # sub-results (single rank): the same step repeated for this long before their warm-up steps -- see --prewarm-steps


def time_steps(torch, dev, fn, steps, warmup, fence=None, prewarm_s=0.0):
    fence = fence or (lambda: torch.cuda.synchronize(dev))
    if prewarm_s > 0.0:                                     # (clock / power state: a sub-result starts after host-side work too)
        t_end = time.perf_counter() + prewarm_s
        while time.perf_counter() < t_end:
            for _ in range(4):
                fn()
            fence()
    for _ in range(warmup):
        fn()
    fence()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    fence()
    return time.perf_counter() - t0


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: start one rank per GPU as CHILDREN of this process (which has not
    touched the GPU and never will -- no exec of a GPU-initialised process anywhere), relay rank 0's JSON line and exit
    with the launcher's code.  The torch.distributed.run form the driver uses keeps working: it sets RANK, so this is
    skipped."""
    import socket
    import subprocess
    with socket.socket() as s:                               # a free rendezvous port on the loopback
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in p.stdout:
        s_ = ln.strip()
        if s_.startswith("{") and '"metric"' in s_:
            line = s_                                        # rank 0's result: printed once, below
        else:
            sys.stderr.write(ln)
    rc = p.wait()
    if line and rc == 0:
        print(line)
        sys.stdout.flush()
    elif rc == 0:
        sys.stderr.write("bench.py: the ranks exited without a result line\n")
        rc = 1
    raise SystemExit(rc)


def main():
    args = parse()
    if (args.gpus > 1 or os.environ.get("GSMCAL_FORCE_DIST") == "1") and "RANK" not in os.environ:
        self_launch(args)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s)")
    import gsmcal
    from gsmcal import dist as gdist
    from gsmcal import synth

    # ---- synthetic input, made on the host cores before this process touches the GPU ----
    frames = args.frames
    N = frames * synth.FRAME_OV
    if args.scaling == "strong":
        total_units = args.streams
        lo, hi = gdist.shard_range(total_units, world, rank)
    else:
        total_units = args.streams * world
        lo, hi = rank * args.streams, (rank + 1) * args.streams
    D = hi - lo
    if D < 1:
        raise SystemExit("more ranks than streams")
    nd = max(1, min(args.distinct, D))
    cand_jobs, cand_raw, mixed_raw = [], [], None
    if args.workload == "calib":
        ncand = nd + nd // 3 + 8                             # about one synthetic seed in eight is rejected by the fine search
        cand_jobs = [(100000 * rank + lo + i, frames, {}) for i in range(ncand)]
        jobs = list(cand_jobs)
        n_mixed = 64 if (args.full and world == 1 and not args.no_sub and args.mode == "table") else 0
        jobs += [(5000 + i, frames, kw) for i, kw in enumerate(mixed_kwargs(n_mixed, 5000))]
        cache = args.cache_streams and f"{args.cache_streams}.r{rank}.n{len(jobs)}.f{frames}.npy"
        if cache and os.path.exists(cache):
            raws = list(np.load(cache))
        else:
            raws = gen_streams(jobs)
            if cache:
                np.save(cache, np.stack(raws))
        cand_raw = raws[:ncand]
        mixed_raw = np.stack(raws[ncand:]) if n_mixed else None

    import torch
    import torch.distributed as dist

    ndev = torch.cuda.device_count()                         # (counting devices does not initialise the GPU)
    if ndev < world or local_rank >= ndev:
        raise SystemExit(f"bench.py: --gpus {world} needs {world} devices, this node exposes {ndev} "
                         "(one process per GPU; GSMCAL_FORCE_DIST=1 with --gpus 1 exercises the RCCL path on one device)")

    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # one process per GPU; the collective runs whenever a process group exists (GSMCAL_FORCE_DIST=1 lets a
    # single-rank torchrun exercise the RCCL path on a 1-GPU box)
    use_dist = world > 1 or (os.environ.get("GSMCAL_FORCE_DIST") == "1" and "RANK" in os.environ)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    if args.workload == "scan":
        return bench_scan_main(args, rank, world, dev, use_dist)
    fc = 957.4e6                                            # gsm_sync_demod.m:14
    coef = np.ascontiguousarray(synth.fir1(46, 200e3 / synth.FS))   # gsm_sync_demod.m:34
    ts = np.ascontiguousarray(synth.sch_training_sequence())
    # units of this rank: weak scaling = --streams per GPU; strong = --streams in total, block-contiguous shards
    sizes = gdist.shard_sizes(total_units, world) if args.scaling == "strong" else [args.streams] * world
    Dmax = max(sizes)

    # ---- resident in HBM before the timed region (unit u = global stream index) ----
    # The reference's fine search rejects streams whose FCCH tone falls between two FFT bins (about one synthetic stream in
    # eight: tests/test_oracle_cpu.py::test_fine_search_rejection_rate_on_bin_vs_half_bin); such a stream leaves the chain
    # after the fine search and would make the step cheaper than a calibrated one.  The headline batch therefore takes the
    # first `nd` seeds of its range that the chain calibrates (status 0), so every stream does the full work; the
    # unselected distribution (low SNR, large ppm, carriers without a BCCH) is timed as sub_results.mixed_batch.
    stream0 = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream0):
        ctx0 = gsmcal.Context(local_rank, stream=stream0.cuda_stream)
        picked, skipped, cand = [], [], 0
        while len(picked) < nd and cand < 8 * nd + 64:
            if cand >= len(cand_raw):                        # (rare) the first draw held too many rejected seeds
                more = [(100000 * rank + lo + cand + i, frames, {}) for i in range(16)]
                cand_raw += [_gen_one(jb) for jb in more]
            hi_c = min(len(cand_raw), cand + 64)
            res = gsmcal.calibrate_batch(np.stack(cand_raw[cand:hi_c]), coef, ts, fc, ctx=ctx0)
            for i in range(hi_c - cand):
                if res["table"][i, 9] == 0 and len(picked) < nd:
                    picked.append(cand_raw[cand + i])
                elif res["table"][i, 9] != 0:
                    skipped.append(cand + i)
            cand = hi_c
        ctx0.close()
    if len(picked) < nd:
        raise SystemExit("could not find enough calibratable synthetic streams")
    distinct = np.stack(picked)
    del cand_raw
    raw_t = torch.from_numpy(distinct).to(dev).repeat(((D + nd - 1) // nd, 1))[:D].contiguous()   # tiled on the device when nd < D

    # a dedicated (non-default) stream: the library forks its internal lanes off this stream, and torch's copies and
    # collectives are enqueued on it too, so one synchronize covers the whole step
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx = gsmcal.Context(local_rank, stream=stream.cuda_stream)
    NBUF = max(4, min(8, args.pipeline_depth))          # output sets taken in turn: at least as many as steps may be in flight
    nraw = max(1, args.raw_buffers)
    cal = Calib(torch, gsmcal, dev, ctx, raw_t, N, args.mode, coef, ts, fc, zero_copy=not use_dist, nbuf=NBUF, nraw=nraw)

    # The all-gather of step i overlaps the kernels of step i+1: the library writes its table alternately into one of
    # two buffers (it keeps a replay graph for each), RCCL gathers from the one just written, and the only wait is
    # before a buffer is written again two steps later (gsmcal.dist.TableGatherer; uneven shards are padded).
    # N > 1: the C ABI's own all-gather, in line on the chain's stream (GSMCAL_BENCH_GATHER=async: on the library's side stream;
    # =torch: torch.distributed's collective, round 3's path) -- tools/dist_cost.py has what each costs per step on one rank
    NG = 4                                               # gather buffer pairs: as many as steps may be in flight (the async collective has four slots)
    tg, gather_kind, ncomm, gather_fallback = setup_gatherer(torch, gsmcal, gdist, ctx, dev, stream, local_rank, sizes, gsmcal.TABLE_COLS, pairs=NG) if use_dist else (None, "none", None, None)
    host_gath = [torch.zeros((sum(sizes), gsmcal.TABLE_COLS), dtype=torch.float64).pin_memory() for _ in range(NG)] if use_dist else None
    nstep = [0]
    loop = {"nraw": nraw}
    # Steps in flight inside the one context (gsmcal_ctx_set_pipeline_depth): each step is the same full chain, on output set
    # k mod 4 and raw buffer k mod nraw; step k's table is complete when step k + depth is enqueued or at the fence.  With torch's
    # collective (it runs on torch's stream, not behind the call's last stage) or uneven shards (torch pad copies) the depth stays 1.
    depth = max(1, min(8 if not use_dist else NG, args.pipeline_depth))
    if use_dist and (gather_kind == "torch" or any(sz != Dmax for sz in sizes)):
        depth = 1
    if args.mode == "stream" and "--pipeline-depth" not in " ".join(sys.argv):
        depth = 1          # (with r_correct written the stream kernel saturates both pipes: calls in flight measured 0.60-0.62 against 0.585-0.589 ms)
    ctx.set_pipeline_depth(depth)
    # (steps in flight at N > 1: the in-line collective of step k rides on step k's own internal stream, and the library chains the
    # collectives of consecutive steps by events -- one communicator never runs two of them at once; which combination of depth and
    # placement is fastest is measured below, max over ranks)

    def step():
        k = nstep[0]
        nstep[0] += 1
        b, g = k % NBUF, k % NG
        if use_dist:
            tg.wait(g)
        cal.launch(b, r=k % loop["nraw"])
        if use_dist:
            tg.post(g, cal.table_t[b])                               # one RCCL all-gather of the ppm table
        else:
            cal.to_host(b)
        if args.one_in_flight:
            ctx.sync()

    def fence():
        ctx.sync()                                                   # (joins the steps still in flight on the library's stage streams)
        if use_dist:
            for g in range(NG):
                if tg.work[g] is not None:
                    host_gath[g].copy_(tg.rows(g), non_blocking=True)   # gathered table to the host (every rank)
        torch.cuda.synchronize(dev)
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize(dev)

    # clocks and power state first: a GPU that has just been generating / selecting streams on the host side for tens of seconds is
    # idle, and W = 3 steps (0.55 ms) do not bring it to the state a service runs in -- the same step, --prewarm-steps times,
    # before the W warm-up steps of the contract (20 timed steps read 0.184 ms without this, 0.174 with it and in every longer run)
    # ... and the same W + K steps WITHOUT them first (`ms_per_step_no_prewarm`: the protocol of rounds 1-3, kept in the line so
    # that rounds stay comparable -- VERDICT r4 #2; a plain run does these steps too, so that its headline follows the
    # same earlier steps, and leaves their figure to --full)
    elapsed_cold = time_steps(torch, dev, step, args.steps, args.warmup, fence) if args.prewarm_steps > 0 else None
    for _ in range(args.prewarm_steps):
        step()
    fence()
    # N > 1, native collective, no explicit choice: where the all-gather sits is decided by measurement during the warm-up -- in
    # line on the chain's stream (costs RCCL's small-message latency per step: 1.6 us on one rank, unknown over xGMI) or on the
    # library's side stream behind an event (costs ~14 us per step on one rank, hides the collective under the next step).  Both
    # timed over 40 steps, max over ranks, every rank takes the same decision.
    # Round 6: with steps in flight (depth > 1) the choice has a third candidate -- one step at a time with the collective in line, the
    # round-5 configuration: on ONE rank the collective's event traffic costs the pipelined loop more than the overlap gains (0.19-0.23
    # against 0.18 ms), over xGMI nobody has measured; whichever is fastest, max over ranks, is what the timed loop runs.
    autotune = None
    if use_dist and gather_kind == "native" and "GSMCAL_BENCH_GATHER" not in os.environ:
        cands = [f"inline_depth{depth}", f"async_depth{depth}"] + (["inline_depth1"] if depth > 1 else [])

        def configure(label):
            mode, d_ = label.split("_depth")
            fence()
            tg.reset(mode)
            ctx.set_pipeline_depth(int(d_))

        def measure(label):
            configure(label)
            return time_steps(torch, dev, step, 40, 4, fence) / 40
        autotune = gdist.autotune_choice(cands, measure, dev)
        configure(autotune["chosen"])
        mode_, d_ = autotune["chosen"].split("_depth")
        gather_kind = "native" if mode_ == "inline" else "async"
        depth = int(d_)
        nstep[0] = 0
    elapsed = time_steps(torch, dev, step, args.steps, args.warmup, fence)
    if use_dist:
        tt = torch.tensor([elapsed, elapsed_cold if elapsed_cold is not None else elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt[0].item())
        elapsed_cold = float(tt[1].item()) if elapsed_cold is not None else None
    last_b = (nstep[0] - 1) % NBUF
    last = (nstep[0] - 1) % NG                                       # (gather buffer pair of the last step)
    table = cal.table(last_b).numpy().copy()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, calib_outputs(torch, cal, last_b, table, host_gath[last].numpy() if use_dist else None), D)
    # every output set of the loop holds the same table: the steps in flight did not disturb each other
    tables_identical = all(bool(np.array_equal(cal.table(b).numpy(), table, equal_nan=True)) for b in range(min(NBUF, nstep[0]))) if args.full else None
    # ... and the same K steps (a) one at a time, (b) on ONE raw buffer (which the Infinity Cache then serves), single rank only
    variants = {}
    if args.full and not use_dist and args.mode == "table" and os.environ.get("GSMCAL_BENCH_NO_VARIANTS") != "1":     # (=1: profiler passes that want the headline loop last)
        def timed_variant(d_, nraw_, k_=None):
            k_ = k_ or args.steps
            ctx.set_pipeline_depth(d_)
            loop["nraw"] = nraw_
            nstep[0] = 0
            t_ = time_steps(torch, dev, step, k_, args.warmup, fence, prewarm_s=SUB_PREWARM_S)
            same_ = all(bool(np.array_equal(cal.table(b).numpy(), table, equal_nan=True)) for b in range(NBUF))
            return round(1e3 * t_ / k_, 4), same_
        if depth > 1:
            variants["ms_per_step_depth1"], s1 = timed_variant(1, nraw)          # one step at a time (fused tail), rotated input
            # the same loop over 20 x K steps between the same fences: the K-step figure carries the pipeline's fill and drain (the
            # first call starts on an idle GPU, the last runs alone), a service that keeps calling does not
            variants["ms_per_step_sustained"], s0 = timed_variant(depth, nraw, 20 * args.steps)
            tables_identical = tables_identical and s1 and s0
        if nraw > 1:
            variants["ms_per_step_llc_resident"], s2 = timed_variant(depth, 1)   # the headline's depth on ONE re-read raw buffer
            tables_identical = tables_identical and s2
            if depth > 1:
                variants["ms_per_step_llc_resident_depth1"], s3 = timed_variant(1, 1)   # the protocol of rounds 1-5
                tables_identical = tables_identical and s3
        loop["nraw"] = nraw
    ctx.set_pipeline_depth(1)                                        # everything below (checks, event passes, sub-results): one call at a time
    if args.full:
        cal.launch(last_b, r=0)
        ctx.sync()
        assert np.array_equal(cal.table(last_b).numpy(), table, equal_nan=True)

    # ---- --full: every rank checks rows of its OWN shard against the CPU oracle before anything is reported, whatever the
    # other flags (the check used to ride on the CPU-baseline leg) ----
    n_rank_checked = 0
    if args.full:
        from oracle import gsmcal_oracle as oracle
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import parity
        det = gsmcal.last_batch_details(min(D, nd), ctx=ctx)
        pos_host = cal.pos_ts[last_b].cpu().numpy()
        for i in range(min(nd, 4)):
            parity.compare_stream(oracle.calibrate_stream(distinct[i], coef, ts, fc), table[i], det, i, _pos_info(pos_host, table, i))
            n_rank_checked += 1
    gathered_ok = None
    if use_dist and args.full:
        # the collective's result, checked against what every rank says it sent: digests of the local tables travel
        # through a second, independent group (gloo over TCP), and each rank compares every peer's block of the
        # RCCL-gathered table with that peer's digest -- not only its own rows (gsmcal.dist.check_gathered_table)
        chk = dist.new_group(backend="gloo")
        gdist.check_gathered_table(host_gath[last].numpy(), table, sizes, rank, group=chk)
        assert np.array_equal(tg.own_rows(last).cpu().numpy(), table, equal_nan=True), "all-gathered table differs from this rank's rows"
        gathered_ok = True

    n_ok = int(np.sum(table[:, 9] == 0))
    total_samples = sum(sizes) * N * args.steps
    value = total_samples / elapsed / 1e6
    bps = 2 if args.mode == "table" else 18
    out = {
        "metric": "IQ Msamples/s through FCCH+SCH calib",
        "value": round(value, 3), "unit": "Msample/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 4), "prewarm_steps": args.prewarm_steps,
        **({"ms_per_step_no_prewarm": round(1e3 * (elapsed_cold if elapsed_cold is not None else elapsed) / args.steps, 4),
            "ms_per_step_no_prewarm_what": "the same W + K steps, timed FIRST (before the pre-warm steps" + (" and before the placement autotune: "
                                           "collective in line" if use_dist else "") + "); the headline follows W + K + prewarm_steps earlier steps"}
           if args.full else {}),
        "pipeline_depth": depth, **({"one_in_flight": "--one-in-flight: the host fenced behind every step (a profiler pass, not the headline)"}
                                    if args.one_in_flight else {}),
        "input": (f"rotated over {nraw} buffers ({nraw} x {D * 2 * N / 1e6:.1f} MB: beyond the 256 MB Infinity Cache, every raw byte from HBM)"
                  if nraw > 1 else "one raw buffer re-read every step (served by the Infinity Cache)"),
        **({"tables_identical": tables_identical} if args.full else {}), **variants,
        "higher_is_better": True, "scaling": args.scaling,
        "vs_baseline": None, "dtype": "f64",
        "data": f"synthetic 8x-oversampled GSM BCCH-carrier uint8 IQ (seed {synth.DEFAULT_SEED}); {nd} distinct "
                f"streams per GPU" + (f" tiled to {D}" if nd < D else "") + f" (the first {nd} seeds the chain calibrates; "
                f"{len(skipped)} rejected seeds skipped; SNR 15-30 dB -- the unselected low-SNR / large-ppm / no-BCCH mix is "
                "sub_results.mixed_batch)",
        "config": {"workload": f"cfg4 full chain gsm_sync_demod.m:107-124: {sum(sizes)} dongle streams ({Dmax}/GPU) x {N} IQ samples "
                               f"({frames} frames), fir1(46), FCCH+SCH+total_ppm_calculation, table on the host",
                   "streams_per_gpu": Dmax, "streams_total": sum(sizes), "samples_per_stream": N, "output": args.mode,
                   "bytes_per_sample_algorithmic": bps,
                   "collective": COLLECTIVE_NAMES.get(gather_kind, gather_kind),
                   "streams_calibrated_ok": n_ok, "rows_checked_vs_oracle_per_rank": n_rank_checked,
                   "gathered_table_checked_against_every_rank": gathered_ok},
    }
    if gather_fallback:
        out["config"]["collective_fallback_from_native"] = gather_fallback
    if autotune:
        out["config"]["collective_autotune"] = autotune
    if rank == 0 and args.full:
        path_gbs = value * 1e6 * bps / 1e9
        roof = {"bound": "hbm", "achieved": round(path_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(path_gbs / HBM_PEAK_GBS, 4), "traffic": None,
                "what": f"WHOLE PATH (SURVEY 8d): Msample/s x {bps} B/sample; every raw byte is read once, by the front-end "
                        "kernel; the rest of the chain works on a few KB per burst and is latency-bound (DESIGN.md 4)"}
        # ---- HIP-event passes (untimed): the same K steps again with events on every kernel ----
        if not args.no_kernel_events:
            kk = [0]

            def ev_step():                                   # one call at a time (events on every dispatch), raw buffers in turn like the headline
                cal.launch(0, r=kk[0] % nraw)
                kk[0] += 1
            ctx.set_pipeline_depth(depth)                    # (with events on every dispatch the library runs one call at a time, but the kernels of
            for _ in range(2 * nraw):                        #  the depth it is set to: the four-launch tail of the headline loop)
                ev_step()
            prof = event_pass(ctx, ev_step, args.steps, torch, dev)
            prof_llc = event_pass(ctx, lambda: cal.launch(0), args.steps, torch, dev) if nraw > 1 else None
            ctx.set_pipeline_depth(1)
            if prof:
                tot = {k: v[0] for k, v in prof.items()}
                dom = max(tot, key=tot.get)
                out["kernels_ms_per_step_untimed_pass"] = {k: round(v[0] / args.steps, 4)
                                                           for k, v in sorted(prof.items(), key=lambda kv: -kv[1][0])}
                front = [k for k in prof if k.startswith("k_front") and prof[k][1]]
                if front:
                    k = front[0]
                    tot_ms, launches = prof[k]
                    avg = tot_ms / launches
                    per_launch = D * N * 2.25 * args.steps / launches        # the batch may be split over the library's lanes
                    ach = per_launch / 1e9 / (avg * 1e-3)
                    traffic, src = pmc_traffic(k, D, N)
                    roof["kernel"] = {"name": k, "achieved": round(ach, 1), "frac": round(ach / HBM_PEAK_GBS, 4),
                                      "avg_launch_ms": round(avg, 5), "launches_per_step": launches // args.steps,
                                      "algorithmic_bytes_per_launch": int(per_launch),
                                      "share_of_step_time": round(tot[k] / sum(tot.values()), 3),
                                      "traffic": traffic, "traffic_source": src,
                                      "what": "the one HBM-streaming kernel: 2 B/sample raw read + 16/64 B/sample decimated write; "
                                              "HIP events on its own dispatch, second run of the same K steps (one call at a time, raw "
                                              f"batch rotated over {nraw} device buffers like the headline: HBM proper)"}
                    rp = rocprof_kernel_avg_ms(k, D, N)
                    if rp:
                        roof["kernel"]["rocprofv3"] = {**rp, "what": "the committed rocprofv3 --kernel-trace --stats summaries of this command (tools/"
                                                       "profile.sh, same sources): one_call_at_a_time = the loop fenced behind every step, the figure "
                                                       "avg_launch_ms above must agree with; calls_in_flight = the headline loop itself, where the "
                                                       f"kernel shares the chip with the kernels of up to {depth - 1} other calls and takes longer"}
                    if prof_llc and k in prof_llc and prof_llc[k][1]:
                        avg2 = prof_llc[k][0] / prof_llc[k][1]
                        roof["kernel"]["avg_launch_ms_llc_resident"] = round(avg2, 5)
                        roof["kernel"]["achieved_llc_resident"] = round(per_launch / 1e9 / (avg2 * 1e-3), 1)
                        roof["kernel"]["frac_llc_resident"] = round(per_launch / 1e9 / (avg2 * 1e-3) / HBM_PEAK_GBS, 4)
                roof["time_dominant_kernel"] = {"name": dom, "ms_per_step": round(tot[dom] / args.steps, 4),
                                                "bound": "latency (serial fp64 dependency chains, one to three workgroups per CU)",
                                                "note": "per-kernel times of ONE call at a time; in the headline loop the kernels of up to "
                                                        f"{depth} calls overlap, so these do not add up to ms_per_step"}
        step_traffic, step_src = pmc_step_traffic(D, N)
        roof["traffic"] = step_traffic
        roof["traffic_source"] = step_src
        roof["algorithmic_bytes_per_step"] = int(D * N * bps)
        if step_traffic:
            roof["traffic_over_algorithmic"] = round(step_traffic / (D * N * bps), 3)
        out["roofline"] = roof
        out["roofline_compute"] = compute_roofline("calib_64" if Dmax == 64 else f"calib_{Dmax}", Dmax, N, len(coef), elapsed / args.steps, args.mode)
        if world == 1 and not args.no_sub:
            out["sub_results"] = sub_results(args, torch, gsmcal, dev, ctx, cal, coef, ts, fc, N, stream, mixed_raw, distinct)
        # ---- CPU baseline: the oracle (fp64 NumPy/SciPy restatement) on the host cores, bounded sample ----
        if world == 1 and not args.no_cpu_baseline:
            done, t_cpu, checked = 0, 0.0, 0
            while t_cpu < args.cpu_seconds and done < 64:
                i = done % nd
                c0 = time.perf_counter()
                orc = oracle.calibrate_stream(distinct[i], coef, ts, fc)
                t_cpu += time.perf_counter() - c0
                done += 1
                if done <= nd:      # checker: the GPU result of this very stream must match the oracle
                    parity.compare_stream(orc, table[i], det, i, _pos_info(pos_host, table, i))
                    checked += 1
            out["cpu_baseline"] = {"value": round(done * N / t_cpu / 1e6, 4), "unit": "Msample/s", "cores": 1,
                                   "kind": "port",
                                   "sample": f"{done} streams x {N} samples through oracle.calibrate_stream "
                                             f"(NumPy/SciPy fp64 restatement, 1 thread) in {t_cpu:.1f} s"}
            out["parity_checked_streams"] = max(checked, n_rank_checked)
            out["speedup_vs_cpu_baseline"] = round(value / out["cpu_baseline"]["value"], 1)
            # the same restatement on every host core, at most 16 (one worker process per core over independent streams): SURVEY 8d
            # asks for the all-core figure next to the single-thread one
            ncpu = min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))
            if ncpu > 1:
                from concurrent.futures import ProcessPoolExecutor
                nrun = min(4 * ncpu, 1024)
                with ProcessPoolExecutor(max_workers=ncpu) as ex:
                    list(ex.map(_oracle_warm, range(2 * ncpu), chunksize=1))      # workers up and imports done, untimed
                    c0 = time.perf_counter()
                    list(ex.map(_oracle_one, [(distinct[i % nd], coef, ts, fc) for i in range(nrun)], chunksize=1))
                    t_all = time.perf_counter() - c0
                out["cpu_baseline_all_cores"] = {"value": round(nrun * N / t_all / 1e6, 4), "unit": "Msample/s", "cores": ncpu,
                                                 "kind": "port",
                                                 "sample": f"{nrun} streams over {ncpu} worker processes in {t_all:.1f} s"}
                out["speedup_vs_cpu_all_cores"] = round(value / out["cpu_baseline_all_cores"]["value"], 1)
    if rank == 0:
        if "parity_checked_streams" not in out:
            out["parity_checked_streams"] = n_rank_checked
        print(json.dumps(out))
    if use_dist:
        finish_dist(torch, dist, gdist, dev, ncomm, gather_fallback)


COLLECTIVE_NAMES = {"none": "none", "native": "all_gather(table): gsmcal_allgather_table (native RCCL) in line on the chain's stream",
                    "async": "all_gather(table): gsmcal_allgather_table_async (native RCCL on a side stream)",
                    "torch": "all_gather(table): torch.distributed over RCCL"}


def setup_gatherer(torch, gsmcal, gdist, ctx, dev, stream, local_rank, sizes, cols, pairs=2):
    """The table gatherer of an N > 1 run, for either workload (calibration table: 10 columns; scanner table: snr, num_hit).
    Which collective: decided in gsmcal.dist.choose_gatherer, identically on every rank.  The native communicator is set up
    and one CHECKED trial exchange runs on it (both buffer pairs, every peer's block compared), each under a time-out; if
    any rank fails or hangs there, ALL ranks fall back to torch.distributed's collective together and the line says so
    (the native path had only ever run on one rank).  GSMCAL_BENCH_GATHER=torch | native | async skips the choice.
    Returns (gatherer, kind, native communicator or None, fall-back reason or None)."""
    want = os.environ.get("GSMCAL_BENCH_GATHER", "native")
    holder = {}
    # the id travels through the process group HERE, on every rank alike: what follows inside make_native / verify touches no
    # torch collective, so a rank that fails or hangs there cannot put the group's collectives out of step
    uid = gdist.broadcast_unique_id(ctx, dev) if want != "torch" else None

    def make_native():
        if os.environ.get("GSMCAL_BENCH_FAIL_NATIVE") == "1":     # (test hook for the fall-back)
            raise RuntimeError("GSMCAL_BENCH_FAIL_NATIVE=1")
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            holder["comm"] = gdist.native_comm_from_process_group(ctx, dev, unique_id=uid) if uid is not None else None
            if holder["comm"] is None:
                raise RuntimeError("rank 0 could not draw an RCCL unique id")
            return gdist.NativeTableGatherer(ctx, holder["comm"], sizes, cols, dev, mode="async" if want == "async" else "inline", stream=stream, pairs=pairs)

    def verify(g):
        # BOTH placements the autotune may switch to, each on a throw-away context and stream of its own: a trial
        # exchange that hangs leaves that stream stuck and abandoned, never the chain's -- the fall-back to torch's
        # collective then still has a clean stream to run on
        with torch.cuda.device(dev):
            for m in (("async",) if want == "async" else ("inline", "async")):
                vstream = torch.cuda.Stream(device=dev)
                with torch.cuda.stream(vstream):
                    vctx = gsmcal.Context(local_rank, stream=vstream.cuda_stream)
                    vtg = gdist.NativeTableGatherer(vctx, holder["comm"], sizes, cols, dev, mode=m, stream=vstream)
                    gdist.verify_gatherer(vtg, cols, dev, lambda: vstream.synchronize())
                    vstream.synchronize()
                    vctx.close()

    tg, kind, fallback = gdist.choose_gatherer(make_native, lambda: gdist.TableGatherer(sizes, cols, dev, pairs=pairs), dev,
                                               want=want, verify=verify, timeout_s=float(os.environ.get("GSMCAL_BENCH_NATIVE_TIMEOUT_S", "90")))
    return tg, kind, (holder.get("comm") if kind != "torch" else None), fallback


def finish_dist(torch, dist, gdist, dev, ncomm, gather_fallback):
    """Tear-down of an N > 1 run, the same branch on EVERY rank: whether any rank's helper thread is still stuck inside
    an abandoned native bootstrap / trial exchange is agreed by one all-reduce; then every rank joins ONE barrier; only the
    ranks with a stuck thread leave without the tear-down (destroying the communicators under that thread aborts the process
    after all work is done and reported), the others tear down normally."""
    stuck = bool(gather_fallback and "TimeoutError" in gather_fallback)
    any_stuck = gdist.all_max(1.0 if stuck else 0.0, dev) > 0.0
    dist.barrier()
    if stuck:
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)
    if ncomm is not None:
        torch.cuda.synchronize(dev)
        ncomm.close()
    if any_stuck:
        # a peer left without destroying its end of the group: a collective tear-down would wait for it
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)
    dist.destroy_process_group()


def event_pass(ctx, fn, steps, torch, dev, filt=None):
    """K more steps with HIP events attached to every kernel dispatch.  They cannot ride in the timed region: as soon as
    one dispatch carries start/stop events this runtime switches the queue to profiled dispatch and the whole step
    slows by ~13 %."""
    ctx.profile_reset()
    ctx.profile_filter(filt)
    ctx.profile_enable(True)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize(dev)
    prof = dict(ctx.profile_get())
    ctx.profile_enable(False)
    return {k: v for k, v in prof.items() if v[1]}


def _profile_is_current(prof):
    """(ok, note): a committed counter summary describes the kernels in the tree iff the source hash tools/profile.sh recorded
    next to it equals the hash of csrc/ + include/gsmcal.h now."""
    import gsmcal
    have = prof.get("csrc_sha256")
    if have is None:
        return False, "the committed profile carries no source hash (made before round 6)"
    if have != gsmcal.build.csrc_hash():
        sys.stderr.write("bench.py: STALE PROFILE -- the committed counter passes describe other kernels than the ones in the tree; "
                         "roofline.traffic / valu_* are withheld (run tools/profile.sh)\n")
        return False, "STALE: the committed counter passes were taken on other kernel sources than the ones in the tree"
    return True, f"kernels at commit {prof.get('git_commit', '?')}, source hash {have[:12]}"


def pmc_traffic(kernel, D, N):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC passes (separate --pmc FETCH_SIZE / WRITE_SIZE
    runs of this command; FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes).  NOT measured in this run."""
    if not os.path.exists(PMC_FILE):
        return None, "no committed PMC pass for this configuration"
    with open(PMC_FILE) as f:
        pmc = json.load(f)
    if pmc.get("streams_per_gpu") != D or pmc.get("samples_per_stream") != N:
        return None, "committed PMC pass is for another batch shape"
    ok, note = _profile_is_current(pmc)
    if not ok:
        return None, note
    for k, v in pmc.get("hbm_bytes_per_launch", {}).items():
        if k.startswith(kernel[:12]):
            return v, os.path.relpath(PMC_FILE, ROOT) + f" (rocprofv3 --pmc passes of this command, committed; {note}; not measured in this run)"
    return None, "kernel not in the committed PMC pass"


def rocprof_kernel_avg_ms(kernel, D, N):
    """Average duration of `kernel` in the two committed rocprofv3 --kernel-trace --stats summaries of this command (tools/profile.sh):
    the headline loop as it runs (calls in flight: the kernel shares the chip with the other calls' kernels) and the same loop with the
    host fencing behind every step (--one-in-flight: the kernel alone, what the HIP-event pass of this run measures).  NOT measured in
    this run; None unless the summaries were taken with the counter passes whose source hash matches the tree."""
    import csv
    out = {}
    if not os.path.exists(PMC_FILE):
        return out
    with open(PMC_FILE) as f:
        pmc = json.load(f)
    if pmc.get("streams_per_gpu") != D or pmc.get("samples_per_stream") != N or not _profile_is_current(pmc)[0]:
        return out
    stem = kernel.split("_sym")[0].rstrip("0123456789")         # "k_front_fast47_sym" -> "k_front_fast" (rocprofv3 prints "k_front_fast<47, true>")
    for key, fn in (("calls_in_flight", STATS_FILE), ("one_call_at_a_time", STATS_ISO_FILE)):
        if not os.path.exists(fn):
            continue
        with open(fn) as f:
            for row in csv.DictReader(f):
                if row["Name"].startswith(stem + "<"):
                    out[key] = {"avg_launch_ms": round(float(row["AverageNs"]) / 1e6, 5), "calls": int(row["Calls"]),
                                "file": os.path.relpath(fn, ROOT)}
                    break
    return out


def pmc_step_traffic(D, N):
    """HBM bytes per STEP: the committed PMC pass's per-launch figures summed over the chain's kernels (k_*: one launch each per
    64-stream step).  NOT measured in this run; None when the committed pass is for another batch shape."""
    if not os.path.exists(PMC_FILE):
        return None, "no committed PMC pass for this configuration"
    with open(PMC_FILE) as f:
        pmc = json.load(f)
    if pmc.get("streams_per_gpu") != D or pmc.get("samples_per_stream") != N:
        return None, "committed PMC pass is for another batch shape"
    ok, note = _profile_is_current(pmc)
    if not ok:
        return None, note
    # the kernels of the timed loop's chain only: the stream selection and the one unpipelined check call launch other kernels (the
    # fused tail, the full SNR table) a handful of times in the same profiled run
    nl = pmc.get("launches", {})
    top = max(nl.values()) if nl else 0
    per = {k: v for k, v in pmc.get("hbm_bytes_per_launch", {}).items()
           if k.startswith("k_") and k != "k_make_twiddles" and (not nl or nl.get(k, 0) * 4 >= top)}
    if not per:
        return None, "no chain kernels in the committed PMC pass"
    return int(sum(per.values())), os.path.relpath(PMC_FILE, ROOT) + f" (sum over the chain's kernels of the committed rocprofv3 --pmc passes of this command; {note}; not measured in this run)"


def time_calib(torch, gsmcal, dev, ctx, raw_t, N, coef, ts, fc, K, W):
    """ms per step of one more table-mode batch on `ctx` + its table"""
    c2 = Calib(torch, gsmcal, dev, ctx, raw_t, N, "table", coef, ts, fc)

    def st():
        c2.launch(0)
        c2.to_host(0)
    t = time_steps(torch, dev, st, K, W, prewarm_s=SUB_PREWARM_S) / K
    torch.cuda.synchronize(dev)
    return t, c2.table(0).numpy().copy(), c2


def sub_results(args, torch, gsmcal, dev, ctx, cal, coef, ts, fc, N, stream, mixed_raw=None, distinct=None):
    """The other BASELINE configurations and regimes, timed in this same (driver-run) process."""
    from gsmcal import synth
    from oracle import gsmcal_oracle as oracle
    import parity
    sub = {}
    K, W = args.steps, max(2, args.warmup)
    bps = 2

    def path(v):
        return {"path_GBps": round(v * 1e6 * bps / 1e9, 1), "path_frac_of_hbm": round(v * 1e6 * bps / 1e9 / HBM_PEAK_GBS, 4)}
    # (i) the unselected distribution: low SNR, large ppm, carriers without a BCCH, rejected seeds left in
    if mixed_raw is not None and args.mode == "table":
        try:
            mt = torch.from_numpy(mixed_raw).to(dev)
            t, tab, c2 = time_calib(torch, gsmcal, dev, ctx, mt, N, coef, ts, fc, K, W)
            det = gsmcal.last_batch_details(len(mixed_raw), ctx=ctx)
            pos = c2.pos_t.cpu().numpy()
            nchk = 0
            for i in (1, 2, 3, 4, 6, 9):                     # one of each kind of the mix + plain ones
                try:
                    orc = oracle.calibrate_stream(mixed_raw[i], coef, ts, fc)
                except oracle.MatlabIndexError:              # where MATLAB would stop with an index error the ABI reports a negative status
                    assert tab[i, 9] < 0
                    continue
                parity.compare_stream(orc, tab[i], det, i, _pos_info(pos, tab, i))
                nchk += 1
            v = len(mixed_raw) * N / t / 1e6
            sub["mixed_batch"] = {"streams": len(mixed_raw), "ms_per_step": round(1e3 * t, 4), "Msample_per_s": round(v, 1), **path(v),
                                  "streams_calibrated_ok": int(np.sum(tab[:, 9] == 0)), "rows_checked_vs_oracle": nchk,
                                  "what": "64 distinct streams drawn like tests/sweep_parity.py (every 5th at 5-15 dB, every 7th up to "
                                          "+-300 ppm sampling error, every 11th without BCCH, every 13th up to +-60 ppm carrier "
                                          "error), nothing pre-selected"}
            if not args.no_kernel_events:
                prof = event_pass(ctx, lambda: c2.launch(0), K, torch, dev)
                sub["mixed_batch"]["kernels_ms_per_step_untimed_pass"] = {k: round(v_[0] / K, 4) for k, v_ in sorted(prof.items(), key=lambda kv: -kv[1][0])}
            del c2, mt
        except Exception as e:  # noqa: BLE001 - a sub-result must not take the headline down
            sub["mixed_batch"] = {"error": repr(e)}
    # (ii) the fine search's worst case: no certificate, every 64-shift chunk of every window is swept (GSMCAL_CERT=0)
    if args.mode == "table":
        try:
            os.environ["GSMCAL_CERT"] = "0"
            s2 = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(s2):
                cx = gsmcal.Context(dev.index or 0, stream=s2.cuda_stream)
                os.environ.pop("GSMCAL_CERT", None)
                t, tab, c2 = time_calib(torch, gsmcal, dev, cx, cal.raw_t, N, coef, ts, fc, max(3, K // 4), 2)
                same = bool(np.array_equal(tab, cal.table(0).numpy(), equal_nan=True))
                del c2
                cx.close()
            v = cal.D * N / t / 1e6
            sub["fine_search_worst_case_no_certificate"] = {"streams": cal.D, "ms_per_step": round(1e3 * t, 4), "Msample_per_s": round(v, 1),
                                                            **path(v), "table_identical_to_headline": same}
        except Exception as e:  # noqa: BLE001
            sub["fine_search_worst_case_no_certificate"] = {"error": repr(e)}
        finally:
            os.environ.pop("GSMCAL_CERT", None)
    # (iii) the throughput regime: 1 024 streams per GPU (the distinct set tiled; up to four lanes)
    if args.mode == "table" and cal.D < 1024:
        try:
            reps = (1024 + cal.D - 1) // cal.D
            big = cal.raw_t.repeat((reps, 1))[:1024].contiguous()
            t, tab, c2 = time_calib(torch, gsmcal, dev, ctx, big, N, coef, ts, fc, max(5, K // 2), 3)
            v = 1024 * N / t / 1e6
            ref = cal.table(0).numpy()
            same = all(np.array_equal(tab[k * cal.D: (k + 1) * cal.D], ref[: len(tab[k * cal.D: (k + 1) * cal.D])], equal_nan=True) for k in range(reps))
            sub["streams_1024"] = {"streams": 1024, "ms_per_step": round(1e3 * t, 4), "Msample_per_s": round(v, 1), **path(v),
                                   "tables_identical_to_headline": bool(same),
                                   "roofline_compute": compute_roofline("calib_1024", 1024, N, len(coef), t)}
            if not args.no_kernel_events:
                prof = event_pass(ctx, lambda: c2.launch(0), 5, torch, dev)
                sub["streams_1024"]["kernels_ms_per_step_untimed_pass"] = {k: round(v_[0] / 5, 4) for k, v_ in sorted(prof.items(), key=lambda kv: -kv[1][0])}
            del c2, big
            torch.cuda.empty_cache()
        except Exception as e:  # noqa: BLE001
            sub["streams_1024"] = {"error": repr(e)}
        cal.launch(0)
        torch.cuda.synchronize(dev)
    # config 2: gsm_sync_demod.m on 2 dongle streams (latency-bound)
    if cal.D >= 2 and args.mode == "table":
        def two():
            cal.launch(0, 2)
            cal.to_host(0)
        t = time_steps(torch, dev, two, K, W, prewarm_s=SUB_PREWARM_S) / K
        sub["config2_two_streams"] = {"streams": 2, "ms_per_call": round(1e3 * t, 4), "Msample_per_s": round(2 * N / t / 1e6, 1)}
        # ... and with four such calls in flight inside the context (gsmcal_ctx_set_pipeline_depth(4)): the call is a latency chain that
        # leaves most of the chip idle, so consecutive calls overlap almost entirely (sustained: 10 x K calls between the fences)
        try:
            ref2 = cal.table(0).numpy()[:2].copy()
            kk2 = [0]

            def two_in_flight():
                b_ = kk2[0] % 4
                kk2[0] += 1
                cal.launch(b_, 2)
                cal.to_host(b_)
            ctx.set_pipeline_depth(4)
            t4 = time_steps(torch, dev, two_in_flight, 10 * K, W, prewarm_s=SUB_PREWARM_S) / (10 * K)
            ctx.set_pipeline_depth(1)
            ctx.sync()
            same2 = all(bool(np.array_equal(cal.table(b_).numpy()[:2], ref2, equal_nan=True)) for b_ in range(4))
            sub["config2_two_streams"].update({"ms_per_call_pipeline_depth4": round(1e3 * t4, 4), "Msample_per_s_pipeline_depth4": round(2 * N / t4 / 1e6, 1),
                                               "tables_identical_across_output_sets": same2})
        except Exception as e:  # noqa: BLE001
            ctx.set_pipeline_depth(1)
            sub["config2_two_streams"]["pipeline_depth4_error"] = repr(e)
        cal.launch(0)
        torch.cuda.synchronize(dev)
    # the same streams with the corrected stream written (the API's real output, 18 B/sample)
    if args.mode == "table":
        sdepth = max(1, min(4, args.pipeline_depth))
        cs = Calib(torch, gsmcal, dev, ctx, cal.raw_t, N, "stream", coef, ts, fc, nbuf=sdepth)
        ks = [0]

        def st():                                            # consecutive calls into output sets (table, pos_info, r_correct: 1 GB each) taken in turn
            b = ks[0] % sdepth
            ks[0] += 1
            cs.launch(b)
            cs.to_host(b)

        def sfence():
            ctx.sync()
            torch.cuda.synchronize(dev)
        ns = max(4, K // 4)
        t = time_steps(torch, dev, st, ns, 2, sfence, prewarm_s=SUB_PREWARM_S) / ns           # one call at a time: the figure
        tp = None
        if sdepth > 1:                                       # calls in flight: the next call's table chain under this call's stream kernel --
            ctx.set_pipeline_depth(sdepth)                   # no gain (the stream kernel saturates both pipes), reported beside it
            tp = time_steps(torch, dev, st, ns, sdepth, sfence, prewarm_s=SUB_PREWARM_S) / ns
            ctx.set_pipeline_depth(1)
        v = cal.D * N / t / 1e6
        same_r = all(bool(torch.equal(cs.r_ts[b], cs.r_ts[0])) for b in range(1, sdepth))
        sub["stream_mode"] = {"streams": cal.D, "ms_per_step": round(1e3 * t, 4), "pipeline_depth": 1,
                              **({f"ms_per_step_pipeline_depth{sdepth}": round(1e3 * tp, 4)} if tp is not None else {}),
                              "Msample_per_s": round(v, 1),
                              "bytes_per_sample_algorithmic": 18, "path_GBps": round(v * 1e6 * 18 / 1e9, 1),
                              "path_frac_of_hbm": round(v * 1e6 * 18 / 1e9 / HBM_PEAK_GBS, 4),
                              "r_correct_identical_across_output_sets": same_r,
                              "roofline_compute": compute_roofline("stream_mode_64", cal.D, N, len(coef), t, mode="stream")}
        torch.cuda.synchronize(dev)
        assert all(torch.equal(cs.table(b), cal.table(0)) or bool(torch.allclose(cs.table(b), cal.table(0), equal_nan=True)) for b in range(sdepth))
        del cs
        torch.cuda.empty_cache()
    # scanner path: BASELINE config 3 (200 captures) and config 5 per GPU (12 800 captures, 16.4 GB, generated on the device)
    for name, ncap in (("config3_scan_200", 200), ("config5_scan_12800_per_gpu", 12800)):
        try:
            r = bench_scan(args, torch, gsmcal, dev, ctx, ncap, 64, distinct=32, steps=max(5, K // 2), warmup=2, cpu=(ncap == 200))
            sub[name] = {k: r[k] for k in ("ms_per_step", "ms_per_step_depth1", "pipeline_depth", "value", "hbm_GBps_algorithmic", "path_frac_of_hbm", "captures_with_hits",
                                           "kernels_ms_per_step_untimed_pass", "parity_checked_captures") if k in r}
            if "cpu_baseline" in r:     # BASELINE config 1: the CPU-only FCCH_coarse_position path on 640 000-sample captures
                sub["config1_cpu_scan_path"] = dict(r["cpu_baseline"], what="config 1: raw2iq + fir1(30) + 1:64 + FCCH_coarse_position "
                                                    "+ acceptance on 640 000-sample captures, oracle (NumPy port) on one host thread")
            sub[name]["captures"] = ncap
        except Exception as e:  # noqa: BLE001 - a sub-result must not take the headline down
            sub[name] = {"error": repr(e)}
        torch.cuda.empty_cache()
    # the N > 1 code path on this one GPU: the same K steps in a self-launched child (one rank, RCCL communicator of size 1,
    # table in device memory + the all-gather + the gathered-table digest check) -- what the collective costs a step
    # before the first xGMI byte moves
    if args.mode == "table":
        try:
            sub["single_rank_collective"] = bench_single_rank_collective(args, cal.D)
        except Exception as e:  # noqa: BLE001
            sub["single_rank_collective"] = {"error": repr(e)}
    # two batches in flight: two contexts on two HIP streams, consecutive steps alternate between them.  Every kernel of
    # the chain at this batch size is latency-bound and leaves most of the GPU idle, so a second, independent batch
    # overlaps almost freely -- the throughput a double-buffered deployment sees.  NOT the headline `value` (that is
    # one batch at a time, each step dependent on the previous one's stream).
    if args.mode == "table":
        try:
            sub["two_batches_in_flight"] = bench_two_in_flight(args, torch, gsmcal, dev, cal, coef, ts, fc, N)
        except Exception as e:  # noqa: BLE001
            sub["two_batches_in_flight"] = {"error": repr(e)}
    try:
        sub["ingest_ring"] = bench_ingest(torch, gsmcal, dev, ctx)
    except Exception as e:  # noqa: BLE001
        sub["ingest_ring"] = {"error": repr(e)}
    return sub


def bench_single_rank_collective(args, D):
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["GSMCAL_FORCE_DIST"] = "1"
    cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--streams", str(D), "--frames", str(args.frames), "--distinct", str(args.distinct),
           "--full", "--no-sub", "--no-cpu-baseline", "--no-kernel-events"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    if p.returncode != 0 or not line:
        return {"error": f"child exited {p.returncode}", "stderr_tail": p.stderr[-600:]}
    r = json.loads(line[-1])
    return {"streams": D, "ms_per_step": r["ms_per_step"], "Msample_per_s": r["value"], "steps": r["steps"],
            "collective": r["config"]["collective"],
            "gathered_table_checked_against_every_rank": r["config"]["gathered_table_checked_against_every_rank"],
            "rows_checked_vs_oracle": r["config"]["rows_checked_vs_oracle_per_rank"],
            "what": "GSMCAL_FORCE_DIST=1 python bench.py --gpus 1 as a child process: one rank under torch.distributed.run, table in "
                    "device memory, one all-gather per step, digest check of the gathered table"}


def bench_two_in_flight(args, torch, gsmcal, dev, cal, coef, ts, fc, N):
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    ctxs = [gsmcal.Context(dev.index or 0, stream=s.cuda_stream) for s in streams]
    cals = [Calib(torch, gsmcal, dev, c, cal.raw_t, N, "table", coef, ts, fc) for c in ctxs]
    k = [0]

    def step():
        i = k[0] & 1
        k[0] += 1
        with torch.cuda.stream(streams[i]):
            cals[i].launch(0)
            cals[i].to_host(0)
    try:
        t = time_steps(torch, dev, step, 2 * args.steps, 4, prewarm_s=SUB_PREWARM_S) / (2 * args.steps)
        torch.cuda.synchronize(dev)
        ok = bool(torch.equal(cals[0].table(0), cal.table(0)) or torch.allclose(cals[0].table(0), cal.table(0), equal_nan=True))
    finally:
        for c in ctxs:
            c.close()
    return {"streams_per_batch": cal.D, "ms_per_step": round(1e3 * t, 4), "Msample_per_s": round(cal.D * N / t / 1e6, 1),
            "tables_identical_to_headline": ok}


def bench_ingest(torch, gsmcal, dev, ctx, D=256, nbatch=8):
    """scanner batches through the pinned ring (H2D of batch k+1 under the detector of batch k) -- sustained
    input rate next to the plain pinned hipMemcpy rate of the same bytes (the PCIe ceiling of this box)."""
    from gsmcal import synth
    N = 64 * synth.FRAME_OV
    coef = np.ascontiguousarray(synth.fir1(30, 200e3 / synth.FS))
    nbytes = D * 2 * N
    ring = gsmcal.ingest.Ring(ctx, nbytes, slots=2)
    out_t = torch.zeros((nbatch, D, 2), dtype=torch.float64, device=dev)
    base = np.stack([synth.make_stream(dongle=1200, arfcn=i, num_frames=64, bcch=(i % 4 != 3))[0] for i in range(8)])
    for s in range(2):
        ring.host(s).reshape(D, 2 * N)[:] = np.tile(base, (D // 8, 1))      # the producer's bytes are already in the pinned slots
    try:
        def run(with_compute):
            ctx.sync()
            t0 = time.perf_counter()
            for k in range(nbatch):
                s = k % 2
                if k >= 2:
                    ring.host_ready(s)
                ring.submit(s)
                dev_p = ring.acquire(s)
                if with_compute:
                    gsmcal.fcch_scan_batch_dev(dev_p, D, N, coef, out_t[k].data_ptr(), ctx=ctx)
                ring.release(s)
            ctx.sync()
            return time.perf_counter() - t0
        run(True)
        t_pipe = min(run(True) for _ in range(3))
        t_copy = min(run(False) for _ in range(3))
    finally:
        ring.close()
    tot = nbatch * nbytes
    return {"batches": nbatch, "captures_per_batch": D, "bytes_per_batch": nbytes,
            "sustained_GBps_with_detector": round(tot / t_pipe / 1e9, 2), "h2d_only_GBps": round(tot / t_copy / 1e9, 2),
            "Msample_per_s": round(nbatch * D * N / t_pipe / 1e6, 1),
            "note": "host-resident input: the path is PCIe-bound; this figure is never `value` (inputs resident in HBM)"}


def bench_scan(args, torch, gsmcal, dev, ctx, D, frames, distinct, steps, warmup, cpu=True, use_dist=False, world=1, rank=0,
               sizes=None, tg=None, first_unit=None, full=True, outputs=None):
    """Scanner path (BASELINE configs 3/5): D captures resident in HBM -> snr, num_hit per capture on the host.
    N > 1 (multi_rtl_sdr_gsm_FCCH_scanner.m:60-65,163-186: the ARFCN split across dongles and the one table every rank needs):
    `sizes` = captures per rank, `tg` = the table gatherer (2 columns: snr, num_hit), `first_unit` = this rank's first global
    capture index; each step ends with ONE all-gather of the (snr, num_hit) table, the GATHERED table goes to the host and is
    digest-checked against every rank's own rows (gsmcal.dist.check_gathered_table), as in the calibration workload.
    full=False: the timed steps only (no one-call-at-a-time figure, event pass, checks or CPU baseline); `outputs`, a dict,
    receives the last timed step's table."""
    import torch.distributed as dist

    from gsmcal import synth
    from oracle import gsmcal_oracle as oracle
    N = frames * synth.FRAME_OV
    coef = np.ascontiguousarray(synth.fir1(30, 200e3 / synth.FS))     # multi_rtl_sdr_gsm_FCCH_scanner.m:53
    nd = max(1, min(distinct, D))
    base = np.stack([synth.make_stream(dongle=1000 + rank, arfcn=i, num_frames=frames, bcch=(i % 4 != 3))[0] for i in range(nd)])
    base_t = torch.from_numpy(base).to(dev)
    raw_t = torch.empty((D, 2 * N), dtype=torch.uint8, device=dev)
    # distinct captures generated on the device (rotation + counter-based dither of the seeded base set; synth.expand_capture
    # is the bit-identical host twin used for the parity check below)
    if first_unit is None:
        first_unit = rank * D
    sizes = list(sizes) if sizes is not None else [D] * world
    gsmcal.synth_expand_dev(base_t.data_ptr(), nd, N, raw_t.data_ptr(), D, first_unit=first_unit, ctx=ctx)
    ctx.sync()
    NB = 4                                               # output sets / gather buffer pairs taken in turn: as many as calls may be in flight
    out_t = [torch.zeros((D, 2), dtype=torch.float64, device=dev) for _ in range(NB)]
    host_outs = [torch.zeros((D, 2), dtype=torch.float64).pin_memory() for _ in range(NB)]
    host_gath = [torch.zeros((sum(sizes), 2), dtype=torch.float64).pin_memory() for _ in range(NB)] if use_dist else None
    cp = coef.ctypes.data_as(gsmcal._lib.c_double_p)
    nstep = [0]
    # calls in flight inside the context (single-stage batches, i.e. below 1 200 captures: bigger ones are pipelines of stages inside
    # ONE call already): the detector of call i under the front kernel of call i+1
    pdepth = max(1, min(NB, args.pipeline_depth)) if D < 1200 and (not use_dist or all(sz == sizes[0] for sz in sizes)) else 1
    if use_dist and type(tg).__name__ == "TableGatherer":
        pdepth = 1                                           # (torch's collective runs on torch's stream, not behind the call it follows)

    def step():
        # single rank: the acceptance kernel stores (snr, num_hit) straight into pinned host memory (no copy queued).
        # N > 1: the table stays in device memory, in one of four buffers in turn; the all-gather of step i (posted behind the
        # kernels that fill buffer i mod 4) overlaps the kernels of the next steps, the only wait is before a buffer is written again
        b = nstep[0] % NB
        nstep[0] += 1
        if use_dist:
            tg.wait(b)
        dst_t = out_t[b] if use_dist else host_outs[b]
        ctx.check(ctx.lib.gsmcal_fcch_scan_batch_dev(ctx.h, C.c_void_p(raw_t.data_ptr()), D, N, cp, len(coef),
                                                     C.c_void_p(dst_t.data_ptr()), None, None, None), "scan")
        if use_dist:
            tg.post(b, out_t[b])                                     # one RCCL all-gather of the (snr, num_hit) table

    def fence():
        ctx.sync()                                                   # (joins the calls still in flight on the library's streams)
        if use_dist:
            for b in range(NB):
                if tg.work[b] is not None:
                    host_gath[b].copy_(tg.rows(b), non_blocking=True)   # the GATHERED table to the host (every rank)
        torch.cuda.synchronize(dev)
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize(dev)

    elapsed1 = None
    if full and pdepth > 1 and not use_dist:                         # one call at a time first (reported beside the figure)
        elapsed1 = time_steps(torch, dev, step, steps, warmup, fence, prewarm_s=SUB_PREWARM_S)
    ctx.set_pipeline_depth(pdepth)
    elapsed = time_steps(torch, dev, step, steps, warmup + pdepth - 1, fence, prewarm_s=0.0 if use_dist else SUB_PREWARM_S)
    fence()
    ctx.set_pipeline_depth(1)
    host_out = host_outs[(nstep[0] - 1) % NB]
    gathered_ok = None
    if use_dist:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
        last = (nstep[0] - 1) % NB
        res = out_t[last].cpu().numpy()
        if outputs is not None:
            outputs.update(table=res.copy(), table_gathered=host_gath[last].numpy().copy())
    else:
        res = host_out.numpy().copy()
        if outputs is not None:
            outputs["table"] = res.copy()
    if use_dist and full:
        # every rank checks every peer's block of the gathered table against that peer's own digest (independent gloo group)
        from gsmcal import dist as gdist
        chk = dist.new_group(backend="gloo")
        g_all = host_gath[last].numpy()
        gdist.check_gathered_table(g_all, res, sizes, rank, group=chk)
        off = sum(sizes[:rank])
        assert np.array_equal(g_all[off: off + D], res, equal_nan=True), "gathered scan table differs from this rank's rows"
        gathered_ok = True
    value = sum(sizes) * N * steps / elapsed / 1e6
    out = {"ms_per_step": round(1e3 * elapsed / steps, 4), "value": round(value, 3), "pipeline_depth": pdepth,
           **({"ms_per_step_depth1": round(1e3 * elapsed1 / steps, 4)} if elapsed1 is not None else {}),
           "hbm_GBps_algorithmic": round(value * 1e6 * 2.25 / 1e9, 1),
           "path_frac_of_hbm": round(value * 1e6 * 2.25 / 1e9 / HBM_PEAK_GBS / world, 4),
           "captures_with_hits": int(np.sum(res[:, 1] > 0)),
           "gathered_table_checked_against_every_rank": gathered_ok}
    if not full:
        del raw_t
        return out
    if not args.no_kernel_events and rank == 0:
        def launch_only():                                   # (no collective in here: only rank 0 runs this pass)
            ctx.check(ctx.lib.gsmcal_fcch_scan_batch_dev(ctx.h, C.c_void_p(raw_t.data_ptr()), D, N, cp, len(coef),
                                                         C.c_void_p((out_t[0] if use_dist else host_outs[0]).data_ptr()), None, None, None), "scan")
        prof = event_pass(ctx, launch_only, steps, torch, dev)
        out["kernels_ms_per_step_untimed_pass"] = {k: round(v[0] / steps, 4) for k, v in sorted(prof.items(), key=lambda kv: -kv[1][0])}
        if D >= 1200:     # pipelined batch: stage k's detector and the tail of its front kernel run UNDER stage k+1's front kernel
            out["kernels_ms_per_step_untimed_pass"]["note"] = ("OVERLAPPED launches on the pipeline's internal streams: the per-kernel sums exceed the "
                                                               "step and are not separable evidence; only ms_per_step / path_frac_of_hbm are")
        for k, v in prof.items():
            if k.startswith("k_front"):
                ms = v[0] / v[1]
                per_launch = D * N * 2.25 * steps / v[1]
                out["front_kernel"] = {"name": k, "achieved_GBps": round(per_launch / 1e9 / (ms * 1e-3), 1), "avg_launch_ms": round(ms, 5)}
    # parity: sampled captures through the CPU oracle (the host twin rebuilds their bytes)
    rng = np.random.default_rng(11)
    units = sorted(set([0, D - 1] + [int(x) for x in rng.integers(0, D, 14)]))
    t_cpu = 0.0
    for u in units:
        cap = synth.expand_capture(base, first_unit + u)
        c0 = time.perf_counter()
        o = oracle.scan_capture(cap, coef)
        t_cpu += time.perf_counter() - c0
        assert o["num_hit"] == res[u, 1] and abs(o["snr"] - res[u, 0]) < 1e-8, f"scan parity, capture {u}"
    out["parity_checked_captures"] = len(units)
    if cpu:
        out["cpu_baseline"] = {"value": round(len(units) * N / t_cpu / 1e6, 4), "unit": "Msample/s", "cores": 1, "kind": "port",
                               "sample": f"{len(units)} captures through oracle.scan_capture in {t_cpu:.1f} s"}
    del raw_t
    return out


def bench_scan_main(args, rank, world, dev, use_dist):
    import torch
    import torch.distributed as dist

    import gsmcal
    from gsmcal import dist as gdist
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    ctx = gsmcal.Context(local_rank, stream=stream.cuda_stream)
    # units = captures (dongle x ARFCN, multi_rtl_sdr_gsm_FCCH_scanner.m:60-65): --scaling weak = --streams captures per GPU,
    # strong = --streams captures in total, block-contiguous shards (uneven shards are padded inside the gatherer)
    if args.scaling == "strong":
        sizes = gdist.shard_sizes(args.streams, world)
        first_unit = gdist.shard_range(args.streams, world, rank)[0]
    else:
        sizes = [args.streams] * world
        first_unit = rank * args.streams
    D = sizes[rank]
    if D < 1:
        raise SystemExit("more ranks than captures")
    tg, gather_kind, ncomm, gather_fallback = setup_gatherer(torch, gsmcal, gdist, ctx, dev, stream, local_rank, sizes, 2, pairs=4) if use_dist else (None, "none", None, None)
    outputs = {}
    r = bench_scan(args, torch, gsmcal, dev, ctx, D, args.frames, args.distinct, args.steps, args.warmup,
                   cpu=not args.no_cpu_baseline and world == 1, use_dist=use_dist, world=world, rank=rank, sizes=sizes, tg=tg, first_unit=first_unit,
                   full=args.full, outputs=outputs)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, outputs, D)
    N = args.frames * 10000
    out = {"metric": "IQ Msamples/s through FCCH scanner path", "value": r["value"], "unit": "Msample/s",
           "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": r["ms_per_step"],
           "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": "f64",
           "data": f"synthetic GSM uint8 IQ: {min(args.distinct, D)} seeded captures expanded on the device to {D} distinct ones "
                   "(3 of 4 base captures carry a BCCH carrier)",
           "config": {"workload": f"scanner path multi_rtl_sdr_gsm_FCCH_scanner.m:60-65,132-135,164-185: {sum(sizes)} captures ({max(sizes)}/GPU) x {N} "
                                  f"IQ samples ({args.frames} frames), fir1(30), snr/num_hit table on the host of every rank",
                      "captures_per_gpu": max(sizes), "captures_total": sum(sizes),
                      "captures_with_hits": r["captures_with_hits"], "bytes_per_sample_algorithmic": 2.25,
                      "collective": COLLECTIVE_NAMES.get(gather_kind, gather_kind),
                      "gathered_table_checked_against_every_rank": r["gathered_table_checked_against_every_rank"]},
           "roofline": {"bound": "hbm", "achieved": r["hbm_GBps_algorithmic"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": r["path_frac_of_hbm"], "traffic": None,
                        "what": "WHOLE PATH: Msample/s x 2.25 B/sample (2 B raw read + 16/64 B decimated write)",
                        "kernel": r.get("front_kernel")}}
    for k in ("kernels_ms_per_step_untimed_pass", "parity_checked_captures", "cpu_baseline"):
        if k in r:
            out[k] = r[k]
    if gather_fallback:
        out["config"]["collective_fallback_from_native"] = gather_fallback
    if rank == 0:
        print(json.dumps(out))
    if use_dist:
        finish_dist(torch, dist, gdist, dev, ncomm, gather_fallback)


DUMP_LIMIT_BYTES = 60 << 20      # (under 64 MB with the .npy headers)


def calib_outputs(torch, cal, b, table, gathered=None):
    """What a caller of the timed calibration step receives from output set b: the table, the burst positions (pos_info as the
    library writes it, [D][2][MAX_POS_ROWS]), r_len and, in stream mode, a fixed seeded sample of r_correct's samples (the whole
    array is 16 B per sample), the same sample positions in every stream."""
    out = {"table": table, "pos_info": cal.pos_ts[b].cpu().numpy(), "r_len": cal.rlen_ts[b].cpu().numpy().astype(np.float64)}
    if gathered is not None:
        out["table_gathered"] = gathered
    if cal.r_ts is not None:
        k = max(1, min(cal.N, (DUMP_LIMIT_BYTES // 2) // (16 * cal.D)))
        idx = np.sort(np.random.default_rng(1234).choice(cal.N, size=k, replace=False))
        out["r_correct_sample"] = cal.r_ts[b][:, torch.from_numpy(idx).to(cal.dev), :].cpu().numpy()
        out["r_correct_sample_index"] = idx.astype(np.float64)
    return out


def dump_outputs(directory, arrays, rows):
    """--dump-outputs: one DIR/<name>.npy per array, float64, at most DUMP_LIMIT_BYTES in all.  Past that, every array with
    `rows` rows (one per stream / capture) keeps the same fixed, seeded sample of its rows, listed in DIR/rows.npy."""
    os.makedirs(directory, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()}
    per_row = sum(a.nbytes for a in arrays.values() if a.ndim and len(a) == rows) / rows
    other = sum(a.nbytes for a in arrays.values() if not (a.ndim and len(a) == rows))
    if other + per_row * rows > DUMP_LIMIT_BYTES:
        keep = max(1, min(rows, int((DUMP_LIMIT_BYTES - other) // (per_row + 8))))
        sample = np.sort(np.random.default_rng(4321).choice(rows, size=keep, replace=False))
        arrays = {k: (a[sample] if a.ndim and len(a) == rows else a) for k, a in arrays.items()}
        arrays["rows"] = sample.astype(np.float64)
    for k, a in arrays.items():
        np.save(os.path.join(directory, k + ".npy"), a)


def _oracle_warm(_):
    from oracle import gsmcal_oracle as oracle  # noqa: F401
    time.sleep(0.05)
    return 0


def _oracle_one(args):
    raw, coef, ts, fc = args
    from oracle import gsmcal_oracle as oracle
    return oracle.calibrate_stream(raw, coef, ts, fc)["total_sampling_ppm"]


def _pos_info(pos, table, i):
    """pos: (D, 2, MAX_POS_ROWS) host array"""
    k = int(table[i, 7])
    if table[i, 8] == -1.0:
        return -np.ones((k, 2))
    return np.ascontiguousarray(pos[i, :, :k].T)


if __name__ == "__main__":
    main()
