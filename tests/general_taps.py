"""Shared inputs of the general-tap tests: channel filters of other lengths than the drivers' 47 taps, some of them NOT
mirror-symmetric, and the six streams they are run on.

The batch chain exists in two forms: instantiations with the reference geometry compiled in (47 taps) and any-geometry
ones; which one runs is decided on the host from the tap count and from whether coef[k] == coef[nt-1-k] holds exactly.
A mirrored filter cannot tell a kernel that applies its taps in the right order from one that applies them reversed, so
the set holds `ramp` filters -- a low-pass multiplied by a rising exponential -- whose reverse is a different filter:
tests/test_general_taps_cpu.py proves, with the oracle alone, that the reversed filter moves the results by far more than
the parity bars of tests/parity.py.

Plain module: numpy, synth and the oracle only -- nothing here touches the GPU, so it is safe in spawned pool workers."""
import math

import numpy as np

from gsmcal import synth
from oracle import gsmcal_oracle as oracle

FC = 957.4e6
WN = 200e3 / synth.FS


def ramp(n):
    """n taps, not mirror-symmetric: fir1(n-1, 200e3/FS) .* exp(linspace(0, log(4), n)), unit DC gain"""
    h = synth.fir1(n - 1, WN) * np.exp(np.linspace(0.0, math.log(4.0), n))
    return h / np.sum(h)


# name -> taps, in increasing tap count (the order the GPU tests go through them: a wrong LDS size shows at the smallest
# filter that has it).  fir64 / fir65 / ramp66: n_head = ceil((ntaps-1)/64) = 1, 1, 2 head rows with a partial tap sum.
# fir769: stream_tile_lds(769) = 66 528 bytes > 64 KiB (the bound is crossed at 737 taps), so r_correct takes the tile gather.
FILTERS = {
    "one": np.array([1.0]),
    "fir5": synth.fir1(4, 0.4),
    "fir31": synth.fir1(30, WN),              # exactly mirrored
    "fir31_scipy": oracle.fir1(30, WN),       # scipy's firwin: mirrored to the last ulp only
    "ramp31": ramp(31),
    "ramp47": ramp(47),                       # the compiled-in tap count, but no mirrored pair to add
    "fir48": synth.fir1(47, WN),              # even length, exactly mirrored
    "fir64": synth.fir1(63, WN),
    "fir65": synth.fir1(64, WN),
    "ramp66": ramp(66),
    "fir129": synth.fir1(128, WN),
    "ramp200": ramp(200),
    "fir769": synth.fir1(768, WN),
}
RAMPS = tuple(k for k in FILTERS if k.startswith("ramp"))

DONGLES = (0, 1, 3, 4, 10, 12)
NUM_FRAMES = 61
UNALIGNED_BYTES = 2 * 609991      # per stream no multiple of 16: streams after the first start off a 16-byte boundary


def make_streams():
    """(6, 1 220 000) uint8: the six 61-frame captures"""
    return np.stack([synth.make_stream(dongle=d, num_frames=NUM_FRAMES)[0] for d in DONGLES])


def cut(raw, unaligned):
    return np.ascontiguousarray(raw[:, :UNALIGNED_BYTES]) if unaligned else raw


def calibrates(orc):
    """the oracle calibrated this stream: finite totals and a corrected stream"""
    return bool(math.isfinite(orc["total_sampling_ppm"]) and math.isfinite(orc["total_carrier_ppm"]) and orc["r_len"] > 0)


def oracle_job_r(job):
    """job = (raw, coef, ts, fc) -> oracle.calibrate_stream dict WITH the corrected stream (pool worker, see parity.pool_map)"""
    import os
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    raw, coef, ts, fc = job
    return oracle.calibrate_stream(raw, coef, ts, fc, keep_r=True)


def scan_job(job):
    """job = (raw, coef) -> oracle.scan_capture dict (pool worker)"""
    import os
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    raw, coef = job
    return oracle.scan_capture(raw, coef)
