"""Shared inputs of the tail-gather tests: small batches (3-4 streams, at most 61 frames) that drive the per-window gathers
of the four-launch tail -- k_burst_tone<1|0, 8, 47> and k_window_sch<8, 512, 47> -- through every branch their lean window
builds take, and two batches on other filters that must stay on the generic kernels.

  plain      three captures on an unaligned capture length (general_taps.UNALIGNED_BYTES: streams after the first start off
             a 16-byte boundary, so the aligned raw chunks of the SCH window begin in front of the window); the second one
             leaves at the fine stage's SNR gate, so its workgroups have no SCH window
  ppm        sampling errors of +-300 ppm and carrier errors of +-60 ppm: LERP factors far from 1, a large rotator argument,
             burst ranges that may leave every fine window (the raw-byte fallback of the burst gather)
  ends       the end-of-capture constructions of tests/exit_paths.py (the capture ends `delta` samples behind the fifth
             first-round FCCH position), on a 61-frame capture: the last SCH window drops out (:40), just fits (ENDS_FIT is the
             smallest delta at which the oracle keeps five SCH windows: the window closest to n0 the chain can reach) and fits
  copy       streams whose SCH stage measures no sampling error (e == 0: the resampling is skipped, OP_COPY at level 3)
  fir31      a 31-tap filter: the generic kernels, which keep gather_core
  ramp47     an asymmetric 47-tap filter: the tap count of the reference geometry, so the lean gathers with taps whose
             reverse is another filter
  other      a second plain batch of the same shape as `plain`: the two alternate at pipeline depth 4

Every batch must take at least one stream through the SCH stage in the ORACLE (tests/test_tail_gathers_cpu.py holds that),
so that no comparison of the GPU test is empty.

Plain module: numpy, synth, the oracle and the other plain helper modules -- nothing here touches the GPU."""
import numpy as np

import exit_paths as ep
import general_taps as gt
from gsmcal import synth
from oracle import gsmcal_oracle as oracle

FC = gt.FC
NUM_FRAMES = gt.NUM_FRAMES
PLAIN_DONGLES = (0, 1, 3)
OTHER_DONGLES = (4, 10, 12)
# (dongle, sampling_ppm, carrier_ppm)
PPM_STREAMS = ((12, 300.0, 60.0), (1, -300.0, -60.0), (5, 300.0, -60.0), (4, -300.0, 60.0))      # (seeds the oracle calibrates at these errors)
COPY_DONGLES = (5, 6, 9)                           # sampling_ppm(2) == 0 in the oracle
ENDS_SOURCE = dict(dongle=0, num_frames=NUM_FRAMES)
ENDS_FIT = 10911                                   # see the module text; found with find_ends_fit()
ENDS_DELTAS = (ENDS_FIT - 1, ENDS_FIT, 11500)      # (the first two: four and five SCH windows)
ENDS_HIT = 4                                       # the cuts are placed behind this first-round FCCH position (0-based)


def coef():
    return synth.fir1(46, gt.WN)


def captures(dongles):
    return np.stack([synth.make_stream(dongle=d, num_frames=NUM_FRAMES)[0] for d in dongles])


def ends_source():
    """(raw, first-round FCCH positions) of the capture the `ends` batch is cut from: one oracle run"""
    raw = synth.make_stream(**ENDS_SOURCE)[0]
    orc = oracle.calibrate_stream(raw, coef(), synth.sch_training_sequence(), FC)
    return raw, orc["fine_first_round_pos"].astype(np.int64)


def ends_batch(deltas=ENDS_DELTAS, src=None):
    """exit_paths' head-offset cuts: stream j is raw[2a : 2(a + N)] with a + N = p + deltas[j], N = p + min(deltas)"""
    raw, pos = src or ends_source()
    p = int(pos[ENDS_HIT])
    n = p + min(deltas)
    return np.stack([np.ascontiguousarray(ep.samples(raw, p + d - n, p + d)) for d in deltas])


def find_ends_fit(lo=10000, hi=11000):
    """the smallest delta at which the oracle keeps the SCH window behind FCCH ENDS_HIT (how ENDS_FIT was chosen)"""
    src = ends_source()
    c, ts = coef(), synth.sch_training_sequence()

    def n_sch(delta):
        raw = ends_batch((delta,), src)[0]
        return len(oracle.calibrate_stream(raw, c, ts, FC)["sch_first_round_pos"])
    top = n_sch(hi)
    assert n_sch(lo) < top
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if n_sch(mid) < top:
            lo = mid
        else:
            hi = mid
    return hi


def build():
    """-> {name: (raw (S, bytes) uint8, taps)}"""
    c = coef()
    plain = gt.cut(captures(PLAIN_DONGLES), True)
    other = gt.cut(captures(OTHER_DONGLES), True)
    ppm = np.stack([synth.make_stream(dongle=d, num_frames=NUM_FRAMES, sampling_ppm=sp, carrier_ppm=cp)[0] for d, sp, cp in PPM_STREAMS])
    return {"plain": (plain, c), "ppm": (ppm, c), "ends": (ends_batch(), c), "copy": (captures(COPY_DONGLES), c),
            "fir31": (plain, gt.FILTERS["fir31"]), "ramp47": (plain, gt.FILTERS["ramp47"]), "other": (other, c)}


GENERIC = ("fir31",)          # another tap count than 47: the any-geometry instantiations <..., 0, 0>; every other batch runs <8, 512, 47>


def context_under(g, env, **kw):
    """a context of the library module g created under `env` (the switches are read when a context is created)"""
    import os
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return g.Context(0, **kw)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def launches(names, part):
    """launches of the kernels whose name holds `part` in a {kernel name: launches} profile"""
    return sum(n for k, n in names.items() if part in k)


def through_sch(orc):
    """the oracle took this stream through the SCH stage: its correlation ran over at least one search window"""
    return len(orc["sch_first_round_pos"]) > 0


def oracle_batch(raw, taps):
    """oracle.calibrate_stream of every stream of a batch (spawned pool; a reference index error -> None)"""
    import parity
    ts = synth.sch_training_sequence()
    return [o for o, _ in parity.pool_map(parity.oracle_job_safe, [(r, taps, ts, FC) for r in raw], max_workers=16)]
