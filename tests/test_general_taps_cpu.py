"""The inputs of tests/test_gpu_general_taps.py, pinned by the reference algorithm alone (no GPU): for every filter of
general_taps.FILTERS the oracle calibrates at least four of the six streams and leaves at least one uncalibrated (so
the GPU test compares real numbers AND sentinel rows), on the full captures and on the cut to 2*609991 bytes; and for
every ramp (non-mirrored) filter the reversed taps give a result that the parity bars tell from the forward one -- a
kernel that stages or pairs its taps in the wrong order cannot pass the GPU test."""
import numpy as np
import pytest

import general_taps as gt
import parity

CASES = [(name, unaligned) for name in gt.FILTERS for unaligned in (False, True)]


@pytest.fixture(scope="module")
def runs():
    """(filter, unaligned, stream index, reversed taps) -> oracle.calibrate_stream dict, all through one spawned pool"""
    raw = gt.make_streams()
    ts = gt.synth.sch_training_sequence()
    keys, jobs = [], []
    for name, unaligned in CASES:
        r = gt.cut(raw, unaligned)
        for i in range(len(gt.DONGLES)):
            keys.append((name, unaligned, i, False))
            jobs.append((r[i], gt.FILTERS[name], ts, gt.FC))
            if name in gt.RAMPS:
                keys.append((name, unaligned, i, True))
                jobs.append((r[i], np.ascontiguousarray(gt.FILTERS[name][::-1]), ts, gt.FC))
    return dict(zip(keys, parity.pool_map(parity.oracle_job, jobs, max_workers=16)))


def test_the_filter_set_is_what_the_gpu_tests_assume():
    f = gt.FILTERS
    assert [len(v) for v in f.values()] == [1, 5, 31, 31, 31, 47, 48, 64, 65, 66, 129, 200, 769]
    for name, h in f.items():
        assert abs(np.sum(h) - 1.0) < 1e-12, name
        mirrored = np.array_equal(h, h[::-1])
        if name in gt.RAMPS:
            assert not mirrored and np.max(np.abs(h - h[::-1])) > 1e-3, name     # far from a rounding difference
        elif name == "fir31_scipy":
            assert not mirrored and np.max(np.abs(h - h[::-1])) < 1e-15          # mirrored to the last ulp only
        else:
            assert mirrored, name
    assert [(len(f[k]) - 1 + 63) // 64 for k in ("fir64", "fir65", "ramp66")] == [1, 1, 2]     # head rows (ensure_head)
    assert gt.UNALIGNED_BYTES % 16 != 0 and gt.UNALIGNED_BYTES < gt.NUM_FRAMES * 20000


@pytest.mark.parametrize("name,unaligned", CASES)
def test_most_streams_calibrate_and_one_does_not(runs, name, unaligned):
    ok = [gt.calibrates(runs[(name, unaligned, i, False)]) for i in range(len(gt.DONGLES))]
    print(name, "unaligned" if unaligned else "full", "calibrating streams:", [d for d, k in zip(gt.DONGLES, ok) if k])
    assert sum(ok) >= 4, ok
    assert not all(ok), ok


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("name", gt.RAMPS)
def test_reversed_ramp_taps_give_another_answer(runs, name, unaligned):
    """on at least one calibrating stream: a total ppm off by more than 100 x the parity bar, or another pos_info"""
    told = []
    for i in range(len(gt.DONGLES)):
        fwd, rev = runs[(name, unaligned, i, False)], runs[(name, unaligned, i, True)]
        if not gt.calibrates(fwd):
            continue
        ppm = any(abs(float(rev[k]) - float(fwd[k])) > 100.0 * (parity.PPM_RTOL * abs(float(fwd[k])) + parity.PPM_ATOL)
                  for k in ("total_sampling_ppm", "total_carrier_ppm"))
        pos = not np.array_equal(np.asarray(rev["pos_info"]), np.asarray(fwd["pos_info"]))
        print(name, "dongle", gt.DONGLES[i], "reversed taps: total carrier ppm", fwd["total_carrier_ppm"], "->",
              rev["total_carrier_ppm"], "| pos_info differs:", pos)
        told.append(ppm or pos)
    assert any(told), told
