"""The batches of tests/tail_gathers.py, held to their design with the oracle alone: every batch takes at least one stream
through the SCH stage (so no comparison of tests/test_gpu_tail_gathers.py is empty), the `ends` batch sits on the :40
threshold of SCH_corr_rate_correction.m, the `copy` batch skips the SCH resampling, the `ppm` batch carries the errors it
was built with.  No GPU."""
import numpy as np
import pytest

import tail_gathers as tg


@pytest.fixture(scope="module")
def batches():
    return tg.build()


@pytest.fixture(scope="module")
def oracles(batches):
    return {name: tg.oracle_batch(raw, taps) for name, (raw, taps) in batches.items()}


def test_shapes(batches):
    for name, (raw, _) in batches.items():
        assert raw.dtype == np.uint8 and 3 <= len(raw) <= 4 and raw.shape[1] <= 2 * tg.NUM_FRAMES * 10000, name
    assert batches["plain"][0].shape[1] % 16 != 0, "the plain batch should sit on an unaligned capture length"
    assert batches["plain"][0].shape == batches["other"][0].shape
    assert len(batches["fir31"][1]) == 31 and len(batches["ramp47"][1]) == 47
    assert not np.array_equal(batches["ramp47"][1], batches["ramp47"][1][::-1])


def test_every_batch_reaches_the_sch_stage(oracles):
    for name, orcs in oracles.items():
        assert all(o is not None for o in orcs), f"{name}: the reference stops with an index error"
        assert any(tg.through_sch(o) for o in orcs), f"{name}: no stream reaches the SCH stage in the oracle"
    for name in ("other", "copy", "ppm"):
        assert all(o["status"] == 0 and len(o["sch_first_round_pos"]) >= 5 for o in oracles[name]), name
    st = [o["status"] for o in oracles["plain"]]
    assert st == [0, 6, 0], f"plain: two calibrating streams around one that leaves at the fine stage's SNR gate: {st}"


def test_ends_batch_sits_on_the_threshold(oracles):
    short, fit, full = oracles["ends"]
    n = [len(o["sch_first_round_pos"]) for o in (short, fit, full)]
    assert n[1] == n[0] + 1 and n[2] == n[1], f"SCH windows at ENDS_FIT - 1, ENDS_FIT, 11500: {n}"
    assert all(len(o["fine_first_round_pos"]) >= n[1] for o in (short, fit, full))


def test_copy_batch_skips_the_sch_resampling(oracles):
    assert all(tg.through_sch(o) and o["sampling_ppm"][1] == 0.0 for o in oracles["copy"])
    assert any(o["sampling_ppm"][1] != 0.0 for o in oracles["plain"]), "and the plain batch resamples (LERP at level 3)"


def test_ppm_batch_carries_its_errors(oracles):
    for (_, sp, cp), o in zip(tg.PPM_STREAMS, oracles["ppm"]):
        assert abs(o["total_sampling_ppm"] - sp) < 5.0 and abs(o["total_carrier_ppm"] - cp) < 5.0, (sp, cp, o["total_sampling_ppm"], o["total_carrier_ppm"])
