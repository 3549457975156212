"""GPU test of the raw scanners above one grid of captures (-m gpu): gsmcal_band_power_batch, gsmcal_subband_power_batch and
gsmcal_cw_check_batch cut a batch into grids of at most 65 535 captures (the y limit of a launch) and offset every per-capture
buffer by hand for each further grid.  A batch of 65 535 + 3 captures runs the second grid; the captures on both sides of the cut
must carry the bits they have in a batch of five -- the "any position, any batch size" contract of test_reproducible_*."""
import numpy as np
import pytest

import gsmcal.dist  # noqa: F401

pytestmark = pytest.mark.gpu

D = 65535 + 3
N = 64
PICK = [0, 65534, 65535, 65536, 65537]
THR = 0.5


@pytest.fixture(scope="module")
def raw():
    """65 538 captures of 64 samples, seeded random bytes (8.4 MB): made once, shared, read-only"""
    a = np.random.default_rng(65535).integers(0, 256, size=(D, 2 * N), dtype=np.uint8)
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def coef():
    """32 exactly mirrored taps (the symmetric 32-tap kernel instance)"""
    h = np.hamming(32)[:16] * np.sinc((np.arange(16) - 15.5) * 0.2)
    c = np.concatenate([h, h[::-1]])
    assert np.array_equal(c, c[::-1])
    return c / c.sum()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_band_power_beyond_one_grid_of_captures(g_mod, ctx, raw, coef):
    big = g_mod.band_power_batch(raw, coef, 5, ctx=ctx)
    five = g_mod.band_power_batch(raw[PICK], coef, 5, ctx=ctx)
    assert big.shape == (D,) and np.all(five > 0.0)
    assert same_bits(big[PICK], five), (big[PICK], five)


def test_subband_power_beyond_one_grid_of_captures(g_mod, ctx, raw, coef):
    w = np.tile(np.array([0.3, np.nan, -1.1]), (D, 1))
    w[1::2, 0] = 0.7                                                             # neighbours differ from capture to capture
    big = g_mod.subband_power_batch(raw, coef, w, decim=5, ctx=ctx)
    five = g_mod.subband_power_batch(raw[PICK], coef, w[PICK], decim=5, ctx=ctx)
    assert big.shape == (D, 3) and np.all(np.isnan(five[:, 1])) and np.all(five[:, [0, 2]] > 0.0)
    assert same_bits(big[PICK], five), (big[PICK], five)


def test_cw_check_beyond_one_grid_of_captures(g_mod, ctx, raw):
    big_s, big_r = g_mod.cw_check_batch(raw, THR, want_r=True, ctx=ctx)
    five_s, five_r = g_mod.cw_check_batch(raw[PICK], THR, want_r=True, ctx=ctx)
    assert big_r.shape == (D, N - 1) and np.all(np.isfinite(five_r)) and np.any(five_r != 0.0)
    assert same_bits(big_s[PICK], five_s), (big_s[PICK], five_s)
    assert same_bits(big_r[PICK], five_r)
