"""GPU tests of the row selection the demod family shares (-m gpu): FCCH_demod, BCCH_demod, SCH_decode and BCCH_decode pick
"the b-th row of pos_info that matches" with one wave-level selector (pos_rows in csrc/kernels_demod.h), 64 rows per step of a
144-row table.  Every other test puts its rows at the front of the table; here filler rows -- type 3 at position 1, which no
function selects -- push them to the chunk seams (63 | 64, 127 | 128), into the last chunk and to the last row, and a matching
row further up makes slot b differ from row b.

Per function the smallest designed stream of its restatement at oversampling ratio 2, and per table
  * the restatement finds on the table with fillers exactly what it finds on the table without (asserted, not assumed),
  * everything the function's own test file asserts against the restatement (its compare(), same bounds),
  * the counts equal the number of planted rows,
  * the batch row equals the single-stream call bit for bit.
A block of BCCH_decode is five rows: block rows at 62 (its bursts straddle the seam), 63, 64 and 139 (the last legal one), and a
type-1 row at 140 with type 2 in all the rows behind it, which is no block (140 + 4 is past the table) -- in the batch the table
behind it starts with the value 2.0, which a selector that read past the end of its own table would take for the fourth row."""
import numpy as np
import pytest

import bcch_decode_ref
import bcch_demod_ref
import fcch_demod_ref
import sch_decode_ref
from test_gpu_bcch_decode import compare as compare_bcch_decode
from test_gpu_bcch_demod import compare as compare_bcch_demod
from test_gpu_fcch_demod import compare as compare_fcch_demod, single_row as fcch_single_row
from test_gpu_sch_decode import compare as compare_sch_decode

pytestmark = pytest.mark.gpu

OV = 2
FC = 957.4e6
ROWS = 144                                       # GSMCAL_MAX_POS_ROWS: three 64-lane chunks, the last one 16 rows
FILLER = (1.0, 3.0)
SINGLE = (0, 63, 64, 127, 128, 143)              # either side of both seams, the first and the last row


@pytest.fixture(scope="module")
def g(gsmcal_mod):
    assert gsmcal_mod.MAX_POS_ROWS == ROWS
    return gsmcal_mod


@pytest.fixture(scope="module")
def own(g):
    """a context of its own: nothing is calibrated here, and the shared one's buffers stay as the other files left them"""
    c = g.Context(0)
    yield c
    c.close()


def spread(planted, at, fill=FILLER):
    """The planted rows (in their order) at the table indices `at`, fillers in front of each; the table ends with the last one."""
    assert len(planted) == len(at) and list(at) == sorted(set(at)) and at[-1] < ROWS
    t = np.tile(np.asarray(fill, dtype=np.float64), (at[-1] + 1, 1))
    t[list(at)] = planted
    return t


def raw_table(pos):
    t = -np.ones((2, ROWS))
    t[:, :len(pos)] = np.asarray(pos, dtype=np.float64).T
    return t


def same_bits(a, b):
    a, b = (np.ascontiguousarray(v, dtype=np.float64).view(np.uint64) for v in (a, b))
    return a.shape == b.shape and np.array_equal(a, b)


def same_result(a, b, keys):
    """two results of a restatement: the named entries equal, NaN at the same places"""
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def test_fcch_demod_rows_at_the_seams(g, own):
    s, pos = fcch_demod_ref.tone_windows(OV, 37)                     # three type-0 rows
    plain = fcch_demod_ref.fcch_demod(s, pos, OV, FC)
    tables = [spread(pos, at) for at in (SINGLE[:3], SINGLE[3:], (0, 64, 143), (63, 127, 128))]
    singles = []
    for t in tables:
        want = fcch_demod_ref.fcch_demod(s, t, OV, FC)
        same_result(want, plain, ("freq", "snr", "max_idx", "mean_freq", "carrier_ppm"))
        got = g.FCCH_demod(s, t, OV, FC, ctx=own)
        compare_fcch_demod(got, want, fs_rel=1e-6 * fcch_demod_ref.SYMBOL_RATE * OV)
        assert len(got["freq"]) == len(pos) == 3
        singles.append(fcch_single_row(g, got))
    tab = g.fcch_demod_batch(np.stack([s] * len(tables)), [len(s)] * len(tables), np.stack([raw_table(t) for t in tables]), OV, FC, ctx=own)
    for i, one in enumerate(singles):
        assert same_bits(tab[i], one), (i, tab[i][:8], one[:8])
    assert g.demod_rows(tab)["num_fcch"].tolist() == [3.0] * len(tables)


def test_bcch_demod_rows_at_the_seams(g, own):
    nts = g.synth.normal_training_sequences(OV)
    s, pos = bcch_demod_ref.designed_stream(g.synth, OV, [2, 2, 2, 2], nf=2)       # two type-0 rows, then four type-2 rows
    plain = bcch_demod_ref.bcch_demod(s, pos, nts, OV, FC)
    # the six rows at the six indices; the type-2 rows first (type 0 in the last chunk); type 0 either side of the first seam
    tables = [spread(pos, SINGLE), spread(pos[[2, 3, 4, 5, 0, 1]], SINGLE), spread(pos[[2, 0, 1, 3, 4, 5]], SINGLE)]
    singles = []
    for t in tables:
        want = bcch_demod_ref.bcch_demod(s, t, nts, OV, FC)
        same_result(want, plain, ("status", "idx", "num_bcch", "fo", "mean_fo", "max_idx", "peak", "runner_up", "phase", "num_agree"))
        got = g.BCCH_demod(s, t, nts, OV, FC, ctx=own)
        compare_bcch_demod(got, want, s, t, OV)
        assert got["num_bcch"] == 4 and got["status"] == 0 and got["idx"] == 3 and got["num_agree"] == 4
        singles.append(got)
    res = g.bcch_demod_batch(np.stack([s] * len(tables)), [len(s)] * len(tables), np.stack([raw_table(t) for t in tables]), OV, nts, FC,
                             ctx=own, want_corr=True, want_r=True)
    for i, one in enumerate(singles):
        assert same_bits(res["table"][i], one["row"]), (i, res["table"][i][:8], one["row"][:8])
        assert res["r_len"][i] == len(s) and same_bits(np.ascontiguousarray(res["r"][i]).view(np.float64), one["r"].view(np.float64))
        assert same_bits(np.ascontiguousarray(res["corr"][i, :4].T).view(np.float64), np.ascontiguousarray(one["corr_val"]).view(np.float64))
    assert g.bcch_rows(res["table"])["num_bcch"].tolist() == [4.0] * len(tables)


def test_sch_decode_rows_at_the_seams(g, own):
    ts = g.synth.gmsk_modulate(g.synth.diff_precode(g.synth.SCH_TRAINING_BITS), OV, g.synth.gmsk_frequency_pulse(sps=OV))
    s, pos, expect = sch_decode_ref.designed_case(OV, "clean")       # five type-1 rows
    plain = sch_decode_ref.sch_decode(s, pos, OV)
    tables = [spread(pos, SINGLE[:5]), spread(pos, SINGLE[1:]), spread(pos, (0, 63, 64, 128, 143))]
    singles = []
    for t in tables:
        want = sch_decode_ref.sch_decode(s, t, OV)
        same_result(want, plain, ("status", "num_sch", "num_ok", "num_consistent", "bsic", "fn_anchor", "pos_anchor", "ok", "fn", "soft", "u"))
        got = g.SCH_decode(s, t, ts, OV, ctx=own, want_soft=True)
        compare_sch_decode(got, want, s, t, OV)
        assert got["num_sch"] == 5 and got["status"] == 0 and got["ok"].tolist() == [1.0] * 5 and got["fn_anchor"] == expect["fn0"]
        singles.append(got)
    res = g.sch_decode_batch(np.stack([s] * len(tables)), [len(s)] * len(tables), np.stack([raw_table(t) for t in tables]), OV, ts,
                             ctx=own, want_soft=True, want_u=True)
    for i, one in enumerate(singles):
        assert same_bits(res["table"][i], one["row"]), (i, res["table"][i][:8], one["row"][:8])
        assert same_bits(res["soft"][i, :5], one["soft"]) and np.all(np.isnan(res["soft"][i, 5:]))
        assert np.array_equal(res["u"][i, :5], one["u"]) and np.all(res["u"][i, 5:] == 255)
    assert g.sch_rows(res["table"])["num_sch"].tolist() == [5.0] * len(tables)


def test_bcch_decode_blocks_at_the_seams(g, own):
    s, pos, tsc, expect = bcch_decode_ref.designed_case(OV, "good_bad")            # two blocks of five rows: the first decodes
    plain = bcch_decode_ref.bcch_decode(s, pos, tsc, OV)
    assert plain["num_blocks"] == 2 and plain["ok"].tolist() == [1.0, 0.0]
    first, second = pos[:5], pos[5:]
    tables, blocks = [], []
    for at in (62, 63, 64, 139):                                     # the first block at the front: slot 1 is not row 1
        tables.append(np.concatenate([first, spread(second, range(at - 5, at))]))
        assert bcch_decode_ref.block_rows(tables[-1]) == [0, at]
        blocks.append(2)
    tables.append(np.concatenate([first, spread(second[:4], range(135, 139))]))    # type 1 at 140, type 2 at 141..143: no block
    assert len(tables[-1]) == ROWS and tables[-1][140:, 1].tolist() == [1.0, 2.0, 2.0, 2.0]
    blocks.append(1)
    singles = []
    for t, nb in zip(tables, blocks):
        want = bcch_decode_ref.bcch_decode(s, t, tsc, OV)
        assert want["num_blocks"] == nb
        same_result({k: want[k][:nb] for k in ("ok", "pos", "soft", "octets")}, {k: plain[k][:nb] for k in ("ok", "pos", "soft", "octets")},
                    ("ok", "pos", "soft", "octets"))
        got = g.BCCH_decode(s, t, tsc, OV, ctx=own, want_soft=True)
        compare_bcch_decode(got, want, s, t, OV)
        assert got["num_blocks"] == nb and got["status"] == 0 and got["first_ok"] == 1 and got["ok"].tolist() == [1.0, 0.0][:nb]
        assert np.array_equal(got["octets"][0], bcch_decode_ref.DESIGNED_SI)
        singles.append(got)
    # the batch: behind the table whose row 140 is no block, one that starts with a filler at position 2.0 -- what a read of
    # "row 144" of the table before it would find
    last = spread(pos, range(62, 72), fill=(2.0, 3.0))
    batch = tables + [last]
    res = g.bcch_decode_batch(np.stack([s] * len(batch)), [len(s)] * len(batch), np.stack([raw_table(t) for t in batch]), OV, tsc,
                              ctx=own, want_soft=True)
    for i, (one, nb) in enumerate(zip(singles, blocks)):
        assert same_bits(res["table"][i], one["row"]), (i, res["table"][i][:8], one["row"][:8])
        assert np.array_equal(res["octets"][i, :nb], one["octets"]) and np.all(res["octets"][i, nb:] == 0)
        assert same_bits(res["soft"][i, :nb], one["soft"]) and np.all(np.isnan(res["soft"][i, nb:]))
    rows = g.si_rows(res["table"])
    assert rows["num_blocks"].tolist() == [float(nb) for nb in blocks] + [2.0] and rows["status"].tolist() == [0.0] * len(batch)
    one = g.BCCH_decode(s, last, tsc, OV, ctx=own, want_soft=True)
    compare_bcch_decode(one, bcch_decode_ref.bcch_decode(s, last, tsc, OV), s, last, OV)
    assert same_bits(res["table"][-1], one["row"])
