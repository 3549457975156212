"""The hand-over of a call in flight (-m gpu): the slot's stream takes the context's stream position FIRST, and only then does the
context's stream wait for the call that used the slot `depth` calls ago.  What the contract of gsmcal_ctx_set_pipeline_depth
promises is checked from the caller's side at depth 2 and 4, with 2*depth + 1 consecutive calls on two 61-frame streams (a
26-frame capture is too short for the SCH stage: every stream ends with the same sentinel row, status 2, and the table
could not tell which of two captures a call has read; the scanner's captures are 26 frames):

  input order   work enqueued on the context's stream before call k (a device-to-device copy that overwrites the call's raw
                buffer with the capture it is meant to see) is complete when call k reads its input;
  output order  the outputs of call k - depth are complete in the context's stream order when call k returns (a copy of that
                table enqueued on the context's stream right behind call k, with nothing but that stream synchronised);
  mixed calls   a scanner call of 16 captures in flight between calibration calls returns the one-at-a-time bits.

The depth-1 tables the calls in flight must reproduce bit for bit are compared with the oracle once."""
import numpy as np
import pytest

import parity
from oracle import gsmcal_oracle as o

pytestmark = pytest.mark.gpu

FC = 957.4e6
FRAMES = 61
SCAN_FRAMES = 26


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


@pytest.fixture(scope="module")
def setup(g):
    s = g.synth
    coef, ts = s.fir1(46, 200e3 / s.FS), s.sch_training_sequence()
    # two different captures of two streams each (different dongles: different tables)
    caps = [np.stack([s.make_stream(dongle=d, num_frames=FRAMES)[0] for d in ds]) for ds in ((0, 3), (5, 6))]
    one = []
    for c in caps:                                                          # depth 1, default context
        ref = g.calibrate_batch(c, coef, ts, FC)
        det = g.last_batch_details(2)
        for i in range(2):
            parity.compare_stream(o.calibrate_stream(c[i], coef, ts, FC), ref["table"][i], det, i, ref["pos_info"][i])
        one.append(ref)
    assert all(ref["table"][i, 9] == 0.0 for ref in one for i in range(2))      # calibrated: finite ppm, different per stream
    assert not np.array_equal(one[0]["table"], one[1]["table"], equal_nan=True)
    return {"coef": coef, "ts": ts, "caps": caps, "one": one}


@pytest.mark.parametrize("depth", [2, 4])
def test_input_and_output_order_of_calls_in_flight(g, setup, depth):
    import torch
    dev = torch.device("cuda", 0)
    caps, one = setup["caps"], setup["one"]
    d, n = caps[0].shape[0], caps[0].shape[1] // 2
    calls = 2 * depth + 1
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        cx = g.Context(0, stream=st.cuda_stream)
        try:
            src = [torch.from_numpy(c).to(dev) for c in caps]
            # call k's raw buffer starts out holding the OTHER capture: a call that ran ahead of its copy would show it
            raws = [src[(k + 1) & 1].clone() for k in range(calls)]
            tabs = [torch.zeros((d, g.TABLE_COLS), dtype=torch.float64, device=dev) for _ in range(calls)]
            poss = [torch.zeros((d, 2, g.MAX_POS_ROWS), dtype=torch.float64, device=dev) for _ in range(calls)]
            rls = [torch.zeros((d,), dtype=torch.int64, device=dev) for _ in range(calls)]
            early = [torch.zeros((d, g.TABLE_COLS), dtype=torch.float64).pin_memory() for _ in range(calls)]
            torch.cuda.synchronize()
            cx.set_pipeline_depth(depth)
            for k in range(calls):
                raws[k].copy_(src[k & 1], non_blocking=True)                 # on the context's stream, in front of call k
                g.calibrate_batch_dev(raws[k].data_ptr(), d, n, setup["coef"], setup["ts"], FC, tabs[k].data_ptr(),
                                      poss[k].data_ptr(), None, rls[k].data_ptr(), ctx=cx)
                if k >= depth:                                               # call k - depth: complete in this stream's order
                    early[k - depth].copy_(tabs[k - depth], non_blocking=True)
                    st.synchronize()                                         # (that stream alone)
                    assert np.array_equal(early[k - depth].numpy(), one[(k - depth) & 1]["table"], equal_nan=True), (k, "output order")
            cx.sync()
            for k in range(calls):
                ref = one[k & 1]
                assert np.array_equal(tabs[k].cpu().numpy(), ref["table"], equal_nan=True), (k, "input order")
                assert np.array_equal(rls[k].cpu().numpy(), ref["r_len"]), k
                assert np.array_equal(poss[k].cpu().numpy(), ref["pos_info_raw"], equal_nan=True), k
        finally:
            cx.close()


@pytest.mark.parametrize("depth", [2, 4])
def test_a_scanner_call_in_flight_between_calibration_calls(g, setup, depth):
    import torch
    dev = torch.device("cuda", 0)
    s = g.synth
    caps, one = setup["caps"], setup["one"]
    d, n = caps[0].shape[0], caps[0].shape[1] // 2
    sweep = np.stack([s.make_stream(dongle=9300, arfcn=i, num_frames=SCAN_FRAMES, bcch=i % 3 != 2)[0] for i in range(16)])
    want = g.fcch_scan_batch(sweep, setup["coef"])        # the chain's own taps: no call joins the ones in flight to upload others
    want = np.stack([want["snr"], want["num_hit"]], axis=1)
    plan = ["cal"] * depth + ["scan"] + ["cal"] * depth
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        cx = g.Context(0, stream=st.cuda_stream)
        try:
            src = [torch.from_numpy(c).to(dev) for c in caps]
            sweep_t = torch.from_numpy(sweep).to(dev)
            sn = torch.full((16, 2), float("nan"), dtype=torch.float64, device=dev)
            tabs = [torch.zeros((d, g.TABLE_COLS), dtype=torch.float64, device=dev) for _ in plan]
            torch.cuda.synchronize()
            cx.set_pipeline_depth(depth)
            for k, kind in enumerate(plan):
                if kind == "scan":
                    g.fcch_scan_batch_dev(sweep_t.data_ptr(), 16, sweep.shape[1] // 2, setup["coef"], sn.data_ptr(), ctx=cx)
                else:
                    g.calibrate_batch_dev(src[k & 1].data_ptr(), d, n, setup["coef"], setup["ts"], FC, tabs[k].data_ptr(), ctx=cx)
            cx.sync()
            assert np.array_equal(sn.cpu().numpy(), want, equal_nan=True)
            for k, kind in enumerate(plan):
                if kind == "cal":
                    assert np.array_equal(tabs[k].cpu().numpy(), one[k & 1]["table"], equal_nan=True), k
        finally:
            cx.close()
