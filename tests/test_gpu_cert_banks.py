"""GPU tests (-m gpu) of k_fine_cert's conflict-free LDS maps (csrc/fc_layout.h): the slide phase deals the chunks round the slide
waves (wave w walks chunks w, w + nslide, ...: neighbouring chunks now sit in DIFFERENT waves) and the E/C scans take shift
l + 64 u in lane l, with the prefix sums formed across the lanes by DPP.  Neither changes what is computed: (P*, t*, k*) is the
first maximum over all (shift, bin) whichever lane finds it, and E and C feed only the certificate (which chunks k_fine_chunk /
k_fine_verify still sweep).  So every output must be what the routes without the certificate give, and what the oracle gives, bit
for bit.  tests/test_fc_banks_cpu.py holds the maps themselves to the bank rule, without a GPU.

Reference geometry (k_fine_cert<8, 47>, two slide waves, the E wave and the C wave) through the batch entry, 48-frame captures as
in tests/test_gpu_cert_roles.py (the shortest whole number of frames on which the chain completes):
  high         30 dB: every window certified at once
  low          6.5 dB: the certificate leaves chunks open in front of and behind t*
  end          the fifth fine window ends 32 samples in front of the capture's last one (the nearest the reference admits:
               FCCH_fine_correction.m:35); the last raw chunk the kernel stages is not a whole one
  const_near   300 samples at the head of the third fine window hold one byte value: a run of exactly equal filtered samples, so
               the powers p of neighbouring shifts tie exactly across chunk borders -- chunks that now belong to different waves --
               and the lowest shift has to win in the wave and the block reduction
General geometry (k_fine_cert<0, 0>) through FCCH_fine_correction at 4 samples per symbol (one slide wave, three idle: split), 5
(odd ratio: 80 slide lanes, two slide waves of five groups each, odd FC_XP pad steps), 12 (three slide waves, one idle: block scan)
and 16 (four slide waves fill the block), each against the route without the certificate."""
import numpy as np
import pytest

import geometry_cases as gc
import parity
import worstcase as wc
from oracle import gsmcal_oracle as o

pytestmark = pytest.mark.gpu

FC = 957.4e6
FRAMES = 48
NAMES = ("high", "low", "end", "const_near")


def slide_waves(ov):
    """csrc/fc_layout.h fc_threads, fc_nslide: (waves of the block, waves that hold slide lanes)"""
    nslide = (8 * (128 * ov // 64) + 63) // 64
    return max(256, nslide * 64) // 64, nslide


@pytest.fixture(scope="module")
def g(gsmcal_mod, ctx):
    return gsmcal_mod


@pytest.fixture(scope="module")
def setup(g):
    s = g.synth
    return {"coef": s.fir1(46, 200e3 / s.FS), "ts": s.sch_training_sequence()}


@pytest.fixture(scope="module")
def batch(g, setup):
    """the four captures and the oracle's calibrate_stream of each (computed once, never changed)"""
    s, coef, ts = g.synth, setup["coef"], setup["ts"]
    caps = {"high": s.make_stream(dongle=0, num_frames=FRAMES, start_frame=8, frac_start=8000.0, snr_db=30.0)[0],
            "low": s.make_stream(dongle=0, num_frames=FRAMES, start_frame=8, frac_start=8000.0, snr_db=6.5)[0],
            "end": s.make_stream(dongle=1, num_frames=FRAMES, start_frame=43, frac_start=1704.0, snr_db=30.0, sampling_ppm=0.0)[0]}
    pos = np.atleast_1d(o.FCCH_coarse_position(o.front_end(caps["high"], coef)[0::64], 8)[0])
    ws = (int(pos[2]) - 65) * 8                            # FCCH_fine_correction.m:40, 0-based: the third window's first sample
    made = wc.constant_stretch_captures(caps["high"], starts=(ws,), length=300, level=int(round(float(np.mean(caps["high"][0::2])))))
    caps["const_near"] = next(v for k, v in made.items() if k.startswith("near_mean"))
    raw = np.stack([caps[k] for k in NAMES])
    orc = parity.pool_map(parity.oracle_job, [(c, coef, ts, FC) for c in raw])
    return {"raw": raw, "orc": orc, "stretch": ws}


@pytest.fixture(scope="module")
def routes(g, setup, batch):
    """route -> outputs of the batch: default, GSMCAL_CERT=0, GSMCAL_PRESCREEN=0 (read when a context is made), and four calls in
    flight on a context of depth 4"""
    import torch
    dev = torch.device("cuda", 0)
    mp = pytest.MonkeyPatch()
    made, out = {}, {}
    raw, coef, ts = batch["raw"], setup["coef"], setup["ts"]
    d, n = raw.shape[0], raw.shape[1] // 2
    try:
        for name, var in (("no_cert", "GSMCAL_CERT"), ("no_prescreen", "GSMCAL_PRESCREEN")):
            mp.setenv(var, "0")
            made[name] = g.Context(0)
            mp.delenv(var)
        out["default"] = {"cal": g.calibrate_batch(raw, coef, ts, FC), "det": g.last_batch_details(d)}
        for name, cx in made.items():
            out[name] = {"cal": g.calibrate_batch(raw, coef, ts, FC, ctx=cx), "det": g.last_batch_details(d, ctx=cx)}
        st = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(st):
            cx = made["depth4"] = g.Context(0, stream=st.cuda_stream)
            raw_t = torch.from_numpy(raw).to(dev)
            tabs = [torch.zeros((d, g.TABLE_COLS), dtype=torch.float64, device=dev) for _ in range(4)]
            poss = [torch.zeros((d, 2, g.MAX_POS_ROWS), dtype=torch.float64, device=dev) for _ in range(4)]
            rls = [torch.zeros((d,), dtype=torch.int64, device=dev) for _ in range(4)]
            cx.set_pipeline_depth(4)
            for k in range(4):
                g.calibrate_batch_dev(raw_t.data_ptr(), d, n, coef, ts, FC, tabs[k].data_ptr(), poss[k].data_ptr(), None, rls[k].data_ptr(), ctx=cx)
            cx.sync()
            out["depth4"] = [{"table": tabs[k].cpu().numpy(), "pos_info_raw": poss[k].cpu().numpy(), "r_len": rls[k].cpu().numpy()}
                             for k in range(4)]
        yield out
    finally:
        mp.undo()
        for cx in made.values():
            cx.close()


def test_the_captures_are_what_they_are_named_for(batch):
    orc = dict(zip(NAMES, batch["orc"]))
    print({k: (r["status"], len(r["fine_first_round_pos"])) for k, r in orc.items()})
    assert orc["high"]["status"] == 0 and orc["low"]["status"] == 0 and orc["const_near"]["status"] == 0
    assert all(len(r["fine_first_round_pos"]) == 5 for r in orc.values())        # five fine windows each
    len_s = FRAMES * 1250
    last = float(np.atleast_1d(orc["end"]["coarse_pos"])[-1])
    assert last + 64 == len_s - 148 + 1 - 4                # :35 holds with 4 symbols = 32 samples to spare; positions come in steps of 8
    c, ws = batch["raw"][NAMES.index("const_near")], batch["stretch"]
    assert len(set(c[2 * ws: 2 * (ws + 300): 2])) == 1 and len(set(c[2 * ws + 1: 2 * (ws + 300): 2])) == 1
    # 300 equal bytes less the filter's 46 samples of memory: more than three chunks of 64 shifts start on exactly equal samples
    assert (300 - 46) // 64 >= 3
    assert slide_waves(8) == (4, 2)                        # two slide waves: even chunks in wave 0, odd chunks in wave 1


def _cut_pos_info(row, pos_raw):
    k = int(row[7])
    return -np.ones((k, 2)) if row[8] == -1.0 else pos_raw[:, :k].T.copy()


def test_the_default_route_matches_the_oracle(batch, routes):
    r = routes["default"]
    for i, nm in enumerate(NAMES):
        print(nm, r["det"]["counts"][i], r["cal"]["table"][i, 6:10])
        parity.compare_stream(batch["orc"][i], r["cal"]["table"][i], r["det"], i, r["cal"]["pos_info"][i])


@pytest.mark.parametrize("other", ["no_cert", "no_prescreen"])
def test_the_certificate_changes_no_output(routes, other):
    a, b = routes["default"]["cal"], routes[other]["cal"]
    for key in ("table", "pos_info_raw", "r_len"):
        assert np.array_equal(a[key], b[key], equal_nan=True), (other, key)
    for key in ("fine_first", "fcch_pos", "sch_first", "counts"):
        assert np.array_equal(routes["default"]["det"][key], routes[other]["det"][key], equal_nan=True), (other, key)


def test_four_calls_in_flight_give_the_outputs_of_one(batch, routes):
    a = routes["default"]["cal"]
    for k, call in enumerate(routes["depth4"]):
        for key in ("table", "pos_info_raw", "r_len"):
            assert np.array_equal(a[key], call[key], equal_nan=True), (k, key)
        for i in range(len(NAMES)):
            parity.assert_positions(_cut_pos_info(call["table"][i], call["pos_info_raw"][i]), a["pos_info"][i], f"call {k}, {NAMES[i]}")


# ---- general geometry: k_fine_cert<0, 0> ----------------------------------------------------------------------------------
GEOM = {4: (4, 1), 5: (4, 2), 12: (4, 3), 16: (4, 4)}      # ov -> (waves, slide waves): split / split, odd ratio / one idle wave / full block


@pytest.fixture(scope="module")
def geom_contexts(g):
    mp = pytest.MonkeyPatch()
    made = {"default": g.Context(0)}
    mp.setenv("GSMCAL_CERT", "0")
    try:
        made["no_cert"] = g.Context(0)
    finally:
        mp.undo()
    for cx in made.values():
        cx.profile_enable()
    yield made
    for cx in made.values():
        cx.close()


@pytest.fixture(scope="module")
def base8():
    return gc.ov_base_streams()["plain"]


@pytest.mark.parametrize("ov", sorted(GEOM))
def test_general_geometry_against_the_route_without_the_certificate(g, geom_contexts, base8, ov):
    assert slide_waves(ov) == GEOM[ov]
    r = gc.resample(base8, ov)
    got = {}
    for name, cx in geom_contexts.items():
        cp, _ = g.FCCH_coarse_position(r[0::8 * ov], 8, ctx=cx)
        cx.profile_reset()
        fp, _, sp, cpm = g.FCCH_fine_correction(r, cp, ov, FC, ctx=cx, want_r=False)
        names = {k: v[1] for k, v in cx.profile_get().items() if v[1]}
        det = g.last_batch_details(1, ctx=cx)
        got[name] = (np.atleast_1d(fp), float(sp), float(cpm), det["fine_first"][0, :det["counts"][0, 1]].copy())
        print(ov, name, sorted(names.items()), got[name][0], sp, cpm)
        ncert = sum(v for k, v in names.items() if "k_fine_cert<0, 0>" in k)
        assert ncert == (1 if name == "default" else 0), names
        assert sum(v for k, v in names.items() if "k_fine_openall" in k) == (0 if name == "default" else 1), names
    a, b = got["default"], got["no_cert"]
    assert len(a[3]) >= 5 and np.array_equal(a[3], b[3]) and np.array_equal(a[0], b[0])
    assert np.array([a[1]]).tobytes() == np.array([b[1]]).tobytes() and np.array([a[2]]).tobytes() == np.array([b[2]]).tobytes()
