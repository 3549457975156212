#!/usr/bin/env python3
"""One SHA-256 per output array of the resampling chain, over one fixed input set, on every route that evaluates it.  Two builds
of the library compute the same bits iff their digests are equal:

    python tools/chain_digest.py > new.txt;  GSMCAL_LIB=/path/to/other/libgsmcal.so python tools/chain_digest.py > other.txt

calibrate_batch (device-pointer form, outputs zeroed before the call so that the WHOLE r_correct is hashed): table, pos_info, r_len,
r_correct and last_batch_details, for the batches of tests/tail_gathers.py and the 31-tap, asymmetric-47-tap and 769-tap filters of
tests/general_taps.py, on the default route, with GSMCAL_FUSE_POST=0, with GSMCAL_FUSE_GATHER=0 and at pipeline depth 4 (five calls).
The per-function entry points FCCH_fine_correction, SCH_corr_rate_correction and carrier_correct_post_SCH (k_gather at every level
and source kind) at 8, 4 and 2 samples per symbol on the two captures of tests/geometry_cases.py: every output, r included."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def sha(v):
    v = np.ascontiguousarray(np.asarray(v))
    return "%s %s %s" % (v.dtype, v.shape, hashlib.sha256(v.tobytes()).hexdigest())


def main():
    import torch

    import gsmcal
    import general_taps as gt
    import geometry_cases as gc
    import tail_gathers as tg

    synth = gsmcal.synth
    ts = synth.sch_training_sequence()
    print("# lib", os.path.basename(os.path.dirname(gsmcal.lib_path())) + "/" + os.path.basename(gsmcal.lib_path()))
    dev = torch.device("cuda", 0)

    def batch_route(tag, order, env, depth):
        """tests/test_gpu_tail_gathers.py's run_dev with r_correct: the calls of `order` on one fresh context"""
        st = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(st):
            cx = tg.context_under(gsmcal, env, stream=st.cuda_stream)
            try:
                on_dev = {}
                for raw, _ in order:
                    if id(raw) not in on_dev:
                        on_dev[id(raw)] = torch.from_numpy(raw).to(dev)
                st.synchronize()
                if depth > 1:
                    cx.set_pipeline_depth(depth)
                outs = []
                for raw, taps in order:
                    t = on_dev[id(raw)]
                    d, n = t.shape[0], t.shape[1] // 2
                    tab = torch.zeros((d, gsmcal.TABLE_COLS), dtype=torch.float64, device=dev)
                    pos = torch.zeros((d, 2, gsmcal.MAX_POS_ROWS), dtype=torch.float64, device=dev)
                    rl = torch.zeros((d,), dtype=torch.int64, device=dev)
                    rc = torch.zeros((d, n), dtype=torch.complex128, device=dev)
                    st.synchronize()                      # (the zeros are in place before the library's stream work starts)
                    gsmcal.calibrate_batch_dev(t.data_ptr(), d, n, taps, ts, tg.FC, tab.data_ptr(), pos.data_ptr(), rc.data_ptr(), rl.data_ptr(), ctx=cx)
                    outs.append((tab, pos, rl, rc))
                cx.sync()
                det = gsmcal.last_batch_details(len(order[-1][0]), ctx=cx)
                for c, (tab, pos, rl, rc) in enumerate(outs):
                    for k, v in (("table", tab), ("pos_info", pos), ("r_len", rl), ("r_correct", rc)):
                        print(tag, "call%d" % c, k, sha(v.cpu().numpy()))
                for k in sorted(det):
                    print(tag, "details", k, sha(det[k]))
            finally:
                cx.close()

    batches = tg.build()
    plain = batches["plain"][0]
    batches["fir769"] = (plain, gt.FILTERS["fir769"])
    routes = (("default", {}, 1), ("fuse_post0", {"GSMCAL_FUSE_POST": "0"}, 1), ("fuse_gather0", {"GSMCAL_FUSE_GATHER": "0"}, 1), ("depth4", {}, 4))
    for name in ("plain", "ppm", "ends", "copy", "fir31", "ramp47", "fir769", "other"):
        for route, env, depth in routes:
            batch_route("batch %s %s" % (name, route), [batches[name]] * (5 if depth > 1 else 1), env, depth)
    batch_route("batch plain|other depth4", [batches["plain"], batches["other"]] * 4, {}, 4)

    # ---- function by function: gather_core at every level, array source ----
    ctx = gsmcal.Context(0)
    bases = gc.ov_base_streams()
    for name in ("plain", "ppm"):
        for ov in (8, 4, 2):
            r = bases[name] if ov == 8 else gc.resample(bases[name], ov)
            tag = "functions %s ov%d" % (name, ov)
            cp, cs = gsmcal.FCCH_coarse_position(r[0::8 * ov], 8, ctx=ctx)
            fp, r1, sp1, cp1 = gsmcal.FCCH_fine_correction(r, cp, ov, gc.FC, ctx=ctx)
            pi, r2, sp2 = gsmcal.SCH_corr_rate_correction(r1, fp, gc.training_sequence(ov), ov, ctx=ctx)
            r3, cp2 = gsmcal.carrier_correct_post_SCH(r2, pi, ov, gc.FC, ctx=ctx)
            for k, v in (("coarse_pos", cp), ("coarse_snr", cs), ("fcch_pos", fp), ("r1", r1), ("sp1", sp1), ("cp1", cp1), ("pos_info", pi),
                         ("r2", r2), ("sp2", sp2), ("r3", r3), ("cp2", cp2)):
                print(tag, k, sha(v))
    ctx.close()


if __name__ == "__main__":
    main()
