#!/usr/bin/env python3
"""One SHA-256 per output array of fcch_demod_batch, bcch_demod_batch, sch_decode_batch and bcch_decode_batch with every optional
output on, over one fixed input set: the chain cases the GPU tests calibrate (tests/sch_decode_ref.py, tests/bcch_decode_ref.py and
dongle 1, which the chain rejects) at 8x, and the designed streams of the four restatements at every oversampling ratio they
support.  Two builds of the library compute the same bits iff their digests are equal:

    python tools/demod_digest.py > new.txt;  GSMCAL_LIB=/path/to/other/libgsmcal.so python tools/demod_digest.py > other.txt
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
FC = 957.4e6


def main():
    import gsmcal
    import bcch_decode_ref
    import bcch_demod_ref
    import fcch_demod_ref
    import sch_decode_ref

    synth, ctx = gsmcal.synth, gsmcal.Context(0)
    print("# lib", os.path.basename(os.path.dirname(gsmcal.lib_path())) + "/" + os.path.basename(gsmcal.lib_path()))

    def table(pos):
        t = -np.ones((2, gsmcal.MAX_POS_ROWS))
        t[:, :len(pos)] = np.asarray(pos, dtype=np.float64).T
        return t[None]

    def digest(tag, res):
        for k, v in sorted(res.items() if isinstance(res, dict) else [("table", res)]):
            print(tag, k, v.shape, hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest())

    def run_all(tag, r, r_len, pos, ov, tsc, which="fbsd"):
        if "f" in which:
            digest(tag + " fcch_demod", gsmcal.fcch_demod_batch(r, r_len, pos, ov, FC, ctx=ctx))
        if "b" in which:
            digest(tag + " bcch_demod", gsmcal.bcch_demod_batch(r, r_len, pos, ov, synth.normal_training_sequences(ov), FC, ctx=ctx,
                                                                 want_corr=True, want_r=True))
        if "s" in which:
            digest(tag + " sch_decode", gsmcal.sch_decode_batch(r, r_len, pos, ov, np.zeros(64 * ov, complex), ctx=ctx, want_soft=True,
                                                                 want_u=True))
        if "d" in which:
            digest(tag + " bcch_decode", gsmcal.bcch_decode_batch(r, r_len, pos, ov, tsc, ctx=ctx, want_soft=True))

    # ---- the chain cases, calibrated here ----
    made = [synth.make_stream(**sch_decode_ref.chain_stream_args(name)) for name, *_ in sch_decode_ref.CHAIN_CASES]
    made += [synth.make_stream(**bcch_decode_ref.chain_stream_args(name)) for name, *_ in bcch_decode_ref.CHAIN_CASES]
    made += [synth.make_stream(dongle=1)]
    cal = gsmcal.calibrate_batch(np.stack([m[0] for m in made]), synth.fir1(46, 200e3 / synth.FS), synth.sch_training_sequence(), FC,
                                 want_r=True, ctx=ctx)
    print("# chain status", cal["table"][:, 9].tolist())
    run_all("chain", cal["r_correct"], cal["r_len"], cal["pos_info_raw"], 8, bcch_decode_ref.CHAIN_TSC)

    # ---- the designed streams ----
    for ov in (1, 2, 4, 8):
        for k in (37, -30):
            s, pos = fcch_demod_ref.tone_windows(ov, k)
            run_all("tone ov%d k%d" % (ov, k), s[None], [len(s)], table(pos), ov, 0, "f")
        for codes in ([6, 6, 6, 6], [2, 2, 5, 2], list(range(8))):
            s, pos = bcch_demod_ref.designed_stream(synth, ov, codes)
            run_all("tsc ov%d %s" % (ov, "".join(map(str, codes))), s[None], [len(s)], table(pos), ov, 0, "fb")
        if ov in bcch_decode_ref.SUPPORTED_OV:
            for kind in sch_decode_ref.DESIGNED_KINDS:
                s, pos, _ = sch_decode_ref.designed_case(ov, kind)
                run_all("sch ov%d %s" % (ov, kind), s[None], [len(s)], table(pos), ov, 0, "s")
            for kind in bcch_decode_ref.DESIGNED_KINDS:
                s, pos, tsc, _ = bcch_decode_ref.designed_case(ov, kind)
                run_all("si ov%d %s" % (ov, kind), s[None], [len(s)], table(pos), ov, tsc, "sd")
    ctx.close()


if __name__ == "__main__":
    main()
