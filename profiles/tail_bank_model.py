#!/usr/bin/env python3
"""Per-site LDS bank-conflict model of the four-launch tail at the reference geometry -- k_window_sch<8, 512, 47> and
k_burst_tone<1|0, 8, 47> (csrc/kernels_estim.h, the lean gathers and the transforms they call) -- and of k_fine_chunk
(csrc/kernels_detect.h), by the rule and the evaluator of
profiles/fc_bank_model.py.  Pure arithmetic on the kernels' address expressions; nothing here touches a GPU.

Data-dependent addresses are taken at the chain's usual values: resampling factors within 1e-4 of 1 (lane i interpolates between
samples i and i + 1), the tone's prior bin at 37 (symbol rate / 4) or at the bin given with --bin, staging offset 3.

    python profiles/tail_bank_model.py [--bin K] [--sch-windows N] [--burst-windows N]
"""
import sys
from collections import defaultdict

from fc_bank_model import extra

NT = 512


class Table:
    def __init__(self):
        self.rows = defaultdict(lambda: [0, 0, 0])

    def add(self, site, kind, fn, nthr=NT):
        for w in range(nthr // 64):
            addr = {l: fn(64 * w + l) for l in range(64)}
            addr = {l: a for l, a in addr.items() if a is not None}
            if addr:
                e, wy = extra(kind, addr)
                r = self.rows[site]
                r[0] += 1; r[1] += e; r[2] = max(r[2], wy)

    def show(self, title, windows, measured_inst, measured_conf):
        print(f"### {title}")
        print("| site | wave instr | ways | extra / workgroup |")
        print("|---|---|---|---|")
        for s, r in self.rows.items():
            print(f"| {s} | {r[0]} | {r[2]} | {r[1]} |")
        ins = sum(r[0] for r in self.rows.values()); tot = sum(r[1] for r in self.rows.values())
        print(f"| **total** | {ins} | | **{tot}** |")
        print(f"{tot} x {windows} working workgroups = {tot * windows / 1e6:.3f} M per launch, measured {measured_conf / 1e6:.3f} M "
              f"({100.0 * (tot * windows - measured_conf) / measured_conf:+.0f} %); modelled LDS instructions {ins * windows / 1e6:.3f} M "
              f"of {measured_inst / 1e6:.3f} M measured\n")


def xs_pad(p):
    return p + (p >> 2)


def gather_carve(length, level, ntaps, compact):
    bufn = length + 40
    span_max = length + 8 + ntaps + 24
    xs_n = span_max + 16 if compact else span_max + span_max // 4 + 16
    r1 = max(bufn, xs_n)
    off_region1 = bufn * 16
    off_coef = off_region1 + r1 * 16
    off_raw = off_coef + ((ntaps + 3) & ~3) * 8
    total = (off_raw + ((span_max + 7) & ~7) * 2 + 15) & ~15
    off_rot = off_raw
    rot_end = off_rot + (1 + 72 + 32) * 16
    if level >= 2 and rot_end > total:
        total = (rot_end + 15) & ~15
    return dict(bufn=bufn, r1=off_region1, coef=off_coef, rot=off_rot, total=total)


def window_sch(off=3):
    t = Table()
    L, NTAPS, NSH, LT = 600, 47, 89, 512
    gc = gather_carve(L, 2, NTAPS, False)
    BUF0, BUF1, CS, T = 0, gc["r1"], gc["coef"], gc["rot"]
    cnt0 = L + 1
    span = cnt0 + NTAPS - 1
    nchunk = (off + span + 15) >> 3
    for u in range(8):
        t.add("sch_gather_fast: staged input stores (w128, lanes 10 slots apart)", "w128",
              lambda tid, u=u: BUF1 + xs_pad(8 * tid - off + u) * 16 if tid < nchunk and 0 <= 8 * tid - off + u < span + 8 else None)
    nwc = (nchunk + 63) >> 6
    t.add("sch_gather_fast: rotator table and tap stores", "w128",
          lambda tid: T + (tid - 64 * nwc) * 16 if 0 <= tid - 64 * nwc < 52 else None)
    t.add("sch_gather_fast: rotator table and tap stores", "w64",
          lambda tid: CS + (tid - 64 * nwc - 64) * 8 if 0 <= tid - 64 * nwc - 64 < 48 else None)
    act = lambda tid: 4 * tid < cnt0
    for k in range(4):
        t.add("fir4_lds: sample reads (r128, lanes 5 slots apart)", "r128", lambda tid, k=k: BUF1 + (xs_pad(4 * tid) + k) * 16 if act(tid) else None)
    for tr in range(12):
        for h in range(2):
            t.add("fir4_lds: tap reads (r128, one address)", "r128", lambda tid, tr=tr, h=h: CS + (4 * tr + 2 * h) * 8 if act(tid) else None)
        for k in range(4):
            t.add("fir4_lds: sample reads (r128, lanes 5 slots apart)", "r128",
                  lambda tid, tr=tr, k=k: BUF1 + (xs_pad(4 * tid + 4 * tr + 4) + k) * 16 if act(tid) else None)
    for k in range(4):
        t.add("sch_gather_fast: level-0 stores (w128, lanes 4 slots apart)", "w128",
              lambda tid, k=k: BUF0 + (4 * tid + k) * 16 if 4 * tid + k < cnt0 else None)
    for r in range(2):
        i_of = lambda tid, r=r: tid + 512 * r if tid + 512 * r < L else None
        for d in range(2):
            t.add("sch_gather_fast: interpolation reads (r128, consecutive)", "r128",
                  lambda tid, d=d: None if i_of(tid) is None else BUF0 + (i_of(tid) + d) * 16)
        t.add("sch_gather_fast: rotator reads S, A[i >> 5], B[i & 31] (r128)", "r128", lambda tid: None if i_of(tid) is None else T)
        t.add("sch_gather_fast: rotator reads S, A[i >> 5], B[i & 31] (r128)", "r128",
              lambda tid: None if i_of(tid) is None else T + (1 + (i_of(tid) >> 5)) * 16)
        t.add("sch_gather_fast: rotator reads S, A[i >> 5], B[i & 31] (r128)", "r128",
              lambda tid: None if i_of(tid) is None else T + (1 + 72 + (i_of(tid) & 31)) * 16)
        t.add("sch_gather_fast: window stores (w128, consecutive)", "w128", lambda tid: None if i_of(tid) is None else BUF1 + i_of(tid) * 16)
    # sch_corr_rows<89, 512>
    R, Q, M = 4, 16, 39
    NG = (NSH + R - 1) // R
    PADL, NTC, WL = R * NG, R * NG + Q * M, NSH - 1 + LT
    TC = gc["total"]
    CV = TC + (LT + NSH * 4) * 16
    for r in range(2):
        t.add("sch_corr_rows: padded tap copy and zero stores (w128, consecutive)", "w128",
              lambda tid, r=r: TC + (tid + 512 * r) * 16 if tid + 512 * r < NTC else None)
    t.add("sch_corr_rows: padded tap copy and zero stores (w128, consecutive)", "w128", lambda tid: BUF1 + (WL + tid) * 16 if WL + tid < Q * M else None)
    on = lambda tid: tid < NG * Q
    for s in (-1, -2, -3):
        t.add("sch_corr_rows: tap reads tp[s] (r128: stretches 39 slots apart, offset groups 4 apart)", "r128",
              lambda tid, s=s: TC + (PADL + (tid & 15) * M - R * (tid >> 4) + s) * 16 if on(tid) else None)
    for s in range(M):
        t.add("sch_corr_rows: sample reads xp[s] (r128: stretches 39 slots apart, 4 rows per address)", "r128",
              lambda tid, s=s: BUF1 + ((tid & 15) * M + s) * 16 if on(tid) else None)
        t.add("sch_corr_rows: tap reads tp[s] (r128: stretches 39 slots apart, offset groups 4 apart)", "r128",
              lambda tid, s=s: TC + (PADL + (tid & 15) * M - R * (tid >> 4) + s) * 16 if on(tid) else None)
    t.add("sch_corr_rows: power stores, argmax reads (w64 / r64)", "w64",
          lambda tid: CV + (R * (tid >> 4) + (tid & 15)) * 8 if on(tid) and (tid & 15) < R and R * (tid >> 4) + (tid & 15) < NSH else None)
    for r in range(2):
        t.add("sch_corr_rows: power stores, argmax reads (w64 / r64)", "r64", lambda tid, r=r: CV + (tid + 64 * r) * 8 if tid < 64 and tid + 64 * r < NSH else None)
    return t


def burst_tone(gate, kbin, jm):
    """level 1 (GATE = 1, bursts of the fine stage) / level 3 (GATE = 0); kbin: the prior bin; jm: the winning bin's shift"""
    t = Table()
    N, N2, LDB = 1184, 32, 33
    gc = gather_carve(N, 1 if gate else 3, 47, True)
    BUF0, BUF1 = 0, gc["r1"]
    T = gc["rot"]
    W37 = gc["total"]
    WN2 = W37 + 40 * 16
    P = WN2 + N2 * 16
    rounds = lambda n: range((n + NT - 1) // NT)
    idx = lambda tid, r, n: tid + NT * r if tid + NT * r < n else None
    for r in rounds(N):
        t.add("burst_gather_fast: twiddle table and window stores (w128, consecutive)", "w128", lambda tid, r=r: None if idx(tid, r, N) is None else BUF1 + idx(tid, r, N) * 16)
        t.add("burst_gather_fast: twiddle table and window stores (w128, consecutive)", "w128", lambda tid, r=r: None if idx(tid, r, N) is None else BUF0 + idx(tid, r, N) * 16)
    if not gate:        # level 3: level 1 into buf1, rotated pairs read back (consecutive), table reads as in sch_gather_fast
        for r in rounds(N):
            t.add("burst_gather_fast: level-1 stores (w128, consecutive)", "w128", lambda tid, r=r: None if idx(tid, r, N) is None else BUF1 + idx(tid, r, N) * 16)
            for d in range(2):
                t.add("burst_gather_fast: level-1 reads for level 3 (r128, consecutive)", "r128",
                      lambda tid, r=r, d=d: None if idx(tid, r, N) is None else BUF1 + (idx(tid, r, N) + d) * 16)
                t.add("burst_gather_fast: rotator reads S, A[i >> 5], B[i & 31] (r128)", "r128", lambda tid, r=r: None if idx(tid, r, N) is None else T)
                t.add("burst_gather_fast: rotator reads S, A[i >> 5], B[i & 31] (r128)", "r128",
                      lambda tid, r=r, d=d: None if idx(tid, r, N) is None else T + (1 + ((idx(tid, r, N) + d) >> 5)) * 16)
                t.add("burst_gather_fast: rotator reads S, A[i >> 5], B[i & 31] (r128)", "r128",
                      lambda tid, r=r, d=d: None if idx(tid, r, N) is None else T + (1 + 72 + ((idx(tid, r, N) + d) & 31)) * 16)
    for r in rounds(N):
        t.add("energy: xs reads (r128, consecutive)", "r128", lambda tid, r=r: None if idx(tid, r, N) is None else BUF0 + idx(tid, r, N) * 16)
    for r in range((N + 63) // 64):     # seven candidate bins, one wave each: wave w takes bin kbin - 3 + w
        t.add("candidate DFTs: xs reads (r128, consecutive)", "r128",
              lambda tid, r=r: BUF0 + ((tid & 63) + 64 * r) * 16 if tid < 448 and (tid & 63) + 64 * r < N else None)
        t.add("candidate DFTs: twiddle reads twl[(k n) mod nfft] (r128, lanes k slots apart)", "r128",
              lambda tid, r=r: BUF1 + (((kbin - 3 + (tid >> 6)) % N * ((tid & 63) + 64 * r)) % N) * 16 if tid < 448 and (tid & 63) + 64 * r < N else None)
    for r in rounds(N - 1):
        for d in range(2):
            t.add("phase estimate: xs[n], xs[n + 1] reads (r128, consecutive)", "r128",
                  lambda tid, r=r, d=d: None if idx(tid, r, N - 1) is None else BUF0 + (idx(tid, r, N - 1) + d) * 16)
            t.add("phase estimate: twiddle reads twl[(n j) mod nfft] (r128, lanes j slots apart)", "r128",
                  lambda tid, r=r, d=d: None if idx(tid, r, N - 1) is None else BUF1 + (((idx(tid, r, N - 1) + d) * jm) % N) * 16)
    if gate:
        # SNR gate: fft37_step1_sym<true> (both rotations applied on read), then fft37_step2_bin over the 2 * hnl = 176 band bins
        PW, BASE = P, P + 16 * 16
        for r in range(2):
            o_of = lambda tid, r=r: tid + NT * r if tid + NT * r < 19 * N2 else None
            def ia(tid):
                o = o_of(tid)
                return None if o is None else (o - 18 * N2 if o >= 18 * N2 else N2 * (1 + o // N2) + o % N2)
            def ib(tid):
                o = o_of(tid)
                return None if o is None or o >= 18 * N2 else N2 * (36 - o // N2) + o % N2
            for f in (ia, ib):
                t.add("gate, pass A: xs reads and stores (r128 / w128, runs of 32)", "r128", lambda tid, f=f: None if f(tid) is None else BUF0 + f(tid) * 16)
                t.add("gate, pass A: xs reads and stores (r128 / w128, runs of 32)", "w128", lambda tid, f=f: None if f(tid) is None else BUF0 + f(tid) * 16)
                t.add("gate, pass A: twiddle reads twl[(n j) mod nfft] (r128, lanes j slots apart)", "r128",
                      lambda tid, f=f: None if f(tid) is None else BUF1 + ((f(tid) * jm) % N) * 16)
                t.add("gate, pass A: base[n >> 4], pw[n & 15] reads (r128)", "r128", lambda tid, f=f: None if f(tid) is None else BASE + (f(tid) >> 4) * 16)
                t.add("gate, pass A: base[n >> 4], pw[n & 15] reads (r128)", "r128", lambda tid, f=f: None if f(tid) is None else PW + (f(tid) & 15) * 16)
        BB = BUF1                                      # B[37][33] takes the twiddle table's place
        for r in range(2):
            o_of = lambda tid, r=r: tid + NT * r if tid + NT * r < 19 * N2 else None
            t.add("gate, pass B: xs and w37 reads (r128, runs of 32 / one address per run)", "r128", lambda tid: None if o_of(tid) is None else BUF0 + (o_of(tid) % N2) * 16)
            for n1 in range(1, 19):
                t.add("gate, pass B: xs and w37 reads (r128, runs of 32 / one address per run)", "r128",
                      lambda tid, n1=n1: None if o_of(tid) is None else BUF0 + (N2 * n1 + o_of(tid) % N2) * 16)
                t.add("gate, pass B: xs and w37 reads (r128, runs of 32 / one address per run)", "r128",
                      lambda tid, n1=n1: None if o_of(tid) is None else BUF0 + (N2 * (37 - n1) + o_of(tid) % N2) * 16)
                t.add("gate, pass B: xs and w37 reads (r128, runs of 32 / one address per run)", "r128",
                      lambda tid, n1=n1: None if o_of(tid) is None else W37 + ((n1 * (o_of(tid) // N2)) % 37) * 16)
            t.add("gate, pass B: B stores (w128, rows 33 apart)", "w128", lambda tid: None if o_of(tid) is None else BB + ((o_of(tid) // N2) * LDB + o_of(tid) % N2) * 16)
            t.add("gate, pass B: B stores (w128, rows 33 apart)", "w128",
                  lambda tid: None if o_of(tid) is None or o_of(tid) < N2 else BB + ((37 - o_of(tid) // N2) * LDB + o_of(tid) % N2) * 16)
        kk = lambda tid: None if tid >= 176 else (tid if tid < 88 else N - 176 + tid)
        for n2 in range(N2):
            t.add("gate, step 2: B row reads (r128, rows 33 apart)", "r128", lambda tid, n2=n2: None if kk(tid) is None else BB + ((kk(tid) % 37) * LDB + n2) * 16)
            t.add("gate, step 2: wN2[(n2 k2) mod 32] reads (r128, a few addresses per wave)", "r128",
                  lambda tid, n2=n2: None if kk(tid) is None else WN2 + ((n2 * (kk(tid) // 37)) % N2) * 16)
        t.add("gate: band power stores and reads (w64 / r64, consecutive)", "w64", lambda tid: None if tid >= 176 else P + tid * 8)
        for r in range(3):
            t.add("gate: band power stores and reads (w64 / r64, consecutive)", "r64", lambda tid, r=r: P + (3 + tid + 64 * r) * 8 if tid < 64 and 3 + tid + 64 * r < 174 else None)
    return t


def fine_chunk():
    """one open (window, chunk) item of k_fine_chunk: 640 threads, nfft = 1184, N2 = 32"""
    t = Table()
    FK, N, N2, LDB = 640, 1184, 32, 33
    XS = 0
    BB = (N + 64) * 16
    W37 = BB + 37 * LDB * 16
    WN2 = W37 + 40 * 16
    D = WN2 + N2 * 16
    idx = lambda tid, r, n: tid + FK * r if tid + FK * r < n else None
    for r in range(2):
        t.add("window copy and error-bound reads (w128 / r128, consecutive)", "w128", lambda tid, r=r: None if idx(tid, r, N + 64) is None else XS + idx(tid, r, N + 64) * 16, FK)
        t.add("window copy and error-bound reads (w128 / r128, consecutive)", "r128", lambda tid, r=r: None if idx(tid, r, N) is None else XS + idx(tid, r, N) * 16, FK)
    t.add("steps d[t]: reads and store (r128 / w64, consecutive)", "r128", lambda tid: XS + (tid + N) * 16 if tid < 64 else None, FK)
    t.add("steps d[t]: reads and store (r128 / w64, consecutive)", "r128", lambda tid: XS + tid * 16 if tid < 64 else None, FK)
    t.add("steps d[t]: reads and store (r128 / w64, consecutive)", "w64", lambda tid: D + tid * 8 if tid < 64 else None, FK)
    ia = lambda tid: N2 * (1 + tid // N2) + tid % N2 if tid < 18 * N2 else None
    ib = lambda tid: N2 * (36 - tid // N2) + tid % N2 if tid < 18 * N2 else None
    for f in (ia, ib):
        t.add("fft37_step1_sym, pass A: xs reads and stores (runs of 32)", "r128", lambda tid, f=f: None if f(tid) is None else XS + f(tid) * 16, FK)
        t.add("fft37_step1_sym, pass A: xs reads and stores (runs of 32)", "w128", lambda tid, f=f: None if f(tid) is None else XS + f(tid) * 16, FK)
    on = lambda tid: tid < 19 * N2
    t.add("fft37_step1_sym, pass B: xs and w37 reads (runs of 32 / one address per run)", "r128", lambda tid: XS + (tid % N2) * 16 if on(tid) else None, FK)
    for n1 in range(1, 19):
        t.add("fft37_step1_sym, pass B: xs and w37 reads (runs of 32 / one address per run)", "r128", lambda tid, n1=n1: XS + (N2 * n1 + tid % N2) * 16 if on(tid) else None, FK)
        t.add("fft37_step1_sym, pass B: xs and w37 reads (runs of 32 / one address per run)", "r128", lambda tid, n1=n1: XS + (N2 * (37 - n1) + tid % N2) * 16 if on(tid) else None, FK)
        t.add("fft37_step1_sym, pass B: xs and w37 reads (runs of 32 / one address per run)", "r128", lambda tid, n1=n1: W37 + ((n1 * (tid // N2)) % 37) * 16 if on(tid) else None, FK)
    t.add("fft37_step1_sym, pass B: B stores (w128, rows 33 apart)", "w128", lambda tid: BB + ((tid // N2) * LDB + tid % N2) * 16 if on(tid) else None, FK)
    t.add("fft37_step1_sym, pass B: B stores (w128, rows 33 apart)", "w128", lambda tid: BB + ((37 - tid // N2) * LDB + tid % N2) * 16 if on(tid) and tid >= N2 else None, FK)
    row = lambda tid: BB + (tid % 37) * LDB * 16
    for n2 in range(N2):                                # lanes 0..36: the pair (k1, k1 + 37 * 16), every column of the row
        t.add("fft37_step2_pair, j = 0: B row reads (r128, rows 33 apart)", "r128", lambda tid, n2=n2: row(tid) + n2 * 16 if tid < 37 else None, FK)
    gen = lambda tid: 37 <= tid < N // 2
    for n2 in (0, 16):
        t.add("fft37_step2_pair: B row reads (r128, rows 33 apart, wrapping at row 37)", "r128", lambda tid, n2=n2: row(tid) + n2 * 16 if gen(tid) else None, FK)
    for n2 in range(1, 16):
        t.add("fft37_step2_pair: B row reads (r128, rows 33 apart, wrapping at row 37)", "r128", lambda tid, n2=n2: row(tid) + n2 * 16 if gen(tid) else None, FK)
        t.add("fft37_step2_pair: B row reads (r128, rows 33 apart, wrapping at row 37)", "r128", lambda tid, n2=n2: row(tid) + (N2 - n2) * 16 if gen(tid) else None, FK)
        t.add("fft37_step2_pair: wN2[(n2 j) mod 32] reads (r128, two or three addresses per wave)", "r128",
              lambda tid, n2=n2: WN2 + ((n2 * (tid // 37)) % N2) * 16 if gen(tid) else None, FK)
    for tt in range(64):                                # every wave that sweeps (data: whole waves skip it); all ten counted
        t.add("sweep: d[t] reads (r64, one address)", "r64", lambda tid, tt=tt: D + tt * 8 if tid < N // 2 else None, FK)
    return t


def main():
    argv = sys.argv[1:]
    opt = lambda name, d: int(argv[argv.index(name) + 1]) if name in argv else d
    kbin = opt("--bin", 37)
    window_sch().show("k_window_sch<8, 512, 47> (per launch: 576 207 LDS instructions, 773 950 conflict cycles)", opt("--sch-windows", 580), 576207, 773950)
    burst_tone(1, kbin, kbin).show(f"k_burst_tone<1, 8, 47> with the tone at bin {kbin} (per launch: 872 712 LDS instructions, 1 102 056 conflict cycles)",
                                   opt("--burst-windows", 626), 872712, 1102056)
    # GATE = 1 runs before the carrier is corrected: the tone's bin is 37 plus the stream's carrier offset in bins (1.83 kHz each, about
    # half a bin per ppm at 957 MHz).  The totals per bin, and their mean over a range of offsets:
    tots = {k: sum(r[1] for r in burst_tone(1, k, k).rows.values()) for k in range(17, 58)}
    print("k_burst_tone<1>: extra cycles per workgroup by the tone's bin 17..57:", list(tots.values()))
    for lo, hi in ((27, 47), (17, 57)):
        m = sum(tots[k] for k in range(lo, hi + 1)) / (hi - lo + 1)
        print(f"  mean over bins {lo}..{hi}: {m:.0f} per workgroup, x 626 = {m * 626 / 1e6:.3f} M per launch (measured 1.102 M, {100.0 * (m * 626 - 1102056) / 1102056:+.0f} %)")
    print()
    fine_chunk().show("k_fine_chunk, per open (window, chunk) item (per launch: 278 511 LDS instructions, 139 717 conflict cycles, 214 items)",
                      opt("--chunk-items", 214), 278511, 139717)
    burst_tone(0, 37, 37).show("k_burst_tone<0, 8, 47>: carrier corrected, tone at bin 37 (per launch: 452 519 LDS instructions, 559 185 conflict cycles)", opt("--burst0-windows", 560), 452519, 559185)


if __name__ == "__main__":
    main()
