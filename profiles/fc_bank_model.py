#!/usr/bin/env python3
"""Per-site LDS bank-conflict model of k_fine_cert<8, 47> (reference geometry: 1025 shifts, 1184-point windows, 256 threads, three
staging passes of 736 outputs), the table of profiles/NOTES_r30.md.  Pure arithmetic on the address expressions of
csrc/kernels_detect.h / kernels_frontend.h / fc_layout.h; nothing here touches a GPU.

Rule (gfx950): a wave instruction is served in fixed lane groups, one LDS cycle per group; lanes of a group with the same address
are served together; every further distinct address on a busy bank costs the group one more cycle.  extra(site) = sum over the
instructions of the site and their groups of (ways - 1) -- what SQ_LDS_BANK_CONFLICT counts.

    python profiles/fc_bank_model.py [parent|new] [--windows N] [--off K]

--windows: workgroups of a launch that hold a window (default 626: the fine windows of the headline's 64 streams; the other
workgroups of the 752 return at their first line and touch no LDS).  --off: the staging offset first - first_al of the window
build (0..7, default 3); without it the totals of all eight offsets are printed behind the table.
"""
import sys
from collections import defaultdict

NSHIFT, NFFT, NTHR, NB, PER, NTAPS = 1025, 1184, 256, 8, 736, 47
NSTEP = NSHIFT - 1
WLEN = NSTEP + NFFT
B, NA, NM, LD1, NCHUNK = 32, 37, 69, 34, 16
STATIC = 144


def XP(p):
    return p + (p >> 7)


def xs_pad(p):
    return p + (p >> 2)


XS = 0
REG1 = XP(WLEN) * 16
REG2 = REG1 + NB * NM * 16
SUMS = REG2
CS = SUMS + XP(NSTEP + 2) * 4
TW1 = REG2
TW2 = TW1 + NB * LD1 * 16

G128 = [0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1]
KINDS = {  # name: (banks, dwords, group of lane)
    "r128": (64, 4, lambda l: 2 * (l >> 5) + G128[l & 31]),
    "r64": (64, 2, lambda l: l >> 5),
    "r32": (32, 1, lambda l: l >> 5),
    "w128": (32, 4, lambda l: l >> 3),
    "w64": (32, 2, lambda l: l >> 4),
    "w32": (32, 1, lambda l: l >> 5),
}


def extra(kind, addr):
    """addr: {lane: byte offset into the dynamic LDS} of the active lanes of one wave instruction -> (extra cycles, worst ways)"""
    nb, dw, grp = KINDS[kind]
    on = defaultdict(lambda: defaultdict(set))
    for l, a in addr.items():
        a += STATIC
        for d in range(dw):
            on[grp(l)][(a // 4 + d) % nb].add(a)
    ways = [max(len(s) for s in banks.values()) for banks in on.values()]
    return sum(w - 1 for w in ways), max(ways) if ways else 0


class Table:
    def __init__(self):
        self.rows = defaultdict(lambda: [0, 0, 0])     # site -> [wave instructions, extra cycles, worst ways]

    def add(self, site, kind, fn, lanes_of_wave=None):
        """fn(tid) -> byte offset or None (lane off); one wave instruction per wave that has an active lane"""
        for w in range(NTHR // 64):
            addr = {}
            for l in range(64):
                a = fn(64 * w + l)
                if a is not None:
                    addr[l] = a
            if addr:
                e, wy = extra(kind, addr)
                r = self.rows[site]
                r[0] += 1; r[1] += e; r[2] = max(r[2], wy)


def model(new, off=3):
    t = Table()
    # ---- window build: three passes ----
    for o0 in range(0, WLEN, PER):
        cnt = min(PER, WLEN - o0)
        span = cnt + NTAPS - 1
        for off in (off,):                                # first - first_al, 0..7
            r = (-off) & 3
            for u in range(8):
                def f(tid, u=u):
                    ib = 8 * tid - off
                    if ib < 0 or ib + 8 > span + 8:
                        return None
                    return REG1 + (xs_pad(ib) + u + ((r + u) >> 2)) * 16 if ib + 8 <= span else (REG1 + xs_pad(ib + u) * 16 if ib + u < span + 8 else None)
                t.add("raw_chunk_to_lds: xq stores (w128, lanes 10 slots apart)", "w128", f)
        for s in range(50):
            t.add("fir4_sym47: xq reads (r128, lanes 5 slots apart)", "r128",
                  lambda tid, s=s: REG1 + (xs_pad(4 * tid) + s + (s >> 2)) * 16 if 4 * tid < cnt else None)
        for k in range(4):
            t.add("fc_window_raw: xs stores (w128, lanes 4 slots apart)", "w128",
                  lambda tid, k=k: XS + XP(o0 + 4 * tid + k) * 16 if 4 * tid + k < cnt else None)
    # ---- tone estimate ----
    n0 = NSTEP // 2
    for i in range(8):
        t.add("fc_choose_bins: decimating read (r128, lanes 8 slots apart)", "r128",
              lambda tid, i=i: XS + XP(n0 + 8 * tid + i) * 16 if tid < 148 else None)
    t.add("fc_choose_bins: yd / t148 stores (w128)", "w128", lambda tid: REG1 + tid * 16 if tid < 148 else None)
    t.add("fc_choose_bins: yd / t148 stores (w128)", "w128", lambda tid: REG1 + (148 + tid) * 16 if tid < 148 else None)
    PW = REG1 + 296 * 16
    A = PW + 148 * 8
    for n1 in range(37):
        t.add("fc_choose_bins: 37-point stage (r128: yd broadcast, t148 scattered)", "r128",
              lambda tid, n1=n1: REG1 + (4 * n1 + tid // 37) * 16 if tid < 148 else None)
        t.add("fc_choose_bins: 37-point stage (r128: yd broadcast, t148 scattered)", "r128",
              lambda tid, n1=n1: REG1 + (148 + (4 * (tid % 37) * n1) % 148) * 16 if tid < 148 else None)
    t.add("fc_choose_bins: A / pw stores", "w128", lambda tid: A + tid * 16 if tid < 148 else None)
    for n2 in range(4):
        t.add("fc_choose_bins: 4-point stage (r128)", "r128", lambda tid, n2=n2: A + (n2 * 37 + tid % 37) * 16 if tid < 148 else None)
        t.add("fc_choose_bins: 4-point stage (r128)", "r128", lambda tid, n2=n2: REG1 + (148 + (tid * n2) % 148) * 16 if tid < 148 else None)
    t.add("fc_choose_bins: A / pw stores", "w64", lambda tid: PW + tid * 8 if tid < 148 else None)
    for r in range(3):
        t.add("fc_choose_bins: pw reads of wave 0 (r64)", "r64", lambda tid, r=r: PW + (tid + 64 * r) * 8 if tid < 64 and tid + 64 * r < 148 else None)
    # ---- tables, level 1, level 2 ----
    t.add("fc_twiddles: tw1 / tw2 stores (w128)", "w128", lambda tid: TW1 + ((tid // B) * LD1 + tid % B) * 16)
    for r in range(2):
        t.add("fc_twiddles: tw1 / tw2 stores (w128)", "w128",
              lambda tid, r=r: TW2 + (tid + 256 * r) * 16 if tid + 256 * r < NB * NA else None)
    for r in range(3):
        for i in range(B):
            def m_of(tid, r=r):
                m = tid // NB + 32 * r
                return m if m < NM else None
            t.add("fc_level1: xs reads (r128, start rotated by group)", "r128",
                  lambda tid, i=i: None if m_of(tid) is None else XS + (XP(B * m_of(tid)) + ((tid // NB + i) & (B - 1))) * 16)
            t.add("fc_level1: tw1 reads (r128, plane stride 34)", "r128",
                  lambda tid, i=i: None if m_of(tid) is None else TW1 + ((tid % NB) * LD1 + ((tid // NB + i) & (B - 1))) * 16)
        t.add("fc_level1: Sp stores (w128, j rows 69 apart)", "w128",
              lambda tid: None if m_of(tid) is None else REG1 + ((tid % NB) * NM + m_of(tid)) * 16)

    def chunk(tid):
        if new:
            return 2 * ((tid & 63) >> 3) + (tid >> 6) if (tid >> 6) < 2 else None
        return tid // NB if tid // NB < NCHUNK else None
    for a in range(NA):
        t.add("fc_level2_anchor: Sp reads (r128: j rows 69 apart, chunks 2 apart)", "r128",
              lambda tid, a=a: None if chunk(tid) is None else REG1 + ((tid % NB) * NM + 2 * chunk(tid) + a) * 16)
        t.add("fc_level2_anchor: tw2 reads (r128, 8 consecutive)", "r128",
              lambda tid, a=a: None if chunk(tid) is None else TW2 + (a * NB + tid % NB) * 16)
    # ---- E / C scans: wave 2 = E, wave 3 = C ----
    for r in range(19):
        t.add("fc_scan_role: E(0) reads (r128, consecutive)", "r128",
              lambda tid, r=r: XS + XP(tid - 128 + 64 * r) * 16 if 128 <= tid < 192 and tid - 128 + 64 * r < NFFT else None)
    for u in range(16):
        q = (lambda tid, u=u: (tid & 63) + 64 * u) if new else (lambda tid, u=u: 16 * (tid & 63) + u)
        t.add("fc_scan_role: x[q + nfft], x[q] reads (r128)", "r128", lambda tid: XS + XP(q(tid) + NFFT) * 16 if tid >= 128 else None)
        t.add("fc_scan_role: x[q + nfft], x[q] reads (r128)", "r128", lambda tid: XS + XP(q(tid)) * 16 if tid >= 128 else None)
        t.add("fc_scan_role: Et stores (w64)", "w64", lambda tid: REG1 + q(tid) * 8 if 128 <= tid < 192 else None)
        t.add("fc_scan_role: Cs stores (w32)", "w32", lambda tid: CS + XP(q(tid)) * 4 if tid >= 192 else None)
    # ---- slides ----
    for qq in range(64):
        t.add("slides: x[t + nfft], x[t] reads (r128, 8 lanes per address)", "r128",
              lambda tid: None if chunk(tid) is None else XS + XP(64 * chunk(tid) + NFFT + qq) * 16)
        t.add("slides: x[t + nfft], x[t] reads (r128, 8 lanes per address)", "r128",
              lambda tid: None if chunk(tid) is None else XS + XP(64 * chunk(tid) + qq) * 16)
        t.add("slides: sumS stores (w32, 8 lanes per address)", "w32",
              lambda tid: None if chunk(tid) is None else SUMS + XP(64 * chunk(tid) + qq + 1) * 4)
    # ---- certificate: 5 shifts per thread ----
    for k in range(5):
        tt = lambda tid, k=k: 5 * tid + k if 5 * tid + k <= NSTEP else None
        t.add("fc_certificate: Et reads (r64, lanes 40 bytes apart)", "r64", lambda tid: None if tt(tid) is None else REG1 + tt(tid) * 8)
        for rep in range(3):                              # sumS: first loop, forward pass, backward pass; Cs the same
            t.add("fc_certificate: sumS / Cs reads (r32, lanes 20 bytes apart)", "r32", lambda tid: None if tt(tid) is None else SUMS + XP(tt(tid)) * 4)
            t.add("fc_certificate: sumS / Cs reads (r32, lanes 20 bytes apart)", "r32", lambda tid: None if tt(tid) is None else CS + XP(tt(tid)) * 4)
        t.add("fc_certificate: s(t) stores (w32)", "w32", lambda tid: None if tt(tid) is None else SUMS + XP(tt(tid)) * 4)
    return t


def main():
    argv = sys.argv[1:]
    windows, off = 626, None
    if "--windows" in argv:
        i = argv.index("--windows"); windows = int(argv[i + 1]); del argv[i:i + 2]
    if "--off" in argv:
        i = argv.index("--off"); off = int(argv[i + 1]); del argv[i:i + 2]
    which = argv or ["parent", "new"]
    tabs = {w: model(w == "new", 3 if off is None else off) for w in which}
    sites = list(next(iter(tabs.values())).rows)
    print("| site | wave instr | " + " | ".join(f"extra cycles ({w}) | ways ({w})" for w in which) + " |")
    print("|---|---|" + "---|---|" * len(which))
    for s in sites:
        print(f"| {s} | {tabs[which[0]].rows[s][0]} | " + " | ".join(f"{tabs[w].rows[s][1]} | {tabs[w].rows[s][2]}" for w in which) + " |")
    for w in which:
        tot = sum(r[1] for r in tabs[w].rows.values())
        ins = sum(r[0] for r in tabs[w].rows.values())
        print(f"{w}: {ins} modelled wave instructions, {tot} extra cycles per workgroup; x {windows} working workgroups = "
              f"{tot * windows / 1e6:.2f} M per launch (x 752 launched = {tot * 752 / 1e6:.2f} M)")
    if off is None:
        for w in which:
            tots = [sum(r[1] for r in model(w == "new", o).rows.values()) for o in range(8)]
            print(f"{w}: extra cycles per workgroup by staging offset 0..7: {tots} (spread {100.0 * (max(tots) - min(tots)) / min(tots):.1f} %)")


if __name__ == "__main__":
    main()
