// fc_layout.h -- k_fine_cert's geometry, its dynamic LDS and its lane maps as plain constexpr functions.  The kernel
// (kernels_detect.h), run_fine() (host_plan.h) and the stand-alone bank check (tests/fc_banks_main.cpp, a host program) all read
// this one text; nothing of HIP is needed to include it.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define FC_HD __host__ __device__
#else
#define FC_HD
#endif

#define FC_NB 8        /* k_fine_cert: candidate bins around the tone */
#define FS_CHUNK 64    /* shifts per chunk of the fine search (see the comment block in kernels_detect.h) */
#define FC_CPLX_BYTES 16   /* sizeof(cplx): two doubles */

FC_HD constexpr int fc_gcd64(int n) { int b = 64; while (n % b) b >>= 1; return b; }
// threads of k_fine_cert: 8 per chunk, at least 256.  (320 would save the nearly empty third round of the level-1 phase --
// 69 blocks handed out 32 at a time -- but five-wave workgroups no longer sit three to a CU: measured 77 us against 59.)
FC_HD constexpr int fc_threads(int nshift) {
    return ((nshift - 1) / FS_CHUNK * FC_NB + 63) / 64 * 64 < 256 ? 256 : ((nshift - 1) / FS_CHUNK * FC_NB + 63) / 64 * 64;
}
// One element of padding after every 128: two samples 128 apart lie one bank group (16 bytes) apart instead of on the same banks.
// (Padding every 64 costs the third workgroup per CU: the kernel sits 100 bytes under the 53 760-byte line.  The slide phase gets
// by without it: fc_slide_chunk() below puts chunks 128 shifts apart side by side, not chunks 64 apart.)
#define FC_XP(p) ((p) + ((p) >> 7))

// k_fine_cert's geometry and its dynamic LDS, written down once: the kernel's pointers, the size of the launch and run_fine()'s
// fit test of a staging pass all come from here.  Byte offsets from the base of the dynamic LDS:
//   xs    the window, FC_XP(wlen) samples
//   reg1  Sp[FC_NB][nM], the S partials (level 1 -> level 2); from the E/C scans on Et[t], t = 0..nstep
//   reg2  tw1[FC_NB][ld1] = W^(k_j b) and tw2[nA][FC_NB] = W^(k_j B a) (twiddles -> level 2); from the slides on sumS[t] (the sum
//         over S of P(t,k), later s(t)) and Cs[t] (C(t) = sum_{q<t} |d_q|, the slack of the recurrence), FC_XP(nstep + 2) floats
//         each, and behind them the 2 x 8 scan partials sh_scan / sh_scan2 (block scan, certificate)
// Before the tone estimate regions 1 and 2 are free: the bin choice keeps its 148-point spectrum at reg1, and a window built from
// the raw bytes stages its passes there (`stage` bytes: what is left of the launch behind the window, less 16).
struct FcCarve {
    int nstep, wlen, B, nA, nM, nchunk, ld1;
    size_t xs, reg1, reg2;
    size_t Sp, Et, tw1, tw2, sumS, Cs, sh_scan, sh_scan2;
    size_t total, launch, stage;     // bytes used | dynamic LDS of the launch (whole 16 bytes) | room of a staging pass
};
FC_HD constexpr FcCarve fc_carve(int nshift, int nfft) {
    FcCarve c{};
    c.nstep = nshift - 1; c.wlen = c.nstep + nfft;
    c.B = fc_gcd64(nfft); c.nA = nfft / c.B; c.nM = c.wlen / c.B; c.nchunk = c.nstep / FS_CHUNK;
    c.ld1 = c.B + 2;                                      // plane stride of tw1: spreads the 8 bins over the banks
    const int xp = FC_XP(c.nstep + 2);
    const size_t r1 = (size_t)FC_NB * c.nM * FC_CPLX_BYTES, e1 = (size_t)(c.nstep + 2) * sizeof(double);
    const size_t r2 = (size_t)FC_NB * (c.B + 2 + nfft / c.B) * FC_CPLX_BYTES, e2 = (size_t)2 * (size_t)(xp + 1) * sizeof(float) + 16 * sizeof(double);
    c.xs = 0;
    c.reg1 = (size_t)FC_XP(c.wlen) * FC_CPLX_BYTES;
    c.reg2 = c.reg1 + (r1 > e1 ? r1 : e1);
    c.Sp = c.Et = c.reg1;
    c.tw1 = c.reg2;
    c.tw2 = c.tw1 + (size_t)(FC_NB * c.ld1) * FC_CPLX_BYTES;
    c.sumS = c.reg2;
    c.Cs = c.sumS + (size_t)xp * sizeof(float);
    c.sh_scan = c.Cs + (size_t)(xp + (xp & 1)) * sizeof(float);
    c.sh_scan2 = c.sh_scan + 8 * sizeof(double);
    c.total = c.reg2 + (r2 > e2 ? r2 : e2);
    c.launch = (c.total + 15) & ~(size_t)15;
    c.stage = c.launch - c.reg1 - 16;
    return c;
}
static_assert(fc_carve(1025, 1184).total == 53520, "reference geometry: with the 144 bytes of static LDS, 100 bytes under the 53 760-byte line (three workgroups per CU)");

// ---- lane maps of the two phases behind the level-2 barrier --------------------------------------------------------------
// Slides: the 8 lanes of a group walk one chunk (one lane per bin, all reading the same sample: a broadcast).  A ds_read_b128 is
// served in groups of 16 lanes, that is two groups of one wave, and a wave's groups used to hold CONSECUTIVE chunks: 64 samples =
// 1 024 bytes apart, the same banks, with the FC_XP pad separating only every second pair -- every read 2-way.  Dealing the
// chunks round the slide waves instead (wave w takes chunks w, w + nslide, ...) puts a wave's neighbouring groups 64 * nslide
// samples apart: with two slide waves (the reference geometry) that is 128 samples, one pad, 16 bytes further on for each group --
// the four chunks of a 16-lane group on four different bank groups.
FC_HD constexpr int fc_nslide(int nchunk) { return (FC_NB * nchunk + 63) >> 6; }      // waves that hold slide lanes
// the chunk thread `tid` walks, or FC_NO_CHUNK in a wave without slide lanes (a result >= nchunk: the lane only helps with the shared phases)
#define FC_NO_CHUNK (1 << 20)
FC_HD constexpr int fc_slide_chunk(int tid, int nslide) {
    return (tid >> 6) < nslide ? nslide * ((tid & 63) / FC_NB) + (tid >> 6) : FC_NO_CHUNK;
}
// E/C scans (one wave each): in round u lane l takes shift l + 64 u -- consecutive samples across the wave, consecutive slots of
// Et / Cs for the stores; the prefix sums run ACROSS the lanes (a DPP scan per round), the rounds' totals are carried in order.
FC_HD constexpr int fc_scan_rounds(int nstep) { return (nstep + 63) >> 6; }
FC_HD constexpr int fc_scan_shift(int lane, int u) { return lane + 64 * u; }
