// chain_ops.h -- the per-sample arithmetic of the lazy chain (state.h), written ONCE:
//
//   raw bytes -> raw2iq -> filter(coef,1,.) -> interp1 -> exp derotation -> interp1 -> exp derotation
//
// gather_core, burst_gather_fast, sch_gather_fast, k_stream_tile, k_stream_tile_s47, k_fine_cert's window build and stage_raw
// organise these pieces differently (phases, buffers, lanes); none of them spells a piece out itself, so every route gives the
// same bits because it runs the same text.
//
//   raw staging   raw_align_off / raw_first_al / raw_nchunk, ffast_chunk, iq_of, raw_span_to_lds, raw_chunk_to_lds
//   FIR           fir_stage_taps, fir4_lds<NTP, PAD, UNR>, fir4_store, fir4_sym47
//   interp1       lerp_pos, lerp_tap (index and weight), lerp_blend, lerp_at; lerp_src_range (the source range of a level)
//   rotators      sincos_large; rot_table_fill / rot_at (a window's S | A | B); tile_rot_fill / tile_rot_s (a stream tile's A | B, S)
//   plans         st_chain (the stream-tile prologue), fine_window_holding
//
// The first part needs nothing of HIP (tests/chain_ops_main.cpp is a host program that includes this file and holds it to the
// spellings it replaced); the second part (LDS, wave operations, the stream's state) is device code.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define CH_HD __host__ __device__ __forceinline__
#else
#define CH_HD inline
struct double2 { double x, y; };                                 // stand-ins for the HIP names the plain part uses
struct uint4 { unsigned x, y, z, w; };
inline double2 make_double2(double x, double y) { double2 v; v.x = x; v.y = y; return v; }
inline uint4 make_uint4(unsigned x, unsigned y, unsigned z, unsigned w) { uint4 v; v.x = x; v.y = y; v.z = z; v.w = w; return v; }
#endif

typedef double2 cplx;

CH_HD cplx cmul(cplx a, cplx b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// sin/cos of a LARGE fp64 argument t (|t| up to ~1e6 rad: t = k*comp_phase_rotate, k up to 1e6) with the
// accuracy of a correctly reduced argument, several times cheaper than the library's general path:
// n = round(t/2pi); y = t - n*2pi with 2pi = C1 + C2 split so that the first fma is EXACT (t and n*C1 are
// both multiples of 2^-50 and the difference is < 8, so it fits a double), the second adds n*C2 <= 4e-11
// with an error <= ulp(y); then the library routine on |y| <= pi (its cheap small-argument path).
CH_HD void sincos_large(double t, double* sn, double* cs) {
    const double n = rint(t * 0.15915494309189535);            // 1/(2*pi)
    double y = fma(-n, 6.28318530717958623e+00, t);            // C1 = fl(2*pi)
    y = fma(-n, 2.44929359829470641e-16, y);                   // C2 = 2*pi - C1
    sincos(y, sn, cs);
}

// ---- raw staging -------------------------------------------------------------------------------------------------------
// A span [first, first + span) of raw samples (I | Q<<8 per ushort) is fetched by whole 16-byte chunks: `ao` = samples past a
// 16-byte boundary at g = 0; raw_first_al() <= first is the sample the first chunk starts at (its address is 16-byte aligned);
// chunk c is ffast_chunk(base, first_al + 8 c, n), c < raw_nchunk().
CH_HD long raw_align_off(const unsigned short* base) { return (long)(((uintptr_t)base >> 1) & 7); }
CH_HD long raw_first_al(long first, long ao) {
    long m = (first + ao) % 8;
    if (m < 0) m += 8;
    return first - m;
}
CH_HD int raw_nchunk(long first, int span, long first_al) { return (int)((first + span - first_al + 7) >> 3); }
CH_HD uint4 ch_ld16(const unsigned short* p) {
#if defined(__HIPCC__)
    return *(const uint4*)p;
#else
    uint4 v;
    memcpy(&v, p, 16);
    return v;
#endif
}
CH_HD uint4 ffast_chunk(const unsigned short* __restrict__ base, long g0, long n) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);                   // 8 samples from g0, zeros outside [0, n)
    if (g0 >= 0 && g0 + 8 <= n) {
        v = ch_ld16(base + g0);
    } else if (g0 + 8 > 0 && g0 < n) {                      // straddles an end of the stream
        unsigned short q[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) q[i] = (g0 + i >= 0 && g0 + i < n) ? base[g0 + i] : (unsigned short)0;
        v.x = q[0] | ((unsigned)q[1] << 16); v.y = q[2] | ((unsigned)q[3] << 16);
        v.z = q[4] | ((unsigned)q[5] << 16); v.w = q[6] | ((unsigned)q[7] << 16);
    }
    return v;
}
// raw2iq.m:6-8 of one sample (its 16 bits are the low half of q; whatever lies above them is ignored): (I - mean) + 1i (Q - mean)
CH_HD cplx iq_of(unsigned q, double mr, double mi) {
    return make_double2((double)(q & 0xFFu) - mr, (double)((q >> 8) & 0xFFu) - mi);
}

// LDS positions.  lds_pad: 8 ushorts (16 B) after every 64 raw samples, so that lanes whose samples are 64 apart (the
// decimate-by-64 FIR) do not all hit the same bank.  xs_pad: one 16-byte pad after every 4 staged complex samples, so that lanes
// reading samples 4 apart (the 4-outputs-per-lane FIR below) hit distinct banks with ds_read_b128.
CH_HD int lds_pad(int rel) { return rel + ((rel >> 6) << 3); }
CH_HD int xs_pad(int p) { return p + (p >> 2); }

// ---- interp1 -----------------------------------------------------------------------------------------------------------
// Query position k*(1+e) of interp1 (interp_seq, FCCH_fine_correction.m:123, SCH_corr_rate_correction.m:126), ROUNDED to
// double as the reference rounds it before interp1 sees it.  Contraction must stay off here: left to the compiler, the
// weight xq - floor(xq) behind it becomes fma(k, f, -floor(xq)) -- the weight of the UNROUNDED product, up to an ulp of xq
// (1.2e-10 at k = 6e5) away from the reference's.  On unfiltered samples that moved the tone estimate by 2e-11 ppm and the
// end of the corrected stream by 4e-8 rad (tests/test_gpu_general_taps.py, the one-tap filter).
CH_HD double lerp_pos(double k, double f) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return k * f;
}
// Output sample k of a LERP level with factor f, from a source level of which samples lo_src .. lo_src + last are at hand: the two
// source samples (indices relative to lo_src; beyond the last sample the weight is 0, so the index is clamped) and the weight.
// k and lo_src come as doubles (integers below 2^53: exact); the spelling through a 64-bit index -- i0 = (long)floor(xq),
// t = xq - (double)i0 -- names the same j0, j1 and t (tests/chain_ops_main.cpp).
struct LerpTap { int j0, j1; double t; };
CH_HD LerpTap lerp_tap(double k, double f, double lo_src, int last) {
    const double xq = lerp_pos(k, f);                            // interp_seq = (0:max_len-1)'.*(1+e)
    const double j0f = floor(xq);
    LerpTap p;
    p.j0 = (int)(j0f - lo_src);
    p.j1 = p.j0 + 1 > last ? last : p.j0 + 1;
    p.t = xq - j0f;
    return p;
}
CH_HD cplx lerp_blend(cplx v0, cplx v1, double t) {
    return make_double2(v0.x + t * (v1.x - v0.x), v0.y + t * (v1.y - v0.y));
}
CH_HD cplx lerp_at(const cplx* src, double k, double f, double lo_src, int last) {   // src[j]: source sample lo_src + j
    const LerpTap p = lerp_tap(k, f, lo_src, last);
    return lerp_blend(src[p.j0], src[p.j1], p.t);
}
// The source samples that outputs lo .. hi of a LERP level read: floor(lo f) .. floor(hi f) + 1, the end clamped to the source's
// last sample n_prev - 1.
struct LerpRange { long lo, hi; };
CH_HD LerpRange lerp_src_range(long lo, long hi, double f, long n_prev) {
    LerpRange r;
    r.lo = (long)floor((double)lo * f);
    const long h = (long)floor((double)hi * f) + 1;
    r.hi = h > n_prev - 1 ? n_prev - 1 : h;
    return r;
}

// ---- rotators ----------------------------------------------------------------------------------------------------------
// exp(1i*(0:len-1)'*comp_phase_rotate) (FCCH_fine_correction.m:165, carrier_correct_post_SCH.m:83) for a window of cnt samples
// from k0 on, from a two-level table: exp(1i*k*c) = S * A[(k-k0)>>5] * B[(k-k0)&31], S = exp(1i*fl(k0*c)), A[q] = exp(1i*fl(32q*c)),
// B[m] = exp(1i*fl(m*c)) -- 1 + ceil(cnt/32) + 32 accurate sincos per window instead of one per sample.  The reference rounds k*c
// once; the three rounded pieces differ from that by < 2 ulp(k*c) ~ 3e-11 rad at k = 1e6 (see k_stream_tile).
// Layout: T[0] = S | T[1 .. 1+GC_ROT_A) = A | T[1+GC_ROT_A .. +32) = B; entry e of the 1 + na + 32 to compute sits in rot_slot(e, na).
#define GC_ROT_A 72                     /* windows of up to 32*GC_ROT_A samples */
#define GC_ROT_N (1 + GC_ROT_A + 32)
CH_HD int rot_na(int cnt) { return (cnt + 31) >> 5; }
CH_HD int rot_slot(int e, int na) { return e == 0 ? 0 : (e <= na ? e : 1 + GC_ROT_A + (e - 1 - na)); }
CH_HD void rot_table_fill(cplx* T, long k0, double c, int cnt, int e_first, int e_step) {
    const int na = rot_na(cnt);
    for (int e = e_first; e < 1 + na + 32; e += e_step) {
        const double arg = e == 0 ? (double)k0 * c : (e <= na ? (double)(32 * (e - 1)) * c : (double)(e - 1 - na) * c);
        double sn, cs;
        sincos_large(arg, &sn, &cs);
        T[rot_slot(e, na)] = make_double2(cs, sn);
    }
}
CH_HD cplx rot_at(const cplx* T, int i) {                        // exp(1i*(k0+i)*c), associated (S*A)*B
    return cmul(cmul(T[0], T[1 + (i >> 5)]), T[1 + GC_ROT_A + (i & 31)]);
}
// The stream-tile kernels keep one table per derotation for ALL tiles of a stream, T[TR_A + j] = A[j] (j < 34) and
// T[TR_B + m] = B[m] (m < 32) -- entry e < 132 of tile_rot_fill is entry e % 66 of derotation e / 66 -- and one S per tile,
// tile_rot_s().  (T[0], T[1] are k_stream_tile's S of the current / next tile.)  How the three factors are associated is the
// kernels' business: k_stream_tile (S*A)*B, k_stream_tile_s47 S*(A*B).
#define TR_A 2
#define TR_B 36
#define TR_N 68
CH_HD void tile_rot_fill(cplx* T2, cplx* T4, double c2, double c4, int e) {
    const int i = e % 66, which = e / 66;
    const double c = which ? c4 : c2;
    double sn, cs;
    sincos_large(i < 34 ? (double)(32 * i) * c : (double)(i - 34) * c, &sn, &cs);
    (which ? T4 : T2)[TR_A + i] = make_double2(cs, sn);
}
CH_HD cplx tile_rot_s(int which, long lo2, long lo3, double c2, double c4) {   // S = exp(1i*fl(k0*c)) of a tile: level 2 | level 4
    double sn, cs;
    sincos_large(which ? (double)lo3 * c4 : (double)lo2 * c2, &sn, &cs);
    return make_double2(cs, sn);
}

#if defined(__HIPCC__)
// =========================================================================================================================
// device part
// =========================================================================================================================
#include "state.h"

// raw2iq.m:6-8 on a span staged in LDS (stage_raw: sample first + i at r_s[off + i]): entries 0 .. span + tail - 1 of the complex
// FIR input, (I - mean) + 1i (Q - mean); zero before the stream starts (filter()'s zero initial state), past its end, and in
// the `tail` entries behind the span (finite values for the padding taps and for outputs that are not stored).
__device__ __forceinline__ void raw_span_to_lds(cplx* xs, const unsigned short* r_s, int off, long first, int span, int tail, long n,
                                                double mr, double mi, bool compact, int tid, int nthreads) {
    for (int i = tid; i < span + tail; i += nthreads) {
        const long g = first + i;
        cplx v = make_double2(0.0, 0.0);
        if (i < span && g >= 0 && g < n) v = iq_of(r_s[off + i], mr, mi);
        xs[compact ? i : xs_pad(i)] = v;
    }
}
// The same from the registers: the eight samples of chunk `tid` (in `pre`) go to the xs_pad layout at xq, staged entry
// i = 8*tid + u - off with off = first - first_al; zeros outside the span and outside the stream [0, n).
// Entries below 0 are never written, entries from `hi` on neither (the caller's bound: the zeros it wants behind the span).
__device__ __forceinline__ void raw_chunk_to_lds(cplx* xq, const uint4 pre, int tid, int off, long first, int span, int hi, long n,
                                                 double mr, double mi) {
    const int i_base = 8 * tid - off;
    const long g_base = first + i_base;
    const unsigned wv[4] = {pre.x, pre.y, pre.z, pre.w};
    if (i_base >= 0 && i_base + 8 <= span && g_base >= 0 && g_base + 8 <= n) {
        // the usual chunk: all eight samples inside the span and the stream -- no per-sample tests (they were most of this loop).
        // xs_pad(i_base + u) = xs_pad(i_base) + u + ((r + u) >> 2) with r = i_base & 3 = (-off) & 3, the same in every lane: the
        // eight slots are one lane address plus scalar offsets (three vector instructions per slot before)
        const int r = __builtin_amdgcn_readfirstlane((-off) & 3);
        cplx* xp = xq + xs_pad(i_base);
#pragma unroll
        for (int u = 0; u < 8; ++u) xp[u + ((r + u) >> 2)] = iq_of(wv[u >> 1] >> (16 * (u & 1)), mr, mi);
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i_base + u;
            const long g = first + i;
            cplx v = make_double2(0.0, 0.0);
            if (i < span && g >= 0 && g < n) v = iq_of(wv[u >> 1] >> (16 * (u & 1)), mr, mi);
            if (i >= 0 && i < hi) xq[xs_pad(i)] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// filter(coef,1,.) for FOUR consecutive outputs i0 .. i0+3 from the padded LDS copy xq (xs_pad indexing; i0 a multiple of
// 4): y[i] = sum_k coef[k] x[i-k], every accumulator taking its taps oldest first (transposed direct-form order) -- the
// one FIR loop of gather_core, sch_gather_fast, k_stream_tile and k_fine_cert's fused window build.
// NTP > 0: the tap count is a compile-time constant (the production fir1(46) filter): two trips per iteration with known
// bounds.  (Unrolled completely the compiler hoists every coefficient and sample load: 256 registers and scratch.)
// Tried and dropped (round 3): the taps through scalar loads from constant-address-space memory instead of LDS -- a third
// of this loop's LDS bytes are coefficient broadcasts, and the 1024-stream step gained 2.5 % -- but SMEM shares the LDS
// counter (lgkmcnt), every wait for a tap became a wait for the sample reads in flight, and the 64-stream step lost 3 us;
// pipelining it by hand (next trip's samples and taps requested before this trip's FMAs) cost registers the 80-register
// burst kernels do not have (scratch in the loop).
// PAD = false: the input is staged without xs_pad's bank padding (gather_carve's compact_xs).
// ------------------------------------------------------------------------------------------------
// UNR: trips of the four-tap loop the compiler may overlap (2: the next trip's LDS reads under this trip's FMAs, ~20 more
// registers; 1 where the caller has none to spare).
// taps of fir4_lds in LDS: rev[j] = coef[ntaps-1-j] (oldest tap first), zero-padded to a multiple of four
__host__ __device__ inline int fir_taps_padded(int ntaps) { return (ntaps + 3) & ~3; }
__device__ __forceinline__ void fir_stage_taps(double* c_s, const double* __restrict__ coef, int ntaps, int first, int step) {
    for (int i = first; i < fir_taps_padded(ntaps); i += step) c_s[i] = i < ntaps ? coef[ntaps - 1 - i] : 0.0;
}
template <int NTP, bool PAD = true, int UNR = 2>
__device__ __forceinline__ void fir4_lds(const cplx* __restrict__ xq, const double* __restrict__ c_s, int i0, int ntp_rt,
                                         cplx* y0, cplx* y1, cplx* y2, cplx* y3) {
#define XSP(p_) (PAD ? xs_pad(p_) : (p_))
    const int ntp = NTP > 0 ? NTP : ntp_rt;
    const int ntp4 = (ntp + 3) & ~3;
    double ar0 = 0.0, ai0 = 0.0, ar1 = 0.0, ai1 = 0.0, ar2 = 0.0, ai2 = 0.0, ar3 = 0.0, ai3 = 0.0;
    cplx w0 = xq[XSP(i0)], w1 = xq[XSP(i0 + 1)], w2 = xq[XSP(i0 + 2)], w3 = xq[XSP(i0 + 3)];
#define GSMCAL_FIR_TAP(C, A, B, D, E)                                   \
    ar0 = fma(C, A.x, ar0); ai0 = fma(C, A.y, ai0);                     \
    ar1 = fma(C, B.x, ar1); ai1 = fma(C, B.y, ai1);                     \
    ar2 = fma(C, D.x, ar2); ai2 = fma(C, D.y, ai2);                     \
    ar3 = fma(C, E.x, ar3); ai3 = fma(C, E.y, ai3);
    // four taps per trip: the next four samples are one aligned, contiguous 64-byte group (i0 is a multiple of 4),
    // fetched together, and so are the four taps (c_s holds them REVERSED -- oldest tap first -- and zero-padded to a multiple
    // of four: fir_stage_taps; two 16-byte reads per trip instead of four 8-byte ones, and no remainder loop:
    // fma(0, x, acc) = acc for the finite samples the callers stage behind the span).  Every accumulator still takes its
    // taps in the same order (oldest first), so the sums are bit-identical to a one-tap loop.
#pragma unroll UNR
    for (int t = 0; t < ntp4; t += 4) {
        const cplx* nx = xq + XSP(i0 + t + 4);
        const double c0 = c_s[t], c1 = c_s[t + 1], c2 = c_s[t + 2], c3 = c_s[t + 3];   // (before the samples: LDS returns in order, and the first taps need only these)
        const cplx n0s = nx[0], n1s = nx[1], n2s = nx[2], n3s = nx[3];
        GSMCAL_FIR_TAP(c0, w0, w1, w2, w3)
        GSMCAL_FIR_TAP(c1, w1, w2, w3, n0s)
        GSMCAL_FIR_TAP(c2, w2, w3, n0s, n1s)
        GSMCAL_FIR_TAP(c3, w3, n0s, n1s, n2s)
        w0 = n0s; w1 = n1s; w2 = n2s; w3 = n3s;
    }
#undef GSMCAL_FIR_TAP
#undef XSP
    *y0 = make_double2(ar0, ai0); *y1 = make_double2(ar1, ai1); *y2 = make_double2(ar2, ai2); *y3 = make_double2(ar3, ai3);
}
// outputs i0 .. i0+3 of a pass of cnt: the first exists (i0 < cnt is the caller's loop test), the other three may lie behind the end
__device__ __forceinline__ void fir4_store(cplx* out, int i0, int cnt, cplx y0, cplx y1, cplx y2, cplx y3) {
    out[i0] = y0;
    if (i0 + 1 < cnt) out[i0 + 1] = y1;
    if (i0 + 2 < cnt) out[i0 + 2] = y2;
    if (i0 + 3 < cnt) out[i0 + 3] = y3;
}

// four consecutive outputs i0 .. i0+3 (i0 a multiple of 4) of the 47-tap symmetric filter from the padded copy xq; c[t] = coef[t], t < 24:
// the 24 distinct taps live in registers, and the FIR of a lane's four outputs is one unrolled pass over its 50 input samples, each
// read ONCE and used at once by the up to four outputs it belongs to -- every output still takes its taps oldest first, so the sums
// are those of fir4_lds bit for bit
template <int S0, int G>
__device__ __forceinline__ void fir4_sym47_load(const cplx* __restrict__ x0, cplx (&v)[G]) {
#pragma unroll
    for (int u = 0; u < G; ++u) { constexpr int dummy = 0; (void)dummy; const int sn = S0 + u; v[u] = x0[sn + (sn >> 2)]; }
}
template <int S0, int G>
__device__ __forceinline__ void fir4_sym47_mac(const cplx (&v)[G], const double (&c)[24], double (&ar)[4], double (&ai)[4]) {
#pragma unroll
    for (int u = 0; u < G; ++u) {
        const int s = S0 + u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = s - j;                          // output i0+j takes sample i0+s with tap rev[t] = coef[46-t] = coef[t]
            if (t >= 0 && t < 47) {
                const double cc = c[t < 24 ? t : 46 - t];
                ar[j] = fma(cc, v[u].x, ar[j]);
                ai[j] = fma(cc, v[u].y, ai[j]);
            }
        }
    }
}
__device__ __forceinline__ void fir4_sym47(const cplx* __restrict__ xq, const double (&c)[24], int i0, cplx* y) {
    double ar[4] = {0.0, 0.0, 0.0, 0.0}, ai[4] = {0.0, 0.0, 0.0, 0.0};
    const cplx* x0 = xq + xs_pad(i0);                    // i0 % 4 == 0: xs_pad(i0 + s) = xs_pad(i0) + s + (s >> 2)
    // ten groups of five samples in two register sets: the next group's LDS reads are issued ahead of this group's FMAs, and a
    // scheduling barrier per group keeps the compiler from hoisting all fifty reads to the top (255 registers, one wave per SIMD)
    constexpr int G = 5;
    cplx A[G], B[G];
    fir4_sym47_load<0, G>(x0, A);
#define FIR47_PAIR(g)                                                   \
    fir4_sym47_load<G * ((g) + 1), G>(x0, B);                           \
    fir4_sym47_mac<G * (g), G>(A, c, ar, ai);                           \
    __builtin_amdgcn_sched_barrier(0);                                  \
    if ((g) + 2 < 50 / G) fir4_sym47_load<G * ((g) + 2), G>(x0, A);     \
    fir4_sym47_mac<G * ((g) + 1), G>(B, c, ar, ai);                     \
    __builtin_amdgcn_sched_barrier(0);
    FIR47_PAIR(0) FIR47_PAIR(2) FIR47_PAIR(4) FIR47_PAIR(6) FIR47_PAIR(8)
#undef FIR47_PAIR
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = make_double2(ar[j], ai[j]);
}

// ---- plans -------------------------------------------------------------------------------------------------------------
// What the stream-tile kernels need of a stream's chain (all fields fetched up front).  ok: the chain is
// (lerp, mix, lerp|copy, mix); a stream with another chain has no r_correct.  A COPY at level 3 is a LERP with factor 1.
struct StChain { bool ok; double f1, c2, f3, c4; long nq, n0, n2; double mr, mi; };
__device__ __forceinline__ StChain st_chain(const StreamState* st) {
    StChain c;
    c.n0 = st->n0;
    c.mr = st->mean_re; c.mi = st->mean_im;
    int ty[NLEVELS]; double pa[NLEVELS]; long ln[NLEVELS];
    ty[0] = OP_NONE; pa[0] = 0.0; ln[0] = c.n0;
#pragma unroll
    for (int j = 1; j < NLEVELS; ++j) { ty[j] = st->op[j].type; pa[j] = st->op[j].param; ln[j] = st->op[j].n; }
    c.ok = ty[1] == OP_LERP && ty[2] == OP_MIX && (ty[3] == OP_LERP || ty[3] == OP_COPY) && ty[4] == OP_MIX;
    c.f1 = pa[1]; c.c2 = pa[2]; c.f3 = ty[3] == OP_COPY ? 1.0 : pa[3]; c.c4 = pa[4];
    c.nq = ln[4]; c.n2 = ln[2];
    return c;
}
// The window the fine search has filtered already (lane l < nf holds its start fw; l0_len level-0 samples each) that holds all
// of [lo0, hi0]: its index, or -1, and the offset of lo0 inside it.  One ballot: every lane of the wave must call this.
struct FineWin { int h; long off; };
__device__ __forceinline__ FineWin fine_window_holding(long fw, int nf, long lo0, long hi0, int l0_len, int lane) {
    FineWin w;
    w.h = -1; w.off = 0;
    const unsigned long long m = __ballot(lane < nf && lane < MAXH && fw <= lo0 && hi0 < fw + l0_len);
    if (m) {
        w.h = __ffsll((long long)m) - 1;
        w.off = lo0 - __shfl(fw, w.h, 64);
    }
    return w;
}
#endif  // __HIPCC__
