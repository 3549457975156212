// kernels_pair.h -- pair_coherence: how far apart two corrected streams are in time, to a fraction of a sample, and in
// carrier phase; how coherent they are; how fast they still drift.  The project's own function: the reference names the goal
// ("to let them work together coherently") and stops at a difference of integer burst positions (gsm_sync_demod.m:149-158).  The
// definition is DESIGN 19's and tests/pair_coherence_ref.py restates it.
//
// Per pair (a, b) of streams and per type-1 / type-2 row of a's table (1-based start pos, p = round(pos) - 1): the burst's
// L = 148 ov samples of a in K = 4 segments of Ls = 37 ov, correlated with b at the lags lag0 + m, m = -M..M:
//   c[m][k] = sum_n b[p + lag0 + m + k Ls + n] conj(a[p + k Ls + n]),  Ea[k] = sum |a|^2,  Eb[m][k] = sum |b|^2 over the same samples
// (one whole-burst sum loses coherence under the carrier offset the chain leaves; four segments measure it).
//
// k_pair_xcorr: grid (GSMCAL_MAX_PAIR_BURSTS, P), block 256 -- one workgroup per (burst slot, pair); every wave finds the slot's row
// itself (pos_row_select under PosBurst).  The two windows, L and L + 2M complex samples, go to LDS once and are read as 16-byte
// values; wave k owns segment k.  Its 64 lanes are 16 lags x 4 sample phases: lane l takes the lags (l & 15) + 16 j and the samples
// (l >> 4) + 4 i, so a lane holds at most PX_NJ = 5 lag accumulators (65 lags at ov 8, M 32), as compile-time indexed registers.
// The four sample phases are added by two xor exchanges, the same order in every lane; nothing is accumulated in memory.  Wave 0
// then forms y[m] = sum_k |c[m][k]|^2 and takes the FIRST maximum m* (a ballot: the lowest lag among equal values).  Written per
// slot: part[pair][slot][PX_PART] (PX_* below) -- c, Ea, Eb at m* and y at m* - 1, m*, m* + 1: what k_pair_finish needs, 192
// bytes instead of the 12 KB of all lags -- and, when asked for, corr_out[pair][slot][2M+1][4], NaN for a slot that is not
// evaluated.  Evaluated iff the slot has a row, neither stream is empty, the table has at most GSMCAL_MAX_PAIR_BURSTS such rows and
// both windows lie inside their streams: decided before a sample is read.
//
// k_pair_finish: grid P, block 64 -- one wave per pair, lane l holds bursts l and l + 64.  Per burst the parabola through y around
// m*, the segment-to-segment phase step (freq), the phase at the burst's centre and the coherence; per pair the line through the
// delays, the mean frequency refined by the phase steps between adjacent bursts, and the phase at the first used burst.  Every sum
// over bursts is wave_sum: one fixed order.  out[pair] = one row of GSMCAL_PAIR_COLS doubles (GSMCAL_P_*), written here and nowhere
// else.
#pragma once
#include "kernels_demod.h"

#define PX_THREADS 256
#define PX_K 4                      /* segments per burst */
#define PX_NJ 5                     /* lag accumulators per lane: ceil((2 * 32 + 1) / 16) */
#define PX_MAX_NL 65                /* 2 M + 1 at the largest M = 4 * 8 */
#define PX_SLOTS GSMCAL_MAX_PAIR_BURSTS
#define PX_PART 24
enum { PX_EVAL = 0, PX_P = 1, PX_POS = 2, PX_MSTAR = 3, PX_YM = 4, PX_Y0 = 5, PX_YP = 6, PX_C = 7, PX_EA = 15, PX_EB = 19 };

inline size_t px_lds_bytes(int ov, int M) { return ((size_t)2 * 148 * ov + 2 * M) * sizeof(cplx); }

__device__ __forceinline__ double px_shfl_xor(double v, int mask) {
    return __hiloint2double(__shfl_xor(__double2hiint(v), mask, 64), __shfl_xor(__double2loint(v), mask, 64));
}
// the four sample phases of a lag sit in lanes g, g + 16, g + 32, g + 48: (v0 + v1) + (v2 + v3) in every one of them
__device__ __forceinline__ double px_phase_sum(double v) {
    v += px_shfl_xor(v, 16);
    v += px_shfl_xor(v, 32);
    return v;
}
__device__ __forceinline__ double px_wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, px_shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ double px_wave_min(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, px_shfl_xor(v, off));
    return v;
}

// pairs[q] = {a, b, lag0}: stream indices checked on the host
__global__ void __launch_bounds__(PX_THREADS) k_pair_xcorr(const cplx* __restrict__ r, long stride, const long* __restrict__ r_len,
                                                           const double* __restrict__ pos_info, int ov, int M,
                                                           const int* __restrict__ pairs, double* __restrict__ part,
                                                           cplx* __restrict__ corr_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ cplx cs[PX_MAX_NL][PX_K];
    __shared__ double ebs[PX_MAX_NL][PX_K];
    __shared__ double eas[PX_K];
    const int q = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sa = pairs[3 * q], sb = pairs[3 * q + 1], lag0 = pairs[3 * q + 2];
    const int L = 148 * ov, Ls = 37 * ov, NL = 2 * M + 1;
    const long len_a = stream_len(r_len, sa, stride), len_b = stream_len(r_len, sb, stride);
    const double* pi = pos_info + (size_t)sa * 2 * MAXROWS;
    double* out = part + ((size_t)q * PX_SLOTS + b) * PX_PART;
    cplx* oc = corr_out ? corr_out + ((size_t)q * PX_SLOTS + b) * NL * PX_K : nullptr;
    int row;
    const int nb = pos_row_select(pi, lane, b, PosBurst(), row);
    const double pos = row >= 0 ? pi[row] : 0.0;
    // ---- evaluated?  block-uniform, before a sample is read.  pos >= 0.5 is round(pos) >= 1; beyond len_a + 1 no window fits ----
    bool ev = len_a >= 1 && len_b >= 1 && row >= 0 && nb <= PX_SLOTS && pos >= 0.5 && pos <= (double)len_a + 1.0;
    long p = 0, lo_b = 0;
    if (ev) {
        p = (long)round(pos) - 1;                                  // MATLAB's round: half away from zero
        lo_b = p + (long)lag0 - M;
        ev = p + L <= len_a && lo_b >= 0 && lo_b + 2 * M + L <= len_b;
    }
    if (!ev) {
        if (tid == 0) out[PX_EVAL] = 0.0;
        if (oc)
            for (int i = tid; i < NL * PX_K; i += PX_THREADS) oc[i] = make_double2(NAN_D, NAN_D);
        return;
    }
    // ---- the two windows ----
    cplx* a_s = (cplx*)smem;
    cplx* b_s = a_s + L;
    const cplx* xa = r + (size_t)sa * stride + p;
    const cplx* xb = r + (size_t)sb * stride + lo_b;
    for (int i = tid; i < L; i += PX_THREADS) a_s[i] = xa[i];
    for (int i = tid; i < L + 2 * M; i += PX_THREADS) b_s[i] = xb[i];
    __syncthreads();
    // ---- segment `wave`: lane = 16 lags x 4 sample phases ----
    const cplx* as = a_s + wave * Ls;
    const cplx* bs = b_s + wave * Ls;
    const int g = lane & 15, sp = lane >> 4;
    const int nj = (NL + 15) >> 4;                                 // (uniform) lag rounds in use
    double cr[PX_NJ], ci[PX_NJ], eb[PX_NJ], ea = 0.0;
    int mi[PX_NJ];
#pragma unroll
    for (int j = 0; j < PX_NJ; ++j) {
        cr[j] = 0.0; ci[j] = 0.0; eb[j] = 0.0;
        mi[j] = g + 16 * j < NL ? g + 16 * j : NL - 1;             // a lane past the last lag repeats it: no branch in the loop
    }
    for (int n = sp; n < Ls; n += 4) {
        const cplx av = as[n];
        ea = fma(av.x, av.x, fma(av.y, av.y, ea));
#pragma unroll
        for (int j = 0; j < PX_NJ; ++j)
            if (j < nj) {                                          // (uniform)
                const cplx bv = bs[n + mi[j]];                     // b conj(a)
                cr[j] = fma(bv.x, av.x, fma(bv.y, av.y, cr[j]));
                ci[j] = fma(bv.y, av.x, fma(-bv.x, av.y, ci[j]));
                eb[j] = fma(bv.x, bv.x, fma(bv.y, bv.y, eb[j]));
            }
    }
    ea = px_phase_sum(ea);
#pragma unroll
    for (int j = 0; j < PX_NJ; ++j)
        if (j < nj) {
            const double sr = px_phase_sum(cr[j]), si = px_phase_sum(ci[j]), se = px_phase_sum(eb[j]);
            if (sp == 0 && g + 16 * j < NL) {
                cs[g + 16 * j][wave] = make_double2(sr, si);
                ebs[g + 16 * j][wave] = se;
            }
        }
    if (lane == 0) eas[wave] = ea;
    __syncthreads();
    if (oc)
        for (int i = tid; i < NL * PX_K; i += PX_THREADS) oc[i] = cs[i >> 2][i & 3];
    if (wave != 0) return;
    // ---- y[m] and its first maximum: lane l holds lags l and l + 64 ----
    double y0 = -1.0, y1 = -1.0;
    if (lane < NL) {
        y0 = 0.0;
        for (int k = 0; k < PX_K; ++k) y0 += cs[lane][k].x * cs[lane][k].x + cs[lane][k].y * cs[lane][k].y;
    }
    if (lane + 64 < NL) {
        y1 = 0.0;
        for (int k = 0; k < PX_K; ++k) y1 += cs[lane + 64][k].x * cs[lane + 64][k].x + cs[lane + 64][k].y * cs[lane + 64][k].y;
    }
    const double ymax = px_wave_max(fmax(y0, y1));
    const unsigned long long m0 = __ballot(lane < NL && y0 == ymax), m1 = __ballot(lane + 64 < NL && y1 == ymax);
    const int ms = m0 ? __ffsll((long long)m0) - 1 : m1 ? 64 : 0;  // (y NaN everywhere: lag index 0, an edge)
    const bool inner = ms > 0 && ms < NL - 1;
    if (lane == 0) {
        const int lo = inner ? ms - 1 : ms, hi = inner ? ms + 1 : ms;
        double yl = 0.0, yc = 0.0, yh = 0.0;
        for (int k = 0; k < PX_K; ++k) {
            yl += cs[lo][k].x * cs[lo][k].x + cs[lo][k].y * cs[lo][k].y;
            yc += cs[ms][k].x * cs[ms][k].x + cs[ms][k].y * cs[ms][k].y;
            yh += cs[hi][k].x * cs[hi][k].x + cs[hi][k].y * cs[hi][k].y;
        }
        out[PX_EVAL] = 1.0;
        out[PX_P] = (double)p;
        out[PX_POS] = pos;
        out[PX_MSTAR] = (double)(ms - M);
        out[PX_YM] = yl; out[PX_Y0] = yc; out[PX_YP] = yh;
        for (int k = 0; k < PX_K; ++k) {
            out[PX_C + 2 * k] = cs[ms][k].x;
            out[PX_C + 2 * k + 1] = cs[ms][k].y;
            out[PX_EA + k] = eas[k];
            out[PX_EB + k] = ebs[ms][k];
        }
    }
}

// what one lane of k_pair_finish knows about one burst
struct PxBurst {
    bool ev, edge, used;
    double p, pos, delay, phase, freq, coh;
};
__device__ __forceinline__ PxBurst px_burst(const double* __restrict__ rec, bool mine, int lag0, int M, double fs, int Ls,
                                            double min_coh) {
    PxBurst u;
    u.ev = mine && rec[PX_EVAL] == 1.0;
    u.edge = false; u.used = false;
    u.p = 0.0; u.pos = NAN_D; u.delay = NAN_D; u.phase = NAN_D; u.freq = NAN_D; u.coh = NAN_D;
    if (!u.ev) return u;
    u.p = rec[PX_P];
    u.pos = rec[PX_POS];
    const double ms = rec[PX_MSTAR];
    u.edge = ms == (double)-M || ms == (double)M;
    if (u.edge) return u;
    const double ym = rec[PX_YM], y0 = rec[PX_Y0], yp = rec[PX_YP];
    u.delay = (double)lag0 + ms + 0.5 * (ym - yp) / (ym - 2.0 * y0 + yp);
    cplx c[PX_K];
    double sabs = 0.0, sea = 0.0, seb = 0.0;
#pragma unroll
    for (int k = 0; k < PX_K; ++k) {
        c[k] = make_double2(rec[PX_C + 2 * k], rec[PX_C + 2 * k + 1]);
        sabs += hypot(c[k].x, c[k].y);
        sea += rec[PX_EA + k];
        seb += rec[PX_EB + k];
    }
    double zr = 0.0, zi = 0.0;
#pragma unroll
    for (int k = 0; k < PX_K - 1; ++k) {                           // c[k+1] conj(c[k])
        zr += c[k + 1].x * c[k].x + c[k + 1].y * c[k].y;
        zi += c[k + 1].y * c[k].x - c[k + 1].x * c[k].y;
    }
    const double th = atan2(zi, zr);
    u.freq = th * fs / (TWO_PI_D * (double)Ls);
    double sr = 0.0, si = 0.0;
#pragma unroll
    for (int k = 0; k < PX_K; ++k) {
        double sn, cn;
        sincos(-th * ((double)k - 1.5), &sn, &cn);
        sr += c[k].x * cn - c[k].y * sn;
        si += c[k].x * sn + c[k].y * cn;
    }
    u.phase = atan2(si, sr);
    const double den = sqrt(sea * seb);
    u.coh = den > 0.0 ? sabs / den : NAN_D;
    u.used = u.coh >= min_coh;                                     // (NaN is not used)
    return u;
}

// The per-pair summaries over the used bursts (windows) of one pair, shared by k_pair_finish and k_row_finish (kernels_rowcoh.h): one
// wave, lane l holds the entries l (u0) and l + 64 (u1); k0, k1: the ballots of their `used`, at least two of them set; gap_limit:
// the largest distance in samples between two consecutive used entries whose phase step refines the carrier; up, uph: LDS for the
// used entries' p and phase in table order (one slot per entry).  Every sum over the entries is wave_sum: one fixed order.
struct PxSummary {
    double delay0 = NAN_D, ppm = NAN_D, drms = NAN_D, rel = NAN_D, fc = NAN_D, phase0 = NAN_D, prms = NAN_D, cmean = NAN_D, cmin = NAN_D;
    int nadj = 0;
};
__device__ __forceinline__ PxSummary px_summaries(const PxBurst& u0, const PxBurst& u1, unsigned long long k0, unsigned long long k1,
                                                  double gap_limit, double fs, int lane, double* up, double* uph) {
    PxSummary s;
    const int n = __popcll(k0) + __popcll(k1);
    const double dn = (double)n;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int r0 = __popcll(k0 & below), r1 = __popcll(k0) + __popcll(k1 & below);      // ranks among the used bursts
    if (u0.used) { up[r0] = u0.p; uph[r0] = u0.phase; }
    if (u1.used) { up[r1] = u1.p; uph[r1] = u1.phase; }
    __syncthreads();
    const double p_first = up[0];
    const double t0 = u0.p - p_first, t1 = u1.p - p_first;
    // ---- the line of delay on t, two passes ----
    const double tbar = wave_sum((u0.used ? t0 : 0.0) + (u1.used ? t1 : 0.0)) / dn;
    const double dbar = wave_sum((u0.used ? u0.delay : 0.0) + (u1.used ? u1.delay : 0.0)) / dn;
    const double a0 = t0 - tbar, a1 = t1 - tbar;
    const double sxx = wave_sum((u0.used ? a0 * a0 : 0.0) + (u1.used ? a1 * a1 : 0.0));
    const double sxy = wave_sum((u0.used ? a0 * (u0.delay - dbar) : 0.0) + (u1.used ? a1 * (u1.delay - dbar) : 0.0));
    const double slope = sxy / sxx;
    s.delay0 = dbar - slope * tbar;
    s.ppm = 1e6 * slope;
    const double q0 = u0.delay - (s.delay0 + slope * t0), q1 = u1.delay - (s.delay0 + slope * t1);
    s.drms = sqrt(wave_sum((u0.used ? q0 * q0 : 0.0) + (u1.used ? q1 * q1 : 0.0)) / dn);
    const double fc = wave_sum((u0.used ? u0.freq : 0.0) + (u1.used ? u1.freq : 0.0)) / dn;
    s.fc = fc;
    // ---- the phase steps between adjacent used bursts: lane l takes the steps l -> l + 1 and l + 64 -> l + 65 ----
    double zr = 0.0, zi = 0.0, gs = 0.0;
    int na = 0;
    for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h;
        if (i + 1 < n) {
            const double gp = up[i + 1] - up[i];
            if (gp <= gap_limit) {
                double sn, cn;
                sincos(uph[i + 1] - uph[i] - TWO_PI_D * fc * gp / fs, &sn, &cn);
                zr += cn; zi += sn; gs += gp; ++na;
            }
        }
    }
    zr = wave_sum(zr); zi = wave_sum(zi); gs = wave_sum(gs);
    s.nadj = (int)wave_sum_u32((unsigned)na);
    const double rel = s.nadj > 0 ? fc + atan2(zi, zr) * fs / (TWO_PI_D * (gs / (double)s.nadj)) : fc;
    s.rel = rel;
    // ---- the phase at the first used burst ----
    const double w0 = u0.phase - TWO_PI_D * rel * t0 / fs, w1 = u1.phase - TWO_PI_D * rel * t1 / fs;
    double s0 = 0.0, c0 = 0.0, s1 = 0.0, c1 = 0.0;
    if (u0.used) sincos(w0, &s0, &c0);
    if (u1.used) sincos(w1, &s1, &c1);
    const double phase0 = atan2(wave_sum(s0 + s1), wave_sum(c0 + c1));
    s.phase0 = phase0;
    double d0 = 0.0, d1 = 0.0;
    if (u0.used) { double sn, cn; sincos(w0 - phase0, &sn, &cn); d0 = atan2(sn, cn); }
    if (u1.used) { double sn, cn; sincos(w1 - phase0, &sn, &cn); d1 = atan2(sn, cn); }
    s.prms = sqrt(wave_sum(d0 * d0 + d1 * d1) / dn);
    s.cmean = wave_sum((u0.used ? u0.coh : 0.0) + (u1.used ? u1.coh : 0.0)) / dn;
    s.cmin = px_wave_min(fmin(u0.used ? u0.coh : 2.0, u1.used ? u1.coh : 2.0));
    return s;
}

__global__ void __launch_bounds__(64) k_pair_finish(const long* __restrict__ r_len, long stride, const double* __restrict__ pos_info,
                                                    int ov, int M, double min_coh, const int* __restrict__ pairs,
                                                    const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double up[PX_SLOTS], uph[PX_SLOTS];                 // the used bursts in table order: p and phase
    const int q = blockIdx.x, lane = threadIdx.x;
    const int sa = pairs[3 * q], sb = pairs[3 * q + 1], lag0 = pairs[3 * q + 2];
    const double* pi = pos_info + (size_t)sa * 2 * MAXROWS;
    const double* ps = part + (size_t)q * PX_SLOTS * PX_PART;
    double* o = out + (size_t)q * GSMCAL_PAIR_COLS;
    const double fs = GSM_SYMBOL_RATE * (double)ov;
    const int Ls = 37 * ov;
    StreamHead head = stream_head(r_len, sa, stride, pi, lane);
    if (stream_len(r_len, sb, stride) < 1) head.len = 0;            // either stream empty: the same exit
    int nb = pos_rows_count(pi, lane, PosBurst());
    int status = head.status(nb, PX_SLOTS);
    const bool run = status == 0;
    const int j1 = lane + 64;
    const PxBurst u0 = px_burst(ps + (size_t)lane * PX_PART, run && lane < nb, lag0, M, fs, Ls, min_coh);
    const PxBurst u1 = px_burst(ps + (size_t)(j1 < PX_SLOTS ? j1 : 0) * PX_PART, run && j1 < nb && j1 < PX_SLOTS, lag0, M, fs, Ls, min_coh);
    const unsigned long long e0 = __ballot(u0.ev), e1 = __ballot(u1.ev), k0 = __ballot(u0.used), k1 = __ballot(u1.used);
    const int num_eval = __popcll(e0) + __popcll(e1), n = __popcll(k0) + __popcll(k1);
    // ---- the per-burst columns ----
    o[GSMCAL_P_POS + lane] = u0.pos;
    o[GSMCAL_P_DELAY + lane] = u0.delay;
    o[GSMCAL_P_PHASE + lane] = u0.phase;
    o[GSMCAL_P_FREQ + lane] = u0.freq;
    o[GSMCAL_P_COH + lane] = u0.coh;
    o[GSMCAL_P_EDGE + lane] = u0.ev ? (u0.edge ? 1.0 : 0.0) : NAN_D;
    if (j1 < PX_SLOTS) {
        o[GSMCAL_P_POS + j1] = u1.pos;
        o[GSMCAL_P_DELAY + j1] = u1.delay;
        o[GSMCAL_P_PHASE + j1] = u1.phase;
        o[GSMCAL_P_FREQ + j1] = u1.freq;
        o[GSMCAL_P_COH + j1] = u1.coh;
        o[GSMCAL_P_EDGE + j1] = u1.ev ? (u1.edge ? 1.0 : 0.0) : NAN_D;
    }
    if (run && n < 2) status = GSMCAL_S_PAIR_FEW;
    PxSummary s;
    if (status == 0) s = px_summaries(u0, u1, k0, k1, 1875.0 * (double)ov, fs, lane, up, uph);    // (uniform)
    if (lane == 0) {
        o[GSMCAL_P_STATUS] = (double)status;
        o[GSMCAL_P_NUM_BURSTS] = (double)nb;
        o[GSMCAL_P_NUM_EVAL] = (double)num_eval;
        o[GSMCAL_P_NUM_USED] = (double)n;
        o[GSMCAL_P_NUM_ADJACENT] = (double)s.nadj;
        o[GSMCAL_P_LAG0] = (double)lag0;
        o[GSMCAL_P_DELAY0] = s.delay0;
        o[GSMCAL_P_REL_SAMPLING_PPM] = s.ppm;
        o[GSMCAL_P_DELAY_RMS] = s.drms;
        o[GSMCAL_P_REL_CARRIER_HZ] = s.rel;
        o[GSMCAL_P_BURST_CARRIER_HZ] = s.fc;
        o[GSMCAL_P_PHASE0] = s.phase0;
        o[GSMCAL_P_PHASE_RMS] = s.prms;
        o[GSMCAL_P_MEAN_COHERENCE] = s.cmean;
        o[GSMCAL_P_MIN_COHERENCE_SEEN] = s.cmin;
        o[GSMCAL_P_MAX_LAG] = (double)M;
    }
}
