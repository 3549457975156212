// kernels_rowcoh.h -- row_coherence: pair_coherence's estimator (kernels_pair.h) on any rows on one nominal
// time base -- the output rows of apply_calibration, for instance -- over a caller's list of windows of one length.  The project's
// own function; the definition is DESIGN 24's and tests/row_coherence_ref.py restates it.
//
// Per pair (a, b) of rows and per window start p: the 4 Ls first samples of the window (Ls = win_len / 4) in K = 4 segments,
// correlated with b at the lags lag0 + m, m = -M..M, M <= 64:
//   c[m][k] = sum_n b[p + lag0 + m + k Ls + n] conj(a[p + k Ls + n]),  Ea[k] = sum |a|^2,  Eb[m][k] = sum |b|^2 over the same samples.
//
// k_row_xcorr<NJ>: grid (W, P), block 256 -- one workgroup per (window, pair), wave k owns segment k, its 64 lanes are 16 lags x 4
// sample phases as in k_pair_xcorr: lane l takes the lags (l & 15) + 16 j, j < NJ, and the samples (l >> 4) + 4 i.  A segment may be
// 16 384 samples long, so it does not go to LDS whole: every wave stages its segment tile by tile, RX_TILE samples of a and
// RX_TILE + 2 M of b, read back as 16-byte values (24 KB for the four waves; with the results' 12 KB below 40 KB per workgroup, so
// four workgroups fit a CU).  Lane (sp, g) reads b at the complex index n + sp + g + 16 j: the 16 lanes ds_read_b128 serves together
// hold indices within a span of 19, and two indices of one such group never differ by 16 (the groups are {0-3, 12-15, 20-27}, ...:
// the second sample phase of a group starts where the first one's lanes leave a hole), so every distinct address of a group has a
// 16-byte slot of its own; the a value is one address per sample phase.  tests/test_row_coherence_cpu.py counts it.
// The order of the sums (include/gsmcal.h): chunks of GSMCAL_ROW_CHUNK samples from the segment's start -- a multiple of RX_TILE, so
// a chunk is whole tiles --, in a chunk one partial sum per sample phase, ascending, the explicit fma nesting of k_pair_xcorr, the
// four phases added by two xor exchanges ((s0 + s1) + (s2 + s3) in every lane), the chunk sums added in chunk order.  For Ls <= 512
// this is k_pair_xcorr's order to the bit.  Nothing is accumulated in memory.
// NJ = ceil((2 M + 1) / 16) rounded up to 1, 2, 3, 5 or 9: the lag accumulators are compile-time indexed registers (9 rounds: 27
// running and 27 chunk-total doubles per lane; tools/resource_usage.sh shows no scratch).
// Wave 0 then forms y[m] = sum_k |c[m][k]|^2 and takes the FIRST maximum by ballots over the three lags l, l + 64, l + 128 of a lane.
// Written per window: part[pair][window][PX_PART], the PX_* record of kernels_pair.h (PX_POS holds the start), and, when asked for,
// corr_out[pair][window][2M+1][4], NaN for a window that is not evaluated.  Evaluated iff both spans lie inside the rows' valid
// intervals: decided before a sample is read.
//
// k_row_finish: grid P, block 64 -- one wave per pair, lane l holds windows l and l + 64: px_burst per window, px_summaries per pair
// (both kernels_pair.h's), out[pair] = one row of GSMCAL_ROW_COLS doubles (GSMCAL_R_*), written here and nowhere else.
#pragma once
#include "kernels_pair.h"

#define RX_TILE 128                  /* samples of a per wave and staging step; GSMCAL_ROW_CHUNK is a multiple of it */
#define RX_MAX_NL (2 * GSMCAL_MAX_ROW_LAG + 1)
#define RX_MAX_NJ 9                  /* ceil(129 / 16) */
static_assert(GSMCAL_ROW_CHUNK % RX_TILE == 0 && RX_TILE % 4 == 0, "a chunk of the sums is whole staging tiles");
static_assert(GSMCAL_ROW_COLS == GSMCAL_R_EDGE + GSMCAL_MAX_ROW_WINDOWS && GSMCAL_MAX_ROW_WINDOWS <= 128, "two windows per lane of k_row_finish");

// what a call uploads: in[0 .. 2d) the rows' {first, end}, then W starts, then per pair {a, b, lag0}
struct RowIn {
    const long* valid;
    const long* starts;
    const long* pairs;
};

template <int NJ>
__global__ void __launch_bounds__(PX_THREADS) k_row_xcorr(const cplx* __restrict__ x, long stride, RowIn in, int Ls, int M,
                                                          double* __restrict__ part, cplx* __restrict__ corr_out) {
    __shared__ __attribute__((aligned(16))) cplx a_t[PX_K][RX_TILE];
    __shared__ __attribute__((aligned(16))) cplx b_t[PX_K][RX_TILE + 2 * GSMCAL_MAX_ROW_LAG];
    __shared__ cplx cs[RX_MAX_NL][PX_K];
    __shared__ double ebs[RX_MAX_NL][PX_K];
    __shared__ double eas[PX_K];
    const int q = blockIdx.y, w = blockIdx.x, W = gridDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long sa = in.pairs[3 * q], sb = in.pairs[3 * q + 1], lag0 = in.pairs[3 * q + 2];
    const long p = in.starts[w];
    const int NL = 2 * M + 1;
    const long L4 = 4L * Ls;
    double* out = part + ((size_t)q * W + w) * PX_PART;
    cplx* oc = corr_out ? corr_out + ((size_t)q * W + w) * NL * PX_K : nullptr;
    // ---- evaluated?  block-uniform, before a sample is read (p <= end_a - L4 first: p is then no larger than stride) ----
    const long first_a = in.valid[2 * sa], end_a = in.valid[2 * sa + 1], first_b = in.valid[2 * sb], end_b = in.valid[2 * sb + 1];
    bool ev = first_a <= p && p <= end_a - L4;
    long lo_b = 0;
    if (ev) {
        lo_b = p + lag0 - M;
        ev = first_b <= lo_b && lo_b + 2 * M + L4 <= end_b;
    }
    if (!ev) {
        if (tid == 0) out[PX_EVAL] = 0.0;
        if (oc)
            for (int i = tid; i < NL * PX_K; i += PX_THREADS) oc[i] = make_double2(NAN_D, NAN_D);
        return;
    }
    // ---- segment `wave`, tile by tile: lane = 16 lags x 4 sample phases ----
    const cplx* xa = x + (size_t)sa * stride + p + (long)wave * Ls;
    const cplx* xb = x + (size_t)sb * stride + lo_b + (long)wave * Ls;
    const cplx* as = a_t[wave];
    const cplx* bs = b_t[wave];
    const int g = lane & 15, sp = lane >> 4;
    const int nj = (NL + 15) >> 4;                                 // (uniform) lag rounds in use, <= NJ
    double cr[NJ], ci[NJ], eb[NJ], ea = 0.0;                       // the running chunk
    double tr[NJ], ti[NJ], te[NJ], ta = 0.0;                       // the chunks before it
    int mi[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        cr[j] = 0.0; ci[j] = 0.0; eb[j] = 0.0; tr[j] = 0.0; ti[j] = 0.0; te[j] = 0.0;
        mi[j] = g + 16 * j < NL ? g + 16 * j : NL - 1;             // a lane past the last lag repeats it: no branch in the loop
    }
    bool first_chunk = true;
    for (int t0 = 0; t0 < Ls; t0 += RX_TILE) {                     // (uniform: the four segments have one length)
        const int tn = min(RX_TILE, Ls - t0);
        __syncthreads();                                           // the tile before has been read
        for (int i = lane; i < tn; i += 64) a_t[wave][i] = xa[t0 + i];
        for (int i = lane; i < tn + 2 * M; i += 64) b_t[wave][i] = xb[t0 + i];
        __syncthreads();
        for (int n = sp; n < tn; n += 4) {
            const cplx av = as[n];
            ea = fma(av.x, av.x, fma(av.y, av.y, ea));
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (j < nj) {                                      // (uniform)
                    const cplx bv = bs[n + mi[j]];                 // b conj(a)
                    cr[j] = fma(bv.x, av.x, fma(bv.y, av.y, cr[j]));
                    ci[j] = fma(bv.y, av.x, fma(-bv.x, av.y, ci[j]));
                    eb[j] = fma(bv.x, bv.x, fma(bv.y, bv.y, eb[j]));
                }
        }
        const int done = t0 + tn;
        if (done == Ls || done % GSMCAL_ROW_CHUNK == 0) {          // (uniform) the chunk ends here
            const double sea = px_phase_sum(ea);
            ta = first_chunk ? sea : ta + sea;
            ea = 0.0;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (j < nj) {
                    const double sr = px_phase_sum(cr[j]), si = px_phase_sum(ci[j]), se = px_phase_sum(eb[j]);
                    tr[j] = first_chunk ? sr : tr[j] + sr;
                    ti[j] = first_chunk ? si : ti[j] + si;
                    te[j] = first_chunk ? se : te[j] + se;
                    cr[j] = 0.0; ci[j] = 0.0; eb[j] = 0.0;
                }
            first_chunk = false;
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (j < nj && sp == 0 && g + 16 * j < NL) {
            cs[g + 16 * j][wave] = make_double2(tr[j], ti[j]);
            ebs[g + 16 * j][wave] = te[j];
        }
    if (lane == 0) eas[wave] = ta;
    __syncthreads();
    if (oc)
        for (int i = tid; i < NL * PX_K; i += PX_THREADS) oc[i] = cs[i >> 2][i & 3];
    if (wave != 0) return;
    // ---- y[m] and its first maximum: lane l holds lags l, l + 64 and l + 128 ----
    double y[3];
    unsigned long long hit[3];
#pragma unroll
    for (int h = 0; h < 3; ++h) {
        const int m = lane + 64 * h;
        y[h] = -1.0;
        if (m < NL) {
            y[h] = 0.0;
            for (int k = 0; k < PX_K; ++k) y[h] += cs[m][k].x * cs[m][k].x + cs[m][k].y * cs[m][k].y;
        }
    }
    const double ymax = px_wave_max(fmax(fmax(y[0], y[1]), y[2]));
#pragma unroll
    for (int h = 0; h < 3; ++h) hit[h] = __ballot(lane + 64 * h < NL && y[h] == ymax);
    const int ms = hit[0] ? __ffsll((long long)hit[0]) - 1 : hit[1] ? 63 + __ffsll((long long)hit[1]) : hit[2] ? 127 + __ffsll((long long)hit[2]) : 0;
    const bool inner = ms > 0 && ms < NL - 1;                      // (y NaN everywhere: lag index 0, an edge)
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
        out[PX_POS] = (double)p;
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

// par = {win_len, sample_rate, min_coherence, max_gap}: columns 16..19 of the row, as given
struct RowPar { double win_len, fs, min_coh, max_gap; };

__global__ void __launch_bounds__(64) k_row_finish(RowIn in, int W, int Ls, int M, RowPar par, const double* __restrict__ part,
                                                   double* __restrict__ out) {
    __shared__ double up[GSMCAL_MAX_ROW_WINDOWS], uph[GSMCAL_MAX_ROW_WINDOWS];   // the used windows in list order: start and phase
    const int q = blockIdx.x, lane = threadIdx.x, j1 = lane + 64;
    const int lag0 = (int)in.pairs[3 * q + 2];
    const double* ps = part + (size_t)q * W * PX_PART;
    double* o = out + (size_t)q * GSMCAL_ROW_COLS;
    const PxBurst u0 = px_burst(ps + (size_t)(lane < W ? lane : 0) * PX_PART, lane < W, lag0, M, par.fs, Ls, par.min_coh);
    const PxBurst u1 = px_burst(ps + (size_t)(j1 < W ? j1 : 0) * PX_PART, j1 < W, lag0, M, par.fs, Ls, par.min_coh);
    const unsigned long long e0 = __ballot(u0.ev), e1 = __ballot(u1.ev), k0 = __ballot(u0.used), k1 = __ballot(u1.used);
    const int num_eval = __popcll(e0) + __popcll(e1), n = __popcll(k0) + __popcll(k1);
    // ---- the per-window columns (a window at or beyond W is not `mine`: NaN everywhere) ----
    o[GSMCAL_R_START + lane] = u0.pos;
    o[GSMCAL_R_DELAY + lane] = u0.delay;
    o[GSMCAL_R_PHASE + lane] = u0.phase;
    o[GSMCAL_R_FREQ + lane] = u0.freq;
    o[GSMCAL_R_COH + lane] = u0.coh;
    o[GSMCAL_R_EDGE + lane] = u0.ev ? (u0.edge ? 1.0 : 0.0) : NAN_D;
    o[GSMCAL_R_START + j1] = u1.pos;
    o[GSMCAL_R_DELAY + j1] = u1.delay;
    o[GSMCAL_R_PHASE + j1] = u1.phase;
    o[GSMCAL_R_FREQ + j1] = u1.freq;
    o[GSMCAL_R_COH + j1] = u1.coh;
    o[GSMCAL_R_EDGE + j1] = u1.ev ? (u1.edge ? 1.0 : 0.0) : NAN_D;
    const int status = n < 2 ? GSMCAL_S_PAIR_FEW : 0;
    PxSummary s;
    if (status == 0) s = px_summaries(u0, u1, k0, k1, par.max_gap, par.fs, lane, up, uph);      // (uniform)
    if (lane == 0) {
        o[GSMCAL_R_STATUS] = (double)status;
        o[GSMCAL_R_NUM_WINDOWS] = (double)W;
        o[GSMCAL_R_NUM_EVAL] = (double)num_eval;
        o[GSMCAL_R_NUM_USED] = (double)n;
        o[GSMCAL_R_NUM_ADJACENT] = (double)s.nadj;
        o[GSMCAL_R_LAG0] = (double)lag0;
        o[GSMCAL_R_DELAY0] = s.delay0;
        o[GSMCAL_R_REL_SAMPLING_PPM] = s.ppm;
        o[GSMCAL_R_DELAY_RMS] = s.drms;
        o[GSMCAL_R_REL_CARRIER_HZ] = s.rel;
        o[GSMCAL_R_WINDOW_CARRIER_HZ] = s.fc;
        o[GSMCAL_R_PHASE0] = s.phase0;
        o[GSMCAL_R_PHASE_RMS] = s.prms;
        o[GSMCAL_R_MEAN_COHERENCE] = s.cmean;
        o[GSMCAL_R_MIN_COHERENCE_SEEN] = s.cmin;
        o[GSMCAL_R_MAX_LAG] = (double)M;
        o[GSMCAL_R_WIN_LEN] = par.win_len;
        o[GSMCAL_R_SAMPLE_RATE] = par.fs;
        o[GSMCAL_R_MIN_COHERENCE] = par.min_coh;
        o[GSMCAL_R_MAX_GAP] = par.max_gap;
    }
}
