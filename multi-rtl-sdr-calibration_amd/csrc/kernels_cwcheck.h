// kernels_cwcheck.h -- the CW sample-loss check of CW_check.m:6-8 (check_CW_samples_loss_tcp.m:70,89-90) on raw captures:
//
//   s = raw2iq(bytes);  q_n = s(n+1)./s(n), n = 1..N-1;  phase_rotate = angle(mean(q));  r_n = angle(q_n) - phase_rotate
//
// r is NOT wrapped (the reference does not wrap it): values lie in (-2pi, 2pi).  A lost run of k samples is one spike of
// k*phase_rotate mod 2pi.  Two passes over the bytes, nothing in between goes through memory but one complex partial per block:
//
//   k_band_power_clear, k_dc_sum   (kernels_spectrum.h, kernels_frontend.h) exact integer I/Q byte sums per capture
//   k_cw_ratio_sum<RAW>            the ratios of a tile, summed per lane, then over the block in a fixed order; one partial per block
//   k_cw_finish_mean               a capture's partials added in block order -> phase_rotate and the status
//   k_cw_residual<RAW, NT>         the same tile, q recomputed from the bytes: r_n (when a buffer is given), and per block the count
//                                  of |r_n| > thr, the block maximum of |r| and the first ratio at which it occurs
//   k_cw_finish_summary<RAW>       one workgroup per capture: the block records in order -> the summary row; for the event list
//                                  only the first blocks that reported exceeds are evaluated again
//
// RAW = true: samples are formed from the bytes exactly as k_raw2iq forms them, (double)byte - (double)sum/N (one divide, one
// subtract).  RAW = false: samples are read from a complex array (gsmcal_CW_check) -- the load stage differs, nothing else.
// Every ratio goes through cw_ratio(): contraction off, so a ratio and its angle have the same bits in every kernel and instance.
// No atomics, and nothing depends on which block finishes first.  The tiling depends on N only: a capture's outputs are
// bit-identical at any position in a batch of any size, with or without the residual buffer.
#pragma once
#include "kernels_spectrum.h"

#define CW_PER_LANE 8
#define CW_TILE (256 * CW_PER_LANE)      // ratios per block == GSMCAL_CW_TILE
#define CW_MAX_EVENTS 16                 // == GSMCAL_CW_MAX_EVENTS
#define CW_COLS (5 + 2 * CW_MAX_EVENTS)  // == GSMCAL_CW_COLS
#define CW_ST_OK 0
#define CW_ST_SHORT 1                    // N < 2: no ratio exists
#define CW_ST_ZERO 2                     // a denominator s(n) is exactly 0+0i

struct CwPart { double re, im, zero, pad; };                 // block sum of the ratios; zero != 0: a denominator was 0+0i
struct CwRec { double maxabs; long first; long exceed; long pad; };   // block maximum of |r|, first ratio (0-based, in the capture) at which it occurs, count of |r| > thr
struct CwMean { double phase_rotate; long status; };

__device__ __forceinline__ double cw_nan() { return __longlong_as_double(0x7FF8000000000000LL); }

// q = a ./ b in MATLAB's scaled form (Smith's algorithm: dm_cdiv of kernels_demod.h), every product and sum rounded on its own.
// dm_cdiv's two branches are one formula with the components swapped -- |b.x| >= |b.y|: p = b.x, o = b.y,
//   q = ((a.x + a.y*r)/d, (a.y - a.x*r)/d);   else p = b.y, o = b.x:  q = ((a.y + a.x*r)/d, (a.y*r - a.x)/d),   r = o/p, d = p + o*r
// -- so the operands are selected and the three divisions run once (lanes of a wave take either side: as two branches every
// wave would run six).  Sums commute: the same bits as the branching form, the sign of a zero included.
__device__ __forceinline__ cplx cw_ratio(cplx a, cplx b) {
#pragma clang fp contract(off)
    const bool x_big = fabs(b.x) >= fabs(b.y);
    const double p = x_big ? b.x : b.y, o = x_big ? b.y : b.x;
    const double u = x_big ? a.x : a.y, v = x_big ? a.y : a.x;
    const double r = o / p;
    const double orr = o * r, vr = v * r, ur = u * r;
    const double d = p + orr;
    const double m1 = x_big ? v : ur, m2 = x_big ? ur : v;
    return make_double2((u + vr) / d, (m1 - m2) / d);
}

// r_n = angle(q_n) - phase_rotate, the difference rounded on its own whatever the last operation of atan2 is
__device__ __forceinline__ double cw_resid(cplx q, double phase_rotate) {
#pragma clang fp contract(off)
    const double a = atan2(q.y, q.x);
    return a - phase_rotate;
}

// Stage samples [first, first+span) of one capture into LDS with 16-byte loads (stage_raw's layout: sample g at r_s[g - first_al],
// zeros outside [0, n)).  NT: the bytes are not read again by a later launch -- non-temporal loads.
template <bool NT>
__device__ __forceinline__ long cw_stage(unsigned short* r_s, const unsigned short* base, long n, long first, int span, int tid) {
    const long ao = (long)(((uintptr_t)base >> 1) & 7);
    const long first_al = first - ((first + ao) & 7);            // first >= 0: the address of sample first_al is 16-byte aligned
    const int nchunk = (int)((first + span - first_al + 7) >> 3);
    for (int c = tid; c < nchunk; c += 256) {
        const long g0 = first_al + 8L * c;
        uint4 v;
        if (g0 >= 0 && g0 + 8 <= n) v = NT ? ld_stream16((const uint4*)(base + g0)) : *(const uint4*)(base + g0);
        else v = ffast_chunk(base, g0, n);
        *(uint4*)(r_s + 8 * c) = v;
    }
    return first_al;
}

// The samples of a capture as the ratio kernels see them.  RAW: LDS copy of the tile's bytes + the capture's exact mean.
template <bool RAW>
struct CwSrc {
    const unsigned short* r_s; long first_al; double mr, mi;   // RAW
    const cplx* arr;                                           // !RAW
    __device__ __forceinline__ cplx at(long g) const {
        if (RAW) {
            const unsigned v = r_s[g - first_al];
            return make_double2((double)(v & 0xFFu) - mr, (double)(v >> 8) - mi);
        }
        return arr[g];
    }
};
#define CW_LDS_SAMPLES (CW_TILE + 1 + 8 + 16)    // tile + halo, up to 7 samples of alignment in front, stage_raw's slack

// Source of block `blk` of capture s: stages the tile's bytes + ONE halo sample (the first sample of the next tile).
template <bool RAW, bool NT>
__device__ __forceinline__ CwSrc<RAW> cw_open(unsigned short* r_s, const uint8_t* raw, long stream_bytes, const StreamState* st,
                                             const cplx* arr, long arr_stride, long n, int s, long blk, int cnt, int t) {
    CwSrc<RAW> src;
    src.r_s = r_s; src.first_al = 0; src.mr = 0.0; src.mi = 0.0; src.arr = nullptr;
    if (RAW) {
        const unsigned short* base = (const unsigned short*)(raw + (size_t)s * stream_bytes);
        src.first_al = cw_stage<NT>(r_s, base, n, blk * CW_TILE, cnt + 1, t);
        src.mr = (double)st[s].sum_i / (double)n;              // k_finish_mean's mean
        src.mi = (double)st[s].sum_q / (double)n;
    } else {
        src.arr = arr + (size_t)s * arr_stride;
    }
    return src;
}

// ratios of block blk: [blk*CW_TILE, blk*CW_TILE + cnt), lane t takes t, t+256, ... in ascending order
__device__ __forceinline__ int cw_count(long n, long blk) {
    const long left = (n - 1) - blk * CW_TILE;
    return (int)(left > CW_TILE ? CW_TILE : left);
}

// grid (nblk, S), block 256.  part[s*nblk + blk].
template <bool RAW>
__global__ void __launch_bounds__(256) k_cw_ratio_sum(const uint8_t* __restrict__ raw, long stream_bytes, const StreamState* __restrict__ st,
                                                     const cplx* __restrict__ arr, long arr_stride, long n, CwPart* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) unsigned short r_s[RAW ? CW_LDS_SAMPLES : 8];
    __shared__ double w_s[4][3];
    const int s = blockIdx.y, t = threadIdx.x;
    const long blk = blockIdx.x;
    const int cnt = cw_count(n, blk);
    const CwSrc<RAW> src = cw_open<RAW, false>(r_s, raw, stream_bytes, st, arr, arr_stride, n, s, blk, cnt, t);
    if (RAW) __syncthreads();
    double sr = 0.0, si = 0.0, zero = 0.0;
#pragma unroll 2
    for (int j = t; j < cnt; j += 256) {
        const long g = blk * CW_TILE + j;
        const cplx b = src.at(g), a = src.at(g + 1);
        if (b.x == 0.0 && b.y == 0.0) zero = 1.0;
        const cplx q = cw_ratio(a, b);
        sr += q.x;
        si += q.y;
    }
    // block sums in a fixed order: the wave's lanes (DPP tree), then the four waves in order
    const double wr = wave_sum(sr), wi = wave_sum(si), wz = wave_sum(zero);
    if ((t & 63) == 0) { w_s[t >> 6][0] = wr; w_s[t >> 6][1] = wi; w_s[t >> 6][2] = wz; }
    __syncthreads();
    if (t == 0) {
        CwPart p;
        p.re = ((w_s[0][0] + w_s[1][0]) + w_s[2][0]) + w_s[3][0];
        p.im = ((w_s[0][1] + w_s[1][1]) + w_s[2][1]) + w_s[3][1];
        p.zero = ((w_s[0][2] + w_s[1][2]) + w_s[2][2]) + w_s[3][2];
        p.pad = 0.0;
        part[(size_t)s * gridDim.x + blk] = p;
    }
}

// phase_rotate = angle(sum(q)/(N-1)), the partials added in block order.  grid ceil(S/64), block 64.
__global__ void k_cw_finish_mean(const CwPart* __restrict__ part, int nblk, int S, long n, CwMean* __restrict__ mean) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const CwPart* p = part + (size_t)s * nblk;
    double sr = 0.0, si = 0.0, zero = 0.0;
    for (int b = 0; b < nblk; ++b) { sr += p[b].re; si += p[b].im; zero += p[b].zero; }
    const double m = (double)(n - 1);
    CwMean o;
    o.status = zero != 0.0 ? CW_ST_ZERO : CW_ST_OK;
    o.phase_rotate = zero != 0.0 ? cw_nan() : atan2(si / m, sr / m);
    mean[s] = o;
}

// grid (nblk, S), block 256.  r == nullptr: summary only.  rec[s*nblk + blk].
template <bool RAW, bool NT>
__global__ void __launch_bounds__(256) k_cw_residual(const uint8_t* __restrict__ raw, long stream_bytes, const StreamState* __restrict__ st,
                                                    const cplx* __restrict__ arr, long arr_stride, long n, const CwMean* __restrict__ mean,
                                                    double thr, double* __restrict__ r, long r_stride, CwRec* __restrict__ rec) {
    __shared__ __attribute__((aligned(16))) unsigned short r_s[RAW ? CW_LDS_SAMPLES : 8];
    __shared__ double wm_s[4];
    __shared__ long wf_s[4];
    __shared__ unsigned wc_s[4];
    const int s = blockIdx.y, t = threadIdx.x;
    const long blk = blockIdx.x;
    const int cnt = cw_count(n, blk);
    double* out = r ? r + (size_t)s * r_stride + blk * CW_TILE : nullptr;
    if (mean[s].status != CW_ST_OK) {                          // (block-uniform) a zero denominator: every r_n of the capture is NaN
        if (out)
            for (int j = t; j < cnt; j += 256) __builtin_nontemporal_store(cw_nan(), out + j);
        if (t == 0) { CwRec o; o.maxabs = 0.0; o.first = 0; o.exceed = 0; o.pad = 0; rec[(size_t)s * gridDim.x + blk] = o; }
        return;
    }
    const CwSrc<RAW> src = cw_open<RAW, NT>(r_s, raw, stream_bytes, st, arr, arr_stride, n, s, blk, cnt, t);
    if (RAW) __syncthreads();
    const double pr = mean[s].phase_rotate;
    double mx = -1.0;
    long first = 0;
    unsigned exceed = 0;
#pragma unroll 2
    for (int j = t; j < cnt; j += 256) {
        const long g = blk * CW_TILE + j;
        const cplx q = cw_ratio(src.at(g + 1), src.at(g));
        const double v = cw_resid(q, pr);
        if (out) __builtin_nontemporal_store(v, out + j);
        const double av = fabs(v);
        exceed += av > thr ? 1u : 0u;
        if (av > mx) { mx = av; first = g; }                   // ascending g per lane: the first of equal values stays
    }
    // the block's maximum and the first ratio at which it occurs: a selection, the same whatever the order
    for (int off = 32; off > 0; off >>= 1) {
        const double om = __shfl_xor(mx, off, 64);
        const long of = __shfl_xor(first, off, 64);
        if (om > mx || (om == mx && of < first)) { mx = om; first = of; }
    }
    const unsigned wc = wave_sum_u32(exceed);
    if ((t & 63) == 0) { wm_s[t >> 6] = mx; wf_s[t >> 6] = first; wc_s[t >> 6] = wc; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 4; ++w)
            if (wm_s[w] > mx || (wm_s[w] == mx && wf_s[w] < first)) { mx = wm_s[w]; first = wf_s[w]; }
        CwRec o;
        o.maxabs = mx; o.first = first; o.exceed = (long)wc_s[0] + wc_s[1] + wc_s[2] + wc_s[3]; o.pad = 0;
        rec[(size_t)s * gridDim.x + blk] = o;
    }
}

// One workgroup per capture: summary[s][CW_COLS] = {phase_rotate, count, max |r|, 1-based n of its first occurrence, status,
// CW_MAX_EVENTS pairs (1-based n, r_n) of the first exceeds in index order, NaN in unused slots}.  nblk == 0 (N < 2): status 1.
// grid S, block 256.
template <bool RAW>
__global__ void __launch_bounds__(256) k_cw_finish_summary(const uint8_t* __restrict__ raw, long stream_bytes, const StreamState* __restrict__ st,
                                                          const cplx* __restrict__ arr, long arr_stride, long n, const CwMean* __restrict__ mean,
                                                          const CwRec* __restrict__ rec, int nblk, double thr, double* __restrict__ summary) {
    __shared__ __attribute__((aligned(16))) unsigned short r_s[RAW ? CW_LDS_SAMPLES : 8];
    __shared__ double wm_s[4];
    __shared__ long wf_s[4], wc_s[4];
    __shared__ int we_s[4];
    const int s = blockIdx.x, t = threadIdx.x;
    double* row = summary + (size_t)s * CW_COLS;
    const long status = nblk == 0 ? CW_ST_SHORT : mean[s].status;
    if (status != CW_ST_OK) {                                  // (block-uniform)
        for (int i = 5 + t; i < CW_COLS; i += 256) row[i] = cw_nan();
        if (t == 0) { row[0] = cw_nan(); row[1] = 0.0; row[2] = cw_nan(); row[3] = cw_nan(); row[4] = (double)status; }
        return;
    }
    const CwRec* rc = rec + (size_t)s * nblk;
    double mx = -1.0;
    long first = 0, count = 0;
    for (int b = t; b < nblk; b += 256) {
        const CwRec o = rc[b];
        count += o.exceed;
        if (o.maxabs > mx) { mx = o.maxabs; first = o.first; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double om = __shfl_xor(mx, off, 64);
        const long of = __shfl_xor(first, off, 64);
        count += __shfl_xor(count, off, 64);
        if (om > mx || (om == mx && of < first)) { mx = om; first = of; }
    }
    if ((t & 63) == 0) { wm_s[t >> 6] = mx; wf_s[t >> 6] = first; wc_s[t >> 6] = count; }
    __syncthreads();
    for (int w = 0; w < 4; ++w)
        if (wm_s[w] > mx || (wm_s[w] == mx && wf_s[w] < first)) { mx = wm_s[w]; first = wf_s[w]; }
    count = wc_s[0] + wc_s[1] + wc_s[2] + wc_s[3];
    const double pr = mean[s].phase_rotate;
    if (t == 0) { row[0] = pr; row[1] = (double)count; row[2] = mx; row[3] = (double)(first + 1); row[4] = (double)CW_ST_OK; }
    // the event list: the blocks that reported exceeds, in order, evaluated again until the list is full
    int found = 0;
    for (int b = 0; b < nblk && found < CW_MAX_EVENTS && found < count; ++b) {
        if (rc[b].exceed == 0) continue;                       // (block-uniform)
        const int cnt = cw_count(n, b);
        __syncthreads();                                       // the previous block's LDS copy is no longer read
        const CwSrc<RAW> src = cw_open<RAW, false>(r_s, raw, stream_bytes, st, arr, arr_stride, n, s, b, cnt, t);
        if (RAW) __syncthreads();
        for (int j0 = 0; j0 < cnt && found < CW_MAX_EVENTS; j0 += 256) {
            const int j = j0 + t;
            double v = 0.0;
            bool ex = false;
            if (j < cnt) {
                const long g = (long)b * CW_TILE + j;
                const cplx q = cw_ratio(src.at(g + 1), src.at(g));
                v = cw_resid(q, pr);
                ex = fabs(v) > thr;
            }
            const unsigned long long m = __ballot(ex);
            if ((t & 63) == 0) we_s[t >> 6] = __popcll(m);
            __syncthreads();
            int pos = found + __popcll(m & ((1ull << (t & 63)) - 1ull));
            for (int w = 0; w < (t >> 6); ++w) pos += we_s[w];
            if (ex && pos < CW_MAX_EVENTS) {
                row[5 + 2 * pos] = (double)((long)b * CW_TILE + j + 1);
                row[5 + 2 * pos + 1] = v;
            }
            found += we_s[0] + we_s[1] + we_s[2] + we_s[3];
            __syncthreads();
        }
    }
    for (int i = (found < CW_MAX_EVENTS ? found : CW_MAX_EVENTS) + t; i < CW_MAX_EVENTS; i += 256) {   // the unused slots
        row[5 + 2 * i] = cw_nan();
        row[5 + 2 * i + 1] = cw_nan();
    }
}
