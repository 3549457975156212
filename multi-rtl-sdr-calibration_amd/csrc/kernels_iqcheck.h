// kernels_iqcheck.h -- the I/Q imbalance and clipping check (the reference's TODO item 4.5; the project's own function).
// Per capture of N samples with I bytes a_n and Q bytes b_n (raw2iq.m:6) the five sums S_I, S_Q, S_II, S_QQ, S_IQ, the minimum,
// maximum and count of bytes at 0 / 255 per rail, and from them DC, variance, gain ratio, quadrature skew, image rejection and level:
//
//   k_iq_moments<RAW>   one tile of IQ_TILE samples per workgroup -> one IqPart per (capture, tile)
//   k_iq_finish<RAW>    a capture's partials added by one wave -> the whole row of IQ_COLS doubles (nothing else writes it)
//   k_iq_correct        out_Q = (Q/g - I*s)/c on complex streams, element-wise and in place
//
// RAW = true: integers only.  A 16-byte load holds eight samples; with the I and Q bytes of a dword masked into two words the five
// sums are 4x8-bit dot products accumulated in 32 bits per lane (a lane sees 64 samples of a tile, a tile's sum of squares stays
// below 2^31), flushed into 64-bit partials per tile.  Integer sums are exact in any order, so a row depends on the bytes alone.
// A capture's row starts at byte 2*n*i, 2-byte aligned only: the samples in front of the first 16-byte boundary of a tile and behind
// its last go through a scalar path.  The bytes are read once: non-temporal loads.
// RAW = false: the same sums in fp64 over a complex array (gsmcal_IQ_imbalance), every lane its samples in ascending order, the wave's
// lanes by the DPP tree, the four waves in order, then the tiles likewise (k_iq_finish): one fixed reduction order that depends on len
// only, no atomics.
#pragma once
#include "kernels_spectrum.h"

#define IQ_TILE 16384                    // samples per workgroup == GSMCAL_IQ_TILE: 32 KB of bytes, eight 16-byte loads per lane
#define IQ_COLS 22                       // == GSMCAL_IQ_COLS
#define IQ_ST_OK 0
#define IQ_ST_SHORT 1                    // N < 2: no variance exists
#define IQ_ST_FLAT 2                     // a rail is constant: A_I == 0 or A_Q == 0
#define IQ_N_MAX (1L << 23)              // N*S_II - S_I^2 stays below 2^62

template <bool RAW> struct IqPart;
template <> struct IqPart<true> { unsigned long long s[5]; unsigned mn_i, mx_i, mn_q, mx_q, clip_i, clip_q; };   // s: S_I, S_Q, S_II, S_QQ, S_IQ of the tile
template <> struct IqPart<false> { double s[5]; double mn_i, mx_i, mn_q, mx_q; };

typedef unsigned short iq_u16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned iq_pk_min(unsigned a, unsigned b) {      // two 16-bit lanes at once (v_pk_min_u16)
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(iq_u16x2_t, a), __builtin_bit_cast(iq_u16x2_t, b)));
}
__device__ __forceinline__ unsigned iq_pk_max(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(iq_u16x2_t, a), __builtin_bit_cast(iq_u16x2_t, b)));
}
__device__ __forceinline__ unsigned iq_pk_add(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_bit_cast(iq_u16x2_t, a) + __builtin_bit_cast(iq_u16x2_t, b));
}
// per 16-bit lane holding a byte value: 1 where it is 0 or 255, else 0  ((x + 1) & 0xFE is 0 exactly there)
__device__ __forceinline__ unsigned iq_pk_clipped(unsigned x) {
    return 0x00010001u - iq_pk_min(iq_pk_add(x, 0x00010001u) & 0x00FE00FEu, 0x00010001u);
}
__device__ __forceinline__ unsigned iq_wave_min_u32(unsigned v) {
    for (int off = 32; off > 0; off >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, off, 64));
    return v;
}

// The integer accumulators of one lane.  mn / mx hold two 16-bit lanes (the samples of a dword side by side).
struct IqAcc {
    unsigned si, sq, sii, sqq, siq, mn_i, mx_i, mn_q, mx_q;
    __device__ __forceinline__ void dword(unsigned w) {        // two samples: bytes I0 Q0 I1 Q1
        const unsigned wi = w & 0x00FF00FFu, sh = w >> 8, wq = sh & 0x00FF00FFu;
        si = __builtin_amdgcn_udot4(w, 0x00010001u, si, false);
        sq = __builtin_amdgcn_udot4(w, 0x01000100u, sq, false);
        sii = __builtin_amdgcn_udot4(wi, w, sii, false);       // wi is zero where w holds Q
        sqq = __builtin_amdgcn_udot4(wq, sh, sqq, false);      // wq is zero where sh holds I
        siq = __builtin_amdgcn_udot4(wi, sh, siq, false);
        mn_i = iq_pk_min(mn_i, wi); mx_i = iq_pk_max(mx_i, wi);
        mn_q = iq_pk_min(mn_q, wq); mx_q = iq_pk_max(mx_q, wq);
    }
    __device__ __forceinline__ void chunk(const uint4 v) { dword(v.x); dword(v.y); dword(v.z); dword(v.w); }
    __device__ __forceinline__ void sample(unsigned v) {       // the scalar path: one sample, I | Q << 8
        const unsigned x = v & 0xFFu, y = v >> 8;
        si += x; sq += y; sii += x * x; sqq += y * y; siq += x * y;
        mn_i = iq_pk_min(mn_i, x * 0x00010001u); mx_i = iq_pk_max(mx_i, x * 0x00010001u);
        mn_q = iq_pk_min(mn_q, y * 0x00010001u); mx_q = iq_pk_max(mx_q, y * 0x00010001u);
    }
};

#define IQ_PER_LANE (IQ_TILE / 8 / 256)  // 16-byte loads per lane of a tile
static_assert(IQ_PER_LANE * 8 * 256 == IQ_TILE && (long)IQ_TILE * 255 * 255 < (1L << 31), "a tile's sums must fit 32 bits");

// grid (nblk, S), block 256.  part[s*nblk + blk].  RAW: raw + s*stream_bytes, 2-byte aligned; !RAW: arr + s*arr_stride.
template <bool RAW>
__global__ void __launch_bounds__(256) k_iq_moments(const uint8_t* __restrict__ raw, long stream_bytes, const cplx* __restrict__ arr,
                                                   long arr_stride, long n, IqPart<RAW>* __restrict__ part) {
    const int s = blockIdx.y, t = threadIdx.x;
    const long lo = (long)blockIdx.x * IQ_TILE;
    const long hi = n - lo > IQ_TILE ? lo + IQ_TILE : n;       // samples [lo, hi) of the capture
    if constexpr (RAW) {
        __shared__ unsigned w_s[4][11];
        const unsigned short* base = (const unsigned short*)(raw + (size_t)s * stream_bytes);
        const long ao = (long)(((uintptr_t)base >> 1) & 7);
        long a = lo + ((8 - ((ao + lo) & 7)) & 7);             // the first sample of the tile on a 16-byte boundary
        if (a > hi) a = hi;
        const int nv = (int)((hi - a) >> 3);                   // whole 16-byte chunks [a, a + 8 nv); nv <= IQ_TILE / 8
        const long b = a + 8L * nv;
        const int head = (int)(a - lo), edge = head + (int)(hi - b);   // scalar samples: fewer than 8 at either end
        IqAcc acc;
        acc.si = acc.sq = acc.sii = acc.sqq = acc.siq = 0u;
        acc.mn_i = acc.mn_q = 0x00FF00FFu; acc.mx_i = acc.mx_q = 0u;
        uint4 v[IQ_PER_LANE];
        const uint4* p = (const uint4*)(base + a) + t;
#pragma unroll
        for (int u = 0; u < IQ_PER_LANE; ++u) v[u] = t + 256 * u < nv ? ld_stream16(p + 256 * u) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int u = 0; u < IQ_PER_LANE; ++u)
            if (t + 256 * u < nv) acc.chunk(v[u]);
        unsigned e = 0u;
        if (t < edge) {
            e = base[t < head ? lo + t : b + (t - head)];
            acc.sample(e);
        }
        // Bytes at a rail are rare in a healthy capture and show in the minimum / maximum: they are counted (from the registers, no
        // second load) only by the waves that saw one
        unsigned ci = 0u, cq = 0u;
        const bool rail = ((acc.mn_i & 0xFFFFu) == 0u) | ((acc.mn_i >> 16) == 0u) | ((acc.mx_i & 0xFFFFu) == 255u) | ((acc.mx_i >> 16) == 255u) |
                          ((acc.mn_q & 0xFFFFu) == 0u) | ((acc.mn_q >> 16) == 0u) | ((acc.mx_q & 0xFFFFu) == 255u) | ((acc.mx_q >> 16) == 255u);
        if (__any(rail)) {                                     // (wave-uniform)
            unsigned pi = 0u, pq = 0u;                         // at most 32 per 16-bit lane
#pragma unroll
            for (int u = 0; u < IQ_PER_LANE; ++u)
                if (t + 256 * u < nv) {
                    const unsigned w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        pi = iq_pk_add(pi, iq_pk_clipped(w[i] & 0x00FF00FFu));
                        pq = iq_pk_add(pq, iq_pk_clipped((w[i] >> 8) & 0x00FF00FFu));
                    }
                }
            ci = (pi & 0xFFFFu) + (pi >> 16);
            cq = (pq & 0xFFFFu) + (pq >> 16);
            if (t < edge) {
                const unsigned x = e & 0xFFu, y = e >> 8;
                ci += (x == 0u || x == 255u) ? 1u : 0u;
                cq += (y == 0u || y == 255u) ? 1u : 0u;
            }
        }
        // the tile's totals: the wave's lanes, then the four waves (integers: any order).  255 - max is reduced as a minimum.
        const unsigned red[7] = {wave_sum_u32(acc.si), wave_sum_u32(acc.sq), wave_sum_u32(acc.sii), wave_sum_u32(acc.sqq),
                                 wave_sum_u32(acc.siq), wave_sum_u32(ci), wave_sum_u32(cq)};
        const unsigned m0 = iq_wave_min_u32(min(acc.mn_i & 0xFFFFu, acc.mn_i >> 16));
        const unsigned m1 = iq_wave_min_u32(255u - max(acc.mx_i & 0xFFFFu, acc.mx_i >> 16));
        const unsigned m2 = iq_wave_min_u32(min(acc.mn_q & 0xFFFFu, acc.mn_q >> 16));
        const unsigned m3 = iq_wave_min_u32(255u - max(acc.mx_q & 0xFFFFu, acc.mx_q >> 16));
        if ((t & 63) == 0) {
            unsigned* w = w_s[t >> 6];
#pragma unroll
            for (int i = 0; i < 7; ++i) w[i] = red[i];
            w[7] = m0; w[8] = m1; w[9] = m2; w[10] = m3;
        }
        __syncthreads();
        if (t == 0) {
            IqPart<true> o;
#pragma unroll
            for (int i = 0; i < 5; ++i) o.s[i] = (unsigned long long)w_s[0][i] + w_s[1][i] + w_s[2][i] + w_s[3][i];
            o.clip_i = w_s[0][5] + w_s[1][5] + w_s[2][5] + w_s[3][5];
            o.clip_q = w_s[0][6] + w_s[1][6] + w_s[2][6] + w_s[3][6];
            o.mn_i = min(min(w_s[0][7], w_s[1][7]), min(w_s[2][7], w_s[3][7]));
            o.mx_i = 255u - min(min(w_s[0][8], w_s[1][8]), min(w_s[2][8], w_s[3][8]));
            o.mn_q = min(min(w_s[0][9], w_s[1][9]), min(w_s[2][9], w_s[3][9]));
            o.mx_q = 255u - min(min(w_s[0][10], w_s[1][10]), min(w_s[2][10], w_s[3][10]));
            part[(size_t)s * gridDim.x + blockIdx.x] = o;
        }
    } else {
        __shared__ double w_s[4][9];
        const cplx* x = arr + (size_t)s * arr_stride;
        const double inf = __longlong_as_double(0x7FF0000000000000LL);
        double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, mn_i = inf, mx_i = -inf, mn_q = inf, mx_q = -inf;
#pragma unroll 4
        for (long g = lo + t; g < hi; g += 256) {
            const cplx z = x[g];
            a[0] += z.x; a[1] += z.y;
            a[2] = fma(z.x, z.x, a[2]); a[3] = fma(z.y, z.y, a[3]); a[4] = fma(z.x, z.y, a[4]);
            mn_i = fmin(mn_i, z.x); mx_i = fmax(mx_i, z.x);
            mn_q = fmin(mn_q, z.y); mx_q = fmax(mx_q, z.y);
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) a[i] = wave_sum(a[i]);
        for (int off = 32; off > 0; off >>= 1) {               // selections: the same whatever the order
            mn_i = fmin(mn_i, __shfl_xor(mn_i, off, 64)); mx_i = fmax(mx_i, __shfl_xor(mx_i, off, 64));
            mn_q = fmin(mn_q, __shfl_xor(mn_q, off, 64)); mx_q = fmax(mx_q, __shfl_xor(mx_q, off, 64));
        }
        if ((t & 63) == 0) {
            double* w = w_s[t >> 6];
#pragma unroll
            for (int i = 0; i < 5; ++i) w[i] = a[i];
            w[5] = mn_i; w[6] = mx_i; w[7] = mn_q; w[8] = mx_q;
        }
        __syncthreads();
        if (t == 0) {
            IqPart<false> o;
#pragma unroll
            for (int i = 0; i < 5; ++i) o.s[i] = ((w_s[0][i] + w_s[1][i]) + w_s[2][i]) + w_s[3][i];
            o.mn_i = fmin(fmin(w_s[0][5], w_s[1][5]), fmin(w_s[2][5], w_s[3][5]));
            o.mx_i = fmax(fmax(w_s[0][6], w_s[1][6]), fmax(w_s[2][6], w_s[3][6]));
            o.mn_q = fmin(fmin(w_s[0][7], w_s[1][7]), fmin(w_s[2][7], w_s[3][7]));
            o.mx_q = fmax(fmax(w_s[0][8], w_s[1][8]), fmax(w_s[2][8], w_s[3][8]));
            part[(size_t)s * gridDim.x + blockIdx.x] = o;
        }
    }
}

// Columns 12.. of a row from N and A_I = N S_II - S_I^2, A_Q = N S_QQ - S_Q^2, C = N S_IQ - S_I S_Q (each already a double, converted
// once), columns 0..11 being the caller's.  Every operation rounded on its own, in the order include/gsmcal.h states.
__device__ __forceinline__ void iq_derive(double* row, long n, double s_i, double s_q, double a_i, double a_q, double cc) {
#pragma clang fp contract(off)
    const double N = (double)n;
    const int status = n < 2 ? IQ_ST_SHORT : (!(a_i > 0.0) || !(a_q > 0.0)) ? IQ_ST_FLAT : IQ_ST_OK;
    row[12] = s_i / N;
    row[13] = s_q / N;
    for (int i = 14; i <= 20; ++i) row[i] = NAN_D;
    row[21] = (double)status;
    if (status == IQ_ST_SHORT) return;
    const double nn = N * N;
    const double var_i = a_i / nn, var_q = a_q / nn;
    row[14] = var_i;
    row[15] = var_q;
    row[20] = 10.0 * log10((var_i + var_q) / 32512.5);         // 2 * 127.5^2: full scale of both rails
    if (status == IQ_ST_FLAT) return;
    const double gain = sqrt(a_q / a_i);
    double sn = cc / (sqrt(a_i) * sqrt(a_q));
    sn = sn > 1.0 ? 1.0 : sn < -1.0 ? -1.0 : sn;
    const double cs = sqrt(1.0 - sn * sn);
    const double k = 2.0 * gain * sn * sn / (1.0 + cs);
    const double num = (gain + 1.0) * (gain + 1.0) - k, den = (gain - 1.0) * (gain - 1.0) + k;
    row[16] = gain;
    row[17] = sn;
    row[18] = asin(sn) * 180.0 / 3.141592653589793;
    row[19] = den == 0.0 ? __longlong_as_double(0x7FF0000000000000LL) : 10.0 * log10(num / den);
}

// One wave per capture (a lane per capture adding its tiles one after the other was 25 us of load latency at 63 tiles): lane l takes
// the partials l, l + 64, ... in ascending order, the wave's lanes are combined (integers: any order; fp64: the DPP tree), lane 0
// writes table[s][IQ_COLS].  The order depends on the tile count only.  grid ceil(S/4), block 256.
template <bool RAW>
__global__ void __launch_bounds__(256) k_iq_finish(const IqPart<RAW>* __restrict__ part, int nblk, int S, long n, double* __restrict__ table) {
#pragma clang fp contract(off)
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= S) return;                                        // (wave-uniform)
    const IqPart<RAW>* p = part + (size_t)s * nblk;
    double* row = table + (size_t)s * IQ_COLS;
    if constexpr (RAW) {
        unsigned long long u[7] = {0, 0, 0, 0, 0, 0, 0};       // the five sums, clip_I, clip_Q
        unsigned mn_i = 255u, nx_i = 255u, mn_q = 255u, nx_q = 255u;   // nx: 255 - max, reduced as a minimum
        for (int b = lane; b < nblk; b += 64) {
            const IqPart<true> o = p[b];
            for (int i = 0; i < 5; ++i) u[i] += o.s[i];
            u[5] += o.clip_i; u[6] += o.clip_q;
            mn_i = min(mn_i, o.mn_i); nx_i = min(nx_i, 255u - o.mx_i);
            mn_q = min(mn_q, o.mn_q); nx_q = min(nx_q, 255u - o.mx_q);
        }
        for (int off = 32; off > 0; off >>= 1)
            for (int i = 0; i < 7; ++i) u[i] += __shfl_xor(u[i], off, 64);
        mn_i = iq_wave_min_u32(mn_i); nx_i = iq_wave_min_u32(nx_i);
        mn_q = iq_wave_min_u32(mn_q); nx_q = iq_wave_min_u32(nx_q);
        if (lane != 0) return;
        row[0] = (double)n;
        for (int i = 0; i < 5; ++i) row[1 + i] = (double)u[i];
        row[6] = (double)mn_i; row[7] = (double)(255u - nx_i); row[8] = (double)mn_q; row[9] = (double)(255u - nx_q);
        row[10] = (double)u[5]; row[11] = (double)u[6];
        const long long N = n, si = (long long)u[0], sq = (long long)u[1];      // N <= 2^23: each of the three stays below 2^62
        const long long a_i = N * (long long)u[2] - si * si, a_q = N * (long long)u[3] - sq * sq, cc = N * (long long)u[4] - si * sq;
        iq_derive(row, n, (double)u[0], (double)u[1], (double)a_i, (double)a_q, (double)cc);
    } else {
        double f[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        const double inf = __longlong_as_double(0x7FF0000000000000LL);
        double mn_i = inf, mx_i = -inf, mn_q = inf, mx_q = -inf;
        for (int b = lane; b < nblk; b += 64) {
            const IqPart<false> o = p[b];
            for (int i = 0; i < 5; ++i) f[i] += o.s[i];
            mn_i = fmin(mn_i, o.mn_i); mx_i = fmax(mx_i, o.mx_i);
            mn_q = fmin(mn_q, o.mn_q); mx_q = fmax(mx_q, o.mx_q);
        }
        for (int i = 0; i < 5; ++i) f[i] = wave_sum(f[i]);
        for (int off = 32; off > 0; off >>= 1) {
            mn_i = fmin(mn_i, __shfl_xor(mn_i, off, 64)); mx_i = fmax(mx_i, __shfl_xor(mx_i, off, 64));
            mn_q = fmin(mn_q, __shfl_xor(mn_q, off, 64)); mx_q = fmax(mx_q, __shfl_xor(mx_q, off, 64));
        }
        if (lane != 0) return;
        row[0] = (double)n;
        for (int i = 0; i < 5; ++i) row[1 + i] = f[i];
        row[6] = mn_i; row[7] = mx_i; row[8] = mn_q; row[9] = mx_q;
        row[10] = NAN_D; row[11] = NAN_D;
        const double N = (double)n;                            // (a DC far above the signal cancels here: include/gsmcal.h)
        iq_derive(row, n, f[0], f[1], N * f[2] - f[0] * f[0], N * f[3] - f[1] * f[1], N * f[4] - f[0] * f[1]);
    }
}

// out_I = I, out_Q = (Q/g - I*s)/c with c = sqrt(1 - s*s), in place.  par[s] = {g, s} per stream.  grid (ceil(len/1024), S), block 256.
__global__ void __launch_bounds__(256) k_iq_correct(cplx* __restrict__ x, long len, const double* __restrict__ par) {
#pragma clang fp contract(off)
    const int s = blockIdx.y;
    const double g = par[2 * s], sn = par[2 * s + 1];
    const double cs = sqrt(1.0 - sn * sn);
    cplx* p = x + (size_t)s * len;
    const long j0 = (long)blockIdx.x * 1024 + threadIdx.x;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long j = j0 + 256 * u;
        if (j < len) {
            cplx v = p[j];
            v.y = (v.y / g - v.x * sn) / cs;
            p[j] = v;
        }
    }
}
