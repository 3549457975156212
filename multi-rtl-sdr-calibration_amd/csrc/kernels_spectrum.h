// kernels_spectrum.h -- band power of raw captures: the per-capture reduction of multi_rtl_sdr_split_scanner.m:154-156 /
// multi_rtl_sdr_diversity_scanner.m:156-158 / scan_band_power_spectrum.m:80-84
//
//   power = mean(abs(filter(coef,1,raw2iq(s))(1:decim:end)).^2)
//
//   k_dc_sum (kernels_frontend.h)  exact integer I/Q byte sums per capture (raw2iq.m:8)
//   k_band_power_clear             zeroes the sums
//   k_band_power<NT>               the FIR at the kept rows only, |y|^2 accumulated in fp64, one partial per block
//   k_band_power_finish            the partials of a capture summed in block order, divided once
//
// DC removal without rounding: with S the capture's byte sum and N its length, N*(c - mean) = N*c - S is an integer, so the
// kernel filters X = N*c - S (pairs of samples that share a tap: N*(a+b) - 2S, the bytes added as integers first) and the
// finishing step divides sum |N*y|^2 by N^2 * ceil(N/decim).  Every X is exact in fp64 (|X| < 2^53 for any N < 2^44), a
// constant capture gives X = 0 everywhere and therefore exactly 0, and no mean*sum(coef) is ever subtracted from a large
// number (k_front_fused's one-pass form would cancel catastrophically when the DC offset is large and the band power small).
// The decimated stream never reaches memory.  The block tiling depends on N, decim and the tap count only: a capture's
// result is bit-identical at any position in a batch of any size.
#pragma once
#include "kernels_frontend.h"

#define BP_MAX_TAPS 1024                 // generic path: any tap count from 1 to this
#define BP_ROWS 256                      // kept rows per block at least (fewer only when the raw span would not fit BP_LDS_BYTES)
#define BP_MAX_ROWS 4096                 // ... and at most: 16 per lane
#define BP_SPAN 4096                     // raw samples a block is sized to cover (decimation 1 or 5: 16 or 3 rows per lane)
#define BP_LDS_BYTES (60 * 1024)         // dynamic LDS of a block at most (raw span + coefficients; under the 64 KiB default)

// LDS bytes of a block of `rows` kept rows (coefficients of the generic path + raw span).  The span is not padded: lane t
// reads from sample t*decim on, and with immediate offsets per tap the u16 reads cost no address arithmetic (decim 20: a
// 2-way bank conflict between lanes 16 apart; odd decim: none).
__host__ __device__ inline size_t bp_lds_bytes(int rows, int decim, int ntaps, bool generic) {
    const size_t span = (size_t)(rows - 1) * decim + ntaps + 24;
    return (generic ? (size_t)((ntaps * 8 + 15) & ~15) : 0) + ((span * 2 + 15) & ~(size_t)15);
}

// NT > 0: exactly symmetric taps (coef[k] == coef[NT-1-k], checked on the host), compile-time count, coefficients through
// uniform (scalar) loads.  NT == 0: any taps (runtime ntaps <= BP_MAX_TAPS), oldest tap first, coefficients in LDS.
// grid (ceil(nd/rows), S), block 256; capture s = raw + s*stream_bytes, partial[s*gridDim.x + blockIdx.x].
template <int NT>
__global__ void __launch_bounds__(256) k_band_power(const uint8_t* __restrict__ raw, long stream_bytes,
                                                   const StreamState* __restrict__ st, const double* __restrict__ coef,
                                                   int ntaps, int decim, long nd, int rows, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nt = NT > 0 ? NT : ntaps;
    double* c_s = (double*)smem;                                                       // generic path only
    unsigned short* r_s = (unsigned short*)(smem + (NT > 0 ? 0 : ((nt * 8 + 15) & ~15)));
    const int s = blockIdx.y, t = threadIdx.x;
    const long n = stream_bytes >> 1;
    const unsigned short* base = (const unsigned short*)(raw + (size_t)s * stream_bytes);
    const long j0 = (long)blockIdx.x * rows;
    long jn = nd - j0;
    if (jn > rows) jn = rows;
    const long first = j0 * decim - (nt - 1);
    const int span = (int)((jn - 1) * decim + nt);
    if (NT == 0)
        for (int i = t; i < nt; i += 256) c_s[i] = coef[i];
    const long first_al = stage_raw<false>(r_s, base, n, first, span, t, 256);
    __syncthreads();
    // X = N*c - S per component (exact integers held in doubles)
    const double Nd = (double)n;
    const double Si = (double)st[s].sum_i, Sq = (double)st[s].sum_q;
    double acc = 0.0;                                      // sum over this lane's rows of |N*y|^2
    for (long r = t; r < jn; r += 256) {
        const long i_out = (j0 + r) * decim;
        const int o = (int)(i_out - (nt - 1) - first_al);  // LDS index of the oldest sample of this output
        double ar = 0.0, ai = 0.0;
        if (NT > 0 && i_out >= NT - 1) {
            // symmetric taps: the two samples sharing a tap added as integers, N*(a+b) - 2S exact, one FMA per pair
            const double Si2 = 2.0 * Si, Sq2 = 2.0 * Sq;
#pragma unroll 16
            for (int k = 0; k < NT / 2; ++k) {
                const unsigned a = r_s[o + k], b = r_s[o + NT - 1 - k];
                const double c = coef[k];
                ar = fma(c, fma((double)((a & 0xFFu) + (b & 0xFFu)), Nd, -Si2), ar);
                ai = fma(c, fma((double)((a >> 8) + (b >> 8)), Nd, -Sq2), ai);
            }
            if (NT & 1) {
                const unsigned a = r_s[o + NT / 2];
                ar = fma(coef[NT / 2], fma((double)(a & 0xFFu), Nd, -Si), ar);
                ai = fma(coef[NT / 2], fma((double)(a >> 8), Nd, -Sq), ai);
            }
        } else {
            // any taps, and the first rows of a capture (zero initial state: samples before 0 contribute nothing)
            const double* cc = NT > 0 ? coef : c_s;
            for (int k = nt - 1; k >= 0; --k) {
                if (i_out - k < 0) continue;
                const unsigned v = r_s[o + nt - 1 - k];
                const double c = cc[k];
                ar = fma(c, fma((double)(v & 0xFFu), Nd, -Si), ar);
                ai = fma(c, fma((double)(v >> 8), Nd, -Sq), ai);
            }
        }
        acc = fma(ar, ar, fma(ai, ai, acc));
    }
    // block sum in a fixed order: the wave's lanes (DPP tree), then the four waves in order
    __shared__ double w_s[4];
    const double ws = wave_sum(acc);
    if ((t & 63) == 0) w_s[t >> 6] = ws;
    __syncthreads();
    if (t == 0) partial[(size_t)s * gridDim.x + blockIdx.x] = ((w_s[0] + w_s[1]) + w_s[2]) + w_s[3];
}

// sum_i = sum_q = 0 ahead of k_dc_sum's atomics (the rest of the state array is not read).  grid ceil(S/256), block 256.
__global__ void k_band_power_clear(StreamState* st, int S) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S) { st[s].sum_i = 0; st[s].sum_q = 0; }
}

// power[s] = (sum over the capture's blocks, in block order) / N^2 / nd.  grid ceil(S/64), block 64.
__global__ void k_band_power_finish(const double* __restrict__ partial, int nblk, int S, long n, long nd,
                                    double* __restrict__ power) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const double* p = partial + (size_t)s * nblk;
    double sum = 0.0;
    for (int b = 0; b < nblk; ++b) sum += p[b];
    const double Nd = (double)n;
    power[s] = sum / (Nd * Nd) / (double)nd;
}
