// kernels_subband.h -- several sub-band powers out of one raw capture: the per-capture loop of
// multi_rtl_sdr_diversity_scanner_another_bak.m:186-210
//
//   power[j] = mean(abs(filter(coef,1, raw2iq(s).*exp(1i*(1:N)'*w_j))(1:decim:end)).^2)
//
// The mixer never runs: filter(c,1, x.*e^{jw(n+1)})[n] = e^{jw(n+1)} * sum_k (c_k e^{-jwk}) x[n-k], so |r_flt[n]|^2 is
// |sum_k h_k x[n-k]|^2 with the complex taps h_k = c_k e^{-jwk}.  The host builds one tap row per distinct w (double,
// stored newest sample last: row[m] = h[ntaps-1-m]) and an index table [capture][slot] into the rows, -1 for an unused slot.
//
//   k_band_power_clear, k_dc_sum   (kernels_spectrum.h, kernels_frontend.h) exact integer I/Q byte sums per capture
//   k_subband_power                the complex FIR at the kept rows, |N*y|^2 in fp64, one partial per (capture, block, slot)
//   k_subband_power_finish         the partials of a (capture, slot) summed in block order, divided once; NaN for unused slots
//
// DC as in k_band_power: X = N*c - S per component is an exact integer in a double, the finishing step divides by
// N^2 * ceil(N/decim); a constant capture gives X = 0 everywhere and exactly 0 in every sub-band.  The block tiling depends on
// N, decim and the tap count only and every sub-band has accumulators of its own, so a (capture, w) pair gives the same bits
// in any slot, beside any other sub-bands, at any position of a batch of any size.
#pragma once
#include "kernels_spectrum.h"

#define SB_MAX_SUBBANDS 16               // == GSMCAL_MAX_SUBBANDS
#define SB_MAX_TAPS 128                  // diversity_scanner_another_bak.m:52-53 caps the order at 127
#define SB_PASS 4                        // sub-bands filtered together: 8 accumulators in registers

// LDS bytes of a block: the tap rows of `nsub` slots + the raw span of `rows` kept rows (stage_raw's slack included)
__host__ __device__ inline size_t sb_lds_bytes(int rows, int decim, int ntaps, int nsub) {
    const size_t span = (size_t)(rows - 1) * decim + ntaps + 24;
    return (size_t)nsub * ntaps * sizeof(cplx) + ((span * 2 + 15) & ~(size_t)15);
}

// One pass: NS sub-bands (tap rows h_s + q*nt, q < NS) over this lane's kept rows, ascending.  acc[q] += |N*y_q|^2.
// EDGE: the block holds rows whose window starts before the capture (zero initial state: those taps are skipped).
template <int NS, bool EDGE>
__device__ __forceinline__ void sb_pass(const cplx* __restrict__ h_s, const unsigned short* __restrict__ r_s, int nt, int decim,
                                        long j0, long jn, long first_al, int t, double Nd, double Si, double Sq, double* acc) {
    for (long r = t; r < jn; r += 256) {
        const long i_out = (j0 + r) * decim;
        const int o = (int)(i_out - (nt - 1) - first_al);      // LDS index of the oldest sample of this output
        int m0 = 0;
        if (EDGE && i_out < nt - 1) m0 = (int)(nt - 1 - i_out);
        double yr[NS], yi[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) { yr[q] = 0.0; yi[q] = 0.0; }
#pragma unroll 2
        for (int m = m0; m < nt; ++m) {                        // oldest tap first
            const unsigned v = r_s[o + m];
            const double xr = fma((double)(v & 0xFFu), Nd, -Si), xi = fma((double)(v >> 8), Nd, -Sq);
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const cplx h = h_s[q * nt + m];
                yr[q] = fma(h.x, xr, fma(-h.y, xi, yr[q]));
                yi[q] = fma(h.x, xi, fma(h.y, xr, yi[q]));
            }
        }
#pragma unroll
        for (int q = 0; q < NS; ++q) acc[q] = fma(yr[q], yr[q], fma(yi[q], yi[q], acc[q]));
    }
}

// grid (ceil(nd/rows), S), block 256; capture s = raw + s*stream_bytes; idx[s*nsub + slot] = tap row or -1;
// partial[((s*gridDim.x) + blockIdx.x)*nsub + slot] (written for used slots only).  Dynamic LDS: sb_lds_bytes(rows, decim, ntaps, nsub).
__global__ void __launch_bounds__(256) k_subband_power(const uint8_t* __restrict__ raw, long stream_bytes,
                                                      const StreamState* __restrict__ st, const cplx* __restrict__ taps,
                                                      const int* __restrict__ idx, int ntaps, int nsub, int decim, long nd,
                                                      int rows, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int slot_s[SB_MAX_SUBBANDS];                    // the used slots, in slot order
    __shared__ int nv_s;
    __shared__ double w_s[4][SB_PASS];
    cplx* h_s = (cplx*)smem;
    unsigned short* r_s = (unsigned short*)(smem + (size_t)nsub * ntaps * sizeof(cplx));
    const int s = blockIdx.y, t = threadIdx.x;
    const long n = stream_bytes >> 1;
    const unsigned short* base = (const unsigned short*)(raw + (size_t)s * stream_bytes);
    const int* my_idx = idx + (size_t)s * nsub;
    const long j0 = (long)blockIdx.x * rows;
    long jn = nd - j0;
    if (jn > rows) jn = rows;
    const long first = j0 * decim - (ntaps - 1);
    const int span = (int)((jn - 1) * decim + ntaps);
    if (t == 0) {
        int nv = 0;
        for (int j = 0; j < nsub; ++j)
            if (my_idx[j] >= 0) slot_s[nv++] = j;
        nv_s = nv;
    }
    __syncthreads();
    const int nv = nv_s;
    if (nv == 0) return;                                       // (block-uniform)
    for (int i = t; i < nv * ntaps; i += 256) {
        const int q = i / ntaps, m = i - q * ntaps;
        h_s[i] = taps[(size_t)my_idx[slot_s[q]] * ntaps + m];
    }
    const long first_al = stage_raw<false>(r_s, base, n, first, span, t, 256);
    __syncthreads();
    const double Nd = (double)n;
    const double Si = (double)st[s].sum_i, Sq = (double)st[s].sum_q;
    double* out = partial + ((size_t)s * gridDim.x + blockIdx.x) * nsub;
    const bool edge = first < 0;
    for (int q0 = 0; q0 < nv; q0 += SB_PASS) {
        const int ns = nv - q0 < SB_PASS ? nv - q0 : SB_PASS;
        const cplx* hp = h_s + (size_t)q0 * ntaps;
        double acc[SB_PASS] = {0.0, 0.0, 0.0, 0.0};
#define SB_CALL(NS)                                                                                                  \
        do {                                                                                                             \
            if (edge) sb_pass<NS, true>(hp, r_s, ntaps, decim, j0, jn, first_al, t, Nd, Si, Sq, acc);                  \
            else sb_pass<NS, false>(hp, r_s, ntaps, decim, j0, jn, first_al, t, Nd, Si, Sq, acc);                       \
        } while (0)
        if (ns == 4) SB_CALL(4);
        else if (ns == 3) SB_CALL(3);
        else if (ns == 2) SB_CALL(2);
        else SB_CALL(1);
#undef SB_CALL
        // block sums in a fixed order: the wave's lanes (DPP tree), then the four waves in order
#pragma unroll
        for (int q = 0; q < SB_PASS; ++q) {
            const double ws = wave_sum(acc[q]);
            if ((t & 63) == 0) w_s[t >> 6][q] = ws;
        }
        __syncthreads();
        if (t < ns) out[slot_s[q0 + t]] = ((w_s[0][t] + w_s[1][t]) + w_s[2][t]) + w_s[3][t];
        __syncthreads();
    }
}

// power[s*nsub + slot] = (sum over the capture's blocks, in block order) / N^2 / nd; NaN where idx < 0.
// grid ceil(S*nsub/64), block 64.
__global__ void k_subband_power_finish(const double* __restrict__ partial, const int* __restrict__ idx, int nblk, int S,
                                       int nsub, long n, long nd, double* __restrict__ power) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= (long)S * nsub) return;
    if (idx[u] < 0) { power[u] = __longlong_as_double(0x7FF8000000000000LL); return; }
    const long s = u / nsub;
    const int slot = (int)(u - s * nsub);
    const double* p = partial + (size_t)s * nblk * nsub + slot;
    double sum = 0.0;
    for (int b = 0; b < nblk; ++b) sum += p[(size_t)b * nsub];
    const double Nd = (double)n;
    power[u] = sum / (Nd * Nd) / (double)nd;
}
