// kernels_apply.h -- apply_calibration: raw capture bytes resampled onto the nominal time base, their carrier error taken
// out, DC and I/Q imbalance removed, in one pass.  The project's own function: what the calibration chain measures, this acts on, at
// any centre frequency and sample rate.  The definition is DESIGN 23's and tests/apply_ref.py restates it.
//
// Per capture (its bytes a_m, b_m and a row {delay, slope_ppm, carrier_hz, phase, anchor, scale, dc_i, dc_q, gain, sin_phase}) and
// output index n, in fp64, with x(n), validity, the interpolator h and the angle exactly as pair_align has them (kernels_align.h:
// pa_x, pa_valid, pa_interp, pa_angle, pa_sincos -- shared, not copied):
//   z[m] = (a_m - dc_i) + j ((b_m - dc_q) / gain - (a_m - dc_i) sin_phase) / c,   c = sqrt(1 - sin_phase^2)
//   out[n] = scale exp(-j angle(n)) sum_k h(k - mu) z[base + k]      (0 where not valid)
//
// k_apply_calibration: grid (tiles of PA_TILE consecutive n, captures), block PA_TILE -- lane = one n.  The workgroup fetches the
// tile's source window (at most PA_TILE + 17 samples = 546 bytes) once, as 16-bit words, and stages it in LDS converted: the pair
// (a - dc_i, b - dc_q) as two doubles, so that a byte is converted once and not once per tap, and pa_interp runs on it unchanged.
// The interpolator's taps are real and the I/Q correction is linear: it is applied to the two sums, not to the sixteen samples
// (Im = Sb / (gain c) - Sa sin_phase / c, the two factors formed once per row on the host).  Outputs are written once, with
// non-temporal stores.  What a lane computes depends on its capture's bytes and row alone.
//
// k_apply_info: lane = one capture -- status and the valid interval [first_valid, end_valid) by bisection on the same x(n).
#pragma once
#include "kernels_align.h"

// One capture's row as the kernels take it: the values of its parameter row that the lanes use, formed once on the host.
struct ApRow {
    double delay, slope, w, phase, anchor, scale;   // slope = slope_ppm * 1e-6, w = 2 pi carrier_hz / sample_rate
    double dc_i, dc_q, q_gain, q_skew;              // q_gain = 1 / (gain c), q_skew = sin_phase / c
    double run, pad;                                // run = 1: every value of the parameter row is finite
};

__device__ __forceinline__ PaMember ap_member(const ApRow& a, long n_samples) {
    PaMember m;
    m.delay = a.delay; m.slope = a.slope; m.w = a.w; m.phase = a.phase; m.anchor = a.anchor; m.weight = a.scale;
    m.len = n_samples;
    m.run = a.run != 0.0;
    return m;
}

// raw + capture * 2 n: a capture's bytes, 2-byte aligned; out + capture * out_stride.  n0: the first output index of this launch's
// first tile.
__global__ void __launch_bounds__(PA_TILE) k_apply_calibration(const uint8_t* __restrict__ raw, long n_samples, const ApRow* __restrict__ rows,
                                                               long out_len, long out_stride, long n0, cplx* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) cplx win[PA_WIN];
    const int tid = threadIdx.x;
    const long t0 = n0 + (long)blockIdx.x * PA_TILE;               // (the host launches only tiles with t0 < out_len)
    const long cnt = out_len - t0 < PA_TILE ? out_len - t0 : PA_TILE;
    const long n = t0 + tid;
    const bool mine = tid < cnt;
    const ApRow a = rows[blockIdx.y];
    const PaMember m = ap_member(a, n_samples);
    cplx* orow = out + (size_t)blockIdx.y * out_stride;
    // ---- the tile's source window, clipped to the capture (uniform) ----
    long lo = 0, hi = -1;
    if (m.run) {
        const double b_lo = floor(pa_x(m, t0)) - 7.0, b_hi = floor(pa_x(m, t0 + cnt - 1)) + 8.0;
        if (b_hi >= 0.0 && b_lo < (double)m.len) {                 // (also false for a value beyond every index)
            lo = b_lo > 0.0 ? (long)b_lo : 0;
            hi = b_hi < (double)m.len ? (long)b_hi : m.len - 1;
            if (hi > lo + PA_WIN - 1) hi = lo + PA_WIN - 1;        // (not reached at |slope_ppm| <= 1000: the window is at most PA_TILE + 17)
        }
    }
    if (hi < lo) {                                                 // skipped, or no valid sample in this tile
        if (mine) st_stream16(orow + n, make_double2(0.0, 0.0));
        return;
    }
    const unsigned short* src = (const unsigned short*)(raw + (size_t)blockIdx.y * 2 * (size_t)n_samples) + lo;
    for (long i = tid; i <= hi - lo; i += PA_TILE) {
        const unsigned v = src[i];                                 // I | Q << 8
        win[i] = make_double2((double)(v & 0xFFu) - a.dc_i, (double)(v >> 8) - a.dc_q);
    }
    __syncthreads();
    if (!mine) return;
    cplx o = make_double2(0.0, 0.0);
    const double x = pa_x(m, n), base = floor(x);
    bool ok = pa_valid(base, m.len);
    long off = 0;
    if (ok) {
        off = (long)base - 7 - lo;
        ok = off >= 0 && off + 15 <= hi - lo;                      // (always true: x is monotone in n)
    }
    if (ok) {
        const cplx s = pa_interp(win + off, x - base);            // {sum h (a - dc_i), sum h (b - dc_q)}
        const double zr = s.x, zi = s.y * a.q_gain - s.x * a.q_skew;
        double sn, cn;
        pa_sincos(pa_angle(m, n), &sn, &cn);                       // scale exp(-j angle) z
        o = make_double2(a.scale * (zr * cn + zi * sn), a.scale * (zi * cn - zr * sn));
    }
    st_stream16(orow + n, o);
}

// info[d][GSMCAL_APPLY_INFO_COLS]: {status, first_valid, end_valid, num_valid} per capture
__global__ void __launch_bounds__(64) k_apply_info(const ApRow* __restrict__ rows, int d, long n_samples, long out_len, double* __restrict__ info) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= d) return;
    const PaMember m = ap_member(rows[s], n_samples);
    long first = 0, end = 0;
    if (m.run) {
        const double dlen = (double)m.len;
        first = pa_first(m, out_len, [](double b) { return b - 7.0 >= 0.0; });
        end = pa_first(m, out_len, [dlen](double b) { return !(b + 8.0 < dlen); });
        if (end <= first) { first = 0; end = 0; }                  // no valid sample: the empty interval at 0
    }
    double* o = info + (size_t)s * GSMCAL_APPLY_INFO_COLS;
    o[0] = m.run ? 0.0 : (double)GSMCAL_S_ALIGN_SKIPPED;
    o[1] = (double)first;
    o[2] = (double)end;
    o[3] = (double)(end - first);
}
