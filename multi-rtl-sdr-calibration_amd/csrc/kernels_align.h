// kernels_align.h -- pair_align: resample calibrated streams onto one dongle's time base, take their carrier out and,
// when asked for, add them up.  The project's own function: what pair_coherence measures, this acts on.  The definition
// is DESIGN 20's and tests/pair_align_ref.py restates it.
//
// Per member g (a stream index and a row {delay, slope_ppm, carrier_hz, phase, anchor, weight}) and output index n, all in fp64:
//   x = (n + delay) + (slope_ppm 1e-6) (n - anchor),  base = floor(x),  mu = x - base          (every operation rounded on its own)
//   valid iff 0 <= base - 7 and base + 8 < len
//   aligned[g][n] = exp(-j (phase + (2 pi carrier_hz / fs) (n - anchor))) sum_{k=-7..8} h(k - mu) s[base + k]      (0 where not valid)
//   h(u) = sinc(u) (0.42 + 0.5 cos(2 pi u / 16) + 0.08 cos(4 pi u / 16)),  h(0) = 1
//   combined[n] = sum_g weight_g aligned[g][n], in list order, over the members valid at n
// A member whose stream is empty or whose row holds a value that is not finite is skipped: its row is zero and it adds nothing.
//
// k_pair_align: grid (tiles of PA_TILE consecutive n, member groups), block PA_TILE -- lane = one n.  With a combined output the
// grid has one member group and the workgroup walks the whole list, every lane adding its members up in a register pair; without,
// every member is a group of its own.  Per member the workgroup stages the tile's source window -- from floor(x) - 7 of its first n
// to floor(x) + 8 of its last, at most PA_TILE + 17 samples at |slope_ppm| <= 1000 -- into LDS as 16-byte values, clipped to the
// stream; validity is decided before a sample is read, in global memory and in LDS.  The sixteen taps cost one sincospi of mu
// (sin pi (k - mu) = -(-1)^k sin pi mu), one of mu / 8 (the window's two cosines from the angle-addition constants of k) and four
// divisions (the sixteen reciprocals 1 / (mu - k) four at a time from the reciprocal of their product).  Outputs are written once,
// with non-temporal stores (st_stream16).  What a lane computes for (g, n) depends on that member's row and stream alone: an aligned
// row is the same bits wherever the member stands in whatever list, with or without the sum.
//
// k_pair_align_info: one wave, lane g = member g (G <= 64) -- status and the valid interval [first_valid, end_valid) by bisection on
// the same x(n) (monotone in n at |slope_ppm| <= 1000), then the sum's row: the interval by max / min over the wave, the weights added in list order.
#pragma once
#include "kernels_demod.h"

#define PA_TILE 256
#define PA_HALF 8                               /* taps k = -(PA_HALF - 1) .. PA_HALF */
#define PA_WIN (PA_TILE + 2 * PA_HALF + 8)      /* staged samples per member and tile: PA_TILE + 16 + the drift over a tile, rounded up */
#define PA_NP GSMCAL_ALIGN_PARAMS

struct PaMember {
    double delay, slope, w, phase, anchor, weight;   // slope = slope_ppm * 1e-6, w = 2 pi carrier_hz / fs
    long len;
    bool run;                                        // status 0: aligned and summed
};

// the six values of a member's row and its stream length -> what the lanes use (uniform)
__device__ __forceinline__ PaMember pa_member(const double* __restrict__ row, long len, double fs) {
#pragma clang fp contract(off)
    PaMember m;
    m.delay = row[0];
    m.slope = row[1] * 1e-6;
    m.w = 2.0 * PI_D * row[2] / fs;
    m.phase = row[3];
    m.anchor = row[4];
    m.weight = row[5];
    m.len = len;
    bool fin = true;
#pragma unroll
    for (int i = 0; i < PA_NP; ++i) fin = fin && isfinite(row[i]);
    m.run = len >= 1 && fin;
    return m;
}
__device__ __forceinline__ int pa_status(const PaMember& m) { return m.len < 1 ? GSMCAL_S_POST_NO_POS : (m.run ? 0 : GSMCAL_S_ALIGN_SKIPPED); }

// x(n): every operation rounded on its own (no fused multiply-add), so that floor(x) is the restatement's
__device__ __forceinline__ double pa_x(const PaMember& m, long n) {
#pragma clang fp contract(off)
    const double dn = (double)n;
    const double a = dn + m.delay;
    const double b = m.slope * (dn - m.anchor);
    return a + b;
}
__device__ __forceinline__ double pa_angle(const PaMember& m, long n) {
#pragma clang fp contract(off)
    const double t = m.w * ((double)n - m.anchor);
    return m.phase + t;
}
// sin and cos of an angle of up to ~1e7 rad: the whole turns go first (2 pi in two parts; angle - k * the first part is exact), the
// rest, at most pi, goes through sincospi.  Within 1e-15 rad of the angle, without the large-argument path of sincos and its registers.
__device__ __forceinline__ void pa_sincos(double angle, double* sn, double* cn) {
    const double k = rint(angle * (1.0 / TWO_PI_D));
    double rem = fma(-k, 6.283185307179586, angle);
    rem = fma(-k, 2.4492935982947064e-16, rem);
    sincospi(rem * (1.0 / PI_D), sn, cn);
}
__device__ __forceinline__ bool pa_valid(double base, long len) { return base - 7.0 >= 0.0 && base + 8.0 < (double)len; }

// cos and sin of pi k / 8 for k = -7 .. 8 (index k + 7); pi k / 4 is every second entry around k = 0
__device__ constexpr double PA_C8[16] = {-0.92387953251128674, -0.70710678118654752, -0.38268343236508977, 0.0, 0.38268343236508977,
                                         0.70710678118654752, 0.92387953251128674, 1.0, 0.92387953251128674, 0.70710678118654752,
                                         0.38268343236508977, 0.0, -0.38268343236508977, -0.70710678118654752, -0.92387953251128674, -1.0};
__device__ constexpr double PA_S8[16] = {-0.38268343236508977, -0.70710678118654752, -0.92387953251128674, -1.0, -0.92387953251128674,
                                         -0.70710678118654752, -0.38268343236508977, 0.0, 0.38268343236508977, 0.70710678118654752,
                                         0.92387953251128674, 1.0, 0.92387953251128674, 0.70710678118654752, 0.38268343236508977, 0.0};
__device__ constexpr double PA_C4[16] = {0.70710678118654752, 0.0, -0.70710678118654752, -1.0, -0.70710678118654752, 0.0, 0.70710678118654752, 1.0,
                                         0.70710678118654752, 0.0, -0.70710678118654752, -1.0, -0.70710678118654752, 0.0, 0.70710678118654752, 1.0};
__device__ constexpr double PA_S4[16] = {0.70710678118654752, 1.0, 0.70710678118654752, 0.0, -0.70710678118654752, -1.0, -0.70710678118654752, 0.0,
                                         0.70710678118654752, 1.0, 0.70710678118654752, 0.0, -0.70710678118654752, -1.0, -0.70710678118654752, 0.0};

// sum_k h(k - mu) win[k + 7], win = the sixteen samples base - 7 .. base + 8 (LDS), 0 <= mu < 1
__device__ __forceinline__ cplx pa_interp(const cplx* __restrict__ win, double mu) {
    double sp, cp, s1, c1;
    sincospi(mu, &sp, &cp);
    sincospi(mu * 0.125, &s1, &c1);
    const double c2 = c1 * c1 - s1 * s1, s2 = 2.0 * s1 * c1;
    const double q = sp * (1.0 / PI_D);
    const bool on_grid = mu == 0.0;                                // h(k) = [k == 0]: the sample itself, whatever the window's rounding
    double ar = 0.0, ai = 0.0;
#pragma unroll 1
    for (int k4 = 0; k4 < 16; k4 += 4) {                           // (not unrolled: sixteen taps in flight at once cost 160 registers)
        // 1 / (mu - k) for four k from one division.  mu > 0 is a multiple of 2^-52 of a number >= 7 and the other factors lie in
        // [1, 8): the product neither overflows nor vanishes.  (mu = 0: the values are not used.)
        double dk[4], inv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) dk[i] = mu - (double)(k4 + i - 7);
        const double p01 = dk[0] * dk[1], p23 = dk[2] * dk[3];
        const double r = 1.0 / (p01 * p23);
        const double r01 = r * p23, r23 = r * p01;
        inv[0] = r01 * dk[1]; inv[1] = r01 * dk[0]; inv[2] = r23 * dk[3]; inv[3] = r23 * dk[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = k4 + i, k = j - 7;
            const double wnd = 0.42 + 0.5 * (PA_C8[j] * c1 + PA_S8[j] * s1) + 0.08 * (PA_C4[j] * c2 + PA_S4[j] * s2);
            double h = ((k & 1) ? -q : q) * inv[i] * wnd;
            if (on_grid) h = k == 0 ? 1.0 : 0.0;
            const cplx v = win[j];
            ar = fma(h, v.x, ar);
            ai = fma(h, v.y, ai);
        }
    }
    return make_double2(ar, ai);
}

// members[g]: stream index (checked on the host); params[g][PA_NP].  aligned ([G][out_len]) and combined ([out_len]) may each be
// null, not both.  n0: the first output index of this launch's first tile.
__global__ void __launch_bounds__(PA_TILE) k_pair_align(const cplx* __restrict__ r, long stride, const long* __restrict__ r_len, int ov,
                                                        const int* __restrict__ members, const double* __restrict__ params, int G,
                                                        long out_len, long n0, cplx* __restrict__ aligned, cplx* __restrict__ combined) {
    __shared__ __attribute__((aligned(16))) cplx win[PA_WIN];
    const int tid = threadIdx.x;
    const long t0 = n0 + (long)blockIdx.x * PA_TILE;               // (the host launches only tiles with t0 < out_len)
    const long cnt = out_len - t0 < PA_TILE ? out_len - t0 : PA_TILE;
    const long n = t0 + tid;
    const bool mine = tid < cnt;
    const double fs = GSM_SYMBOL_RATE * (double)ov;
    const int g_lo = combined ? 0 : (int)blockIdx.y, g_hi = combined ? G : g_lo + 1;
    double cr = 0.0, ci = 0.0;
    for (int g = g_lo; g < g_hi; ++g) {
        const int s = members[g];
        const PaMember m = pa_member(params + (size_t)g * PA_NP, stream_len(r_len, s, stride), fs);
        cplx* arow = aligned ? aligned + (size_t)g * out_len : nullptr;
        // ---- the tile's source window, clipped to the stream (uniform) ----
        long lo = 0, hi = -1;
        if (m.run) {
            const double b_lo = floor(pa_x(m, t0)) - 7.0, b_hi = floor(pa_x(m, t0 + cnt - 1)) + 8.0;
            if (b_hi >= 0.0 && b_lo < (double)m.len) {             // (also false for a value beyond every index)
                lo = b_lo > 0.0 ? (long)b_lo : 0;
                hi = b_hi < (double)m.len ? (long)b_hi : m.len - 1;
                if (hi > lo + PA_WIN - 1) hi = lo + PA_WIN - 1;    // (not reached at |slope_ppm| <= 1000: the window is at most PA_TILE + 17)
            }
        }
        if (hi < lo) {                                             // skipped, or no valid sample in this tile
            if (arow && mine) st_stream16(arow + n, make_double2(0.0, 0.0));
            continue;
        }
        const cplx* src = r + (size_t)s * stride + lo;
        __syncthreads();                                           // the member before is read
        for (long i = tid; i <= hi - lo; i += PA_TILE) win[i] = src[i];
        __syncthreads();
        cplx o = make_double2(0.0, 0.0);
        bool ok = false;
        if (mine) {
            const double x = pa_x(m, n), base = floor(x);
            ok = pa_valid(base, m.len);
            long off = 0;
            if (ok) {
                off = (long)base - 7 - lo;
                ok = off >= 0 && off + 15 <= hi - lo;              // (always true: x is monotone in n)
            }
            if (ok) {
                const cplx a = pa_interp(win + off, x - base);
                double sn, cn;
                pa_sincos(pa_angle(m, n), &sn, &cn);                // exp(-j angle) a
                o = make_double2(a.x * cn + a.y * sn, a.y * cn - a.x * sn);
            }
            if (arow) st_stream16(arow + n, o);
        }
        if (ok) {
            cr = fma(m.weight, o.x, cr);
            ci = fma(m.weight, o.y, ci);
        }
    }
    if (combined && mine) st_stream16(combined + n, make_double2(cr, ci));
}

// the first n in [0, out_len] from which on `pred(floor(x(n)))` holds (pred monotone in n: false ... false true ... true)
template <class F>
__device__ __forceinline__ long pa_first(const PaMember& m, long out_len, F pred) {
    long a = 0, b = out_len;                                       // the answer lies in [a, b]
    while (a < b) {
        const long mid = a + (b - a) / 2;
        if (pred(floor(pa_x(m, mid)))) b = mid; else a = mid + 1;
    }
    return a;
}

// info[G + 1][GSMCAL_ALIGN_INFO_COLS]: member rows {status, first_valid, end_valid, num_valid}, then {members_used, combined_first,
// combined_end, sum of the used members' weights}
__global__ void __launch_bounds__(64) k_pair_align_info(const long* __restrict__ r_len, long stride, int ov, const int* __restrict__ members,
                                                        const double* __restrict__ params, int G, long out_len, double* __restrict__ info) {
    const int lane = threadIdx.x;
    const bool have = lane < G;
    const int g = have ? lane : 0;
    const PaMember m = pa_member(params + (size_t)g * PA_NP, stream_len(r_len, members[g], stride), GSM_SYMBOL_RATE * (double)ov);
    const bool used = have && m.run;
    long first = 0, end = 0;
    if (used) {
        const double dlen = (double)m.len;
        first = pa_first(m, out_len, [](double b) { return b - 7.0 >= 0.0; });
        end = pa_first(m, out_len, [dlen](double b) { return !(b + 8.0 < dlen); });
        if (end <= first) { first = 0; end = 0; }                  // no valid sample: the empty interval at 0
    }
    if (have) {
        double* o = info + (size_t)g * GSMCAL_ALIGN_INFO_COLS;
        o[0] = (double)pa_status(m);
        o[1] = (double)first;
        o[2] = (double)end;
        o[3] = (double)(end - first);
    }
    // ---- the sum's row: every member that is used bounds the interval ----
    long cf = used ? first : 0, ce = used ? end : out_len;
    for (int off = 32; off > 0; off >>= 1) {
        const long of = (long)__shfl_xor((long long)cf, off, 64), oe = (long)__shfl_xor((long long)ce, off, 64);
        cf = of > cf ? of : cf;
        ce = oe < ce ? oe : ce;
    }
    const unsigned long long um = __ballot(used);
    const int nu = __popcll(um);
    double ws = 0.0;                                               // in list order, as the sum itself
    if (lane == 0)
        for (int i = 0; i < G; ++i)
            if ((um >> i) & 1ull) ws += params[(size_t)i * PA_NP + GSMCAL_A_WEIGHT];
    if (nu == 0) { cf = 0; ce = 0; }
    if (ce < cf) ce = cf;
    if (lane == 0) {
        double* o = info + (size_t)G * GSMCAL_ALIGN_INFO_COLS;
        o[0] = (double)nu;
        o[1] = (double)cf;
        o[2] = (double)ce;
        o[3] = ws;
    }
}
