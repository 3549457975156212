// kernels_demod.h -- front end of the SCH burst demodulator: per SCH burst, the frequency-domain channel
// estimate and equalisation of SCH_demod.m:53-59,79-90.  (The Viterbi GMSK demodulator behind it is Communications
// Toolbox code whose output the reference discards; it stays out.)
//
//   len_fde_ov = (148 + 2*8 + 30) * ov            = 1552 at 8x: the burst with 8 symbols either side + the traceback depth
//   td_training = zeros(1, L); td_training(sp_t : sp_t+64*ov-1) = training_sequence, sp_t = (8+42)*ov + 1      :56-58
//   fd_training = fft(td_training)                                                                                 :59
//   per burst i: x = s(sch_pos(i) - 8*ov : +L-1)                                                                :79-81
//       fd_chn = fft(x masked to the training span) ./ fd_training                                              :83-86
//       x_eq   = ifft( fft(x) ./ fd_chn.' )                                                                     :88-90
//
// L = 194*ov = 97 * (2*ov): Cooley-Tukey split n = N2*n1 + n2, k = k1 + 97*k2 with both factors as direct DFTs in
// LDS (97 is prime), twiddles from one exact table tw[m] = exp(-2 pi i m/L) (sincospi).  ~113 complex MACs per output
// instead of 1552.
#pragma once
#include "state.h"
#include "kernels_frontend.h"
#include "kernels_detect.h"
#include "kernels_estim.h"

#define DM_THREADS 512
#define DM_N1 97

// one forward (SIGN = -1) or inverse-without-1/L (SIGN = +1) DFT of in[0..L) -> out[0..L), both in LDS; B: N1 x (N2+1).
// Contains barriers; every thread of the block must call it.
template <int SIGN>
__device__ __forceinline__ void dm_dft(const cplx* in, cplx* out, cplx* B, const cplx* __restrict__ tw, int L, int N2, int tid) {
    const int ldb = N2 + 1;
    for (int o = tid; o < L; o += DM_THREADS) {
        const int k1 = o / N2, n2 = o - k1 * N2;
        double ar0 = 0.0, ai0 = 0.0, ar1 = 0.0, ai1 = 0.0;
        int idx = 0;                                   // (n1*k1 mod 97) * N2: index of W_97^(n1 k1) in the length-L table
        const int stp = k1 * N2;
        int n1 = 0;
        for (; n1 + 2 <= DM_N1; n1 += 2) {
            const cplx v0 = in[N2 * n1 + n2], t0 = tw[idx];
            idx += stp; if (idx >= L) idx -= L;
            const cplx v1 = in[N2 * (n1 + 1) + n2], t1 = tw[idx];
            idx += stp; if (idx >= L) idx -= L;
            const double s0 = SIGN < 0 ? t0.y : -t0.y, s1 = SIGN < 0 ? t1.y : -t1.y;
            ar0 = fma(v0.x, t0.x, fma(-v0.y, s0, ar0)); ai0 = fma(v0.x, s0, fma(v0.y, t0.x, ai0));
            ar1 = fma(v1.x, t1.x, fma(-v1.y, s1, ar1)); ai1 = fma(v1.x, s1, fma(v1.y, t1.x, ai1));
        }
        for (; n1 < DM_N1; ++n1) {
            const cplx v0 = in[N2 * n1 + n2], t0 = tw[idx];
            idx += stp; if (idx >= L) idx -= L;
            const double s0 = SIGN < 0 ? t0.y : -t0.y;
            ar0 = fma(v0.x, t0.x, fma(-v0.y, s0, ar0)); ai0 = fma(v0.x, s0, fma(v0.y, t0.x, ai0));
        }
        const double ar = ar0 + ar1, ai = ai0 + ai1;
        const cplx t = tw[n2 * k1];                    // inter-stage twiddle W_L^(n2 k1), n2*k1 < L
        const double ts = SIGN < 0 ? t.y : -t.y;
        B[k1 * ldb + n2] = make_double2(ar * t.x - ai * ts, ar * ts + ai * t.x);
    }
    __syncthreads();
    for (int k = tid; k < L; k += DM_THREADS) {
        const int k2 = k / DM_N1, k1 = k - k2 * DM_N1;
        double ar = 0.0, ai = 0.0;
        int idx = 0;                                   // (n2*k2 mod N2) * 97
        const int stp = (k2 % N2) * DM_N1;
        const cplx* row = B + k1 * ldb;
        for (int n2 = 0; n2 < N2; ++n2) {
            const cplx v = row[n2], t = tw[idx];
            idx += stp; if (idx >= L) idx -= L;
            const double s = SIGN < 0 ? t.y : -t.y;
            ar = fma(v.x, t.x, fma(-v.y, s, ar)); ai = fma(v.x, s, fma(v.y, t.x, ai));
        }
        out[k] = make_double2(ar, ai);
    }
    __syncthreads();
}

// MATLAB's complex right division a ./ b with scaling against overflow (Smith's algorithm)
__device__ __forceinline__ cplx dm_cdiv(cplx a, cplx b) {
    if (fabs(b.x) >= fabs(b.y)) {
        const double r = b.y / b.x, d = b.x + b.y * r;
        return make_double2((a.x + a.y * r) / d, (a.y - a.x * r) / d);
    }
    const double r = b.x / b.y, d = b.x * r + b.y;
    return make_double2((a.x * r + a.y) / d, (a.y * r - a.x) / d);
}

inline size_t dm_lds_bytes(int L, int N2) { return ((size_t)3 * L + (size_t)DM_N1 * (N2 + 1)) * sizeof(cplx); }

// fd_training (SCH_demod.m:56-59): grid 1, block DM_THREADS.
__global__ void __launch_bounds__(DM_THREADS) k_sch_fd_training(const cplx* __restrict__ ts, int len_ts, int sp_t0, int L, int N2,
                                                                const cplx* __restrict__ tw, cplx* __restrict__ fd_training) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    cplx* a = (cplx*)smem;
    cplx* b = a + L;
    cplx* B = b + 2 * L;
    const int tid = threadIdx.x;
    for (int i = tid; i < L; i += DM_THREADS) a[i] = (i >= sp_t0 && i < sp_t0 + len_ts) ? ts[i - sp_t0] : make_double2(0.0, 0.0);
    __syncthreads();
    dm_dft<-1>(a, b, B, tw, L, N2, tid);
    for (int i = tid; i < L; i += DM_THREADS) fd_training[i] = b[i];
}

// one workgroup per SCH burst: x_eq[burst][0..L).  start[burst] = 0-based index of s(sp); status[burst] != 0: the
// reference would stop with an index error (s(sp:ep) outside the stream) and nothing is written.
__global__ void __launch_bounds__(DM_THREADS) k_sch_equalise(const cplx* __restrict__ s, long len, const long* __restrict__ start,
                                                             int len_ts, int sp_t0, int L, int N2, const cplx* __restrict__ tw,
                                                             const cplx* __restrict__ fd_training, cplx* __restrict__ out,
                                                             int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    cplx* x = (cplx*)smem;               // the burst, later fd_x ./ fd_chn
    cplx* r = x + L;                     // the burst masked to the training span, later its spectrum
    cplx* f = r + L;                     // fft(x), later the equalised burst
    cplx* B = f + L;
    const int tid = threadIdx.x, w = blockIdx.x;
    const long sp = start[w];
    if (sp < 0 || sp + L > len) {        // block-uniform
        if (tid == 0) status[w] = GSMCAL_E_INDEX;
        return;
    }
    if (tid == 0) status[w] = 0;
    for (int i = tid; i < L; i += DM_THREADS) {
        const cplx v = s[sp + i];
        x[i] = v;
        r[i] = (i >= sp_t0 && i < sp_t0 + len_ts) ? v : make_double2(0.0, 0.0);     // :83-84
    }
    __syncthreads();
    dm_dft<-1>(x, f, B, tw, L, N2, tid);         // fd_x = fft(x)                                      :88
    dm_dft<-1>(r, x, B, tw, L, N2, tid);         // fd_received_training = fft(received_training_ov)    :85   (x is free)
    for (int i = tid; i < L; i += DM_THREADS) {
        const cplx chn = dm_cdiv(x[i], fd_training[i]);                                              // :86
        r[i] = dm_cdiv(f[i], chn);                                                                     // :89
    }
    __syncthreads();
    dm_dft<+1>(r, f, B, tw, L, N2, tid);         // ifft                                                :90
    const double inv = 1.0 / (double)L;
    cplx* o = out + (size_t)w * L;
    for (int i = tid; i < L; i += DM_THREADS) o[i] = make_double2(f[i].x * inv, f[i].y * inv);
}

// ------------------------------------------------------------------------------------------------
// FCCH_demod.m:5-66 -- the check behind the calibration: per FCCH burst of a corrected stream the tone frequency (:28-42, the
// estimator of burst_tone_body on an array source), the bin of the spectrum's peak (:34,:66) and the in-band SNR of :51-63 (NOT
// the gate of FCCH_fine_correction.m:185-189: other bins, another rule); per stream the mean frequency and the carrier error
// that is left (:44-48).
//
// k_fcch_demod: one workgroup per (burst slot b, stream s), grid (GSMCAL_MAX_HITS, D), block FD_THREADS.  Slot b is the b-th row
// of the stream's pos_info with type 0 (:18-19); a slot without a burst returns at once.  part[s][b] = {freq, snr, offset, status}.
// LDS: xs[nfft] (the window; after the 37-point step P[nfft], the power spectrum in fftshift order) | B[37][N2+1] | w37 | wN2:
// 39.2 KB at 8x, four workgroups per CU.  The window is read a second time from global memory for the phase step (the 37-point
// step by symmetries consumes its LDS copy; a second copy would cost the third workgroup per CU).
// ------------------------------------------------------------------------------------------------
#define FD_THREADS 512
#define FD_PART 4       /* doubles per burst slot in the workspace */

inline size_t fd_lds_bytes(int nfft) { return ((size_t)nfft + (size_t)37 * (nfft / 37 + 1) + 40 + nfft / 37) * sizeof(cplx); }

__global__ void __launch_bounds__(FD_THREADS) k_fcch_demod(const cplx* __restrict__ r, long stride, const long* __restrict__ r_len,
                                                           const double* __restrict__ pos_info, int nfft, int ov, int hnl,
                                                           const cplx* __restrict__ tw_g, double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned char is_fcch[MAXROWS];
    __shared__ double sh_sp;
    __shared__ int sh_has;
    __shared__ double red_p[FD_THREADS / 64];
    __shared__ int red_t[FD_THREADS / 64];
    __shared__ double red[2 * (FD_THREADS / 64)];
    __shared__ int sh_key;
    const int s = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
    const long len = r_len[s] < stride ? r_len[s] : stride;        // (r_len = -1: the reference returned r = -1)
    if (len < 1) return;                                           // block-uniform
    const double* pi = pos_info + (size_t)s * 2 * MAXROWS;
    // ---- :18-19  fcch_pos = pos_info(pos_info(:,2)==0, 1): the b-th of them ----
    if (tid == 0) sh_has = 0;
    if (tid < MAXROWS) is_fcch[tid] = pi[MAXROWS + tid] == 0.0;
    __syncthreads();
    if (tid < MAXROWS && is_fcch[tid]) {
        int rank = 0;
        for (int i = 0; i < tid; ++i) rank += is_fcch[i];
        if (rank == b) { sh_sp = pi[tid]; sh_has = 1; }
    }
    __syncthreads();
    if (!sh_has) return;                                           // block-uniform
    double* out = part + ((size_t)s * MAXH + b) * FD_PART;
    // ---- :24-26  s(sp:ep): MATLAB stops with an index error outside the stream; decided before any sample is read ----
    const double spd = sh_sp;
    if (!(spd >= 1.0) || !(spd <= (double)len) || (long)spd - 1 + nfft > len) {
        if (tid == 0) { out[0] = 0.0; out[1] = 0.0; out[2] = 0.0; out[3] = (double)GSMCAL_E_INDEX; }
        return;
    }
    const cplx* x = r + (size_t)s * stride + ((long)spd - 1);
    const int N2 = nfft / 37, ldb = N2 + 1;
    cplx* xs = (cplx*)smem;
    cplx* B = xs + nfft;
    cplx* w37 = B + 37 * ldb;
    cplx* wN2 = w37 + 40;
    double* P = (double*)xs;
    for (int i = tid; i < nfft; i += FD_THREADS) xs[i] = x[i];
    fft37_tables(w37, wN2, N2, tid, tw_g);
    __syncthreads();
    // ---- :28,:33-34  abs(fft).^2 in fftshift order and its first maximum ----
    fft37_step1_sym(xs, B, w37, tw_g, nfft, N2, ldb, tid, FD_THREADS);
    __syncthreads();                                               // xs is dead: P takes its place
    double best = -1.0;
    int key = 0x7fffffff;
    const int npair = nfft >> 1, h = N2 >> 1;
    for (int g = tid; g < npair; g += FD_THREADS) {                // a mirror pair of bins per lane (fft37_step2_pair)
        const int jj = g / 37, kr = g - jj * 37;
        const int k0 = kr + 37 * jj, k1 = jj == 0 ? kr + 37 * h : kr + 37 * (N2 - jj);
        cplx X0, X1;
        fft37_step2_pair(B, wN2, N2, ldb, kr, jj, &X0, &X1);
        const double p0 = X0.x * X0.x + X0.y * X0.y, p1 = X1.x * X1.x + X1.y * X1.y;
        const int s0 = k0 < npair ? k0 + npair : k0 - npair, s1 = k1 < npair ? k1 + npair : k1 - npair;   // position after fftshift
        P[s0] = p0;
        P[s1] = p1;
        if (p0 > best || (p0 == best && s0 < key)) { best = p0; key = s0; }
        if (p1 > best || (p1 == best && s1 < key)) { best = p1; key = s1; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double op = __shfl_down(best, off, 64);
        const int ok = __shfl_down(key, off, 64);
        if (op > best || (op == best && ok < key)) { best = op; key = ok; }
    }
    if ((tid & 63) == 0) { red_p[tid >> 6] = best; red_t[tid >> 6] = key; }
    __syncthreads();                                               // ... and P is complete
    if (tid == 0) {
        for (int i = 1; i < FD_THREADS / 64; ++i)
            if (red_p[i] > best || (red_p[i] == best && red_t[i] < key)) { best = red_p[i]; key = red_t[i]; }
        sh_key = key;
    }
    __syncthreads();
    const int max_idx = sh_key + 1;                                // 1-based, after fftshift
    const int jb = max_idx - (nfft / 2 + 1);                       // :36, :66
    // ---- :51-63  the SNR: 2*hnl bins around the centre against the five bins at the peak, both sums in a fixed order ----
    if (tid < 64) {
        const int lo = nfft / 2 - hnl, nb = 2 * hnl;               // :55-56 (0-based)
        double band = 0.0;
        for (int k = tid; k < nb; k += 64) band += P[lo + k];
        band = wave_sum(band);
        if (tid == 0) {
            double sig = 0.0;
            for (int d = -2; d <= 2; ++d) {                        // :58-60  mod(set-1, fft_len)+1
                int k = sh_key + d;
                k = k < 0 ? k + nfft : (k >= nfft ? k - nfft : k);
                sig += P[k];
            }
            const double noi = band - sig;                         // :61 (whether or not the five bins lie in the band)
            out[1] = noi < 0.0 ? __longlong_as_double(0x7ff8000000000000LL) : 10.0 * log10(sig / noi);   // :62 (complex in MATLAB -> NaN)
            out[2] = (double)jb;
            out[3] = 0.0;
        }
    }
    // ---- :36-42  integer-bin rotation from the exact table, unit phasors, phase step: burst_tone_body's statement ----
    const double ipr = (TWO_PI_D * (double)jb) / (double)nfft;
    const unsigned jm = (unsigned)(jb < 0 ? jb + nfft : jb);
    double sr = 0.0, si = 0.0;
    {
        auto unit = [](const cplx& p0) {
            const double m2 = p0.x * p0.x + p0.y * p0.y;
            const double inv = rsqrt(m2);
            return m2 > 0.0 ? make_double2(p0.x * inv, p0.y * inv) : make_double2(1.0, 0.0);   // angle(0) = 0
        };
        for (int n = tid; n < nfft - 1; n += FD_THREADS) {
            const unsigned i0 = ((unsigned)n * jm) % (unsigned)nfft;
            const unsigned i1 = i0 + jm >= (unsigned)nfft ? i0 + jm - (unsigned)nfft : i0 + jm;
            const cplx ub = unit(cmul(x[n], tw_g[i0]));
            const cplx ua = unit(cmul(x[n + 1], tw_g[i1]));
            sr += ua.x * ub.x + ua.y * ub.y;
            si += ua.y * ub.x - ua.x * ub.y;
        }
    }
    sr = wave_sum(sr);
    si = wave_sum(si);
    if ((tid & 63) == 0) { red[2 * (tid >> 6)] = sr; red[2 * (tid >> 6) + 1] = si; }
    __syncthreads();
    if (tid == 0) {
        double tr = 0.0, ti = 0.0;
        for (int i = 0; i < FD_THREADS / 64; ++i) { tr += red[2 * i]; ti += red[2 * i + 1]; }
        const double cnt = (double)(nfft - 1);
        const double phase = atan2(ti / cnt, tr / cnt);            // :40
        out[0] = (GSM_SYMBOL_RATE * (double)ov) * (ipr + phase) / TWO_PI_D;   // :42
    }
}

// k_fcch_demod_finish: one wave per stream, grid D, block 64.  out[s] = {num_fcch, mean_freq, carrier_ppm, status,
// freq[MAXH], snr[MAXH], max_idx[MAXH]} (GSMCAL_DEMOD_COLS doubles), unused entries NaN.
//   r_len < 1 or every element of pos_info -1 (:8-11)   status GSMCAL_S_POST_NO_POS, num_fcch 0, the rest NaN
//   more than MAXH type-0 rows                           status GSMCAL_E_CAPACITY, num_fcch = their number, the rest NaN
//   a window outside the stream                          status GSMCAL_E_INDEX, num_fcch = the number of rows, the rest NaN
//   no type-0 row                                        status 0, num_fcch 0, mean_freq = carrier_ppm = NaN (mean([]))
__global__ void __launch_bounds__(64) k_fcch_demod_finish(const long* __restrict__ r_len, const double* __restrict__ pos_info,
                                                          const double* __restrict__ carrier_freq, const double* __restrict__ part,
                                                          double* __restrict__ out) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const double* pi = pos_info + (size_t)s * 2 * MAXROWS;
    const double* ps = part + (size_t)s * MAXH * FD_PART;
    double* o = out + (size_t)s * GSMCAL_DEMOD_COLS;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    unsigned n0 = 0, not_m1 = 0;
    for (int i = lane; i < MAXROWS; i += 64) {
        const double p = pi[i], t = pi[MAXROWS + i];
        n0 += t == 0.0;
        not_m1 += (p != -1.0) || (t != -1.0);
    }
    n0 = wave_sum_u32(n0);
    not_m1 = wave_sum_u32(not_m1);
    int status = 0, nb = (int)n0;
    if (r_len[s] < 1 || not_m1 == 0) { status = GSMCAL_S_POST_NO_POS; nb = 0; }
    else if (nb > MAXH) status = GSMCAL_E_CAPACITY;
    else
        for (int i = 0; i < nb; ++i)                               // (uniform loop, uniform loads)
            if (status == 0 && ps[i * FD_PART + 3] != 0.0) status = GSMCAL_E_INDEX;
    const bool ok = status == 0;
    for (int i = lane; i < MAXH; i += 64) {
        const bool use = ok && i < nb;
        o[GSMCAL_D_FREQ + i] = use ? ps[i * FD_PART + 0] : nan;
        o[GSMCAL_D_SNR + i] = use ? ps[i * FD_PART + 1] : nan;
        o[GSMCAL_D_MAX_IDX + i] = use ? ps[i * FD_PART + 2] : nan;
    }
    if (lane == 0) {
        double mean = nan, ppm = nan;
        if (ok && nb > 0) {
            double acc = 0.0;
            for (int i = 0; i < nb; ++i) acc += ps[i * FD_PART + 0];                 // :44 mean(freq): left to right
            mean = acc / (double)nb;
            ppm = 1e6 * (mean - GSM_SYMBOL_RATE / 4.0) / carrier_freq[s];            // :47-48
        }
        o[GSMCAL_D_NUM_FCCH] = (double)nb;
        o[GSMCAL_D_MEAN_FREQ] = mean;
        o[GSMCAL_D_CARRIER_PPM] = ppm;
        o[GSMCAL_D_STATUS] = (double)status;
    }
}
