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
// What the kernels below share: they all work on (r, r_len, pos_info) of D streams, pos_info[s] = [2][MAXROWS] with -1 padding
// (DESIGN 11).
//
// pos_rows: one wave ranks the rows i of a stream's table for which pred(i, pi) holds, in table order.  Lane l evaluates rows
// l, l + 64, ... (POS_NCH chunks); visit(c, is, rank) sees every chunk -- `is` and the 0-based `rank` of this lane's row, the
// rank meaningful where `is` -- and the number of matching rows comes back, wave-uniform.  pos_row_pick turns (is, rank) into
// the index of the b-th matching row by one ballot; pos_row_select does both and leaves -1 where there is no b-th row.
// ------------------------------------------------------------------------------------------------
constexpr int POS_NCH = (MAXROWS + 63) / 64;

template <int T>
struct PosType {                                 // pos_info(i, 2) == T: 0 FCCH, 1 SCH, 2 BCCH
    __device__ bool operator()(int i, const double* pi) const { return pi[MAXROWS + i] == (double)T; }
};
struct PosBurst {                                // a burst with content to correlate: SCH or BCCH (an FCCH tone has no delay)
    __device__ bool operator()(int i, const double* pi) const { return pi[MAXROWS + i] == 1.0 || pi[MAXROWS + i] == 2.0; }
};
struct PosBlock {                                // a BCCH block: type 1, and type 2 in the four rows behind it
    __device__ bool operator()(int i, const double* pi) const {
        bool isb = i + 4 < MAXROWS && pi[MAXROWS + i] == 1.0;
        for (int q = 1; q <= 4; ++q) isb = isb && pi[MAXROWS + i + q] == 2.0;
        return isb;
    }
};

// the row lane `lane` evaluates in chunk c, or the last row where the chunk reaches past the table: every lane has a row to
// load, so no load sits behind a branch and the loads of all chunks (and of several passes) go out together
__device__ __forceinline__ int pos_row_clamped(int c, int lane) { return c * 64 + lane < MAXROWS ? c * 64 + lane : MAXROWS - 1; }

template <class Pred, class Visit>
__device__ __forceinline__ int pos_rows(const double* pi, int lane, Pred pred, Visit visit) {
    int n = 0;
    for (int c = 0; c < POS_NCH; ++c) {
        const int i = c * 64 + lane;
        const bool is = pred(pos_row_clamped(c, lane), pi) && i < MAXROWS;
        const unsigned long long m = __ballot(is);
        visit(c, is, n + __popcll(m & ((1ull << lane) - 1ull)));
        n += __popcll(m);
    }
    return n;
}
template <class Pred>
__device__ __forceinline__ int pos_rows_count(const double* pi, int lane, Pred pred) {
    return pos_rows(pi, lane, pred, [](int, bool, int) {});
}
__device__ __forceinline__ void pos_row_pick(int c, bool is, int rank, int b, int& row) {
    const unsigned long long sel = __ballot(is && rank == b);
    if (sel) row = c * 64 + __ffsll((long long)sel) - 1;
}
template <class Pred>
__device__ __forceinline__ int pos_row_select(const double* pi, int lane, int b, Pred pred, int& row) {
    row = -1;
    return pos_rows(pi, lane, pred, [&](int c, bool is, int rank) { pos_row_pick(c, is, rank, b, row); });
}

// The stream header.  len: the samples that can be read, min(r_len, stride) (r_len = -1: the reference returned r = -1; every
// entry point refuses stride < 1, so len < 1 is r_len < 1).  has_pos: not every element of pos_info is -1 (`if pos_info == -1`),
// formed by one wave.  status(): the two exits every *_finish kernel takes first, in this order; the first one reports no rows.
struct StreamHead {
    long len;
    bool has_pos;
    __device__ int status(int& count, int cap) const {
        if (len < 1 || !has_pos) { count = 0; return GSMCAL_S_POST_NO_POS; }
        return count > cap ? GSMCAL_E_CAPACITY : 0;
    }
};
__device__ __forceinline__ long stream_len(const long* __restrict__ r_len, int s, long stride) {
    return r_len[s] < stride ? r_len[s] : stride;
}
__device__ __forceinline__ StreamHead stream_head(const long* __restrict__ r_len, int s, long stride, const double* pi, int lane) {
    const int n = pos_rows_count(pi, lane, [](int i, const double* p) {
        const double pos = p[i], type = p[MAXROWS + i];            // both loads before the test: neither waits for the other
        return pos != -1.0 || type != -1.0;
    });
    return StreamHead{stream_len(r_len, s, stride), n > 0};
}

// ------------------------------------------------------------------------------------------------
// The burst detector of SCH_decode and BCCH_decode: what the two kernels have in common.
//   vt_derotate   v (-j)^k: a swap and a negation.
//   VtLane        the 16-state trellis of the rate-1/2 code G0 = 1 + D^3 + D^4, G1 = 1 + D + D^3 + D^4 (GSM 05.03 4.1.3): lane mod
//                 16 = state u(k-1)<<3 | u(k-2)<<2 | u(k-3)<<1 | u(k-4); its two predecessors p0, p1 (older bit 0, older bit 1)
//                 and the coded pair on either edge.  Start in state 0 (the others at -inf).
//   acs           one add-compare-select step: two additions per candidate -- (+-s0) + (+-s1), then path metric + that: no
//                 product, nothing contracts -- and a strict > that keeps the candidate whose older bit is 0.  pm becomes the
//                 survivor's metric; the return value says that it came from p1.  Survivor storage is the caller's.
//   vt_corrected  the hard channel bits that differ from the re-encoded word c(2k) = u(k)+u(k-3)+u(k-4), c(2k+1) = c(2k)+u(k-1),
//                 counted by one wave from ballots; soft(j) and u(k) (0 for k < 0) are the caller's getters.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ cplx vt_derotate(cplx v, int k) {
    const int q = k & 3;                                           // (-j)^k: 1, -j, -1, j
    return q == 0 ? v : q == 1 ? make_double2(v.y, -v.x) : q == 2 ? make_double2(-v.x, -v.y) : make_double2(-v.y, v.x);
}
struct VtLane {
    int bit, p0, p1;
    bool a0, a1, b0, b1;                                           // c(2k), c(2k+1) coming from p0; ... from p1
    double pm;
    __device__ explicit VtLane(int lane) {
        const int ns = lane & 15;
        bit = ns >> 3; p0 = (ns & 7) << 1; p1 = p0 | 1;
        a0 = (bit ^ (p0 >> 1) ^ p0) & 1; a1 = (a0 ^ (p0 >> 3)) & 1;
        b0 = (bit ^ (p1 >> 1) ^ p1) & 1; b1 = (b0 ^ (p1 >> 3)) & 1;
        pm = ns == 0 ? 0.0 : -__builtin_huge_val();
    }
    __device__ __forceinline__ bool acs(double s0, double s1) {
        const double bm0 = (a0 ? -s0 : s0) + (a1 ? -s1 : s1);
        const double bm1 = (b0 ? -s0 : s0) + (b1 ? -s1 : s1);
        const double c0 = __shfl(pm, p0, 64) + bm0, c1 = __shfl(pm, p1, 64) + bm1;
        const bool take = c1 > c0;                                 // strict: the first candidate stays
        pm = take ? c1 : c0;
        return take;
    }
};
template <class Soft, class U>
__device__ __forceinline__ int vt_corrected(int ncoded, int lane, Soft soft, U u) {
    int corrected = 0;
    for (int j0 = 0; j0 < ncoded; j0 += 64) {                      // (uniform)
        const int j = j0 + lane, k = j >> 1;
        bool differs = false;
        if (j < ncoded) {
            const unsigned c = u(k) ^ u(k - 3) ^ u(k - 4) ^ ((j & 1) ? u(k - 1) : 0u);
            differs = (soft(j) < 0.0) != (c != 0u);
        }
        corrected += __popcll(__ballot(differs));
    }
    return corrected;
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
// step by symmetries consumes its LDS copy; a second copy would cost the third workgroup per CU).  Four workgroups per CU are
// eight waves per SIMD: the launch bound says so, or the compiler spends registers (87 where 59 do) that leave room for two.
// ------------------------------------------------------------------------------------------------
#define FD_THREADS 512
#define FD_PART 4       /* doubles per burst slot in the workspace */

inline size_t fd_lds_bytes(int nfft) { return ((size_t)nfft + (size_t)37 * (nfft / 37 + 1) + 40 + nfft / 37) * sizeof(cplx); }

__global__ void __launch_bounds__(FD_THREADS, 8) k_fcch_demod(const cplx* __restrict__ r, long stride, const long* __restrict__ r_len,
                                                           const double* __restrict__ pos_info, int nfft, int ov, int hnl,
                                                           const cplx* __restrict__ tw_g, double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double red_p[FD_THREADS / 64];
    __shared__ int red_t[FD_THREADS / 64];
    __shared__ double red[2 * (FD_THREADS / 64)];
    __shared__ int sh_key;
    const int s = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
    const long len = stream_len(r_len, s, stride);
    if (len < 1) return;                                           // block-uniform
    const double* pi = pos_info + (size_t)s * 2 * MAXROWS;
    // ---- :18-19  fcch_pos = pos_info(pos_info(:,2)==0, 1): the b-th of them, found by every wave on its own ----
    int row;
    pos_row_select(pi, tid & 63, b, PosType<0>(), row);
    if (row < 0) return;                                           // block-uniform
    double* out = part + ((size_t)s * MAXH + b) * FD_PART;
    // ---- :24-26  s(sp:ep): MATLAB stops with an index error outside the stream; decided before any sample is read ----
    const double spd = pi[row];
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
            out[1] = noi < 0.0 ? NAN_D : 10.0 * log10(sig / noi);   // :62 (complex in MATLAB -> NaN)
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
__global__ void __launch_bounds__(64) k_fcch_demod_finish(const long* __restrict__ r_len, long stride, const double* __restrict__ pos_info,
                                                          const double* __restrict__ carrier_freq, const double* __restrict__ part,
                                                          double* __restrict__ out) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const double* pi = pos_info + (size_t)s * 2 * MAXROWS;
    const double* ps = part + (size_t)s * MAXH * FD_PART;
    double* o = out + (size_t)s * GSMCAL_DEMOD_COLS;
    int nb = pos_rows_count(pi, lane, PosType<0>());
    int status = stream_head(r_len, s, stride, pi, lane).status(nb, MAXH);
    if (status == 0)
        for (int i = 0; i < nb; ++i)                               // (uniform loop, uniform loads)
            if (status == 0 && ps[i * FD_PART + 3] != 0.0) status = GSMCAL_E_INDEX;
    const bool ok = status == 0;
    for (int i = lane; i < MAXH; i += 64) {
        const bool use = ok && i < nb;
        o[GSMCAL_D_FREQ + i] = use ? ps[i * FD_PART + 0] : NAN_D;
        o[GSMCAL_D_SNR + i] = use ? ps[i * FD_PART + 1] : NAN_D;
        o[GSMCAL_D_MAX_IDX + i] = use ? ps[i * FD_PART + 2] : NAN_D;
    }
    if (lane == 0) {
        double mean = NAN_D, ppm = NAN_D;
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

// ------------------------------------------------------------------------------------------------
// BCCH_demod.m -- which of the eight normal training sequences the BCCH bursts carry.  The function body is
// carrier_correct_post_SCH.m:51-83 (:49-76 here: the tone estimate of every FCCH burst, mean(fo), carrier_ppm, the stream
// rotated by comp_phase_rotate) followed by the correlation of :84-106 at the fixed position 61 symbols into each BCCH burst.
// The tone estimate is k_fcch_demod's (FCCH_demod.m:28-42 is the same block): these kernels read its workspace.
//
// k_bcch_corr: grid (BC_GRID_X, D), block BC_THREADS.  Workgroup (g, s) takes the type-2 rows g, g + BC_GRID_X, ... of stream
// s's pos_info (every wave ranks them itself, so a workgroup without a row returns before the first barrier).  Per row: the
// 26*ov window r(sp:ep), sp =
// bcch_pos + 61*ov (:93-95), read once, rotated by exp(1i*n*comp_phase_rotate) at its absolute sample index n (:76) and kept in
// LDS; wave w forms the conjugated dot products with templates 2w and 2w+1 (:97) -- fp64 FMAs, lane l takes samples l, l+64,
// ..., then the wave sum, lane 0 writes: a fixed order, the same for every template.  corr[s][slot][8], flag[s][slot] = 0 or
// GSMCAL_E_INDEX (the window leaves the stream: decided before a sample is read, the eight sums NaN).
// Every workgroup forms mean(fo) itself, left to right like k_bcch_finish: the same bits everywhere.
// ------------------------------------------------------------------------------------------------
#define BC_THREADS 256
#define BC_GRID_X 8
#define BC_SLOTS GSMCAL_MAX_BCCH

__device__ __forceinline__ double bc_mean_fo(const double* __restrict__ ps, int n0) {
    double acc = 0.0;
    for (int i = 0; i < n0; ++i) acc += ps[i * FD_PART];                         // :70 mean(fo): left to right
    return n0 > 0 ? acc / (double)n0 : NAN_D;   // mean([]) = NaN
}
__device__ __forceinline__ double bc_comp_phase(double mean_fo, int ov) {
    return (GSM_SYMBOL_RATE / 4.0 - mean_fo) * 2.0 * PI_D / (GSM_SYMBOL_RATE * (double)ov);   // :74-75
}

__global__ void __launch_bounds__(BC_THREADS) k_bcch_corr(const cplx* __restrict__ r, long stride, const long* __restrict__ r_len,
                                                          const double* __restrict__ pos_info, int ov, const cplx* __restrict__ nts,
                                                          const double* __restrict__ fd_part, cplx* __restrict__ corr,
                                                          int* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    cplx* win = (cplx*)smem;
    const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long len = stream_len(r_len, s, stride);
    if (len < 1) return;                                           // block-uniform
    const double* pi = pos_info + (size_t)s * 2 * MAXROWS;
    // ---- :13, :49  the type-2 and the type-0 rows, ranked by every wave on its own; (is2, rank) stay in registers for the slots ----
    bool is2[POS_NCH];
    int rank[POS_NCH];
    int nb = pos_rows(pi, lane, PosType<2>(), [&](int c, bool is, int rk) { is2[c] = is; rank[c] = rk; });
    const int n0 = pos_rows_count(pi, lane, PosType<0>());
    if (nb < 4 || n0 > MAXH) return;                               // :14 / more FCCH rows than the workspace holds: k_bcch_finish says which
    if (nb > BC_SLOTS) nb = BC_SLOTS;
    if ((int)blockIdx.x >= nb) return;                             // no row for this workgroup
    const double cpr = bc_comp_phase(bc_mean_fo(fd_part + (size_t)s * MAXH * FD_PART, n0), ov);
    const int lts = 26 * ov;
    for (int b = blockIdx.x; b < nb; b += BC_GRID_X) {             // (uniform)
        int row = 0;
        for (int c = 0; c < POS_NCH; ++c) pos_row_pick(c, is2[c], rank[c], b, row);
        cplx* oc = corr + ((size_t)s * BC_SLOTS + b) * 8;
        int* of = flag + (size_t)s * BC_SLOTS + b;
        const double spd = pi[row] + (double)(61 * ov);            // :93
        if (!(spd >= 1.0) || !(spd <= (double)len) || (long)spd - 1 + lts > len) {   // :95 would stop with an index error
            if (tid < 8) oc[tid] = make_double2(NAN_D, NAN_D);
            if (tid == 0) *of = GSMCAL_E_INDEX;
            continue;
        }
        const long n_abs = (long)spd - 1;                          // 0-based index of r(sp)
        const cplx* x = r + (size_t)s * stride + n_abs;
        for (int i = tid; i < lts; i += BC_THREADS) {
            double sn, cs;
            sincos((double)(n_abs + i) * cpr, &sn, &cs);           // :76 the rounded product, then sin and cos
            win[i] = cmul(x[i], make_double2(cs, sn));
        }
        __syncthreads();
        for (int q = 0; q < 2; ++q) {
            const int k = 2 * wave + q;
            const cplx* t = nts + (size_t)k * lts;
            double ar = 0.0, ai = 0.0;
            for (int i = lane; i < lts; i += 64) {                 // conj(t) * w
                const cplx tv = t[i], w = win[i];
                ar = fma(tv.x, w.x, fma(tv.y, w.y, ar));
                ai = fma(tv.x, w.y, fma(-tv.y, w.x, ai));
            }
            ar = wave_sum(ar);
            ai = wave_sum(ai);
            if (lane == 0) oc[k] = make_double2(ar, ai);
        }
        if (tid == 0) *of = 0;
        __syncthreads();                                           // win is rewritten for the next row
    }
}

// k_bcch_finish: one wave per stream, grid D, block 64.  out[s] = one row of GSMCAL_BCCH_COLS doubles (GSMCAL_B_*), written here
// and nowhere else: per evaluated burst the first maximum of |corr| (:99; a later equal value does not replace it), the second
// largest value and the winner's angle; the decision of :100 on the first four; unused entries NaN.
//   r_len < 1 or every element of pos_info -1 (:9)       status GSMCAL_S_POST_NO_POS, num_bcch 0
//   fewer than 4 type-2 rows (:14)                        status GSMCAL_S_POST_FEW_BCCH
//   more than BC_SLOTS type-2 or MAXH type-0 rows         status GSMCAL_E_CAPACITY
//   an FCCH window or one of the first four BCCH windows outside the stream      status GSMCAL_E_INDEX
//   the first four winners differ (:103)                  status GSMCAL_S_BCCH_TSC_MIXED, mean_fo and carrier_ppm valid
// In the first four cases tsc_idx is -1 and mean_fo, carrier_ppm, num_agree NaN.  A row beyond the fourth with its window outside
// the stream has NaN entries and is no error (the reference never reads it).  corr_out (may be NULL): [D][BC_SLOTS][8] complex, NaN
// where no burst was evaluated.  r_len_out (may be NULL): the stream's length where the reference has formed r (status 0 or
// GSMCAL_S_BCCH_TSC_MIXED), -1 elsewhere.
__global__ void __launch_bounds__(64) k_bcch_finish(const long* __restrict__ r_len, long stride, const double* __restrict__ pos_info,
                                                    const double* __restrict__ carrier_freq, const double* __restrict__ fd_part,
                                                    const cplx* __restrict__ corr, const int* __restrict__ flag, double* __restrict__ out,
                                                    cplx* __restrict__ corr_out, long* __restrict__ r_len_out) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const double* pi = pos_info + (size_t)s * 2 * MAXROWS;
    const double* ps = fd_part + (size_t)s * MAXH * FD_PART;
    const cplx* cs = corr + (size_t)s * BC_SLOTS * 8;
    const int* fs = flag + (size_t)s * BC_SLOTS;
    double* o = out + (size_t)s * GSMCAL_BCCH_COLS;
    const int n0 = pos_rows_count(pi, lane, PosType<0>());
    int nb = pos_rows_count(pi, lane, PosType<2>());
    const StreamHead head = stream_head(r_len, s, stride, pi, lane);
    const long len = head.len;
    int status = head.status(nb, BC_SLOTS);
    if (status != GSMCAL_S_POST_NO_POS && nb < 4) status = GSMCAL_S_POST_FEW_BCCH;     // the literal 4 of :14
    else if (status == 0 && n0 > MAXH) status = GSMCAL_E_CAPACITY;
    if (status == 0) {
        for (int i = 0; i < n0; ++i)                               // (uniform loops, uniform loads)
            if (status == 0 && ps[i * FD_PART + 3] != 0.0) status = GSMCAL_E_INDEX;
        for (int i = 0; i < 4; ++i)
            if (status == 0 && fs[i] != 0) status = GSMCAL_E_INDEX;
    }
    const bool ok = status == 0;
    double idx0 = NAN_D, idx1 = NAN_D, idx2 = NAN_D, idx3 = NAN_D;
    unsigned agree = 0;
    for (int b0 = 0; b0 < BC_SLOTS; b0 += 64) {                    // (uniform)
        const int b = b0 + lane;
        const bool use = ok && b < nb && b < BC_SLOTS && fs[b] == 0;
        double best = -1.0, second = -1.0, ph = NAN_D;
        int bi = -1;
        if (use) {
            for (int k = 0; k < 8; ++k) {
                const double m = hypot(cs[b * 8 + k].x, cs[b * 8 + k].y);       // abs()
                if (m > best) { second = best; best = m; bi = k; }
                else if (m > second) second = m;
            }
            if (bi >= 0) ph = atan2(cs[b * 8 + bi].y, cs[b * 8 + bi].x);
        }
        const double idx = bi >= 0 ? (double)(bi + 1) : NAN_D;
        if (b0 == 0) { idx0 = __shfl(idx, 0, 64); idx1 = __shfl(idx, 1, 64); idx2 = __shfl(idx, 2, 64); idx3 = __shfl(idx, 3, 64); }
        agree += idx == idx0;
        if (b < BC_SLOTS) {
            o[GSMCAL_B_IDX + b] = idx;
            o[GSMCAL_B_PEAK + b] = bi >= 0 ? best : NAN_D;
            o[GSMCAL_B_RUNNER_UP + b] = bi >= 0 ? second : NAN_D;
            o[GSMCAL_B_PHASE + b] = ph;
        }
    }
    agree = wave_sum_u32(agree);
    double tsc = -1.0;
    if (ok) {
        if (idx0 == idx1 && idx0 == idx2 && idx0 == idx3) tsc = idx0;            // :100 (NaN equals nothing)
        else status = GSMCAL_S_BCCH_TSC_MIXED;
    }
    if (corr_out)
        for (int i = lane; i < BC_SLOTS * 8; i += 64) {
            const int b = i >> 3;
            corr_out[(size_t)s * BC_SLOTS * 8 + i] = ok && b < nb && fs[b] == 0 ? cs[i] : make_double2(NAN_D, NAN_D);
        }
    if (lane == 0) {
        double mean = NAN_D, ppm = NAN_D;
        if (ok) {
            mean = bc_mean_fo(ps, (int)n0);                                      // :70
            ppm = 1e6 * (mean - GSM_SYMBOL_RATE / 4.0) / carrier_freq[s];        // :71
        }
        o[GSMCAL_B_NUM_BCCH] = (double)nb;
        o[GSMCAL_B_TSC_IDX] = tsc;
        o[GSMCAL_B_MEAN_FO] = mean;
        o[GSMCAL_B_CARRIER_PPM] = ppm;
        o[GSMCAL_B_STATUS] = (double)status;
        o[GSMCAL_B_NUM_AGREE] = ok ? (double)agree : NAN_D;
        if (r_len_out) r_len_out[s] = ok ? len : -1;
    }
}

// k_bcch_rotate: r = s .* exp(1i*(0:len-1)'*comp_phase_rotate) (:76) for the streams k_bcch_finish left a length for; launched only
// when r is asked for.  grid (blocks, D), block 256, grid-stride over the stream.
__global__ void __launch_bounds__(256) k_bcch_rotate(const cplx* __restrict__ r, long stride, const long* __restrict__ r_len_out,
                                                     const double* __restrict__ table, int ov, cplx* __restrict__ r_out) {
    const int s = blockIdx.y;
    const long len = r_len_out[s];
    if (len < 1) return;
    const double cpr = bc_comp_phase(table[(size_t)s * GSMCAL_BCCH_COLS + GSMCAL_B_MEAN_FO], ov);
    const cplx* x = r + (size_t)s * stride;
    cplx* y = r_out + (size_t)s * stride;
    for (long n = (long)blockIdx.x * 256 + threadIdx.x; n < len; n += (long)gridDim.x * 256) {
        double sn, cs;
        sincos((double)n * cpr, &sn, &cs);
        y[n] = cmul(x[n], make_double2(cs, sn));
    }
}

// ------------------------------------------------------------------------------------------------
// SCH_decode -- the payload of the SCH bursts: BSIC and GSM frame number.  The project's own function: SCH_demod.m
// has no outputs and demodulates with Communications Toolbox code, so there is nothing to be in parity with; the definition is
// DESIGN 16's and tests/sch_decode_ref.py restates it line by line.
//
// k_sch_decode: grid (MAXH, D), block 64 -- one wave per SCH burst slot: the blockIdx.x-th type-1 row of its stream's pos_info
// (1-based start p).  delta = (5 ov - 1) div 2.
//   1  y_k = s(p + k ov + delta) (-j)^k, k = 3..144: 142 strided reads, kept in LDS.  A burst whose reads leave the stream, or
//      whose p is NaN or < 1, is not evaluated (decided before a sample is read).
//   2  lane i holds y_{42+i} a_i, a_i = 1 - 2 SCH_TRAINING_BITS[i]; five xor-shuffle steps inside each half of the wave leave h1
//      in lanes 0..31 and h2 in lanes 32..63: one fixed order.  h = h1 + h2, slope = angle(h2 conj(h1)) / 32, amp = |h| / 64.
//   3  soft_k = Re(y_k conj(h)/|h| exp(-j slope (k - 73.5))) for k = 3..144, in LDS.
//   4  the trellis (VtLane) over soft[3..41], soft[106..144]; every group of 16 lanes runs the same one.  The survivor's 39-bit
//      history is one 64-bit register, taken from the predecessor lane by __shfl (register exchange: no traceback memory, no
//      atomics); the answer is state 0's history.
//   5  ts_err from a ballot, corrected by vt_corrected; CRC, tail bits and the fields on lane 0 (SD_INFO_MAP is the bit map, the one
//      table to pin against a capture).
// part[s][slot][SD_PART] = {evaluated, ok, bsic, fn, ts_err, corrected, slope, amp}; every block writes its record.  Optional:
// soft_out[s][slot][148] (NaN outside 3..144 and for a slot that was not evaluated), u_out[s][slot][39] bytes (255 likewise).
// ------------------------------------------------------------------------------------------------
#define SD_PART 8
#define SD_TRAINING_MASK 0xd86ea2b4f020469dull   /* bit i = SCH_TRAINING_BITS[i] (gsm_SCH_training_sequence_gen.m:17-19) */
#define SD_HYPERFRAME 2715648L
#define SD_CRC_POLY 0x575u                       /* g(D) = D^10 + D^8 + D^6 + D^5 + D^4 + D^2 + 1 */

enum { SD_BSIC = 0, SD_T1 = 1, SD_T2 = 2, SD_T3P = 3 };
// information bit d(i) = bit SD_INFO_MAP[i][1] of field SD_INFO_MAP[i][0] (GSM 04.08 9.1.30, 05.03 4.7; synth.SCH_INFO_MAP)
__device__ const unsigned char SD_INFO_MAP[25][2] = {
    {SD_T1, 9}, {SD_T1, 10}, {SD_BSIC, 0}, {SD_BSIC, 1}, {SD_BSIC, 2}, {SD_BSIC, 3}, {SD_BSIC, 4}, {SD_BSIC, 5},
    {SD_T1, 1}, {SD_T1, 2}, {SD_T1, 3}, {SD_T1, 4}, {SD_T1, 5}, {SD_T1, 6}, {SD_T1, 7}, {SD_T1, 8},
    {SD_T3P, 1}, {SD_T3P, 2}, {SD_T2, 0}, {SD_T2, 1}, {SD_T2, 2}, {SD_T2, 3}, {SD_T2, 4}, {SD_T1, 0}, {SD_T3P, 0}};

__device__ __forceinline__ unsigned long long sd_shfl_u64(unsigned long long v, int src) {
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src, 64), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src, 64);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ int sd_soft_index(int j) { return j < 39 ? 3 + j : 67 + j; }      // coded bit c(j) -> burst symbol
__device__ __forceinline__ unsigned sd_u(unsigned long long u, int k) { return k < 0 ? 0u : (unsigned)(u >> k) & 1u; }

__global__ void __launch_bounds__(64) k_sch_decode(const cplx* __restrict__ r, long stride, const long* __restrict__ r_len,
                                                   const double* __restrict__ pos_info, int ov, double* __restrict__ part,
                                                   double* __restrict__ soft_out, unsigned char* __restrict__ u_out) {
    __shared__ cplx ys[148];
    __shared__ double soft[148];
    const int s = blockIdx.y, b = blockIdx.x, lane = threadIdx.x;
    double* out = part + ((size_t)s * MAXH + b) * SD_PART;
    const long len = stream_len(r_len, s, stride);
    const double* pi = pos_info + (size_t)s * 2 * MAXROWS;
    int row;                                                       // the b-th type-1 row
    const int n1 = pos_row_select(pi, lane, b, PosType<1>(), row);
    const int dl = (5 * ov - 1) / 2;
    const double spd = row >= 0 ? pi[row] : 0.0;
    // p NaN or < 1, or symbol 144 behind the last sample: not evaluated (wave-uniform)
    if (len < 1 || row < 0 || n1 > MAXH || !(spd >= 1.0) || !(spd + (double)(144 * ov + dl) <= (double)len)) {
        if (lane == 0) out[0] = 0.0;
        else if (lane < SD_PART) out[lane] = NAN_D;
        if (soft_out)
            for (int k = lane; k < 148; k += 64) soft_out[((size_t)s * MAXH + b) * 148 + k] = NAN_D;
        if (u_out && lane < 39) u_out[((size_t)s * MAXH + b) * 39 + lane] = 255;
        return;
    }
    // ---- 1  the 142 symbols, derotated ----
    const cplx* x = r + (size_t)s * stride + ((long)spd - 1 + dl);
    for (int k = 3 + lane; k <= 144; k += 64) ys[k] = vt_derotate(x[(long)k * ov], k);
    __syncthreads();
    // ---- 2  the two half-sums over the training sequence ----
    const bool tbit = (SD_TRAINING_MASK >> lane) & 1ull;
    double hr = tbit ? -ys[42 + lane].x : ys[42 + lane].x, hi = tbit ? -ys[42 + lane].y : ys[42 + lane].y;
    for (int off = 16; off > 0; off >>= 1) {
        hr += __shfl_xor(hr, off, 64);
        hi += __shfl_xor(hi, off, 64);
    }
    const double h1r = __shfl(hr, 0, 64), h1i = __shfl(hi, 0, 64), h2r = __shfl(hr, 32, 64), h2i = __shfl(hi, 32, 64);
    const double hx = h1r + h2r, hy = h1i + h2i;
    const double mag = hypot(hx, hy);
    const double slope = atan2(h2i * h1r - h2r * h1i, h2r * h1r + h2i * h1i) / 32.0;
    const double amp = mag / 64.0;
    const cplx w = make_double2(hx / mag, -hy / mag);               // conj(h)/|h|
    // ---- 3  the soft values ----
    for (int k = 3 + lane; k <= 144; k += 64) {
        double sn, cs;
        sincos(slope * ((double)k - 73.5), &sn, &cs);
        const cplx q = cmul(w, make_double2(cs, -sn));
        soft[k] = ys[k].x * q.x - ys[k].y * q.y;
    }
    __syncthreads();
    // ---- 4  the trellis; the survivor's history travels with the metric ----
    VtLane vt(lane);
    unsigned long long hist = 0;
    for (int k = 0; k < 39; ++k) {
        const unsigned long long g0 = sd_shfl_u64(hist, vt.p0), g1 = sd_shfl_u64(hist, vt.p1);
        const bool take = vt.acs(soft[sd_soft_index(2 * k)], soft[sd_soft_index(2 * k + 1)]);
        hist = (take ? g1 : g0) | ((unsigned long long)vt.bit << k);
    }
    const unsigned long long u = sd_shfl_u64(hist, 0);             // end in state 0: u(k) = bit k
    // ---- 5  hard errors in the training bits; hard channel bits against the re-encoded word ----
    const int ts_err = __popcll(__ballot((soft[42 + lane] < 0.0) != tbit));
    const int corrected = vt_corrected(78, lane, [&](int j) { return soft[sd_soft_index(j)]; }, [&](int k) { return sd_u(u, k); });
    if (soft_out)
        for (int k = lane; k < 148; k += 64) soft_out[((size_t)s * MAXH + b) * 148 + k] = k >= 3 && k <= 144 ? soft[k] : NAN_D;
    if (u_out && lane < 39) u_out[((size_t)s * MAXH + b) * 39 + lane] = (unsigned char)sd_u(u, lane);
    if (lane == 0) {
        unsigned reg = 0;                                          // u(0..34) divided by g(D): the remainder must be all ones
        for (int k = 0; k < 35; ++k) {
            reg = (reg << 1) | sd_u(u, k);
            if (reg & 0x400u) reg ^= SD_CRC_POLY;
        }
        int f[4] = {0, 0, 0, 0};
        for (int i = 0; i < 25; ++i) f[SD_INFO_MAP[i][0]] |= (int)sd_u(u, i) << SD_INFO_MAP[i][1];
        const int t3 = 10 * f[SD_T3P] + 1;
        const long fn = 1326L * f[SD_T1] + 51L * (((t3 - f[SD_T2]) % 26 + 26) % 26) + t3;
        const bool ok = reg == 0x3ffu && (u >> 35) == 0ull && f[SD_T3P] <= 4 && f[SD_T2] <= 25;
        out[0] = 1.0;
        out[1] = ok ? 1.0 : 0.0;
        out[2] = ok ? (double)f[SD_BSIC] : NAN_D;
        out[3] = ok ? (double)fn : NAN_D;
        out[4] = (double)ts_err;
        out[5] = (double)corrected;
        out[6] = slope;
        out[7] = amp;
    }
}

// k_sch_finish: one wave per stream, grid D, block 64.  out[s] = one row of GSMCAL_SCH_COLS doubles (GSMCAL_C_*), written here and
// nowhere else.  Lane i holds the i-th type-1 row.  The consistency rule: among the ok bursts c_i counts the ok bursts j (i
// included) with bsic_j == bsic_i and (fn_j - fn_i - round((p_j - p_i) / (1250 ov))) mod 2 715 648 == 0 (round: half away from
// zero, MATLAB's); the anchor is the smallest i with the largest c_i; status 0 iff c_anchor >= 2 -- one pass of a 10-bit CRC is
// not evidence -- otherwise GSMCAL_S_SCH_NO_DECODE with bsic, fn_anchor, pos_anchor = -1.
//   r_len < 1 or every element of pos_info -1        status GSMCAL_S_POST_NO_POS, num_sch 0
//   more than MAXH type-1 rows                       status GSMCAL_E_CAPACITY, nothing evaluated
// mean_slope: the mean of slope[] over the ok bursts, summed left to right; NaN without one.
__global__ void __launch_bounds__(64) k_sch_finish(const long* __restrict__ r_len, long stride, const double* __restrict__ pos_info,
                                                   int ov, const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double pos[MAXH];
    const int s = blockIdx.x, lane = threadIdx.x;
    const double* pi = pos_info + (size_t)s * 2 * MAXROWS;
    const double* ps = part + (size_t)s * MAXH * SD_PART;
    double* o = out + (size_t)s * GSMCAL_SCH_COLS;
    const StreamHead head = stream_head(r_len, s, stride, pi, lane);      // (first: its loads are the ones the ranking needs)
    int nb = pos_rows(pi, lane, PosType<1>(), [&](int c, bool is, int rank) {
        const double p = pi[pos_row_clamped(c, lane)];
        if (is && rank < MAXH) pos[rank] = p;
    });
    __syncthreads();
    int status = head.status(nb, MAXH);
    const bool mine = status == 0 && lane < nb;
    const bool ev = mine && ps[lane * SD_PART] == 1.0;
    const bool ok = ev && ps[lane * SD_PART + 1] == 1.0;
    const double bsic = ok ? ps[lane * SD_PART + 2] : NAN_D, fnd = ok ? ps[lane * SD_PART + 3] : NAN_D;
    const long fn = ok ? (long)fnd : 0;
    const double p = mine ? pos[lane] : 0.0, slope = ev ? ps[lane * SD_PART + 6] : NAN_D;
    const double frame = 1250.0 * (double)ov;
    int cnt = 0, num_ok = 0;
    double acc = 0.0;
    for (int j = 0; j < MAXH; ++j) {                               // (uniform)
        const bool okj = __shfl((int)ok, j, 64) != 0;
        const double bj = __shfl(bsic, j, 64), pj = __shfl(p, j, 64), sj = __shfl(slope, j, 64);
        const long fj = (long)sd_shfl_u64((unsigned long long)fn, j);
        if (okj) { ++num_ok; acc += sj; }
        if (ok && okj && bj == bsic) {
            const long dfr = (long)round((pj - p) / frame);
            const long dd = (fj - fn - dfr) % SD_HYPERFRAME;
            cnt += dd == 0;
        }
    }
    int best = 0, anchor = -1;
    for (int i = 0; i < MAXH; ++i) {                               // the smallest i with the largest c_i
        const int ci = __shfl(cnt, i, 64);
        if (ci > best) { best = ci; anchor = i; }
    }
    if (status == 0 && best < 2) status = GSMCAL_S_SCH_NO_DECODE;
    if (lane < MAXH) {
        o[GSMCAL_C_OK + lane] = ev ? (ok ? 1.0 : 0.0) : NAN_D;
        o[GSMCAL_C_BSIC_B + lane] = bsic;
        o[GSMCAL_C_FN + lane] = fnd;
        o[GSMCAL_C_TS_ERR + lane] = ev ? ps[lane * SD_PART + 4] : NAN_D;
        o[GSMCAL_C_CORRECTED + lane] = ev ? ps[lane * SD_PART + 5] : NAN_D;
        o[GSMCAL_C_SLOPE + lane] = slope;
        o[GSMCAL_C_AMP + lane] = ev ? ps[lane * SD_PART + 7] : NAN_D;
    }
    const int an = anchor < 0 ? 0 : anchor;
    const double a_bsic = __shfl(bsic, an, 64), a_fn = __shfl(fnd, an, 64), a_pos = __shfl(p, an, 64);
    if (lane == 0) {
        const bool good = status == 0;
        o[GSMCAL_C_NUM_SCH] = (double)nb;
        o[GSMCAL_C_NUM_OK] = (double)num_ok;
        o[GSMCAL_C_NUM_CONSISTENT] = (double)best;
        o[GSMCAL_C_BSIC] = good ? a_bsic : -1.0;
        o[GSMCAL_C_FN_ANCHOR] = good ? a_fn : -1.0;
        o[GSMCAL_C_POS_ANCHOR] = good ? a_pos : -1.0;
        o[GSMCAL_C_STATUS] = (double)status;
        o[GSMCAL_C_MEAN_SLOPE] = num_ok > 0 ? acc / (double)num_ok : NAN_D;
    }
}

// ------------------------------------------------------------------------------------------------
// BCCH_decode -- the system information in the BCCH blocks: which cell this is.  The project's own function:
// BCCH_demod.m stops at the training sequence index; the definition is DESIGN 17's and tests/bcch_decode_ref.py restates it.
//
// k_bcch_decode: grid (MAXH, D), block 256 -- one workgroup per block slot, wave w takes burst w of the block.  Every wave finds
// the blockIdx.x-th block row (PosBlock) of its stream's pos_info itself; its bursts start at rows +1..+4 (1-based starts p).
// delta = (5 ov - 1) div 2.  A block that is absent, or of which one burst would read outside the stream or has p NaN or < 1,
// writes its empty record and returns before the barrier (the decision is the same in all four waves).
//   1  y_k = s(p + k ov + delta) (-j)^k, k = 3..144: 142 strided reads.  Lane l keeps k = 3 + l, 67 + l and (l < 14) 131 + l in
//      registers: nothing of the detector goes through LDS, so no wave waits for another one's stores before the one barrier.
//   2  pass 0: every lane adds its own mid-amble symbols y_{61+i} a_i (a_i = 1 - 2 TSC[tsc][i], bits of BD_TSC_MASK), six
//      xor-shuffle steps leave h in every lane: one fixed order.  amp = |h| / 26, soft_k = Re(y_k conj(h)/|h|).
//   3  two refinements: b_k = sign(soft_k) (+1 at zero), a_{k-61} inside the mid-amble; g1 (k <= 73), g2 (k >= 74) by the same
//      lane-strided partial sums and xor-shuffle tree; slope = angle(g2 conj(g1)) / 71;
//      soft_k = Re(y_k conj(g)/|g| exp(-j slope (k - 73.5))).
//   4  each wave stores its 114 data values at their places c(0..455) of the coded word in LDS (bd_coded_index: the inverse of
//      the interleaver, the one table to pin), counts its mid-amble errors and the two stealing flags from ballots, and leaves
//      {ts_err, steal, slope, amp} in LDS.  ONE barrier; waves 1..3 are done.
//   5  wave 0: the trellis (VtLane) over 228 steps.  The survivor no longer fits a register: the low 16 bits of __ballot(take)
//      are the step's decision word, stored by lane 0 (456 bytes of LDS), and lane 0 traces back from state 0 into four 64-bit
//      registers that one __shfl hands to the wave.  No atomics, no global traceback memory, no scratch.
//   6  integer work: corrected by vt_corrected, the Fire remainder of u(0..223) (a 40-bit shift
//      register), the tail bits, and lanes 0..22 pack one octet each (bit k of octet n = u(8n + k)).
// part[s][slot][BD_PART] = {evaluated, ok, corrected, ts_err, steal, mean_slope, amp, pos}; oct_out[s][slot][23]: zeros unless ok;
// optional soft_out[s][slot][456]: the de-interleaved soft values, NaN for a slot that was not evaluated.  Every workgroup writes
// all of its slot's outputs.
// ------------------------------------------------------------------------------------------------
#define BD_PART 8
#define BD_FIRE_POLY 0x10004820009ull            /* g(D) = D^40 + D^26 + D^23 + D^17 + D^3 + 1 */
#define BD_FIRE_ONES 0xffffffffffull

// bit i = TSC[code][i] (GSM 05.02 table 5.2.3a; synth.TSC)
__device__ const unsigned BD_TSC_MASK[8] = {0x3a443a4u, 0x3b47bb4u, 0x1c25dc2u, 0x1e22de2u, 0x3582758u, 0x1720d72u, 0x3e51be5u, 0x0f748f7u};

// data bit i(B, j), j = 0..113 -> the coded bit c(k) it carries: k mod 4 = B, j = 2 ((49 k) mod 57) + ((k mod 8) div 4)
// (GSM 05.03 4.1.4; synth.bcch_interleave_map).  49 * 7 = 1 (mod 57), so k mod 57 = 7 (j div 2) mod 57, and k mod 8 = B + 4 (j mod 2).
__device__ __forceinline__ int bd_coded_index(int B, int j) {
    const int r57 = (7 * (j >> 1)) % 57;
    return r57 + 57 * ((B + 4 * (j & 1) - r57) & 7);
}
__device__ __forceinline__ unsigned bd_u(unsigned long long u0, unsigned long long u1, unsigned long long u2, unsigned long long u3, int k) {
    const unsigned long long w = k < 64 ? u0 : k < 128 ? u1 : k < 192 ? u2 : u3;
    return k < 0 ? 0u : (unsigned)(w >> (k & 63)) & 1u;
}

__global__ void __launch_bounds__(256) k_bcch_decode(const cplx* __restrict__ r, long stride, const long* __restrict__ r_len,
                                                     const double* __restrict__ pos_info, int ov, const int* __restrict__ tsc,
                                                     double* __restrict__ part, unsigned char* __restrict__ oct_out,
                                                     double* __restrict__ soft_out) {
    __shared__ double cs[456];
    __shared__ double bstat[4][4];
    __shared__ unsigned short dec[228];
    const int s = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t slot = (size_t)s * MAXH + b;
    double* out = part + slot * BD_PART;
    const long len = stream_len(r_len, s, stride);
    const double* pi = pos_info + (size_t)s * 2 * MAXROWS;
    int row;                                                           // the b-th block row
    const int nb = pos_row_select(pi, lane, b, PosBlock(), row);
    const int dl = (5 * ov - 1) / 2;
    // any of the four p NaN or < 1, or its symbol 144 behind the last sample: the block is not evaluated (uniform in the workgroup)
    bool evaluated = len >= 1 && row >= 0 && nb <= MAXH;
    if (evaluated)
        for (int q = 1; q <= 4; ++q) {
            const double pq = pi[row + q];
            evaluated = evaluated && pq >= 1.0 && pq + (double)(144 * ov + dl) <= (double)len;
        }
    if (!evaluated) {
        if (tid == 0) out[0] = 0.0;
        else if (tid < BD_PART) out[tid] = NAN_D;
        if (tid < 23) oct_out[slot * 23 + tid] = 0;
        if (soft_out)
            for (int k = tid; k < 456; k += 256) soft_out[slot * 456 + k] = NAN_D;
        return;
    }
    // ---- 1  this wave's burst: 142 symbols, derotated, three per lane ----
    const double spd = pi[row + 1 + w];
    const cplx* x = r + (size_t)s * stride + ((long)spd - 1 + dl);
    const unsigned mask = BD_TSC_MASK[tsc[s] & 7];
    cplx y[3];
    double a[3], soft[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const int k = 3 + lane + 64 * m;
        y[m] = make_double2(0.0, 0.0);
        a[m] = 0.0;
        if (k <= 144) {
            y[m] = vt_derotate(x[(long)k * ov], k);
            if (k >= 61 && k <= 86) a[m] = (mask >> (k - 61)) & 1u ? -1.0 : 1.0;
        }
    }
    // ---- 2  pass 0: constant phase from the mid-amble ----
    double hx = 0.0, hy = 0.0;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        hx += y[m].x * a[m];
        hy += y[m].y * a[m];
    }
    for (int off = 32; off > 0; off >>= 1) {
        hx += __shfl_xor(hx, off, 64);
        hy += __shfl_xor(hy, off, 64);
    }
    const double mag = hypot(hx, hy), amp = mag / 26.0;
    {
        const cplx q = make_double2(hx / mag, -hy / mag);              // conj(h)/|h|
#pragma unroll
        for (int m = 0; m < 3; ++m) soft[m] = y[m].x * q.x - y[m].y * q.y;
    }
    // ---- 3  two decision-directed refinements over the whole burst ----
    double slope = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        double g1x = 0.0, g1y = 0.0, g2x = 0.0, g2y = 0.0;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const int k = 3 + lane + 64 * m;
            if (k <= 144) {
                const double bk = a[m] != 0.0 ? a[m] : soft[m] >= 0.0 ? 1.0 : -1.0;
                if (k <= 73) { g1x += y[m].x * bk; g1y += y[m].y * bk; }
                else { g2x += y[m].x * bk; g2y += y[m].y * bk; }
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            g1x += __shfl_xor(g1x, off, 64);
            g1y += __shfl_xor(g1y, off, 64);
            g2x += __shfl_xor(g2x, off, 64);
            g2y += __shfl_xor(g2y, off, 64);
        }
        const double gx = g1x + g2x, gy = g1y + g2y, gm = hypot(gx, gy);
        slope = atan2(g2y * g1x - g2x * g1y, g2x * g1x + g2y * g1y) / 71.0;
        const cplx wq = make_double2(gx / gm, -gy / gm);               // conj(g)/|g|
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            double sn, cn;
            sincos(slope * ((double)(3 + lane + 64 * m) - 73.5), &sn, &cn);
            const cplx q = cmul(wq, make_double2(cn, -sn));
            soft[m] = y[m].x * q.x - y[m].y * q.y;
        }
    }
    // ---- 4  de-interleave into the coded word; mid-amble errors and stealing flags ----
    int ts_err = 0, steal = 0;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const int k = 3 + lane + 64 * m;
        const bool data0 = k <= 59, data1 = k >= 88 && k <= 144;
        if (data0 || data1) cs[bd_coded_index(w, data0 ? k - 3 : k - 31)] = soft[m];
        ts_err += __popcll(__ballot(a[m] != 0.0 && (soft[m] < 0.0) != (a[m] < 0.0)));
        steal += __popcll(__ballot((k == 60 || k == 87) && soft[m] < 0.0));
    }
    if (lane == 0) {
        bstat[w][0] = (double)ts_err;
        bstat[w][1] = (double)steal;
        bstat[w][2] = slope;
        bstat[w][3] = amp;
    }
    __syncthreads();
    if (w != 0) return;
    // ---- 5  the trellis; the decisions of a step are one word in LDS ----
    VtLane vt(lane);
    for (int k = 0; k < 228; ++k) {
        const unsigned long long word = __ballot(vt.acs(cs[2 * k], cs[2 * k + 1]));
        if (lane == 0) dec[k] = (unsigned short)word;                  // bit ns: state ns came from its predecessor p1
    }
    unsigned long long u0 = 0, u1 = 0, u2 = 0, u3 = 0;                // u(k) = bit k & 63 of word k >> 6
    if (lane == 0) {                                                   // trace back from state 0 (the writer reads its own stores)
        int st = 0;
        for (int k = 227; k >= 192; --k) { u3 |= (unsigned long long)(st >> 3) << (k - 192); st = ((st & 7) << 1) | ((dec[k] >> st) & 1); }
        for (int k = 191; k >= 128; --k) { u2 |= (unsigned long long)(st >> 3) << (k - 128); st = ((st & 7) << 1) | ((dec[k] >> st) & 1); }
        for (int k = 127; k >= 64; --k) { u1 |= (unsigned long long)(st >> 3) << (k - 64); st = ((st & 7) << 1) | ((dec[k] >> st) & 1); }
        for (int k = 63; k >= 0; --k) { u0 |= (unsigned long long)(st >> 3) << k; st = ((st & 7) << 1) | ((dec[k] >> st) & 1); }
    }
    u0 = sd_shfl_u64(u0, 0);
    u1 = sd_shfl_u64(u1, 0);
    u2 = sd_shfl_u64(u2, 0);
    u3 = sd_shfl_u64(u3, 0);
    // ---- 6  hard channel bits against the re-encoded word; the Fire code; the octets ----
    const int corrected = vt_corrected(456, lane, [&](int j) { return cs[j]; }, [&](int k) { return bd_u(u0, u1, u2, u3, k); });
    unsigned long long reg = 0;                                        // u(0..223) divided by g(D): the remainder must be all ones
    for (int k = 0; k < 224; ++k) {
        reg = (reg << 1) | bd_u(u0, u1, u2, u3, k);
        if (reg >> 40) reg ^= BD_FIRE_POLY;
    }
    const bool ok = reg == BD_FIRE_ONES && (u3 >> 32) == 0ull;         // ... and u(224..227) = 0
    if (lane < 23) {
        const unsigned long long wd = lane < 8 ? u0 : lane < 16 ? u1 : u2;
        oct_out[slot * 23 + lane] = ok ? (unsigned char)(wd >> ((lane & 7) * 8)) : (unsigned char)0;
    }
    if (soft_out)
        for (int k = lane; k < 456; k += 64) soft_out[slot * 456 + k] = cs[k];
    if (lane == 0) {
        out[0] = 1.0;
        out[1] = ok ? 1.0 : 0.0;
        out[2] = (double)corrected;
        out[3] = ((bstat[0][0] + bstat[1][0]) + bstat[2][0]) + bstat[3][0];
        out[4] = ((bstat[0][1] + bstat[1][1]) + bstat[2][1]) + bstat[3][1];
        out[5] = (((bstat[0][2] + bstat[1][2]) + bstat[2][2]) + bstat[3][2]) / 4.0;
        out[6] = (((bstat[0][3] + bstat[1][3]) + bstat[2][3]) + bstat[3][3]) / 4.0;
        out[7] = pi[row + 1];
    }
}

// k_bcch_decode_finish: one wave per stream, grid D, block 64.  out[s] = one row of GSMCAL_SI_COLS doubles (GSMCAL_I_*), written
// here and nowhere else.  Lane i holds the i-th block.  status 0 iff at least one block is ok -- a 40-bit code is evidence on its
// own -- otherwise GSMCAL_S_BCCH_NO_DECODE; first_ok: the 1-based index of the first ok block, -1 without one.
//   r_len < 1 or every element of pos_info -1        status GSMCAL_S_POST_NO_POS, num_blocks 0
//   more than MAXH blocks                            status GSMCAL_E_CAPACITY, nothing evaluated
__global__ void __launch_bounds__(64) k_bcch_decode_finish(const long* __restrict__ r_len, long stride,
                                                           const double* __restrict__ pos_info, const double* __restrict__ part,
                                                           double* __restrict__ out) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const double* pi = pos_info + (size_t)s * 2 * MAXROWS;
    const double* ps = part + (size_t)s * MAXH * BD_PART;
    double* o = out + (size_t)s * GSMCAL_SI_COLS;
    int nb = pos_rows_count(pi, lane, PosBlock());
    int status = stream_head(r_len, s, stride, pi, lane).status(nb, MAXH);
    const bool mine = status == 0 && lane < nb;
    const bool ev = mine && ps[lane * BD_PART] == 1.0;
    const bool ok = ev && ps[lane * BD_PART + 1] == 1.0;
    const unsigned long long okm = __ballot(ok);
    if (status == 0 && okm == 0ull) status = GSMCAL_S_BCCH_NO_DECODE;
    if (lane < MAXH) {
        o[GSMCAL_I_OK + lane] = ev ? (ok ? 1.0 : 0.0) : NAN_D;
        o[GSMCAL_I_POS + lane] = ev ? ps[lane * BD_PART + 7] : NAN_D;
        o[GSMCAL_I_CORRECTED + lane] = ev ? ps[lane * BD_PART + 2] : NAN_D;
        o[GSMCAL_I_TS_ERR + lane] = ev ? ps[lane * BD_PART + 3] : NAN_D;
        o[GSMCAL_I_STEAL + lane] = ev ? ps[lane * BD_PART + 4] : NAN_D;
        o[GSMCAL_I_MEAN_SLOPE + lane] = ev ? ps[lane * BD_PART + 5] : NAN_D;
        o[GSMCAL_I_AMP + lane] = ev ? ps[lane * BD_PART + 6] : NAN_D;
    }
    if (lane == 0) {
        o[GSMCAL_I_NUM_BLOCKS] = (double)nb;
        o[GSMCAL_I_NUM_OK] = (double)__popcll(okm);
        o[GSMCAL_I_STATUS] = (double)status;
        o[GSMCAL_I_FIRST_OK] = okm ? (double)__ffsll((long long)okm) : -1.0;
    }
}
