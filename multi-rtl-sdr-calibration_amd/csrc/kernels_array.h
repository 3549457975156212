// kernels_array.h -- optimal combining: the spatial covariance of up to 64 aligned streams over a list of windows, and
// the beams w^H x of up to 16 weight vectors.  The project's own functions; tests/array_ref.py restates them.
//
//   cov[w][i][j] = sum_{n = start_w}^{start_w + len_w - 1} x_i[n] conj(x_j[n])          x_i = row rows[i] of x, fp64, not divided by len
//   out[b][n]    = sum_g conj(weights[b][g]) x_g[n]                                      g in list order
//
// k_array_cov: one workgroup per (window, chunk of AC_CHUNK samples counted from the window's own start).  The matrix is cut into
// 4 x 4 blocks; a lane owns one block of the upper triangle (block row <= block column: 136 of them at G = 64; the other lanes of
// the 256 only help staging) and keeps its sixteen complex sums in 64 VGPRs.  The workgroup stages AC_SLICE samples of all G rows
// into LDS -- every input sample is fetched from HBM once per window that covers it; the next slice's values are already in flight
// into registers while the current one is walked -- and every lane then walks the slice: per sample it reads the four values of
// its block row and the four of its block column (8 x 16 bytes) for 64 multiply-adds.  All lanes of a wave read the same
// sample, so the LDS image is [sample][slot] with slot = (row % 4) * NB + row / 4: for one value of row % 4 the sixteen block
// indices a wave can ask for lie in 256 contiguous bytes, one 16-byte bank group each; the sample stride is one slot more than the
// row count, which spreads the staging stores (consecutive lanes = consecutive samples of one row) over the banks.  The vector
// form was chosen over v_mfma_f64_16x16x4_f64 on the stacked 2G real rows: the matrix instruction shares the vector pipe's fp64
// lanes (profiles/NOTES_r06.md), so it would save operand traffic that at 8 reads per 64 multiply-adds is not the limit, and the
// vector form keeps the summation order readable: per entry, re += ar br, re += ai bi, im += ai br, im -= ar bi, sample after
// sample, each a fused multiply-add.  The chunk's sums go to the workspace; nothing is added across workgroups here (no atomics).
//
// k_array_cov_reduce: one workgroup per (window, 4 x 4 block).  Sixteen lanes fetch one chunk's partial of the block, AC_RED_DEPTH
// chunks at a time; they pass through LDS to the sixteen lanes -- one per entry -- that add them in chunk order, write the entry,
// and write its exact conjugate below the diagonal.  The diagonal's imaginary part is written as +0.
// A window's matrix thus depends on its own samples alone: the same bits wherever it stands in whatever list.
//
// k_array_combine<BT>: lane = one output index n, BT >= B complex sums in registers (BT in {1, 2, 4, 8, 16}), the G x BT weights in
// LDS (every lane reads the same one: a broadcast); x is read once for all beams, the beams are written once with streaming
// stores.  re = fma(wr, xr, re), re = fma(wi, xi, re), im = fma(wr, xi, im), im = fma(-wi, xr, im): the same operations for a beam
// whatever BT, so a beam's row is the same bits alone or among others.
#pragma once
#include "kernels_frontend.h"

#define AC_CHUNK GSMCAL_COV_CHUNK
#define AC_SLICE 32                              /* samples staged per step */
#define AC_MAXG GSMCAL_MAX_ALIGN_MEMBERS
#define AC_COV_LANES 256                         /* >= 136, the 4 x 4 blocks of the upper triangle at G = 64; the rest helps staging */
#define AC_ROWS_PER_PASS (AC_COV_LANES / AC_SLICE)                       /* rows one staging pass of the workgroup covers: 8 */
#define AC_STAGE (AC_MAXG / AC_ROWS_PER_PASS)                            /* staging passes, values a lane holds in flight: 8 */
#define AC_RED_DEPTH 128                         /* chunk partials k_array_cov_reduce has in flight per block of the matrix */
#define AC_BLOCK_ENTRIES 16
#define AC_TILE 256                              /* output samples per workgroup of k_array_combine */

// win: [W + 1][3] longs {start, len, first partial of the window among all the call's chunks} (row W: {0, 0, total}); this launch
// covers the windows [w0, w1) and the partials from part_base on; part: [grid.x][ntri][16] complex.
__global__ void __launch_bounds__(AC_COV_LANES) k_array_cov(const cplx* __restrict__ x, long stride, const int* __restrict__ rows, int G,
                                                            const long* __restrict__ win, int w0, int w1, long part_base,
                                                            cplx* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) cplx xs[AC_SLICE * (AC_MAXG + 1)];
    __shared__ long row_off[AC_MAXG];
    const int tid = threadIdx.x;
    const int NB = (G + 3) >> 2, Gp = NB << 2, ld = Gp + 1, ntri = NB * (NB + 1) / 2;
    // ---- which window and chunk (uniform): the last window whose first partial is <= this one ----
    const long p = part_base + (long)blockIdx.x;
    int lo = w0, hi = w1 - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (win[3 * (long)mid + 2] <= p) lo = mid; else hi = mid - 1;
    }
    const long start = win[3 * (long)lo], len = win[3 * (long)lo + 1];
    const long c0 = (p - win[3 * (long)lo + 2]) * AC_CHUNK;
    const int clen = (int)(len - c0 < AC_CHUNK ? len - c0 : AC_CHUNK);          // (>= 1: the host counts ceil(len / AC_CHUNK) chunks)
    if (tid < G) row_off[tid] = (long)rows[tid] * stride;
    // the slots of the rows G .. Gp - 1 (there to fill the last 4 x 4 blocks) stay zero
    for (int it = tid; it < (Gp - G) * AC_SLICE; it += AC_COV_LANES) {
        const int row = G + it / AC_SLICE;
        xs[(it % AC_SLICE) * ld + (row & 3) * NB + (row >> 2)] = make_double2(0.0, 0.0);
    }
    __syncthreads();
    // ---- this lane's block ----
    const bool active = tid < ntri;
    int bi = 0, rem = active ? tid : 0;
    while (rem >= NB - bi) { rem -= NB - bi; ++bi; }
    const int bj = bi + rem;
    double sr[4][4], si[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) { sr[r][c] = 0.0; si[r][c] = 0.0; }
    // ---- staging: lane -> sample tid % AC_SLICE of the rows tid / AC_SLICE + k AC_ROWS_PER_PASS.  The next slice's values are
    // fetched into registers before the current slice is walked, so that their latency passes behind the arithmetic ----
    const int sn = tid % AC_SLICE, srow = tid / AC_SLICE;
    const cplx* src = x + start + c0 + sn;
    cplx pre[AC_STAGE];
#pragma unroll
    for (int k = 0; k < AC_STAGE; ++k) pre[k] = make_double2(0.0, 0.0);
#define AC_FETCH(s0_)                                                                                   \
    do {                                                                                                \
        const bool in_ = (s0_) + sn < clen;                                                             \
        _Pragma("unroll") for (int k = 0; k < AC_STAGE; ++k) {                                          \
            const int row = srow + k * AC_ROWS_PER_PASS;                                                \
            if (in_ && row < G) pre[k] = src[row_off[row] + (s0_)];                                     \
        }                                                                                               \
    } while (0)
    AC_FETCH(0);
    for (int s0 = 0; s0 < clen; s0 += AC_SLICE) {
        const int cnt = clen - s0 < AC_SLICE ? clen - s0 : AC_SLICE;
        __syncthreads();                                           // the slice before is read
        if (sn < cnt) {
#pragma unroll
            for (int k = 0; k < AC_STAGE; ++k) {
                const int row = srow + k * AC_ROWS_PER_PASS;
                if (row < G) xs[sn * ld + (row & 3) * NB + (row >> 2)] = pre[k];
            }
        }
        __syncthreads();
        if (s0 + AC_SLICE < clen) AC_FETCH(s0 + AC_SLICE);
        if (active) {
#pragma unroll 2
            for (int n = 0; n < cnt; ++n) {
                const cplx* sl = xs + n * ld;
                cplx a[4], b[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) { a[r] = sl[r * NB + bi]; b[r] = sl[r * NB + bj]; }
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        sr[r][c] = fma(a[r].x, b[c].x, sr[r][c]);
                        sr[r][c] = fma(a[r].y, b[c].y, sr[r][c]);
                        si[r][c] = fma(a[r].y, b[c].x, si[r][c]);
                        si[r][c] = fma(-a[r].x, b[c].y, si[r][c]);
                    }
            }
        }
    }
#undef AC_FETCH
    if (active) {
        cplx* o = part + ((size_t)blockIdx.x * ntri + tid) * AC_BLOCK_ENTRIES;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) o[r * 4 + c] = make_double2(sr[r][c], si[r][c]);
    }
}

// grid = (the 4 x 4 blocks of the upper triangle, the windows [w0, w1) of the launch before); cov: [W][G][G] complex.  Sixteen lanes
// (one per entry of the block) fetch one chunk's partial, 256 contiguous bytes; AC_RED_DEPTH chunks are in flight at a time and
// go through LDS to the sixteen lanes that add them up, chunk after chunk.
__global__ void __launch_bounds__(256) k_array_cov_reduce(const cplx* __restrict__ part, const long* __restrict__ win, int w0, long part_base,
                                                          int G, cplx* __restrict__ cov) {
    __shared__ __attribute__((aligned(16))) cplx buf[AC_RED_DEPTH * AC_BLOCK_ENTRIES];
    const int tid = threadIdx.x, e = tid & 15, cl = tid >> 4;
    const int w = w0 + (int)blockIdx.y, blk = (int)blockIdx.x;
    const int NB = (G + 3) >> 2, ntri = NB * (NB + 1) / 2;
    const long first = win[3 * (long)w + 2] - part_base, nch = win[3 * (long)(w + 1) + 2] - win[3 * (long)w + 2];
    const cplx* src = part + ((size_t)first * ntri + blk) * AC_BLOCK_ENTRIES + e;
    const size_t step = (size_t)ntri * AC_BLOCK_ENTRIES;
    double re = 0.0, im = 0.0;
    for (long base = 0; base < nch; base += AC_RED_DEPTH) {
        cplx v[AC_RED_DEPTH / 16];
#pragma unroll
        for (int k = 0; k < AC_RED_DEPTH / 16; ++k) {
            const long ch = base + cl + 16 * k;
            v[k] = ch < nch ? src[(size_t)ch * step] : make_double2(0.0, 0.0);
        }
        __syncthreads();                                           // the round before is added up
#pragma unroll
        for (int k = 0; k < AC_RED_DEPTH / 16; ++k) buf[(cl + 16 * k) * AC_BLOCK_ENTRIES + e] = v[k];
        __syncthreads();
        if (cl == 0) {
            const int m = (int)(nch - base < AC_RED_DEPTH ? nch - base : AC_RED_DEPTH);
            for (int i = 0; i < m; ++i) {                          // in chunk order
                const cplx t = buf[i * AC_BLOCK_ENTRIES + e];
                re += t.x;
                im += t.y;
            }
        }
    }
    if (cl != 0) return;
    int bi = 0, rem = blk;
    while (rem >= NB - bi) { rem -= NB - bi; ++bi; }
    const int i = 4 * bi + (e >> 2), j = 4 * (bi + rem) + (e & 3);
    if (i > j || j >= G) return;                                   // below the diagonal of a diagonal block, or a filler row
    cplx* o = cov + (size_t)w * G * G;
    if (i == j) {
        o[(size_t)i * G + i] = make_double2(re, 0.0);
    } else {
        o[(size_t)i * G + j] = make_double2(re, im);
        o[(size_t)j * G + i] = make_double2(re, -im);
    }
}

// weights: [B][G] complex (device copy of the host array); out: [B][out_len]; n0: the first output index of this launch's first tile
template <int BT>
__global__ void __launch_bounds__(AC_TILE) k_array_combine(const cplx* __restrict__ x, long stride, const int* __restrict__ rows, int G,
                                                           const cplx* __restrict__ weights, int B, long out_len, long n0,
                                                           cplx* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) cplx ws[AC_MAXG * BT];             // [g][b], zero for b >= B
    __shared__ long row_off[AC_MAXG];
    const int tid = threadIdx.x;
    for (int it = tid; it < G * BT; it += AC_TILE) {
        const int g = it / BT, b = it % BT;
        ws[it] = b < B ? weights[(size_t)b * G + g] : make_double2(0.0, 0.0);
    }
    if (tid < G) row_off[tid] = (long)rows[tid] * stride;
    __syncthreads();
    const long n = n0 + (long)blockIdx.x * AC_TILE + tid;
    if (n >= out_len) return;
    double ar[BT], ai[BT];
#pragma unroll
    for (int b = 0; b < BT; ++b) { ar[b] = 0.0; ai[b] = 0.0; }
#pragma unroll 4
    for (int g = 0; g < G; ++g) {
        const cplx v = x[row_off[g] + n];
#pragma unroll
        for (int b = 0; b < BT; ++b) {
            const cplx w = ws[g * BT + b];
            ar[b] = fma(w.x, v.x, ar[b]);
            ar[b] = fma(w.y, v.y, ar[b]);
            ai[b] = fma(w.x, v.y, ai[b]);
            ai[b] = fma(-w.y, v.x, ai[b]);
        }
    }
#pragma unroll
    for (int b = 0; b < BT; ++b)
        if (b < B) st_stream16(out + (size_t)b * out_len + n, make_double2(ar[b], ai[b]));
}
