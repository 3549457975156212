// Host program (own main; built and run by tests/test_chain_ops_cpu.py with -fsanitize=address,undefined -ffp-contract=off): the
// plain part of csrc/chain_ops.h against LITERAL copies of the spellings it replaced in gather_core, burst_gather_fast,
// sch_gather_fast, st_range, stage_raw, k_stream_tile and k_stream_tile_s47 -- the copies below are the point of this file and
// must not be "cleaned up" into calls of the header.  Nothing here touches a GPU.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "chain_ops.h"

static std::atomic<long> fails{0};
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            if (fails < 20) { printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
            ++fails;                                                            \
        }                                                                       \
    } while (0)

// ---- the former spellings ------------------------------------------------------------------------------------------------
// gather_core's backward range propagation (one LERP level)
static void old_range_gather_core(long& clo, long& chi, double f, long nprev) {
    clo = (long)floor((double)clo * f);
    const long h = (long)floor((double)chi * f) + 1;
    chi = h > nprev - 1 ? nprev - 1 : h;
}
// burst_gather_fast / sch_gather_fast: level 0 from level 1
static void old_range_fast(long lo1, long hi1, double f1, long n0, long& lo0_out, long& hi0_out) {
    const long lo0 = (long)floor((double)lo1 * f1);
    long hi0 = (long)floor((double)hi1 * f1) + 1;
    hi0 = hi0 > n0 - 1 ? n0 - 1 : hi0;
    lo0_out = lo0; hi0_out = hi0;
}
// st_range: level 2 from level 3
static void old_range_st(long lo3, long hi3, double f3, long n2, long& lo2, long& hi2) {
    lo2 = (long)floor((double)lo3 * f3);
    hi2 = (long)floor((double)hi3 * f3) + 1;
    if (hi2 > n2 - 1) hi2 = n2 - 1;
}
// lerp_pos as the kernels had it (the build has contraction off)
static double old_lerp_pos(double k, double f) { return k * f; }
// interp1 index and weight through a 64-bit index (gather_core, burst_gather_fast, sch_gather_fast): absolute indices i0, i1
static void old_tap_long(long k, double p, long phi, long& i0, long& i1, double& t) {
    const double xq = old_lerp_pos((double)k, p);
    i0 = (long)floor(xq);
    i1 = i0 + 1 > phi ? phi : i0 + 1;
    t = xq - (double)i0;
}
// ... and through doubles (k_stream_tile, k_stream_tile_s47): indices relative to the source's first sample
static void old_tap_double(double dlo_out, int i, double f, double dlo_src, int last, int& j0, int& j1, double& t) {
    const double xq = old_lerp_pos(dlo_out + (double)i, f);
    const double j0f = floor(xq);
    j0 = (int)(j0f - dlo_src);
    j1 = j0 + 1 > last ? last : j0 + 1;
    t = xq - j0f;
}
// stage_raw's / k_stream_tile's alignment and chunk count
static void old_align_stage_raw(long ao, long first, int span, long& first_al, int& nchunk) {
    long m = (first + ao) % 8;
    if (m < 0) m += 8;
    first_al = first - m;
    nchunk = (int)((first + span - first_al + 7) >> 3);
}
// sch_gather_fast's: chunks that cover staged entries 0 .. span+7
static int old_nchunk_sch(long ao, long first, int span) {
    long m = (first + ao) % 8;
    if (m < 0) m += 8;
    return (int)((m + span + 8 + 7) >> 3);
}
// k_stream_tile_s47's count (its first_al came from raw_first_al already)
static int old_nchunk_s47(long first, int cnt0, int ntp, long first_al) { return (int)((first + cnt0 + ntp - 1 - first_al + 7) >> 3); }
// the rotator table's slot map and arguments (gather_core, burst_gather_fast, sch_gather_fast)
static int old_rot_slot(int i, int na) { return i == 0 ? 0 : (i <= na ? i : 1 + GC_ROT_A + (i - 1 - na)); }

static bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }

// ---- 1 + 2: ranges and index spellings -------------------------------------------------------------------------------------
static const double F[] = {1.0, 1.0 + 1e-9, 1.0 - 1e-9, 1.0 + 300e-6, 1.0 - 300e-6, 1.0 + 440e-6, 1.0 - 440e-6, 1.0 + 4400e-6, 1.0 - 4400e-6};
static void check_ranges_and_taps_of(double f, long* windows_out, long* taps_out) {      // one factor: the factors run side by side
    const long n = 1100000;                                      // length of the level the windows lie in
    std::vector<int> lens;
    for (int ov = 1; ov <= 16; ++ov) lens.push_back(148 * ov);
    lens.push_back(1000); lens.push_back(1016);
    std::vector<long> starts;
    starts.push_back(0); starts.push_back(1);
    for (long d = 70; d >= 1; --d) starts.push_back(n - d);
    for (int q = 0; q < 2000; ++q) starts.push_back((long)(((double)q + 0.37) * (1.1e6 / 2000.0)));
    long windows = 0, taps = 0;
    {
        for (int len : lens)
            for (long lo : starts) {
                const long hi = lo + len - 1;
                const long h_unclamped = (long)floor((double)hi * f) + 1;
                const long NP[] = {h_unclamped + 1, h_unclamped, h_unclamped + 1000000};    // n_prev at, one below, far above the unclamped end
                LerpRange rr[3];
                for (int v = 0; v < 3; ++v) {
                    const long n_prev = NP[v];
                    const LerpRange r = lerp_src_range(lo, hi, f, n_prev);
                    rr[v] = r;
                    long a = lo, b = hi;
                    old_range_gather_core(a, b, f, n_prev);
                    CHECK(a == r.lo && b == r.hi, "gather_core f %.17g lo %ld len %d n_prev %ld", f, lo, len, n_prev);
                    old_range_fast(lo, hi, f, n_prev, a, b);
                    CHECK(a == r.lo && b == r.hi, "fast f %.17g lo %ld len %d n_prev %ld", f, lo, len, n_prev);
                    old_range_st(lo, hi, f, n_prev, a, b);
                    CHECK(a == r.lo && b == r.hi, "st_range f %.17g lo %ld len %d n_prev %ld", f, lo, len, n_prev);
                    CHECK(r.hi <= n_prev - 1 && r.lo <= r.hi, "clamp f %.17g lo %ld len %d n_prev %ld", f, lo, len, n_prev);
                }
                CHECK(rr[0].hi == h_unclamped && rr[1].hi == h_unclamped - 1 && rr[2].hi == rr[0].hi && rr[2].lo == rr[0].lo && rr[1].lo == rr[0].lo, "ends f %.17g lo %ld len %d", f, lo, len);
                ++windows;
                // every output of the window, against each of the three source ranges: the header's index stage, the two
                // former spellings, and where the two samples lie
                const double dlo = (double)lo;
                for (int i = 0; i < len; ++i) {
                    const long k = lo + i;
                    ++taps;
                    for (int v = 0; v < 2; ++v) {             // (rr[2] is rr[0]: checked above)
                        const LerpRange r = rr[v];
                        const int last = (int)(r.hi - r.lo);
                        const LerpTap p = lerp_tap((double)k, f, (double)r.lo, last);
                        long i0, i1; double tl;
                        old_tap_long(k, f, r.hi, i0, i1, tl);
                        int j0, j1; double td;
                        old_tap_double(dlo, i, f, (double)r.lo, last, j0, j1, td);
                        if (!(p.j0 == j0 && p.j1 == j1 && same_bits(p.t, td) && i0 - r.lo == j0 && i1 - r.lo == j1 && same_bits(tl, td)))
                            CHECK(false, "spellings f %.17g k %ld: header %d %d %.17g long %ld %ld %.17g double %d %d %.17g", f, k, p.j0, p.j1, p.t,
                                  i0 - r.lo, i1 - r.lo, tl, j0, j1, td);
                        if (!(p.j0 >= 0 && p.j0 <= last && p.j1 >= p.j0 && p.j1 <= last && p.t >= 0.0 && p.t < 1.0))
                            CHECK(false, "inside f %.17g k %ld range [%ld, %ld]: %d %d %.17g", f, k, r.lo, r.hi, p.j0, p.j1, p.t);
                        if (i == 0 && p.j0 != 0) CHECK(false, "lower end not attained f %.17g lo %ld", f, lo);
                    }
                }
            }
    }
    *windows_out = windows; *taps_out = taps;
}
static void check_ranges_and_taps() {
    constexpr int NF = sizeof(F) / sizeof(F[0]);
    long windows[NF], taps[NF];
    std::vector<std::thread> th;
    for (int q = 0; q < NF; ++q) th.emplace_back(check_ranges_and_taps_of, F[q], &windows[q], &taps[q]);
    long w = 0, t = 0;
    for (int q = 0; q < NF; ++q) { th[q].join(); w += windows[q]; t += taps[q]; }
    printf("ranges: %ld windows x 3 source lengths, %ld outputs: three former range spellings and two former index spellings agree with the header\n", w, t);
}

// ---- 3: raw chunk cover -----------------------------------------------------------------------------------------------------
static void check_chunk_cover() {
    long cases = 0;
    std::vector<long> firsts;
    for (long f = -60; f <= 60; ++f) firsts.push_back(f);
    for (long f = 1000000 - 60; f <= 1000000 + 60; ++f) firsts.push_back(f);
    for (long ao = 0; ao < 8; ++ao)
        for (long first : firsts) {
            const long fa = raw_first_al(first, ao);
            CHECK(fa <= first && first - fa < 8, "first_al %ld first %ld ao %ld", fa, first, ao);
            CHECK(((fa + ao) % 8 + 8) % 8 == 0, "alignment first_al %ld ao %ld", fa, ao);
            for (int span = 1; span <= 2200; ++span) {
                const int nc = raw_nchunk(first, span, fa);
                ++cases;
                // chunks 0 .. nc-1 cover [first, first + span), and the last one is needed
                if (!(fa + 8L * nc >= first + span && fa + 8L * (nc - 1) < first + span && nc >= 1))
                    CHECK(false, "cover first %ld span %d ao %ld: first_al %ld nchunk %d", first, span, ao, fa, nc);
                long ofa; int onc;
                old_align_stage_raw(ao, first, span, ofa, onc);
                if (!(ofa == fa && onc == nc)) CHECK(false, "stage_raw first %ld span %d ao %ld", first, span, ao);
                if (span > 8 && old_nchunk_sch(ao, first, span - 8) != nc) CHECK(false, "sch_gather_fast first %ld span %d ao %ld", first, span, ao);
                if (span >= 47 && old_nchunk_s47(first, span - 46, 47, fa) != nc) CHECK(false, "k_stream_tile_s47 first %ld span %d ao %ld", first, span, ao);
            }
        }
    printf("chunks: %ld (ao, first, span) cases covered exactly, three former counts agree\n", cases);
}

// ---- 4: ffast_chunk on a heap buffer of exactly 2n bytes ---------------------------------------------------------------------
static void check_ffast_chunk() {
    long calls = 0;
    for (long n : {1L, 2L, 7L, 8L, 9L, 15L, 16L, 17L, 40L, 257L}) {
        unsigned short* buf = (unsigned short*)malloc(2 * (size_t)n);      // the sanitizer faults on any read outside it
        for (long i = 0; i < n; ++i) buf[i] = (unsigned short)(0x8000u | (unsigned)(i * 2654435761u >> 17));   // never 0
        for (long g0 = -16; g0 <= n + 16; ++g0) {
            const uint4 v = ffast_chunk(buf, g0, n);
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
            ++calls;
            for (int u = 0; u < 8; ++u) {
                const unsigned got = (w[u >> 1] >> (16 * (u & 1))) & 0xFFFFu;
                const long g = g0 + u;
                const unsigned want = (g >= 0 && g < n) ? buf[g] : 0u;
                if (got != want) CHECK(false, "ffast_chunk n %ld g0 %ld u %d: %u != %u", n, g0, u, got, want);
            }
        }
        free(buf);
    }
    const cplx z = iq_of(0xABCD12FFu, 127.5, 0.25);              // only the low 16 bits count: I = 0xFF, Q = 0x12
    CHECK(z.x == 255.0 - 127.5 && z.y == 18.0 - 0.25, "iq_of %g %g", z.x, z.y);
    printf("ffast_chunk: %ld calls, zero fill exact, no read outside the stream\n", calls);
}

// ---- 5: rotator slots ----------------------------------------------------------------------------------------------------------
static void check_rot_table() {
    const long k0 = 600000;
    const double c = 1.0e-3 + 1.0 / 3.0e6;
    double worst = 0.0;
    for (int cnt = 1; cnt <= 32 * GC_ROT_A; ++cnt) {
        cplx* T = (cplx*)malloc(sizeof(cplx) * GC_ROT_N);        // exactly the table: a slot outside it is a sanitizer fault
        for (int i = 0; i < GC_ROT_N; ++i) T[i] = make_double2(NAN, NAN);
        const int na = rot_na(cnt), step = (cnt % 3 == 0) ? 64 : (cnt % 3 == 1 ? 256 : 512);
        std::vector<int> hit(GC_ROT_N, 0);
        for (int e = 0; e < 1 + na + 32; ++e) {
            const int sl = rot_slot(e, na);
            CHECK(sl == old_rot_slot(e, na), "slot map cnt %d e %d", cnt, e);
            CHECK(sl >= 0 && sl < GC_ROT_N, "slot %d outside the table, cnt %d e %d", sl, cnt, e);
            if (sl >= 0 && sl < GC_ROT_N) ++hit[sl];
        }
        for (int i = 0; i < GC_ROT_N; ++i) CHECK(hit[i] <= 1, "slot %d written %d times, cnt %d", i, hit[i], cnt);
        for (int first = 0; first < step; ++first) rot_table_fill(T, k0, c, cnt, first, step);     // the lanes of a workgroup
        int written = 0;
        for (int i = 0; i < GC_ROT_N; ++i) {
            const bool w = T[i].x == T[i].x;
            written += w;
            CHECK(w == (hit[i] == 1), "slot %d cnt %d: written %d, mapped %d", i, cnt, (int)w, hit[i]);
        }
        CHECK(written == 1 + na + 32, "cnt %d: %d slots written", cnt, written);
        for (int i = 0; i < cnt; i += (cnt > 64 && i > 32 && i < cnt - 33) ? 7 : 1) {   // every slot a read can name is named
            const cplx r = rot_at(T, i);
            if (!(r.x == r.x && r.y == r.y)) { CHECK(false, "rot_at(%d) reads an unwritten slot, cnt %d", i, cnt); continue; }
            const double e = hypot(r.x - cos((double)(k0 + i) * c), r.y - sin((double)(k0 + i) * c));
            if (e > worst) worst = e;
        }
        for (int i = 0; i < cnt; ++i) CHECK(hit[1 + (i >> 5)] == 1 && hit[1 + GC_ROT_A + (i & 31)] == 1, "rot_at(%d) slot not written, cnt %d", i, cnt);
        free(T);
    }
    CHECK(worst < 1e-12, "rotator error %g", worst);             // < 2 ulp(k c) = 2.3e-13 at k c = 600 rad, plus three sincos and two products
    printf("rotators: cnt 1 .. %d, slots distinct and inside %d, every read written; worst |rot_at - exp(1i k c)| = %.3g\n", 32 * GC_ROT_A, GC_ROT_N, worst);
}

int main() {
    check_ranges_and_taps();
    check_chunk_cover();
    check_ffast_chunk();
    check_rot_table();
    if (fails) { printf("chain_ops: %ld FAILED\n", fails.load()); return 1; }
    printf("chain_ops ok\n");
    return 0;
}
