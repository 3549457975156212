// Stand-alone driver of csrc/fc_layout.h (k_fine_cert's LDS carve and lane maps) for tests/test_fc_banks_cpu.py: a host program,
// nothing of HIP or of the library is linked.  It evaluates the LDS bank rule of gfx950 over every step of the slide phase and of
// the E/C scans:
//   ds_read_b128   served in 4 groups of 16 lanes {0-3,12-15,20-27} {4-11,16-19,28-31} {32-35,44-47,52-59} {36-43,48-51,60-63},
//                  64 banks of 4 bytes: bank of byte address a = (a / 4) mod 64
//   ds_write_b64   4 groups of 16 consecutive lanes, bank (a / 4) mod 32
//   ds_write_b32   2 groups of 32 consecutive lanes, bank (a / 4) mod 32
// Lanes of one group that give the same address are served together (broadcast); every further DISTINCT address on a bank that is
// already busy costs the group one more cycle: "ways" below is the largest number of distinct addresses on one bank in one group.
#include <algorithm>
#include <cstdio>
#include <set>
#include <vector>

#include "fc_layout.h"

static int fails = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++fails; } \
    } while (0)

enum Kind { READ_B128, WRITE_B64, WRITE_B32 };
static const int STATIC_LDS = 144;      // FcShared in front of the dynamic LDS

static int group_of(Kind k, int lane) {
    if (k == WRITE_B32) return lane >> 5;
    if (k == WRITE_B64) return lane >> 4;
    static const int g32[32] = {0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1};
    return 2 * (lane >> 5) + g32[lane & 31];
}
// ways of one wave instruction: addr[lane] = byte offset into the dynamic LDS, < 0 = lane masked off
static int ways(Kind k, const long (&addr)[64]) {
    const int nbank = k == READ_B128 ? 64 : 32, width = k == READ_B128 ? 4 : (k == WRITE_B64 ? 2 : 1), ngroup = k == WRITE_B32 ? 2 : 4;
    int worst = 0;
    for (int g = 0; g < ngroup; ++g) {
        std::vector<std::set<long>> on(nbank);
        for (int l = 0; l < 64; ++l) {
            if (addr[l] < 0 || group_of(k, l) != g) continue;
            const long a = addr[l] + STATIC_LDS;
            for (int d = 0; d < width; ++d) on[(a / 4 + d) % nbank].insert(a);
        }
        for (const auto& s : on) worst = std::max(worst, (int)s.size());
    }
    return worst;
}

struct Worst { int slide_read = 0, sums_store = 0, scan_read = 0, et_store = 0, cs_store = 0; };

// every instruction of the two phases for one geometry; chunk_of(tid, nslide) is the slide map under test
template <typename ChunkOf>
static Worst walk(int nshift, int nfft, ChunkOf chunk_of, bool check_cover) {
    const FcCarve cv = fc_carve(nshift, nfft);
    const int nthr = fc_threads(nshift), nslide = fc_nslide(cv.nchunk);
    const long xp = FC_XP(cv.nstep + 2);
    Worst w;
    std::vector<int> seen(cv.nchunk, 0);
    CHECK(nthr % 64 == 0 && nthr >= FC_NB * cv.nchunk && nslide * 64 <= nthr);
    for (int wave = 0; wave < nthr / 64; ++wave) {
        bool any = false;
        for (int q = 0; q < FS_CHUNK; ++q) {
            long a1[64], b1[64], st[64];
            for (int l = 0; l < 64; ++l) {
                const int c = chunk_of(64 * wave + l, nslide);
                a1[l] = b1[l] = st[l] = -1;
                if (c >= cv.nchunk) continue;
                any = true;
                if (q == 0 && (l & (FC_NB - 1)) == 0) ++seen[c];
                const long ia = FC_XP(FS_CHUNK * c + nfft + q), ib = FC_XP(FS_CHUNK * c + q), is = FC_XP(FS_CHUNK * c + q + 1);
                if (check_cover) {
                    CHECK(c >= 0 && chunk_of(64 * wave + l, nslide) == chunk_of(64 * wave + (l & ~(FC_NB - 1)), nslide));   // one chunk per group of 8
                    CHECK(ia < FC_XP(cv.wlen) && (size_t)(ia + 1) * FC_CPLX_BYTES <= cv.reg1);
                    CHECK(is < xp && cv.sumS + (size_t)(is + 1) * sizeof(float) <= cv.Cs);
                }
                a1[l] = (long)cv.xs + ia * FC_CPLX_BYTES;
                b1[l] = (long)cv.xs + ib * FC_CPLX_BYTES;
                st[l] = (long)cv.sumS + is * (long)sizeof(float);
            }
            w.slide_read = std::max(w.slide_read, std::max(ways(READ_B128, a1), ways(READ_B128, b1)));
            w.sums_store = std::max(w.sums_store, ways(WRITE_B32, st));
        }
        if (check_cover) CHECK(any == (wave < nslide));         // the waves behind the slide waves hold no slide lane (the E / C roles)
    }
    if (check_cover)
        for (int c = 0; c < cv.nchunk; ++c) CHECK(seen[c] == 1);
    // the scans: one wave, fc_scan_rounds rounds
    std::vector<int> hit(cv.nstep, 0);
    for (int u = 0; u < fc_scan_rounds(cv.nstep); ++u) {
        long a1[64], b1[64], se[64], sc[64];
        for (int l = 0; l < 64; ++l) {
            const int q = fc_scan_shift(l, u);
            a1[l] = b1[l] = se[l] = sc[l] = -1;
            if (q >= cv.nstep) continue;
            ++hit[q];
            if (check_cover) {
                CHECK((size_t)(FC_XP(q + nfft) + 1) * FC_CPLX_BYTES <= cv.reg1);
                CHECK(cv.Et + (size_t)(q + 1) * sizeof(double) <= cv.reg2);
                CHECK(FC_XP(q) < xp && cv.Cs + (size_t)(FC_XP(q) + 1) * sizeof(float) <= cv.sh_scan);
            }
            a1[l] = (long)cv.xs + (long)FC_XP(q + nfft) * FC_CPLX_BYTES;
            b1[l] = (long)cv.xs + (long)FC_XP(q) * FC_CPLX_BYTES;
            se[l] = (long)cv.Et + (long)q * (long)sizeof(double);
            sc[l] = (long)cv.Cs + (long)FC_XP(q) * (long)sizeof(float);
        }
        w.scan_read = std::max(w.scan_read, std::max(ways(READ_B128, a1), ways(READ_B128, b1)));
        w.et_store = std::max(w.et_store, ways(WRITE_B64, se));
        w.cs_store = std::max(w.cs_store, ways(WRITE_B32, sc));
    }
    if (check_cover) {
        for (int q = 0; q < cv.nstep; ++q) CHECK(hit[q] == 1);
        // the last slots, t = nstep
        CHECK(cv.Et + (size_t)(cv.nstep + 1) * sizeof(double) <= cv.reg2);
        CHECK(FC_XP(cv.nstep) < xp && cv.Cs + (size_t)(FC_XP(cv.nstep) + 1) * sizeof(float) <= cv.sh_scan);
        CHECK(cv.sh_scan2 + 8 * sizeof(double) <= cv.total && cv.total <= cv.launch);
    }
    return w;
}

int main() {
    const auto dealt = [](int tid, int nslide) { return fc_slide_chunk(tid, nslide); };
    const auto consecutive = [](int tid, int) { return tid / FC_NB; };        // the map before: group g of the block walks chunk g
    // the evaluator itself, on known cases: 64 lanes on consecutive 16-byte slots are conflict-free, lanes 256 bytes apart 16-way,
    // one address in every lane a broadcast
    {
        long a[64];
        for (int l = 0; l < 64; ++l) a[l] = 16L * l;
        CHECK(ways(READ_B128, a) == 1);
        for (int l = 0; l < 64; ++l) a[l] = 256L * l;
        CHECK(ways(READ_B128, a) == 16);
        for (int l = 0; l < 64; ++l) a[l] = 4096;
        CHECK(ways(READ_B128, a) == 1 && ways(WRITE_B32, a) == 1);
        for (int l = 0; l < 64; ++l) a[l] = 128L * l;
        CHECK(ways(WRITE_B64, a) == 16);
        for (int l = 0; l < 64; ++l) a[l] = 8L * l;
        CHECK(ways(WRITE_B64, a) == 1);
    }
    // reference geometry (k_fine_cert<8, 47>): every read and store of the two phases is 1-way ...
    const Worst ref = walk(1025, 1184, dealt, true);
    std::printf("ov 8 dealt: slide reads %d-way, sumS stores %d-way, scan reads %d-way, Et stores %d-way, Cs stores %d-way\n",
                ref.slide_read, ref.sums_store, ref.scan_read, ref.et_store, ref.cs_store);
    CHECK(ref.slide_read == 1 && ref.sums_store == 1 && ref.scan_read == 1 && ref.et_store == 1 && ref.cs_store == 1);
    // ... where consecutive chunks side by side were 2-way (what the dealing is for)
    const Worst old = walk(1025, 1184, consecutive, false);
    std::printf("ov 8 consecutive: slide reads %d-way, sumS stores %d-way\n", old.slide_read, old.sums_store);
    CHECK(old.slide_read == 2 && old.sums_store == 2);
    // every ratio the general kernel takes: each chunk and each shift exactly once, no index outside its region; the dealt map is
    // never worse than the consecutive one.  The scans' stores stay 1-way; their x[q + nfft] read is 2-way where nfft mod 128 puts an
    // FC_XP pad step inside a group of 16 lanes (the lanes behind the step move on by one slot, onto the bank group of the group's
    // first lane), never more: a round of 64 shifts crosses at most one step
    for (int ov = 1; ov <= 16; ++ov) {
        const Worst a = walk(128 * ov + 1, 148 * ov, dealt, true), b = walk(128 * ov + 1, 148 * ov, consecutive, false);
        std::printf("ov %2d: %d slide wave(s), slide reads %d-way (consecutive: %d), sumS stores %d-way (%d), scans %d/%d/%d\n", ov,
                    fc_nslide(fc_carve(128 * ov + 1, 148 * ov).nchunk), a.slide_read, b.slide_read, a.sums_store, b.sums_store, a.scan_read,
                    a.et_store, a.cs_store);
        CHECK(a.slide_read <= b.slide_read && a.sums_store <= b.sums_store);
        CHECK(a.scan_read <= 2 && a.et_store == 1 && a.cs_store == 1);
    }
    if (fails) return 1;
    std::printf("fc_banks ok\n");
    return 0;
}
