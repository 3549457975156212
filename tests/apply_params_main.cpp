// Stand-alone driver of csrc/apply_params.h (the host arithmetic of gsmcal_apply_params) for tests/test_apply_params_cpu.py: built
// with -fsanitize=address,undefined and run directly.  Nothing of HIP or of the library is linked.
#include <cmath>
#include <cstdio>
#include <vector>

#include "apply_params.h"

using namespace gsmcal_ap;

static int fails = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++fails; } \
    } while (0)

int main() {
    // rows of exactly the lengths the header reads: a read past either end is the sanitizer's to find
    std::vector<double> table(10, 0.0), iq(22, 0.0), out(AP_PARAMS, -7.0);
    table[T_TOTAL_SAMPLING_PPM] = 63.0;
    table[T_TOTAL_CARRIER_PPM] = -21.5;
    CHECK(apply_params(table.data(), 433.92e6, nullptr, 0.5, -0.25, 2.0, out.data()) == AP_OK);
    const double e = 1e-6 * 63.0, f_off = 1e-6 * -21.5 * 433.92e6;
    CHECK(out[AP_DELAY] == 0.5 && out[AP_SLOPE_PPM] == 63.0 && out[AP_CARRIER_HZ] == f_off * (1.0 + e) && out[AP_PHASE] == -0.25);
    CHECK(out[AP_ANCHOR] == 0.0 && out[AP_SCALE] == 2.0 && out[AP_DC_I] == 127.5 && out[AP_DC_Q] == 127.5 && out[AP_GAIN] == 1.0 && out[AP_SIN_PHASE] == 0.0);
    // the sign: a dongle whose carrier reads high has its surplus taken out, (1 + e) times as fast per output sample
    CHECK(out[AP_CARRIER_HZ] < 0.0 && std::fabs(out[AP_CARRIER_HZ]) > std::fabs(f_off));
    // an I/Q row: DC always, gain and sin_phase at status 0 only
    iq[Q_DC_I] = 126.9; iq[Q_DC_Q] = 128.2; iq[Q_GAIN] = 1.07; iq[Q_SIN_PHASE] = 0.0523; iq[Q_STATUS] = 0.0;
    CHECK(apply_params(table.data(), 433.92e6, iq.data(), 0.0, 0.0, 1.0, out.data()) == AP_OK);
    CHECK(out[AP_DC_I] == 126.9 && out[AP_DC_Q] == 128.2 && out[AP_GAIN] == 1.07 && out[AP_SIN_PHASE] == 0.0523);
    for (double st : {1.0, 2.0}) {                                 // GSMCAL_IQ_SHORT, GSMCAL_IQ_FLAT
        iq[Q_STATUS] = st; iq[Q_GAIN] = NAN; iq[Q_SIN_PHASE] = NAN;
        CHECK(apply_params(table.data(), 433.92e6, iq.data(), 0.0, 0.0, 1.0, out.data()) == AP_OK);
        CHECK(out[AP_DC_I] == 126.9 && out[AP_DC_Q] == 128.2 && out[AP_GAIN] == 1.0 && out[AP_SIN_PHASE] == 0.0);
    }
    // a failed row, or totals that are not finite: all NaN
    const double bad[4][3] = {{63.0, -21.5, 10.0}, {INFINITY, INFINITY, 0.0}, {5.0, NAN, 0.0}, {-INFINITY, 1.0, 0.0}};
    for (const double* b : bad) {
        table[T_TOTAL_SAMPLING_PPM] = b[0]; table[T_TOTAL_CARRIER_PPM] = b[1]; table[T_STATUS] = b[2];
        CHECK(apply_params(table.data(), 1090e6, iq.data(), 1.0, 2.0, 3.0, out.data()) == AP_SKIPPED);
        for (int i = 0; i < AP_PARAMS; ++i) CHECK(std::isnan(out[i]));
    }
    // the largest values the chain can report
    table[T_TOTAL_SAMPLING_PPM] = -1000.0; table[T_TOTAL_CARRIER_PPM] = 4000.0; table[T_STATUS] = 0.0;
    CHECK(apply_params(table.data(), 1.7e9, nullptr, -20.0, 0.0, 1.0, out.data()) == AP_OK);
    CHECK(out[AP_CARRIER_HZ] == 1e-6 * 4000.0 * 1.7e9 * (1.0 + 1e-6 * -1000.0) && out[AP_SLOPE_PPM] == -1000.0);
    if (fails) return 1;
    std::printf("apply_params ok\n");
    return 0;
}
