// Stand-alone driver of csrc/apply_refine.h (the host arithmetic of gsmcal_apply_params_refine) for tests/test_apply_refine_cpu.py:
// built with -fsanitize=address,undefined and run directly.  Nothing of HIP or of the library is linked.
#include <cmath>
#include <cstdio>
#include <vector>

#include "apply_refine.h"

using namespace gsmcal_ar;

static int fails = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++fails; } \
    } while (0)

static bool all_nan_but(const std::vector<double>& v, int keep, double value) {
    for (int i = 0; i < (int)v.size(); ++i)
        if (i == keep ? v[i] != value : v[i] == v[i]) return false;
    return true;
}

int main() {
    // rows of exactly the lengths the header reads: a read past either end is the sanitizer's to find
    const int cols = 20 + 6 * R_WINDOWS;
    std::vector<double> coh(cols, NAN), in(AP_PARAMS, 0.0), out(AP_PARAMS, -7.0);
    coh[R_STATUS] = 0.0;
    coh[R_DELAY0] = -11.328; coh[R_REL_SAMPLING_PPM] = 0.61; coh[R_REL_CARRIER_HZ] = 520.2; coh[R_PHASE0] = 0.098;
    coh[R_WIN_LEN] = 1184.0; coh[R_SAMPLE_RATE] = 2.048e6; coh[R_MIN_COHERENCE] = 0.5;
    const double starts[3] = {2000.0, 11000.0, 20000.0};
    for (int j = 0; j < 3; ++j) { coh[R_START + j] = starts[j]; coh[R_COH + j] = 0.9; coh[R_EDGE + j] = 0.0; }
    const double par[AP_PARAMS] = {-3.25, -30.6, 5380.1, 0.7, 30000.0, 0.37, 127.1, 128.2, 1.07, 0.05};
    in.assign(par, par + AP_PARAMS);
    CHECK(apply_params_refine(coh.data(), in.data(), out.data()) == AR_OK);
    const double two_pi = 6.283185307179586476925286766559, fs = 2.048e6;
    const double s = 1e-6 * 0.61, s1 = 1e-6 * -30.6, A1 = 30000.0, p0 = 2000.0, n_c = p0 + (4.0 * 296.0 - 1.0) / 2.0;
    const double Du = -11.328 + s * (A1 - p0);
    CHECK(out[AP_DELAY] == -3.25 + Du * (1.0 + s1) && out[AP_SLOPE_PPM] == 1e6 * (s + s1 + s * s1) && out[AP_ANCHOR] == A1);
    CHECK(out[AP_CARRIER_HZ] == (5380.1 + 520.2) * (1.0 + s));
    CHECK(out[AP_PHASE] == 0.7 + (two_pi * 5380.1 / fs) * Du + 0.098 + (two_pi * 520.2 * (1.0 + s) / fs) * (A1 - n_c));
    for (int i = AP_SCALE; i < AP_PARAMS; ++i) CHECK(out[i] == par[i]);
    // a measured zero leaves the row as it is (the slope goes through 1e-6 and back: to its last bits)
    coh[R_DELAY0] = 0.0; coh[R_REL_SAMPLING_PPM] = 0.0; coh[R_REL_CARRIER_HZ] = 0.0; coh[R_PHASE0] = 0.0;
    CHECK(apply_params_refine(coh.data(), in.data(), out.data()) == AR_OK);
    for (int i = 0; i < AP_PARAMS; ++i) CHECK(i == AP_SLOPE_PPM ? std::fabs(out[i] - par[i]) <= 1e-13 : out[i] == par[i]);
    // the first USED window: not evaluated (NaN), an edge, below the threshold are passed over -- up to the last entry of the row
    coh[R_DELAY0] = 1.5; coh[R_REL_SAMPLING_PPM] = 2.0;
    coh[R_START + 0] = NAN; coh[R_EDGE + 1] = 1.0; coh[R_COH + 1] = NAN;
    CHECK(apply_params_refine(coh.data(), in.data(), out.data()) == AR_OK);
    CHECK(out[AP_DELAY] == -3.25 + (1.5 + 2e-6 * (A1 - 20000.0)) * (1.0 + s1));
    coh[R_COH + 2] = 0.49;
    coh[R_START + R_WINDOWS - 1] = 70000.0; coh[R_COH + R_WINDOWS - 1] = 0.5; coh[R_EDGE + R_WINDOWS - 1] = 0.0;
    CHECK(apply_params_refine(coh.data(), in.data(), out.data()) == AR_OK);
    CHECK(out[AP_DELAY] == -3.25 + (1.5 + 2e-6 * (A1 - 70000.0)) * (1.0 + s1));
    coh[R_COH + R_WINDOWS - 1] = 0.2;                               // no used window at all
    CHECK(apply_params_refine(coh.data(), in.data(), out.data()) == AR_SKIPPED && all_nan_but(out, AP_SCALE, 0.37));
    coh[R_COH + 2] = 0.9;
    // a status that is not 0, summaries or inputs that are not finite: skipped, all NaN but the scale
    coh[R_STATUS] = 16.0;
    CHECK(apply_params_refine(coh.data(), in.data(), out.data()) == AR_SKIPPED && all_nan_but(out, AP_SCALE, 0.37));
    coh[R_STATUS] = 0.0;
    const int summary[5] = {R_DELAY0, R_REL_SAMPLING_PPM, R_REL_CARRIER_HZ, R_PHASE0, R_SAMPLE_RATE};
    for (int k : summary)
        for (double bad : {(double)NAN, (double)INFINITY}) {
            const double keep = coh[k];
            coh[k] = bad;
            CHECK(apply_params_refine(coh.data(), in.data(), out.data()) == AR_SKIPPED && all_nan_but(out, AP_SCALE, 0.37));
            coh[k] = keep;
        }
    for (int k = 0; k < AP_PARAMS; ++k) {
        in[k] = k & 1 ? NAN : -INFINITY;
        CHECK(apply_params_refine(coh.data(), in.data(), out.data()) == AR_SKIPPED);
        for (int i = 0; i < AP_PARAMS; ++i) CHECK(i == AP_SCALE ? (out[i] == in[i] || (in[i] != in[i] && out[i] != out[i])) : out[i] != out[i]);
        in[k] = par[k];
    }
    // |slope'| beyond 1000 ppm: refused, just inside: taken
    coh[R_REL_SAMPLING_PPM] = 1031.0;
    CHECK(apply_params_refine(coh.data(), in.data(), out.data()) == AR_E_ARG && all_nan_but(out, AP_SCALE, 0.37));
    coh[R_REL_SAMPLING_PPM] = 1030.0;
    CHECK(apply_params_refine(coh.data(), in.data(), out.data()) == AR_OK && std::fabs(out[AP_SLOPE_PPM]) <= 1000.0);
    if (fails == 0) std::printf("apply_refine ok\n");
    return fails ? 1 : 0;
}
