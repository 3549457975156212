// apply_refine.h -- the host arithmetic of gsmcal_apply_params_refine: one row of the row_coherence table of the pair
// (reference, b), measured on the output rows of a first apply_calibration pass, composed into the parameter row that produced row b.
// A second pass over the same bytes with the composed row lands on the reference row's time base, carrier and phase.  Plain C++:
// nothing of HIP and nothing of the library is included, so a stand-alone program can use it on its own
// (tests/test_apply_refine_cpu.py builds one under the sanitizers).
//
// The first pass read the capture at x1(u) = (u + d1) + s1 (u - A1) and turned output sample u by -(phi1 + w1 (u - A1)), w1 = 2 pi f1 / fs.
// row_coherence says: what belongs at index n of the reference sits at u(n) = n + delay0 + s (n - p0) of row b, with the carrier f
// (Hz of the first pass's time base) and the phase phase0 at the centre n_c = p0 + (4 Ls - 1)/2 of the first used window.  The second
// pass must therefore read the capture at x1(u(n)) -- two affine maps composed -- and take out, next to the first pass's angle AT u(n),
// the measured one: with Du = u(A1) - A1 = delay0 + s (A1 - p0),
//   x1(u(n)) = (n + d1 + Du (1 + s1)) + (s + s1 + s s1)(n - A1)
//   phi1 + w1 (u(n) - A1) = phi1 + w1 Du + w1 (1 + s)(n - A1)
//   phase0 + w (1 + s)(n - n_c),  w = 2 pi f / fs   (the carrier per sample of b turns (1 + s) times as fast per output sample:
//                                                    gsmcal_pair_align_params' reasoning)
// so  delay' = d1 + Du (1 + s1),  slope' = s + s1 + s s1,  anchor' = A1,  carrier_hz' = (f1 + f)(1 + s),
//     phase' = phi1 + w1 Du + phase0 + w (1 + s)(A1 - n_c).
#pragma once
#include <cmath>
#include <limits>

namespace gsmcal_ar {

// the columns read (== GSMCAL_R_*, GSMCAL_AP_* of include/gsmcal.h; gsmcal.hip asserts it)
enum { R_STATUS = 0, R_DELAY0 = 6, R_REL_SAMPLING_PPM = 7, R_REL_CARRIER_HZ = 9, R_PHASE0 = 11, R_WIN_LEN = 16, R_SAMPLE_RATE = 17,
       R_MIN_COHERENCE = 18, R_WINDOWS = 128, R_START = 20, R_COH = 20 + 4 * R_WINDOWS, R_EDGE = 20 + 5 * R_WINDOWS };
enum { AP_DELAY = 0, AP_SLOPE_PPM, AP_CARRIER_HZ, AP_PHASE, AP_ANCHOR, AP_SCALE, AP_DC_I, AP_DC_Q, AP_GAIN, AP_SIN_PHASE, AP_PARAMS };
enum { AR_OK = 0, AR_SKIPPED = 17, AR_E_ARG = -1 };

inline void all_nan_but_scale(const double* params_in, double* params_out) {
    for (int i = 0; i < AP_PARAMS; ++i) params_out[i] = std::numeric_limits<double>::quiet_NaN();
    params_out[AP_SCALE] = params_in[AP_SCALE];
}

// -> AR_OK; AR_SKIPPED or AR_E_ARG (|slope_ppm'| > 1000) with every value of params_out NaN but the scale
inline int apply_params_refine(const double* coh_row, const double* params_in, double* params_out) {
    bool fin = true;
    for (int i = 0; i < AP_PARAMS; ++i) fin = fin && std::isfinite(params_in[i]);
    int first = -1;
    for (int j = 0; j < R_WINDOWS && first < 0; ++j)
        if (coh_row[R_START + j] == coh_row[R_START + j] && coh_row[R_EDGE + j] == 0.0 && coh_row[R_COH + j] >= coh_row[R_MIN_COHERENCE]) first = j;
    const double fs = coh_row[R_SAMPLE_RATE], delay0 = coh_row[R_DELAY0], ppm = coh_row[R_REL_SAMPLING_PPM], f = coh_row[R_REL_CARRIER_HZ],
                 phase0 = coh_row[R_PHASE0];
    if (!fin || !(coh_row[R_STATUS] == 0.0) || first < 0 || !std::isfinite(delay0) || !std::isfinite(ppm) || !std::isfinite(f) ||
        !std::isfinite(phase0) || !std::isfinite(fs) || !(fs > 0.0)) {
        all_nan_but_scale(params_in, params_out);
        return AR_SKIPPED;
    }
    const double two_pi = 6.283185307179586476925286766559;
    const double d1 = params_in[AP_DELAY], s1 = 1e-6 * params_in[AP_SLOPE_PPM], f1 = params_in[AP_CARRIER_HZ], phi1 = params_in[AP_PHASE],
                 A1 = params_in[AP_ANCHOR];
    const double s = 1e-6 * ppm;
    const double p0 = coh_row[R_START + first];
    const double Ls = std::floor(coh_row[R_WIN_LEN] / 4.0);
    const double n_c = p0 + (4.0 * Ls - 1.0) / 2.0;
    const double Du = delay0 + s * (A1 - p0);
    const double slope_ppm = 1e6 * (s + s1 + s * s1);
    if (!(std::fabs(slope_ppm) <= 1000.0)) {
        all_nan_but_scale(params_in, params_out);
        return AR_E_ARG;
    }
    for (int i = 0; i < AP_PARAMS; ++i) params_out[i] = params_in[i];
    params_out[AP_DELAY] = d1 + Du * (1.0 + s1);
    params_out[AP_SLOPE_PPM] = slope_ppm;
    params_out[AP_ANCHOR] = A1;
    params_out[AP_CARRIER_HZ] = (f1 + f) * (1.0 + s);
    params_out[AP_PHASE] = phi1 + (two_pi * f1 / fs) * Du + phase0 + (two_pi * f * (1.0 + s) / fs) * (A1 - n_c);
    return AR_OK;
}

}  // namespace gsmcal_ar
