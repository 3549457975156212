// apply_params.h -- the host arithmetic of gsmcal_apply_params: one row of the calibration table, and optionally one row
// of the I/Q check, -> the parameter row of gsmcal_apply_calibration_batch that undoes them on a capture tuned to tuned_freq.  Plain
// C++: nothing of HIP and nothing of the library is included, so a stand-alone program can use it on its own
// (tests/test_apply_params_cpu.py builds one under the sanitizers).
//
//   e = 1e-6 total_sampling_ppm,  f_off = 1e-6 total_carrier_ppm tuned_freq
//   slope_ppm = total_sampling_ppm,  anchor = 0,  carrier_hz = f_off (1 + e);  delay, phase, scale as given
// The dongle samples at ideal time k / (1 + e) and its carrier error turns its sample k by 2 pi f_off k / fs: output sample n of the
// nominal time base sits at dongle index n (1 + e), and the angle to take out there is 2 pi f_off n (1 + e) / fs.
#pragma once
#include <cmath>
#include <limits>

namespace gsmcal_ap {

// the columns read (== GSMCAL_T_*, GSMCAL_Q_*, GSMCAL_IQ_* and GSMCAL_AP_* of include/gsmcal.h; gsmcal.hip asserts it)
enum { T_TOTAL_SAMPLING_PPM = 4, T_TOTAL_CARRIER_PPM = 5, T_STATUS = 9 };
enum { Q_DC_I = 12, Q_DC_Q = 13, Q_GAIN = 16, Q_SIN_PHASE = 17, Q_STATUS = 21, IQ_OK = 0 };
enum { AP_DELAY = 0, AP_SLOPE_PPM, AP_CARRIER_HZ, AP_PHASE, AP_ANCHOR, AP_SCALE, AP_DC_I, AP_DC_Q, AP_GAIN, AP_SIN_PHASE, AP_PARAMS };
enum { AP_OK = 0, AP_SKIPPED = 17 };

// -> AP_OK, or AP_SKIPPED with every value of params_row NaN
inline int apply_params(const double* table_row, double tuned_freq, const double* iq_row, double delay, double phase, double scale,
                        double* params_row) {
    const double sampling_ppm = table_row[T_TOTAL_SAMPLING_PPM], carrier_ppm = table_row[T_TOTAL_CARRIER_PPM];
    if (!(table_row[T_STATUS] == 0.0) || !std::isfinite(sampling_ppm) || !std::isfinite(carrier_ppm)) {
        for (int i = 0; i < AP_PARAMS; ++i) params_row[i] = std::numeric_limits<double>::quiet_NaN();
        return AP_SKIPPED;
    }
    const double e = 1e-6 * sampling_ppm;
    const double f_off = 1e-6 * carrier_ppm * tuned_freq;
    params_row[AP_DELAY] = delay;
    params_row[AP_SLOPE_PPM] = sampling_ppm;
    params_row[AP_CARRIER_HZ] = f_off * (1.0 + e);
    params_row[AP_PHASE] = phase;
    params_row[AP_ANCHOR] = 0.0;
    params_row[AP_SCALE] = scale;
    params_row[AP_DC_I] = params_row[AP_DC_Q] = 127.5;
    params_row[AP_GAIN] = 1.0;
    params_row[AP_SIN_PHASE] = 0.0;
    if (iq_row) {
        params_row[AP_DC_I] = iq_row[Q_DC_I];
        params_row[AP_DC_Q] = iq_row[Q_DC_Q];
        if (iq_row[Q_STATUS] == (double)IQ_OK) {                   // (a constant rail or a single sample: no imbalance is defined)
            params_row[AP_GAIN] = iq_row[Q_GAIN];
            params_row[AP_SIN_PHASE] = iq_row[Q_SIN_PHASE];
        }
    }
    return AP_OK;
}

}  // namespace gsmcal_ap
