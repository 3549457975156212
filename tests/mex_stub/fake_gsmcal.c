/* A recording stand-in for libgsmcal.so -- TEST INFRASTRUCTURE: the entry points mex/gsmcal_mex.c calls and no others.
 *
 * Every fake function counts its call, writes one line "name|key=value|..." with its scalar arguments and lengths into a log,
 * reads EVERY element of every input it was promised (the line carries an FNV-1a hash over their bytes, in argument order, so
 * what arrived and in which order shows), fills each output with an index pattern up to the capacity it was given (output j,
 * element k: 1000*(j+1) + k; the imaginary part of a complex one is its negative), sets its count outputs and returns a status
 * -- both preset by the test through fake_preset().  Where include/gsmcal.h fixes what an entry point leaves at a sentinel
 * status (FCCH_coarse_position: one -1; FCCH_demod: no burst, NaN) the fake does the same.
 * Compiled into a gateway object beside mxstub.c, with hidden visibility: only the fake_* control functions are exported. */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "gsmcal.h"

#define FAKE_API __attribute__((visibility("default")))

static char g_log[1 << 15];
static int g_calls = 0, g_created = 0, g_destroyed = 0;
static int p_status = 0, p_count = 3, p_create_rc = 0;
static long p_len_r = 5;
static char g_last[64] = "";
static int g_ctx_dummy;

FAKE_API void fake_reset(void) { g_log[0] = 0; g_calls = 0; g_last[0] = 0; }
FAKE_API void fake_preset(int status, int count, long len_r, int create_rc) { p_status = status; p_count = count; p_len_r = len_r; p_create_rc = create_rc; }
FAKE_API int fake_calls(void) { return g_calls; }
FAKE_API int fake_created(void) { return g_created; }
FAKE_API int fake_destroyed(void) { return g_destroyed; }
FAKE_API const char* fake_log(void) { return g_log; }

static unsigned long long g_h;
static void h_begin(void) { g_h = 0xcbf29ce484222325ull; }
static void h_bytes(const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    size_t i;
    for (i = 0; i < n; ++i) { g_h ^= b[i]; g_h *= 0x100000001b3ull; }
}
static void h_dbl(const double* p, size_t n) { if (p) h_bytes(p, n * sizeof(double)); }
/* rows x 2 with a leading dimension: column 0 then column 1 */
static void h_pos(const double* p, int rows, int ld) { if (p && rows > 0) { h_dbl(p, (size_t)rows); h_dbl(p + ld, (size_t)rows); } }

static void logf_(const char* name, const char* fmt, ...) {
    size_t k = strlen(g_log);
    va_list ap;
    ++g_calls;
    snprintf(g_last, sizeof(g_last), "%s", name);
    k += (size_t)snprintf(g_log + k, sizeof(g_log) - k, "%s|", name);
    va_start(ap, fmt);
    if (k < sizeof(g_log)) k += (size_t)vsnprintf(g_log + k, sizeof(g_log) - k, fmt, ap);
    va_end(ap);
    if (k < sizeof(g_log)) snprintf(g_log + k, sizeof(g_log) - k, "|hash=%016llx\n", g_h);
}
static void fill(double* out, int j, long n) { long k; if (out) for (k = 0; k < n; ++k) out[k] = 1000.0 * (j + 1) + (double)k; }
static void fillc(double* out, int j, long n) {
    long k;
    if (out) for (k = 0; k < n; ++k) { out[2 * k] = 1000.0 * (j + 1) + (double)k; out[2 * k + 1] = -out[2 * k]; }
}

int gsmcal_ctx_create(int device_id, gsmcal_ctx** out) {
    (void)device_id;
    if (p_create_rc != 0) return p_create_rc;
    ++g_created;
    *out = (gsmcal_ctx*)&g_ctx_dummy;
    return 0;
}
void gsmcal_ctx_destroy(gsmcal_ctx* ctx) { if (ctx == (gsmcal_ctx*)&g_ctx_dummy) ++g_destroyed; }
const char* gsmcal_last_error(gsmcal_ctx* ctx) { (void)ctx; return "the fake's last error"; }
long gsmcal_last_call_report(gsmcal_ctx* ctx, char* buf, size_t cap) {
    char t[128];
    long n = (long)snprintf(t, sizeof(t), "report of %s: 100%% fake\n", g_last);
    (void)ctx;
    if (buf && cap) snprintf(buf, cap, "%s", t);
    return n;
}

int gsmcal_raw2iq(gsmcal_ctx* c, const double* a, long rows_2n, int d, double* b) {
    h_begin(); h_dbl(a, (size_t)(rows_2n * d));
    logf_("raw2iq", "ctx=%d|rows_2n=%ld|d=%d", c != NULL, rows_2n, d);
    fillc(b, 0, rows_2n / 2 * d);
    return p_status;
}
int gsmcal_raw2iq_u8(gsmcal_ctx* c, const uint8_t* a, long rows_2n, int d, double* b) {
    h_begin(); if (a) h_bytes(a, (size_t)(rows_2n * d));
    logf_("raw2iq_u8", "ctx=%d|rows_2n=%ld|d=%d", c != NULL, rows_2n, d);
    fillc(b, 0, rows_2n / 2 * d);
    return p_status;
}
int gsmcal_chn_filter_8x_4x(gsmcal_ctx* c, const double* s, long n, int d, const double* num, int ntaps, double* r) {
    h_begin(); h_dbl(s, (size_t)(2 * n * d));
    logf_("chn_filter_8x_4x", "ctx=%d|n=%ld|d=%d|num=%d|ntaps=%d", c != NULL, n, d, num != NULL, ntaps);
    fillc(r, 0, (n + 1) / 2 * d);
    return p_status;
}
int gsmcal_chn_filter_4x(gsmcal_ctx* c, const double* s, long n, int d, const double* num, int ntaps, double* r) {
    h_begin(); h_dbl(s, (size_t)(2 * n * d));
    logf_("chn_filter_4x", "ctx=%d|n=%ld|d=%d|num=%d|ntaps=%d", c != NULL, n, d, num != NULL, ntaps);
    fillc(r, 0, n * d);
    return p_status;
}
int gsmcal_move_fft_snr_runtime_avg(gsmcal_ctx* c, const double* s, long len, int mv_len, int fft_len, double th, int* hit_flag,
                                    double* hit_idx, double* hit_avg_snr, double* hit_snr) {
    h_begin(); h_dbl(s, (size_t)(2 * len));
    logf_("move_fft_snr_runtime_avg", "ctx=%d|len=%ld|mv_len=%d|fft_len=%d|th=%.17g", c != NULL, len, mv_len, fft_len, th);
    *hit_flag = p_count; *hit_idx = 2000.0; *hit_avg_snr = 3000.0; *hit_snr = 4000.0;
    return p_status;
}
int gsmcal_specific_fft_snr_fix_avg(gsmcal_ctx* c, const double* s, long len, const double target_set[2], int fft_len, double th,
                                    double avg_snr, int* hit_flag, double* hit_idx, double* hit_snr) {
    h_begin(); h_dbl(s, (size_t)(2 * len)); h_dbl(target_set, 2);
    logf_("specific_fft_snr_fix_avg", "ctx=%d|len=%ld|fft_len=%d|th=%.17g|avg_snr=%.17g", c != NULL, len, fft_len, th, avg_snr);
    *hit_flag = p_count; *hit_idx = 2000.0; *hit_snr = 3000.0;
    return p_status;
}
int gsmcal_FCCH_coarse_position(gsmcal_ctx* c, const double* s, long len, int decimation_ratio, double* position, double* snr, int cap,
                                int* count) {
    h_begin(); h_dbl(s, (size_t)(2 * len));
    logf_("FCCH_coarse_position", "ctx=%d|len=%ld|decimation_ratio=%d|cap=%d", c != NULL, len, decimation_ratio, cap);
    fill(position, 0, cap); fill(snr, 1, cap);
    *count = p_count;
    if (p_status == GSMCAL_S_NO_FCCH) { position[0] = snr[0] = -1.0; *count = 1; }
    return p_status;
}
int gsmcal_FCCH_fine_correction(gsmcal_ctx* c, const double* s, long len, const double* base_position, int num_base, int ov,
                                double carrier_freq, double* fcch_pos, int cap_pos, int* num_pos, double* r, long cap_r, long* len_r,
                                double* sampling_ppm, double* carrier_ppm) {
    h_begin(); h_dbl(s, (size_t)(2 * len)); h_dbl(base_position, (size_t)num_base);
    logf_("FCCH_fine_correction", "ctx=%d|len=%ld|num_base=%d|ov=%d|carrier_freq=%.17g|cap_pos=%d|r=%d|cap_r=%ld", c != NULL, len,
          num_base, ov, carrier_freq, cap_pos, r != NULL, cap_r);
    fill(fcch_pos, 0, cap_pos); *num_pos = p_count;
    fillc(r, 1, cap_r); *len_r = p_len_r;
    *sampling_ppm = 3000.0; *carrier_ppm = 4000.0;
    return p_status;
}
int gsmcal_SCH_corr_rate_correction(gsmcal_ctx* c, const double* s, long len, const double* fcch_pos, int num_fcch,
                                    const double* sch_training_sequence, int len_ts, int ov, double* pos_info, int cap_rows,
                                    int* num_rows, double* r, long cap_r, long* len_r, double* sampling_ppm) {
    h_begin(); h_dbl(s, (size_t)(2 * len)); h_dbl(fcch_pos, (size_t)num_fcch); h_dbl(sch_training_sequence, (size_t)(2 * len_ts));
    logf_("SCH_corr_rate_correction", "ctx=%d|s=%d|len=%ld|num_fcch=%d|len_ts=%d|ov=%d|cap_rows=%d|r=%d|cap_r=%ld", c != NULL, s != NULL,
          len, num_fcch, len_ts, ov, cap_rows, r != NULL, cap_r);
    fill(pos_info, 0, cap_rows); fill(pos_info + cap_rows, 1, cap_rows); *num_rows = p_count;
    fillc(r, 2, cap_r); *len_r = p_len_r;
    *sampling_ppm = 4000.0;
    return p_status;
}
int gsmcal_carrier_correct_post_SCH(gsmcal_ctx* c, const double* s, long len, const double* pos_info, int rows, int ld, int ov,
                                    double carrier_freq, double* r, long cap_r, long* len_r, double* carrier_ppm) {
    h_begin(); h_dbl(s, (size_t)(2 * len)); h_pos(pos_info, rows, ld);
    logf_("carrier_correct_post_SCH", "ctx=%d|s=%d|len=%ld|rows=%d|ld=%d|ov=%d|carrier_freq=%.17g|r=%d|cap_r=%ld", c != NULL, s != NULL,
          len, rows, ld, ov, carrier_freq, r != NULL, cap_r);
    fillc(r, 0, cap_r); *len_r = p_len_r;
    *carrier_ppm = 2000.0;
    return p_status;
}
int gsmcal_FCCH_demod(gsmcal_ctx* c, const double* s, long len, const double* pos_info, int rows, int ld, int ov, double carrier_freq,
                      double* freq, double* snr, double* max_idx, int cap, int* num_fcch, double* mean_freq, double* carrier_ppm) {
    h_begin(); h_dbl(s, (size_t)(2 * len)); h_pos(pos_info, rows, ld);
    logf_("FCCH_demod", "ctx=%d|s=%d|len=%ld|rows=%d|ld=%d|ov=%d|carrier_freq=%.17g|cap=%d", c != NULL, s != NULL, len, rows, ld, ov,
          carrier_freq, cap);
    fill(freq, 0, cap); fill(snr, 1, cap); fill(max_idx, 2, cap);
    *num_fcch = p_count; *mean_freq = 4000.0; *carrier_ppm = 5000.0;
    if (p_status == GSMCAL_S_POST_NO_POS) { *num_fcch = 0; *mean_freq = *carrier_ppm = NAN; }
    return p_status;
}
int gsmcal_BCCH_demod(gsmcal_ctx* c, const double* s, long len, const double* pos_info, int rows, int ld,
                      const double* normal_training_sequence, int len_ts, int ov, double carrier_freq, int* idx, double* r, long cap_r,
                      long* len_r, double* carrier_ppm, double* corr_val, double* table_row) {
    h_begin(); h_dbl(s, (size_t)(2 * len)); h_pos(pos_info, rows, ld); h_dbl(normal_training_sequence, (size_t)(2 * 8 * len_ts));
    logf_("BCCH_demod", "ctx=%d|s=%d|len=%ld|rows=%d|ld=%d|len_ts=%d|ov=%d|carrier_freq=%.17g|r=%d|cap_r=%ld|table_row=%d", c != NULL,
          s != NULL, len, rows, ld, len_ts, ov, carrier_freq, r != NULL, cap_r, table_row != NULL);
    *idx = p_count; fillc(r, 1, cap_r); *len_r = p_len_r; *carrier_ppm = 3000.0; fillc(corr_val, 3, 32);
    if (p_status == GSMCAL_S_POST_NO_POS || p_status == GSMCAL_S_POST_FEW_BCCH) { *idx = -1; *len_r = -1; *carrier_ppm = -1.0; }
    return p_status;
}
int gsmcal_SCH_decode(gsmcal_ctx* c, const double* s, long len, const double* pos_info, int rows, int ld,
                      const double* sch_training_sequence, int len_ts, int ov, int* bsic, long* fn_anchor, long* pos_anchor,
                      double* table_row, double* soft, unsigned char* u) {
    h_begin(); h_dbl(s, (size_t)(2 * len)); h_pos(pos_info, rows, ld); h_dbl(sch_training_sequence, (size_t)(2 * len_ts));
    logf_("SCH_decode", "ctx=%d|s=%d|len=%ld|rows=%d|ld=%d|len_ts=%d|ov=%d|soft=%d|u=%d", c != NULL, s != NULL, len, rows, ld, len_ts, ov,
          soft != NULL, u != NULL);
    *bsic = 1000; *fn_anchor = 2000; *pos_anchor = 3000;
    fill(table_row, 3, GSMCAL_SCH_COLS);
    if (table_row) table_row[GSMCAL_C_NUM_SCH] = p_count;
    return p_status;
}
int gsmcal_BCCH_decode(gsmcal_ctx* c, const double* s, long len, const double* pos_info, int rows, int ld, int tsc, int ov,
                       unsigned char* octets, double* table_row, double* soft, gsmcal_si_info* first) {
    int k;
    h_begin(); h_dbl(s, (size_t)(2 * len)); h_pos(pos_info, rows, ld);
    logf_("BCCH_decode", "ctx=%d|s=%d|len=%ld|rows=%d|ld=%d|tsc=%d|ov=%d|soft=%d", c != NULL, s != NULL, len, rows, ld, tsc, ov, soft != NULL);
    if (octets) for (k = 0; k < GSMCAL_MAX_HITS * GSMCAL_BLOCK_OCTETS; ++k) octets[k] = (unsigned char)(k % 251);
    fill(table_row, 4, GSMCAL_SI_COLS);
    if (table_row) table_row[GSMCAL_I_NUM_BLOCKS] = p_count;
    if (first) { first->valid = 1; first->msg_type = 0x1b; first->si_type = 3; first->cell_id = 1000; first->mcc = 2000; first->mnc = 2001;
                 first->mnc_digits = 2; first->lac = 2002; }
    return p_status;
}
int gsmcal_CW_check(gsmcal_ctx* c, const double* s, long len, double* r, double* phase_rotate) {
    h_begin(); h_dbl(s, (size_t)(2 * len));
    logf_("CW_check", "ctx=%d|len=%ld", c != NULL, len);
    fill(r, 0, len - 1);
    if (phase_rotate) *phase_rotate = 2000.0;
    return p_status;
}
int gsmcal_IQ_imbalance(gsmcal_ctx* c, const double* s, long len, double* table_row) {
    h_begin(); h_dbl(s, (size_t)(2 * len));
    logf_("IQ_imbalance", "ctx=%d|len=%ld", c != NULL, len);
    fill(table_row, 3, GSMCAL_IQ_COLS);
    return p_status;
}
int gsmcal_pair_coherence(gsmcal_ctx* c, const double* s_a, long len_a, const double* s_b, long len_b, const double* pos_info, int rows,
                          int ld, int ov, int lag0, int max_lag, double min_coherence, double* table_row, double* corr) {
    h_begin(); h_dbl(s_a, (size_t)(2 * len_a)); h_dbl(s_b, (size_t)(2 * len_b)); h_pos(pos_info, rows, ld);
    logf_("pair_coherence", "ctx=%d|s_a=%d|len_a=%ld|s_b=%d|len_b=%ld|rows=%d|ld=%d|ov=%d|lag0=%d|max_lag=%d|min_coherence=%.17g|corr=%d",
          c != NULL, s_a != NULL, len_a, s_b != NULL, len_b, rows, ld, ov, lag0, max_lag, min_coherence, corr != NULL);
    fill(table_row, 5, GSMCAL_PAIR_COLS);
    return p_status;
}
int gsmcal_pair_align(gsmcal_ctx* c, const double* s, long len, int ov, const double* params_row, long out_len, double* out,
                      double* info_row) {
    h_begin(); h_dbl(s, (size_t)(2 * len)); h_dbl(params_row, GSMCAL_ALIGN_PARAMS);
    logf_("pair_align", "ctx=%d|s=%d|len=%ld|ov=%d|out_len=%ld", c != NULL, s != NULL, len, ov, out_len);
    fillc(out, 0, out_len); fill(info_row, 1, GSMCAL_ALIGN_INFO_COLS);
    return p_status;
}
int gsmcal_total_ppm_calculation(const double* ppm_in, int n, double* ppm_out) {
    h_begin(); h_dbl(ppm_in, (size_t)n);
    logf_("total_ppm_calculation", "n=%d", n);
    *ppm_out = 1000.0;
    return p_status;
}
int gsmcal_calibrate_batch(gsmcal_ctx* c, const uint8_t* raw, int d, long n, const double* coef, int ntaps,
                           const double* sch_training_sequence, int len_ts, const double* carrier_freq, double* table, double* pos_info,
                           double* r_correct, long* r_len) {
    int i;
    h_begin(); if (raw) h_bytes(raw, (size_t)(2 * n * d)); h_dbl(coef, (size_t)ntaps); h_dbl(sch_training_sequence, (size_t)(2 * len_ts));
    h_dbl(carrier_freq, (size_t)d);
    logf_("calibrate_batch", "ctx=%d|d=%d|n=%ld|ntaps=%d|len_ts=%d|r_correct=%d|r_len=%d", c != NULL, d, n, ntaps, len_ts, r_correct != NULL,
          r_len != NULL);
    fill(table, 0, (long)d * GSMCAL_TABLE_COLS);
    fill(pos_info, 1, (long)d * 2 * GSMCAL_MAX_POS_ROWS);
    for (i = 0; i < d; ++i) table[i * GSMCAL_TABLE_COLS + GSMCAL_T_N_POS_ROWS] = (double)(p_count + i);   /* another row count per dongle */
    return p_status;
}
int gsmcal_fcch_scan_batch(gsmcal_ctx* c, const uint8_t* raw, int d, long n, const double* coef, int ntaps, double* snr, double* num_hit,
                           double* positions, double* pos_snr, int* counts) {
    h_begin(); if (raw) h_bytes(raw, (size_t)(2 * n * d)); h_dbl(coef, (size_t)ntaps);
    logf_("fcch_scan_batch", "ctx=%d|d=%d|n=%ld|ntaps=%d|positions=%d|pos_snr=%d|counts=%d", c != NULL, d, n, ntaps, positions != NULL,
          pos_snr != NULL, counts != NULL);
    fill(snr, 0, d); fill(num_hit, 1, d);
    return p_status;
}
int gsmcal_band_power_batch(gsmcal_ctx* c, const uint8_t* raw, int d, long n, const double* coef, int ntaps, int decim, double* power) {
    h_begin(); if (raw) h_bytes(raw, (size_t)(2 * n * d)); h_dbl(coef, (size_t)ntaps);
    logf_("band_power_batch", "ctx=%d|d=%d|n=%ld|ntaps=%d|decim=%d", c != NULL, d, n, ntaps, decim);
    fill(power, 0, d);
    return p_status;
}
int gsmcal_subband_power_batch(gsmcal_ctx* c, const uint8_t* raw, int d, long n, const double* coef, int ntaps, int decim,
                               const double* phase_rotate, int nsub, double* power) {
    h_begin(); if (raw) h_bytes(raw, (size_t)(2 * n * d)); h_dbl(coef, (size_t)ntaps); h_dbl(phase_rotate, (size_t)nsub * (size_t)d);
    logf_("subband_power_batch", "ctx=%d|d=%d|n=%ld|ntaps=%d|decim=%d|nsub=%d", c != NULL, d, n, ntaps, decim, nsub);
    fill(power, 0, (long)nsub * d);
    return p_status;
}
