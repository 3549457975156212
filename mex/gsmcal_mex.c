/* gsmcal_mex.c -- MEX gateway: lets gsm_sync_demod.m / multi_rtl_sdr_gsm_FCCH_scanner.m call the
 * MI355X kernels through the reference's own function names, unchanged.
 *
 * It is the binding a maintainer of the reference would add.  The project's suite builds and runs every target without MATLAB,
 * in both complex-storage modes, against a working mxArray stand-in (tests/mex_stub/mxstub.c): tests/test_mex_gateway_cpu.py over
 * a recording fake of the ABI, tests/test_gpu_mex_gateway.py over libgsmcal.so itself, held to the Python API bit for bit.
 * Build one MEX file per function, named like the .m file it shadows, and put
 * the output directory ahead of the reference on the MATLAB path:
 *
 *   for f in raw2iq chn_filter_8x_4x chn_filter_4x move_fft_snr_runtime_avg specific_fft_snr_fix_avg \
 *            FCCH_coarse_position FCCH_fine_correction SCH_corr_rate_correction \
 *            carrier_correct_post_SCH FCCH_demod BCCH_demod SCH_decode BCCH_decode CW_check IQ_imbalance pair_coherence pair_align total_ppm_calculation gsmcal_calibrate gsmcal_fcch_scan \
 *            gsmcal_band_power gsmcal_subband_power; do
 *     mex -R2018a -DGSMCAL_FN_$f -output $f mex/gsmcal_mex.c -Iinclude -Lmulti-rtl-sdr-calibration_amd/lib -lgsmcal
 *   done
 *
 * The last four are not shadows of .m files: they are the fused entry points (one call per driver loop body)
 *   [table, pos_info] = gsmcal_calibrate(s, coef, sch_training_sequence, freq)   replaces gsm_sync_demod.m:107-124
 *   [snr, num_hit]    = gsmcal_fcch_scan(s, coef)                                replaces ..FCCH_scanner.m:132-135,163-186
 *   power_spectrum    = gsmcal_band_power(s_all, coef, decimate_ratio)          replaces ..split_scanner.m:154-156
 *   power             = gsmcal_subband_power(s, coef, phase_rotate)             replaces ..diversity_scanner_another_bak.m:192-204
 * with s the 2N x D uint8 matrix fread() delivers (gsm_sync_demod.m:96; pass uint8(s) if it was read as double).
 * tests/test_abi_cpu.py also compiles every target against the declaration-only mex.h (tests/mex_stub) as a prototype check.
 *
 * Every target decides its arguments before it touches the library: their number, their class (double unless said otherwise;
 * raw2iq takes doubles or uint8) and the shapes it relies on; a call that fails this ends in a gsmcal:args / gsmcal:type error
 * with the usage line, no context is created for it.  pos_info is R x 2, or the scalar -1 the .m files' `pos_info==-1` accepts
 * as well (it is widened to [-1 -1]).
 *
 * Both MEX complex-storage APIs are handled: with -R2018a (MX_HAS_INTERLEAVED_COMPLEX = 1) complex arrays
 * are interleaved like the ABI's double[2] and are passed through without a copy; without the flag -- the only API of the
 * MATLAB releases the reference was written for (README: Ubuntu 12.04, R2008b-era .fda files) and still the default of
 * `mex` -- complex arrays are split (mxGetPr / mxGetPi) and the gateway interleaves inputs / de-interleaves outputs:
 *     mex -DGSMCAL_FN_$f -output $f mex/gsmcal_mex.c -Iinclude -L... -lgsmcal          (split API, any release)
 * Argument lists, 1-based positions, row/column shapes and sentinels follow the .m files
 * (cited per function); negative ABI status codes become mexErrMsgIdAndTxt errors, positive ones
 * (reference sentinels) return normally with the sentinel outputs, as the .m files do.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "gsmcal.h"
#include "mex.h"

static gsmcal_ctx* g_ctx = NULL;

static void at_exit(void) {
    if (g_ctx) { gsmcal_ctx_destroy(g_ctx); g_ctx = NULL; }
}

static gsmcal_ctx* ctx(void) {   /* created lazily, like the `persistent coef` of chn_filter_8x_4x.m:6-11 */
    if (!g_ctx) {
        if (gsmcal_ctx_create(0, &g_ctx) != 0) mexErrMsgIdAndTxt("gsmcal:nodevice", "no usable MI355X (gfx950) device");
        mexAtExit(at_exit);
    }
    return g_ctx;
}

static void chk(int rc, const char* what) {
    if (rc < 0) mexErrMsgIdAndTxt("gsmcal:error", "%s failed (%d): %s", what, rc, gsmcal_last_error(g_ctx));
}

/* The .m file this MEX file shadows disp()s its intermediate results (FCCH_coarse_position.m:92-94, FCCH_fine_correction.m:66,
 * 116,156-161,190, SCH_corr_rate_correction.m:80,118, carrier_correct_post_SCH.m:73-79, FCCH_demod.m:43-66, and a warning at every early exit): print
 * the same lines, from the library's report of the call just made (getenv GSMCAL_QUIET=1: run silent). */
static void say(void) {
    char buf[8192];
    const char* q = getenv("GSMCAL_QUIET");
    if (q && q[0] == '1') return;
    if (gsmcal_last_call_report(g_ctx, buf, sizeof(buf)) > 0) mexPrintf("%s", buf);
}

/* ---- the two complex-storage APIs behind one set of helpers ------------------------------------------------------ */
#if defined(MX_HAS_INTERLEAVED_COMPLEX) && MX_HAS_INTERLEAVED_COMPLEX
#define GSMCAL_INTERLEAVED 1
#define REAL_PTR(a) mxGetDoubles(a)
#define U8_PTR(a) ((const uint8_t*)mxGetUint8s(a))
#else
#define GSMCAL_INTERLEAVED 0
#define REAL_PTR(a) mxGetPr(a)
#define U8_PTR(a) ((const uint8_t*)mxGetData(a))
#endif

/* complex (or real, widened) array -> interleaved doubles; *n = number of elements.  Interleaved API: the array's own
 * storage when it is complex.  Split API: always a copy (freed by MATLAB when the MEX call returns, like every mxCalloc). */
static const double* cplx_in(const mxArray* a, mwSize* n) {
    *n = mxGetNumberOfElements(a);
#if GSMCAL_INTERLEAVED
    if (mxIsComplex(a)) return (const double*)mxGetComplexDoubles(a);
#endif
    {
        double* t = (double*)mxCalloc(2 * (*n) + 2, sizeof(double));
        const double* re = REAL_PTR(a);
        mwSize i;
        for (i = 0; i < *n; ++i) t[2 * i] = re[i];
#if !GSMCAL_INTERLEAVED
        if (mxIsComplex(a)) {
            const double* im = mxGetPi(a);
            for (i = 0; i < *n; ++i) t[2 * i + 1] = im[i];
        }
#endif
        return t;
    }
}

static mxArray* scalar(double v) { return mxCreateDoubleScalar(v); }

/* ---- argument checks: decided before the library is touched ------------------------------------------------------ */
static void usage(const char* line) { mexErrMsgIdAndTxt("gsmcal:args", "usage: %s", line); }
#define ARGS(ok, line) do { if (!(ok)) usage(line); } while (0)
/* The class of an input.  `mex` defines MATLAB_MEX_FILE for everything it builds, and MATLAB's mex.h has mxIsDouble.  Built
 * any other way (a reduced mex.h that declares only the accessors: tests/mex_stub) the class is read off the typed accessors,
 * which answer NULL for an array of another class -- mxGetDoubles / mxGetComplexDoubles do so in MATLAB itself. */
#ifdef MATLAB_MEX_FILE
static int is_dbl(const mxArray* a) { return mxIsDouble(a); }                                   /* real or complex doubles */
#elif GSMCAL_INTERLEAVED
static int is_dbl(const mxArray* a) { return mxGetDoubles(a) != NULL || mxGetComplexDoubles(a) != NULL; }
#else
static int is_dbl(const mxArray* a) { return !mxIsUint8(a) && mxGetPr(a) != NULL; }
#endif
static int is_real(const mxArray* a) { return is_dbl(a) && !mxIsComplex(a); }                   /* what REAL_PTR may be taken of */
static int is_num(const mxArray* a) { return is_real(a) && mxGetNumberOfElements(a) == 1; }     /* what mxGetScalar is taken of */
static int is_u8(const mxArray* a) { return mxIsUint8(a) && !mxIsComplex(a); }
static int all_num(int nrhs, const mxArray* prhs[], int first) {
    int k;
    for (k = first; k < nrhs; ++k) if (!is_num(prhs[k])) return 0;
    return 1;
}
/* the 2N x D uint8 matrix of a fused target -> D captures of 2*(*n) bytes one behind the other, as the ABI reads them.  An odd row
 * count leaves a last byte without its partner in every column: N = floor(rows / 2), and the columns are copied without it --
 * handed over as they are, every capture after the first would start one byte early per column before it. */
static const uint8_t* raw_in(const mxArray* a, long* n) {
    const mwSize rows = mxGetM(a), d = mxGetN(a);
    const uint8_t* src = U8_PTR(a);
    uint8_t* t;
    mwSize i;
    *n = (long)(rows / 2);
    if (rows % 2 == 0 || d == 1) return src;
    t = (uint8_t*)mxMalloc((rows - 1) * d);
    for (i = 0; i < d; ++i) memcpy(t + i * (rows - 1), src + i * rows, rows - 1);
    return t;
}
/* pos_info as the .m files take it: R x 2 real, or the scalar -1 that `pos_info==-1` accepts too -- the ABI reads two columns,
 * so that one is widened to [-1 -1].  Returns the R x 2 column-major table (ld = *rows), NULL for anything else. */
static const double* pos_in(const mxArray* a, int* rows) {
    static const double m1[2] = {-1.0, -1.0};
    if (!is_real(a)) return NULL;
    if (mxGetNumberOfElements(a) == 1 && mxGetScalar(a) == -1.0) { *rows = 1; return m1; }
    if (mxGetN(a) != 2 || mxGetM(a) < 1) return NULL;
    *rows = (int)mxGetM(a);
    return REAL_PTR(a);
}

/* m x n complex output the ABI fills as interleaved doubles: cplx_out_begin() gives the buffer to hand to the ABI,
 * cplx_out_end() the finished mxArray (interleaved API: the array's own storage, no copy; split API: de-interleaved) */
typedef struct { mxArray* arr; double* buf; mwSize m, n; } cplx_out;
static double* cplx_out_begin(cplx_out* o, mwSize m, mwSize n) {
    o->m = m; o->n = n;
#if GSMCAL_INTERLEAVED
    o->arr = mxCreateDoubleMatrix(m, n, mxCOMPLEX);
    o->buf = (double*)mxGetComplexDoubles(o->arr);
#else
    o->arr = NULL;
    o->buf = (double*)mxMalloc((2 * m * n + 2) * sizeof(double));
#endif
    return o->buf;
}
static mxArray* cplx_out_end(cplx_out* o) {
#if !GSMCAL_INTERLEAVED
    mwSize i, tot = o->m * o->n;
    double *re, *im;
    o->arr = mxCreateDoubleMatrix(o->m, o->n, mxCOMPLEX);
    re = mxGetPr(o->arr); im = mxGetPi(o->arr);
    for (i = 0; i < tot; ++i) { re[i] = o->buf[2 * i]; im[i] = o->buf[2 * i + 1]; }
    mxFree(o->buf);
#endif
    return o->arr;
}

static mxArray* cplx_col(const double* data, mwSize n) {   /* n x 1 complex column from interleaved doubles */
    cplx_out o;
    double* b = cplx_out_begin(&o, n, 1);
    memcpy(b, data, 2 * n * sizeof(double));
    return cplx_out_end(&o);
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
#if defined(GSMCAL_FN_raw2iq)
    /* b = raw2iq(a)                                   raw2iq.m:5
     * a: 2N x D byte values, as doubles (the reference) or as the uint8 matrix fread(...,'uint8') delivers */
    mwSize rows, d;
    cplx_out o;
    double* b;
    ARGS(nrhs == 1 && nlhs <= 1 && (is_real(prhs[0]) || is_u8(prhs[0])) && mxGetNumberOfElements(prhs[0]) >= 2,
         "b = raw2iq(a) with a 2N x D real doubles or uint8");
    rows = mxGetM(prhs[0]); d = mxGetN(prhs[0]);
    b = cplx_out_begin(&o, rows / 2, d);
    if (is_u8(prhs[0])) chk(gsmcal_raw2iq_u8(ctx(), U8_PTR(prhs[0]), (long)rows, (int)d, b), "raw2iq");
    else chk(gsmcal_raw2iq(ctx(), REAL_PTR(prhs[0]), (long)rows, (int)d, b), "raw2iq");
    plhs[0] = cplx_out_end(&o);

#elif defined(GSMCAL_FN_chn_filter_8x_4x)
    /* r = chn_filter_8x_4x(s)                         chn_filter_8x_4x.m:5 */
    mwSize n, d, tot;
    const double* s;
    cplx_out o;
    double* b;
    ARGS(nrhs == 1 && nlhs <= 1 && is_dbl(prhs[0]) && mxGetNumberOfElements(prhs[0]) >= 1, "r = chn_filter_8x_4x(s) with s N x D doubles");
    n = mxGetM(prhs[0]); d = mxGetN(prhs[0]);
    s = cplx_in(prhs[0], &tot);
    b = cplx_out_begin(&o, (n + 1) / 2, d);
    chk(gsmcal_chn_filter_8x_4x(ctx(), s, (long)n, (int)d, NULL, 0, b), "chn_filter_8x_4x");
    plhs[0] = cplx_out_end(&o);

#elif defined(GSMCAL_FN_chn_filter_4x)
    /* r = chn_filter_4x(s)                            chn_filter_4x.m:5 */
    mwSize n, d, tot;
    const double* s;
    cplx_out o;
    double* b;
    ARGS(nrhs == 1 && nlhs <= 1 && is_dbl(prhs[0]) && mxGetNumberOfElements(prhs[0]) >= 1, "r = chn_filter_4x(s) with s N x D doubles");
    n = mxGetM(prhs[0]); d = mxGetN(prhs[0]);
    s = cplx_in(prhs[0], &tot);
    b = cplx_out_begin(&o, n, d);
    chk(gsmcal_chn_filter_4x(ctx(), s, (long)n, (int)d, NULL, 0, b), "chn_filter_4x");
    plhs[0] = cplx_out_end(&o);

#elif defined(GSMCAL_FN_move_fft_snr_runtime_avg)
    /* [hit_flag,hit_idx,hit_avg_snr,hit_snr] = move_fft_snr_runtime_avg(s,mv_len,fft_len,th) */
    mwSize n;
    const double* s;
    int hf; double hi, ha, hs;
    ARGS(nrhs == 4 && nlhs <= 4 && is_dbl(prhs[0]) && mxGetNumberOfElements(prhs[0]) >= 1 && all_num(nrhs, prhs, 1),
         "[hit_flag,hit_idx,hit_avg_snr,hit_snr] = move_fft_snr_runtime_avg(s,mv_len,fft_len,th)");
    s = cplx_in(prhs[0], &n);
    chk(gsmcal_move_fft_snr_runtime_avg(ctx(), s, (long)n, (int)mxGetScalar(prhs[1]), (int)mxGetScalar(prhs[2]),
                                        mxGetScalar(prhs[3]), &hf, &hi, &ha, &hs), "move_fft_snr_runtime_avg");
    plhs[0] = mxCreateLogicalScalar(hf != 0);
    if (nlhs > 1) plhs[1] = scalar(hi);
    if (nlhs > 2) plhs[2] = scalar(ha);
    if (nlhs > 3) plhs[3] = scalar(hs);

#elif defined(GSMCAL_FN_specific_fft_snr_fix_avg)
    /* [hit_flag,hit_idx,hit_snr] = specific_fft_snr_fix_avg(s,target_set,fft_len,th,avg_snr) */
    mwSize n;
    const double* s;
    int hf; double hi, hs;
    ARGS(nrhs == 5 && nlhs <= 3 && is_dbl(prhs[0]) && mxGetNumberOfElements(prhs[0]) >= 1 && is_real(prhs[1]) &&
         mxGetNumberOfElements(prhs[1]) >= 2 && all_num(nrhs, prhs, 2),
         "[hit_flag,hit_idx,hit_snr] = specific_fft_snr_fix_avg(s,target_set,fft_len,th,avg_snr) with target_set of two elements");
    s = cplx_in(prhs[0], &n);
    chk(gsmcal_specific_fft_snr_fix_avg(ctx(), s, (long)n, REAL_PTR(prhs[1]), (int)mxGetScalar(prhs[2]),
                                        mxGetScalar(prhs[3]), mxGetScalar(prhs[4]), &hf, &hi, &hs),
        "specific_fft_snr_fix_avg");
    plhs[0] = mxCreateLogicalScalar(hf != 0);
    if (nlhs > 1) plhs[1] = scalar(hi);
    if (nlhs > 2) plhs[2] = scalar(hs);

#elif defined(GSMCAL_FN_FCCH_coarse_position)
    /* [position,snr] = FCCH_coarse_position(s,decimation_ratio)     (row vectors; -1,-1 when none) */
    mwSize n;
    const double* s;
    double pos[GSMCAL_MAX_HITS], snr[GSMCAL_MAX_HITS];
    int cnt = 0;
    ARGS(nrhs == 2 && nlhs <= 2 && is_dbl(prhs[0]) && mxGetNumberOfElements(prhs[0]) >= 1 && is_num(prhs[1]),
         "[position,snr] = FCCH_coarse_position(s,decimation_ratio)");
    s = cplx_in(prhs[0], &n);
    chk(gsmcal_FCCH_coarse_position(ctx(), s, (long)n, (int)mxGetScalar(prhs[1]), pos, snr, GSMCAL_MAX_HITS, &cnt),
        "FCCH_coarse_position");
    say();
    plhs[0] = mxCreateDoubleMatrix(1, cnt, mxREAL);
    memcpy(REAL_PTR(plhs[0]), pos, cnt * sizeof(double));
    if (nlhs > 1) { plhs[1] = mxCreateDoubleMatrix(1, cnt, mxREAL); memcpy(REAL_PTR(plhs[1]), snr, cnt * sizeof(double)); }

#elif defined(GSMCAL_FN_FCCH_fine_correction)
    /* [FCCH_pos,r,sampling_ppm,carrier_ppm] = FCCH_fine_correction(s,base_position,ov,carrier_freq) */
    mwSize n;
    const double* s;
    double pos[GSMCAL_MAX_HITS], sp, cp;
    int npos = 0; long lr = -1;
    double* r;
    ARGS(nrhs == 4 && nlhs <= 4 && is_dbl(prhs[0]) && mxGetNumberOfElements(prhs[0]) >= 1 && is_real(prhs[1]) &&
         mxGetNumberOfElements(prhs[1]) >= 1 && all_num(nrhs, prhs, 2),
         "[FCCH_pos,r,sampling_ppm,carrier_ppm] = FCCH_fine_correction(s,base_position,ov,carrier_freq)");
    s = cplx_in(prhs[0], &n);
    r = (double*)mxMalloc(2 * n * sizeof(double));
    chk(gsmcal_FCCH_fine_correction(ctx(), s, (long)n, REAL_PTR(prhs[1]), (int)mxGetNumberOfElements(prhs[1]),
                                    (int)mxGetScalar(prhs[2]), mxGetScalar(prhs[3]), pos, GSMCAL_MAX_HITS, &npos,
                                    r, (long)n, &lr, &sp, &cp), "FCCH_fine_correction");
    say();
    plhs[0] = mxCreateDoubleMatrix(1, npos, mxREAL);
    memcpy(REAL_PTR(plhs[0]), pos, npos * sizeof(double));
    if (nlhs > 1) plhs[1] = lr < 0 ? scalar(-1.0) : cplx_col(r, (mwSize)lr);
    if (nlhs > 2) plhs[2] = scalar(sp);
    if (nlhs > 3) plhs[3] = scalar(cp);
    mxFree(r);

#elif defined(GSMCAL_FN_SCH_corr_rate_correction)
    /* [pos_info,r,sampling_ppm] = SCH_corr_rate_correction(s,FCCH_pos,sch_training_sequence,ov) */
    mwSize n = 0, nts;
    const double *s, *ts;
    double pi[2 * GSMCAL_MAX_POS_ROWS], sp;
    int rows = 0, i; long lr = -1;
    double* r;
    ARGS(nrhs == 4 && nlhs <= 3 && is_dbl(prhs[0]) && mxGetNumberOfElements(prhs[0]) >= 1 && is_real(prhs[1]) &&
         mxGetNumberOfElements(prhs[1]) >= 1 && is_dbl(prhs[2]) && mxGetNumberOfElements(prhs[2]) >= 1 && is_num(prhs[3]),
         "[pos_info,r,sampling_ppm] = SCH_corr_rate_correction(s,FCCH_pos,sch_training_sequence,ov)");
    s = mxGetNumberOfElements(prhs[0]) > 1 ? cplx_in(prhs[0], &n) : NULL;   /* r = -1 upstream */
    ts = cplx_in(prhs[2], &nts);
    r = n ? (double*)mxMalloc(2 * n * sizeof(double)) : NULL;
    chk(gsmcal_SCH_corr_rate_correction(ctx(), s, (long)n, REAL_PTR(prhs[1]), (int)mxGetNumberOfElements(prhs[1]),
                                        ts, (int)nts, (int)mxGetScalar(prhs[3]), pi, GSMCAL_MAX_POS_ROWS, &rows,
                                        r, (long)n, &lr, &sp), "SCH_corr_rate_correction");
    say();
    plhs[0] = mxCreateDoubleMatrix(rows, 2, mxREAL);
    for (i = 0; i < rows; ++i) {
        REAL_PTR(plhs[0])[i] = pi[i];
        REAL_PTR(plhs[0])[rows + i] = pi[GSMCAL_MAX_POS_ROWS + i];
    }
    if (nlhs > 1) plhs[1] = lr < 0 ? scalar(-1.0) : cplx_col(r, (mwSize)lr);
    if (nlhs > 2) plhs[2] = scalar(sp);
    if (r) mxFree(r);

#elif defined(GSMCAL_FN_carrier_correct_post_SCH)
    /* [r,carrier_ppm] = carrier_correct_post_SCH(s,pos_info,ov,carrier_freq) */
    mwSize n = 0;
    const double *s, *pin = NULL;
    int rows = 0;
    double cp; long lr = -1;
    double* r;
    ARGS(nrhs == 4 && nlhs <= 2 && is_dbl(prhs[0]) && mxGetNumberOfElements(prhs[0]) >= 1 && (pin = pos_in(prhs[1], &rows)) != NULL &&
         all_num(nrhs, prhs, 2), "[r,carrier_ppm] = carrier_correct_post_SCH(s,pos_info,ov,carrier_freq) with pos_info R x 2 (or -1)");
    s = mxGetNumberOfElements(prhs[0]) > 1 ? cplx_in(prhs[0], &n) : NULL;
    r = n ? (double*)mxMalloc(2 * n * sizeof(double)) : NULL;
    chk(gsmcal_carrier_correct_post_SCH(ctx(), s, (long)n, pin, rows, rows, (int)mxGetScalar(prhs[2]),
                                        mxGetScalar(prhs[3]), r, (long)n, &lr, &cp), "carrier_correct_post_SCH");
    say();
    plhs[0] = lr < 0 ? scalar(-1.0) : cplx_col(r, (mwSize)lr);
    if (nlhs > 1) plhs[1] = scalar(cp);
    if (r) mxFree(r);

#elif defined(GSMCAL_FN_FCCH_demod)
    /* FCCH_demod(s,pos_info,ov,carrier_freq): prints what FCCH_demod.m:6-66 prints (it returns nothing); asked for outputs it
     * also hands the printed figures back: [freq, snr, max_idx, carrier_ppm] = FCCH_demod(...), rows of num_fcch entries with
     * max_idx the offset of :66.  At the :8 exit (pos_info == -1) the outputs are empty and carrier_ppm is NaN. */
    mwSize n = 0, i;
    const double *s, *pin = NULL;
    int rows = 0, nb = 0;
    double v[3 * GSMCAL_MAX_HITS], mf, cp;
    ARGS(nrhs == 4 && nlhs <= 4 && is_dbl(prhs[0]) && mxGetNumberOfElements(prhs[0]) >= 1 && (pin = pos_in(prhs[1], &rows)) != NULL &&
         all_num(nrhs, prhs, 2), "[freq, snr, max_idx, carrier_ppm] = FCCH_demod(s,pos_info,ov,carrier_freq) with pos_info R x 2 (or -1)");
    s = mxGetNumberOfElements(prhs[0]) > 1 ? cplx_in(prhs[0], &n) : NULL;
    chk(gsmcal_FCCH_demod(ctx(), s, (long)n, pin, rows, rows, (int)mxGetScalar(prhs[2]), mxGetScalar(prhs[3]),
                          v, v + GSMCAL_MAX_HITS, v + 2 * GSMCAL_MAX_HITS, GSMCAL_MAX_HITS, &nb, &mf, &cp), "FCCH_demod");
    say();
    for (i = 0; i < 3 && (int)i < nlhs; ++i) {
        mwSize k;
        plhs[i] = mxCreateDoubleMatrix(1, (mwSize)nb, mxREAL);
        for (k = 0; k < (mwSize)nb; ++k) REAL_PTR(plhs[i])[k] = v[i * GSMCAL_MAX_HITS + k];
    }
    if (nlhs > 3) plhs[3] = scalar(cp);

#elif defined(GSMCAL_FN_BCCH_demod)
    /* [normal_training_sequence_idx, r, carrier_ppm, corr_val] = BCCH_demod(s,pos_info,normal_training_sequence,ov,carrier_freq)
     * BCCH_demod.m with the two names it leaves undefined as arguments: carrier_freq (:71) is the fifth, the templates of
     * gsm_normal_training_sequence_gen(ov) (26*ov x 8 complex, :97) the third.  Prints the lines of :15,69,72,101,104; the three
     * outputs are the variables of :6-8 (-1 at the :9 and :14 exits), corr_val the 8 x 4 matrix of :97 (empty at those exits). */
    mwSize n = 0, nt = 0;
    const double *s, *ts, *pin = NULL;
    int rows = 0, idx = -1, rc;
    double cp = -1.0; long lr = -1;
    double* r;
    cplx_out cv;
    double* cvb;
    ARGS(nrhs == 5 && nlhs <= 4 && is_dbl(prhs[0]) && mxGetNumberOfElements(prhs[0]) >= 1 && (pin = pos_in(prhs[1], &rows)) != NULL &&
         is_dbl(prhs[2]) && mxGetN(prhs[2]) == 8 && mxGetM(prhs[2]) >= 1 && all_num(nrhs, prhs, 3),
         "[idx, r, carrier_ppm, corr_val] = BCCH_demod(s, pos_info, normal_training_sequence, ov, carrier_freq) with pos_info R x 2 (or -1) "
         "and normal_training_sequence 26*ov x 8");
    s = mxGetNumberOfElements(prhs[0]) > 1 ? cplx_in(prhs[0], &n) : NULL;
    r = n ? (double*)mxMalloc(2 * n * sizeof(double)) : NULL;
    ts = cplx_in(prhs[2], &nt);
    cvb = cplx_out_begin(&cv, 8, 4);
    rc = gsmcal_BCCH_demod(ctx(), s, (long)n, pin, rows, rows, ts, (int)mxGetM(prhs[2]), (int)mxGetScalar(prhs[3]),
                           mxGetScalar(prhs[4]), &idx, r, (long)n, &lr, &cp, cvb, NULL);
    chk(rc, "BCCH_demod");
    say();
    plhs[0] = scalar((double)idx);
    if (nlhs > 1) plhs[1] = lr < 0 ? scalar(-1.0) : cplx_col(r, (mwSize)lr);
    if (nlhs > 2) plhs[2] = scalar(cp);
    {
        mxArray* m = cplx_out_end(&cv);
        if (nlhs > 3) plhs[3] = rc == GSMCAL_S_POST_NO_POS || rc == GSMCAL_S_POST_FEW_BCCH ? mxCreateDoubleMatrix(0, 0, mxREAL) : m;
    }
    if (r) mxFree(r);

#elif defined(GSMCAL_FN_SCH_decode)
    /* [bsic, fn_anchor, pos_anchor, fn, ok] = SCH_decode(s, pos_info, sch_training_sequence, ov): the project's own function
     * (include/gsmcal.h), not SCH_demod.m.  The cell's BSIC, the GSM frame number of the anchor burst and its start sample (-1
     * when fewer than two SCH bursts decode consistently or pos_info == -1), then per SCH burst the frame number and the ok flag
     * (rows of num_sch entries, NaN where a burst was not decoded).  Prints the call's report lines. */
    mwSize n = 0, nt = 0, k;
    const double *s, *ts, *pin = NULL;
    int rows = 0, bsic = -1, nb, rc;
    long fn = -1, pos = -1;
    double row[GSMCAL_SCH_COLS];
    ARGS(nrhs == 4 && nlhs <= 5 && is_dbl(prhs[0]) && mxGetNumberOfElements(prhs[0]) >= 1 && (pin = pos_in(prhs[1], &rows)) != NULL &&
         is_dbl(prhs[2]) && mxGetNumberOfElements(prhs[2]) >= 1 && is_num(prhs[3]),
         "[bsic, fn_anchor, pos_anchor, fn, ok] = SCH_decode(s, pos_info, sch_training_sequence, ov) with pos_info R x 2 (or -1)");
    s = mxGetNumberOfElements(prhs[0]) > 1 ? cplx_in(prhs[0], &n) : NULL;
    ts = cplx_in(prhs[2], &nt);
    rc = gsmcal_SCH_decode(ctx(), s, (long)n, pin, rows, rows, ts, (int)nt, (int)mxGetScalar(prhs[3]), &bsic, &fn, &pos,
                           row, NULL, NULL);
    chk(rc, "SCH_decode");
    say();
    nb = (int)row[GSMCAL_C_NUM_SCH] < GSMCAL_MAX_HITS ? (int)row[GSMCAL_C_NUM_SCH] : GSMCAL_MAX_HITS;
    plhs[0] = scalar((double)bsic);
    if (nlhs > 1) plhs[1] = scalar((double)fn);
    if (nlhs > 2) plhs[2] = scalar((double)pos);
    if (nlhs > 3) {
        plhs[3] = mxCreateDoubleMatrix(1, (mwSize)nb, mxREAL);
        for (k = 0; k < (mwSize)nb; ++k) REAL_PTR(plhs[3])[k] = row[GSMCAL_C_FN + k];
    }
    if (nlhs > 4) {
        plhs[4] = mxCreateDoubleMatrix(1, (mwSize)nb, mxREAL);
        for (k = 0; k < (mwSize)nb; ++k) REAL_PTR(plhs[4])[k] = row[GSMCAL_C_OK + k];
    }

#elif defined(GSMCAL_FN_BCCH_decode)
    /* [cell_id, lai, si_type, octets, ok] = BCCH_decode(s, pos_info, tsc, ov): the project's own function (include/gsmcal.h), not
     * BCCH_demod.m.  tsc: the training sequence code 0..7 (BCCH_demod's idx - 1).  From the first block that passes the Fire code:
     * the cell identity (-1 unless it is a SYSTEM INFORMATION TYPE 3), lai = [mcc mnc lac] (-1 where the message has none) and the
     * type 1..4 (0: not recognised, -1: no block decoded or pos_info == -1); then the blocks as a num_blocks x 23 matrix of octets
     * (zero rows where a block failed) and the ok flag per block (NaN where it was not evaluated).  Prints the report lines. */
    mwSize n = 0, k, j;
    const double *s, *pin = NULL;
    int rows = 0, nb, rc;
    double row[GSMCAL_SI_COLS];
    unsigned char oct[GSMCAL_MAX_HITS * GSMCAL_BLOCK_OCTETS];
    gsmcal_si_info si;
    ARGS(nrhs == 4 && nlhs <= 5 && is_dbl(prhs[0]) && mxGetNumberOfElements(prhs[0]) >= 1 && (pin = pos_in(prhs[1], &rows)) != NULL &&
         all_num(nrhs, prhs, 2), "[cell_id, lai, si_type, octets, ok] = BCCH_decode(s, pos_info, tsc, ov) with pos_info R x 2 (or -1)");
    s = mxGetNumberOfElements(prhs[0]) > 1 ? cplx_in(prhs[0], &n) : NULL;
    rc = gsmcal_BCCH_decode(ctx(), s, (long)n, pin, rows, rows, (int)mxGetScalar(prhs[2]), (int)mxGetScalar(prhs[3]), oct,
                            row, NULL, &si);
    chk(rc, "BCCH_decode");
    say();
    nb = (int)row[GSMCAL_I_NUM_BLOCKS] < GSMCAL_MAX_HITS ? (int)row[GSMCAL_I_NUM_BLOCKS] : GSMCAL_MAX_HITS;
    plhs[0] = scalar((double)si.cell_id);
    if (nlhs > 1) {
        plhs[1] = mxCreateDoubleMatrix(1, 3, mxREAL);
        REAL_PTR(plhs[1])[0] = (double)si.mcc;
        REAL_PTR(plhs[1])[1] = (double)si.mnc;
        REAL_PTR(plhs[1])[2] = (double)si.lac;
    }
    if (nlhs > 2) plhs[2] = scalar(rc == 0 ? (double)si.si_type : -1.0);
    if (nlhs > 3) {
        plhs[3] = mxCreateDoubleMatrix((mwSize)nb, GSMCAL_BLOCK_OCTETS, mxREAL);
        for (k = 0; k < (mwSize)nb; ++k)
            for (j = 0; j < GSMCAL_BLOCK_OCTETS; ++j) REAL_PTR(plhs[3])[j * (mwSize)nb + k] = (double)oct[k * GSMCAL_BLOCK_OCTETS + j];
    }
    if (nlhs > 4) {
        plhs[4] = mxCreateDoubleMatrix(1, (mwSize)nb, mxREAL);
        for (k = 0; k < (mwSize)nb; ++k) REAL_PTR(plhs[4])[k] = row[GSMCAL_I_OK + k];
    }

#elif defined(GSMCAL_FN_CW_check)
    /* r = CW_check(s)     CW_check.m:6-8: s a complex vector of N >= 2 samples (raw2iq's output, check_CW_samples_loss_tcp.m:70,
     * 89-90), r an (N-1) x 1 real column, not wrapped.  [r, phase_rotate] = CW_check(s) also hands back the mean phase step. */
    mwSize n = 0;
    const double* s;
    double pr;
    ARGS(nrhs == 1 && nlhs <= 2 && is_dbl(prhs[0]) && mxGetNumberOfElements(prhs[0]) >= 2, "r = CW_check(s) with at least two samples");
    s = cplx_in(prhs[0], &n);
    plhs[0] = mxCreateDoubleMatrix(n - 1, 1, mxREAL);
    chk(gsmcal_CW_check(ctx(), s, (long)n, REAL_PTR(plhs[0]), &pr), "CW_check");
    if (nlhs > 1) plhs[1] = scalar(pr);

#elif defined(GSMCAL_FN_IQ_imbalance)
    /* [gain, phase_deg, irr_db, row] = IQ_imbalance(s)     the I/Q imbalance check of one complex vector (raw2iq's output, r_correct):
     * gain ratio, quadrature skew in degrees, image rejection in dB and the whole 1 x GSMCAL_IQ_COLS row (columns: GSMCAL_Q_*).
     * No .m file of the reference exists for it (its TODO item 4.5); the line it prints comes from the library's report. */
    mwSize n = 0, k;
    const double* s;
    double row[GSMCAL_IQ_COLS];
    ARGS(nrhs == 1 && nlhs <= 4 && is_dbl(prhs[0]) && mxGetNumberOfElements(prhs[0]) >= 1,
         "[gain, phase_deg, irr_db, row] = IQ_imbalance(s) with at least one sample");
    s = cplx_in(prhs[0], &n);
    chk(gsmcal_IQ_imbalance(ctx(), s, (long)n, row), "IQ_imbalance");
    say();
    plhs[0] = scalar(row[GSMCAL_Q_GAIN]);
    if (nlhs > 1) plhs[1] = scalar(row[GSMCAL_Q_PHASE_DEG]);
    if (nlhs > 2) plhs[2] = scalar(row[GSMCAL_Q_IRR_DB]);
    if (nlhs > 3) {
        plhs[3] = mxCreateDoubleMatrix(1, GSMCAL_IQ_COLS, mxREAL);
        for (k = 0; k < GSMCAL_IQ_COLS; ++k) REAL_PTR(plhs[3])[k] = row[k];
    }

#elif defined(GSMCAL_FN_pair_coherence)
    /* [delay0, rel_carrier_hz, phase0, mean_coherence, rel_sampling_ppm, row] = pair_coherence(s_a, s_b, pos_info_a, ov, lag0, max_lag,
     * min_coherence): the project's own function (include/gsmcal.h), no .m file of the reference exists for it.  The delay of b
     * against a in samples, their carrier difference in Hz and phase in rad at the first used burst, the mean coherence, the drift of
     * the delay in ppm (NaN when fewer than two bursts are used or pos_info == -1) and the whole 1 x GSMCAL_PAIR_COLS row (columns:
     * GSMCAL_P_*).  lag0 defaults to 0, max_lag to 2*ov, min_coherence to 0.5.  Prints the report lines. */
    mwSize na = 0, nb = 0, k;
    const double *sa, *sb, *pin = NULL;
    int rows = 0, rc;
    double* row;
    ARGS(nrhs >= 4 && nrhs <= 7 && nlhs <= 6 && is_dbl(prhs[0]) && mxGetNumberOfElements(prhs[0]) >= 1 && is_dbl(prhs[1]) &&
         mxGetNumberOfElements(prhs[1]) >= 1 && (pin = pos_in(prhs[2], &rows)) != NULL && all_num(nrhs, prhs, 3),
         "[delay0, rel_carrier_hz, phase0, mean_coherence, rel_sampling_ppm, row] = pair_coherence(s_a, s_b, pos_info_a, ov, lag0, max_lag, "
         "min_coherence) with pos_info_a R x 2 (or -1)");
    sa = mxGetNumberOfElements(prhs[0]) > 1 ? cplx_in(prhs[0], &na) : NULL;
    sb = mxGetNumberOfElements(prhs[1]) > 1 ? cplx_in(prhs[1], &nb) : NULL;
    row = (double*)mxCalloc(GSMCAL_PAIR_COLS, sizeof(double));
    rc = gsmcal_pair_coherence(ctx(), sa, (long)na, sb, (long)nb, pin, rows, rows, (int)mxGetScalar(prhs[3]),
                               nrhs > 4 ? (int)mxGetScalar(prhs[4]) : 0, nrhs > 5 ? (int)mxGetScalar(prhs[5]) : 0,
                               nrhs > 6 ? mxGetScalar(prhs[6]) : 0.5, row, NULL);
    chk(rc, "pair_coherence");
    say();
    plhs[0] = scalar(row[GSMCAL_P_DELAY0]);
    if (nlhs > 1) plhs[1] = scalar(row[GSMCAL_P_REL_CARRIER_HZ]);
    if (nlhs > 2) plhs[2] = scalar(row[GSMCAL_P_PHASE0]);
    if (nlhs > 3) plhs[3] = scalar(row[GSMCAL_P_MEAN_COHERENCE]);
    if (nlhs > 4) plhs[4] = scalar(row[GSMCAL_P_REL_SAMPLING_PPM]);
    if (nlhs > 5) {
        plhs[5] = mxCreateDoubleMatrix(1, GSMCAL_PAIR_COLS, mxREAL);
        for (k = 0; k < GSMCAL_PAIR_COLS; ++k) REAL_PTR(plhs[5])[k] = row[k];
    }
    mxFree(row);

#elif defined(GSMCAL_FN_pair_align)
    /* [out, info] = pair_align(s, ov, params, out_len): the project's own function (include/gsmcal.h), no .m file of the reference
     * exists for it.  s resampled at (n + delay) + 1e-6 slope_ppm (n - anchor) and turned by exp(-j (phase + 2 pi carrier_hz
     * (n - anchor) / fs)), n = 0 .. out_len-1; params = [delay slope_ppm carrier_hz phase anchor weight] (the weight is not used
     * here); out_len defaults to numel(s).  out: out_len x 1 complex, 0 where a tap would fall outside s; info = [status
     * first_valid end_valid num_valid] (0-based, end exclusive).  Prints the report line. */
    mwSize n = 0, k;
    const double* s;
    double info[GSMCAL_ALIGN_INFO_COLS];
    double* out;
    long out_len;
    ARGS(nrhs >= 3 && nrhs <= 4 && nlhs <= 2 && is_dbl(prhs[0]) && mxGetNumberOfElements(prhs[0]) >= 1 && is_num(prhs[1]) &&
         is_real(prhs[2]) && mxGetNumberOfElements(prhs[2]) == GSMCAL_ALIGN_PARAMS && all_num(nrhs, prhs, 3),
         "[out, info] = pair_align(s, ov, [delay slope_ppm carrier_hz phase anchor weight], out_len)");
    s = mxGetNumberOfElements(prhs[0]) > 1 ? cplx_in(prhs[0], &n) : NULL;
    out_len = nrhs > 3 ? (long)mxGetScalar(prhs[3]) : (long)n;
    if (out_len < 1) mexErrMsgIdAndTxt("gsmcal:args", "pair_align: out_len must be at least 1");
    out = (double*)mxCalloc(2 * (size_t)out_len, sizeof(double));
    chk(gsmcal_pair_align(ctx(), s, (long)n, (int)mxGetScalar(prhs[1]), REAL_PTR(prhs[2]), out_len, out, info), "pair_align");
    say();
    plhs[0] = cplx_col(out, (mwSize)out_len);
    mxFree(out);
    if (nlhs > 1) {
        plhs[1] = mxCreateDoubleMatrix(1, GSMCAL_ALIGN_INFO_COLS, mxREAL);
        for (k = 0; k < GSMCAL_ALIGN_INFO_COLS; ++k) REAL_PTR(plhs[1])[k] = info[k];
    }

#elif defined(GSMCAL_FN_total_ppm_calculation)
    /* ppm_out = total_ppm_calculation(ppm_in) */
    double out;
    ARGS(nrhs == 1 && nlhs <= 1 && is_real(prhs[0]) && mxGetNumberOfElements(prhs[0]) >= 1, "ppm_out = total_ppm_calculation(ppm_in)");
    {
        const int rc = gsmcal_total_ppm_calculation(REAL_PTR(prhs[0]), (int)mxGetNumberOfElements(prhs[0]), &out);
        chk(rc, "total_ppm_calculation");                                   /* host arithmetic: no context is made for it */
        if (rc == GSMCAL_S_ALL_INF) mexPrintf("total PPM calculation: No valid PPM input!\n");          /* total_ppm_calculation.m:8 */
    }
    plhs[0] = scalar(out);
#elif defined(GSMCAL_FN_gsmcal_calibrate)
    /* [table, pos_info] = gsmcal_calibrate(s, coef, sch_training_sequence, freq)      gsm_sync_demod.m:107-124 for all dongles
     * s: 2N x D uint8 (column = one dongle's interleaved I,Q bytes, exactly the ABI's capture-major layout);
     * table: D x 10 (columns: GSMCAL_T_*); pos_info: 1 x D cell, pos_info{i} = R x 2 (or the all -1 sentinel) */
    mwSize rows2n, d, nts, ncf, i, k;
    long n2 = 0;
    const uint8_t* raw;
    const double* ts;
    double *cf, *tab, *pi;
    ARGS(nrhs == 4 && nlhs <= 2, "[table, pos_info] = gsmcal_calibrate(s, coef, sch_training_sequence, freq)");
    if (!is_u8(prhs[0])) mexErrMsgIdAndTxt("gsmcal:type", "s must be uint8 (the bytes fread(...,'uint8') delivers)");
    rows2n = mxGetM(prhs[0]); d = mxGetN(prhs[0]); ncf = mxGetNumberOfElements(prhs[3]);
    ARGS(rows2n >= 2 && d >= 1 && is_real(prhs[1]) && mxGetNumberOfElements(prhs[1]) >= 1 && is_dbl(prhs[2]) &&
         mxGetNumberOfElements(prhs[2]) >= 1 && is_real(prhs[3]) && (ncf == 1 || ncf == d),
         "[table, pos_info] = gsmcal_calibrate(s, coef, sch_training_sequence, freq) with freq a scalar or one value per column of s");
    raw = raw_in(prhs[0], &n2);
    ts = cplx_in(prhs[2], &nts);
    cf = (double*)mxMalloc(d * sizeof(double));
    tab = (double*)mxMalloc(d * GSMCAL_TABLE_COLS * sizeof(double));
    pi = (double*)mxMalloc(d * 2 * GSMCAL_MAX_POS_ROWS * sizeof(double));
    for (i = 0; i < d; ++i) cf[i] = REAL_PTR(prhs[3])[ncf == d ? i : 0];
    chk(gsmcal_calibrate_batch(ctx(), raw, (int)d, n2, REAL_PTR(prhs[1]),
                               (int)mxGetNumberOfElements(prhs[1]), ts, (int)nts, cf, tab, pi, NULL, NULL), "gsmcal_calibrate");
    plhs[0] = mxCreateDoubleMatrix(d, GSMCAL_TABLE_COLS, mxREAL);
    for (i = 0; i < d; ++i)
        for (k = 0; k < GSMCAL_TABLE_COLS; ++k) REAL_PTR(plhs[0])[k * d + i] = tab[i * GSMCAL_TABLE_COLS + k];
    if (nlhs > 1) {
        plhs[1] = mxCreateCellMatrix(1, d);
        for (i = 0; i < d; ++i) {
            const double nr = tab[i * GSMCAL_TABLE_COLS + GSMCAL_T_N_POS_ROWS];
            const mwSize r = nr >= 0.0 && nr <= GSMCAL_MAX_POS_ROWS ? (mwSize)nr : 0;
            mxArray* m = mxCreateDoubleMatrix(r, 2, mxREAL);
            for (k = 0; k < r; ++k) {
                REAL_PTR(m)[k] = pi[i * 2 * GSMCAL_MAX_POS_ROWS + k];
                REAL_PTR(m)[r + k] = pi[i * 2 * GSMCAL_MAX_POS_ROWS + GSMCAL_MAX_POS_ROWS + k];
            }
            mxSetCell(plhs[1], i, m);
        }
    }
    mxFree(cf); mxFree(tab); mxFree(pi);

#elif defined(GSMCAL_FN_gsmcal_fcch_scan)
    /* [snr, num_hit] = gsmcal_fcch_scan(s, coef)      multi_rtl_sdr_gsm_FCCH_scanner.m:132-135,163-186 for all captures
     * s: 2N x F uint8, one column per (dongle, frequency) capture in the order of s_all (:135); snr, num_hit: 1 x F */
    mwSize rows2n, f;
    long n2 = 0;
    const uint8_t* raw;
    ARGS(nrhs == 2 && nlhs <= 2, "[snr, num_hit] = gsmcal_fcch_scan(s, coef)");
    if (!is_u8(prhs[0])) mexErrMsgIdAndTxt("gsmcal:type", "s must be uint8 (the bytes fread(...,'uint8') delivers)");
    rows2n = mxGetM(prhs[0]); f = mxGetN(prhs[0]);
    ARGS(rows2n >= 2 && f >= 1 && is_real(prhs[1]) && mxGetNumberOfElements(prhs[1]) >= 1, "[snr, num_hit] = gsmcal_fcch_scan(s, coef) with real taps");
    raw = raw_in(prhs[0], &n2);
    plhs[0] = mxCreateDoubleMatrix(1, f, mxREAL);
    {
        mxArray* nh = mxCreateDoubleMatrix(1, f, mxREAL);
        chk(gsmcal_fcch_scan_batch(ctx(), raw, (int)f, n2, REAL_PTR(prhs[1]),
                                   (int)mxGetNumberOfElements(prhs[1]), REAL_PTR(plhs[0]), REAL_PTR(nh), NULL, NULL, NULL),
            "gsmcal_fcch_scan");
        if (nlhs > 1) plhs[1] = nh;
    }
#elif defined(GSMCAL_FN_gsmcal_band_power)
    /* power = gsmcal_band_power(s_all, coef, decimate_ratio)     multi_rtl_sdr_split_scanner.m:154-156 (diversity_scanner.m:
     * 156-158 per dongle) for all captures: mean(abs(r_flt(1:decimate_ratio:end,:)).^2, 1) with r_flt = filter(coef,1,raw2iq(s_all))
     * s_all: 2N x D uint8, one column per capture; coef: real taps; power: 1 x D linear */
    mwSize rows2n, d;
    long n2 = 0;
    const uint8_t* raw;
    ARGS(nrhs == 3 && nlhs <= 1, "power = gsmcal_band_power(s_all, coef, decimate_ratio)");
    if (!is_u8(prhs[0])) mexErrMsgIdAndTxt("gsmcal:type", "s_all must be uint8 (the bytes fread(...,'uint8') delivers)");
    rows2n = mxGetM(prhs[0]); d = mxGetN(prhs[0]);
    ARGS(rows2n >= 2 && d >= 1 && is_real(prhs[1]) && mxGetNumberOfElements(prhs[1]) >= 1 && is_num(prhs[2]),
         "power = gsmcal_band_power(s_all, coef, decimate_ratio) with real taps");
    raw = raw_in(prhs[0], &n2);
    plhs[0] = mxCreateDoubleMatrix(1, d, mxREAL);
    chk(gsmcal_band_power_batch(ctx(), raw, (int)d, n2, REAL_PTR(prhs[1]),
                                (int)mxGetNumberOfElements(prhs[1]), (int)mxGetScalar(prhs[2]), REAL_PTR(plhs[0])),
        "gsmcal_band_power");
#elif defined(GSMCAL_FN_gsmcal_subband_power)
    /* power = gsmcal_subband_power(s, coef, phase_rotate [, decimate_ratio])     multi_rtl_sdr_diversity_scanner_another_bak.m:192-204
     * for all captures and all their sub-frequencies: power(j,c) = mean(abs(filter(coef,1,raw2iq(s(:,c)).*exp(1i*(1:N)'*phase_rotate(j,c)))).^2)
     * s: 2N x D uint8, one column per capture; coef: real taps (at most 128); phase_rotate: J x D (J <= GSMCAL_MAX_SUBBANDS), NaN = unused
     * slot; power: J x D linear, NaN in unused slots.  decimate_ratio (default 1, the script) keeps rows 1:decimate_ratio:end. */
    mwSize rows2n, d;
    long n2 = 0;
    const uint8_t* raw;
    ARGS(nrhs >= 3 && nrhs <= 4 && nlhs <= 1, "power = gsmcal_subband_power(s, coef, phase_rotate, decimate_ratio)");
    if (!is_u8(prhs[0])) mexErrMsgIdAndTxt("gsmcal:type", "s must be uint8 (the bytes fread(...,'uint8') delivers)");
    rows2n = mxGetM(prhs[0]); d = mxGetN(prhs[0]);
    ARGS(rows2n >= 2 && d >= 1 && is_real(prhs[1]) && mxGetNumberOfElements(prhs[1]) >= 1 && is_real(prhs[2]) && mxGetM(prhs[2]) >= 1 &&
         mxGetN(prhs[2]) == d && all_num(nrhs, prhs, 3),
         "power = gsmcal_subband_power(s, coef, phase_rotate, decimate_ratio) with phase_rotate J x size(s,2)");
    raw = raw_in(prhs[0], &n2);
    plhs[0] = mxCreateDoubleMatrix(mxGetM(prhs[2]), d, mxREAL);
    chk(gsmcal_subband_power_batch(ctx(), raw, (int)d, n2, REAL_PTR(prhs[1]),
                                   (int)mxGetNumberOfElements(prhs[1]), nrhs > 3 ? (int)mxGetScalar(prhs[3]) : 1, REAL_PTR(prhs[2]),
                                   (int)mxGetM(prhs[2]), REAL_PTR(plhs[0])), "gsmcal_subband_power");
#else
#error "define one GSMCAL_FN_<function> (see the header comment)"
#endif
    (void)nrhs; (void)nlhs;
}
