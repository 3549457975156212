/* gsmcal.h -- C ABI of libgsmcal.so: the GSM FCCH+SCH calibration DSP chain of
 * JiaoXianjun/multi-rtl-sdr-calibration on AMD MI355X (gfx950), hand-written HIP kernels.
 *
 * The reference has no FFI layer: the path sits behind MATLAB function calls
 * (gsm_sync_demod.m:107-124, multi_rtl_sdr_gsm_FCCH_scanner.m:132-135,164).  Each entry point
 * below replaces one reference function -- the file:line it replaces is cited -- with the same
 * argument meaning, the same 1-based positions held in doubles, and the same sentinel outputs
 * (position = -1, r = -1, ppm = inf, pos_info = [-1 -1]).  A MEX gateway (mex/gsmcal_mex.c) or the
 * ctypes mirror (multi-rtl-sdr-calibration_amd/api.py) binds them; see INTEGRATION.md.
 *
 * Conventions
 *   - complex data: interleaved double[2] (re, im), column-major like MATLAB's interleaved API.
 *   - host entry points (no suffix) take HOST pointers, copy, run on the GPU, and return after the
 *     stream has drained.  `_dev` entry points take DEVICE pointers, only enqueue work on the
 *     context's HIP stream and return; call gsmcal_sync() before reading results.
 *   - return value: 0 = ok; > 0 = the reference's algorithmic sentinel was produced (outputs hold
 *     the sentinel values, exactly as the .m file would return them); < 0 = API / HIP failure
 *     (outputs undefined).  Where MATLAB itself would stop with an index error (SURVEY 8a pitfall
 *     12) the call returns GSMCAL_E_INDEX instead of reading out of bounds.
 *   - a context is bound to one GPU and one HIP stream and is not thread-safe.
 *   - there is no CPU fallback: without a usable gfx950 device gsmcal_ctx_create fails.
 */
#ifndef GSMCAL_H
#define GSMCAL_H

#include <stddef.h>
#include <stdint.h>

#include "gsmcal_si.h"   /* gsmcal_si_info, gsmcal_si_fields: the parser of a decoded BCCH block (plain C, header only) */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsmcal_ctx gsmcal_ctx;

/* ---- status codes ---------------------------------------------------------------------------- */
enum {
    GSMCAL_OK = 0,
    /* > 0: algorithmic sentinels (the reference returns normally with sentinel outputs) */
    GSMCAL_S_NO_FCCH = 1,         /* FCCH_coarse_position.m:27-30   position = snr = -1          */
    GSMCAL_S_FEW_HITS = 2,        /* FCCH_fine_correction.m:12-15 / SCH_corr_rate_correction.m:11 */
    GSMCAL_S_FINE_FEW = 3,        /* FCCH_fine_correction.m:69: fewer than 5 fine positions       */
    GSMCAL_S_FINE_SPACING = 4,    /* FCCH_fine_correction.m:95-102  FCCH_pos = -1                 */
    GSMCAL_S_FINE_FEW_BURSTS = 5, /* FCCH_fine_correction.m:135-142 <5 bursts left, carrier skipped*/
    GSMCAL_S_FINE_LOW_SNR = 6,    /* FCCH_fine_correction.m:192-196 FCCH_pos = -1                 */
    GSMCAL_S_SCH_EDGE = 7,        /* SCH_corr_rate_correction.m:59-63 pos_info = [-1 -1]          */
    GSMCAL_S_SCH_FEW = 8,         /* SCH_corr_rate_correction.m:84: fewer than 5 SCH positions    */
    GSMCAL_S_SCH_SPACING = 9,     /* SCH_corr_rate_correction.m:106-112                           */
    GSMCAL_S_POST_NO_POS = 10,    /* carrier_correct_post_SCH.m:10-13                             */
    GSMCAL_S_POST_FEW_BCCH = 11,  /* carrier_correct_post_SCH.m:15-19                             */
    GSMCAL_S_ALL_INF = 12,        /* total_ppm_calculation.m:7-11                                 */
    GSMCAL_S_BCCH_TSC_MIXED = 13, /* BCCH_demod.m:103-105: the first four BCCH bursts disagree     */
    GSMCAL_S_SCH_NO_DECODE = 14,  /* gsmcal_SCH_decode: fewer than two SCH bursts decode consistently */
    GSMCAL_S_BCCH_NO_DECODE = 15, /* gsmcal_BCCH_decode: no BCCH block passes the Fire code's check   */
    GSMCAL_S_PAIR_FEW = 16,       /* gsmcal_pair_coherence: fewer than two bursts of the pair are used */
    GSMCAL_S_ALIGN_SKIPPED = 17,  /* gsmcal_pair_align: a value of the member's parameter row is not finite */
    GSMCAL_S_WEIGHTS_SINGULAR = 18, /* gsmcal_combine_weights: a value that is not finite, a Cholesky pivot <= 0, or lambda_1 <= 0 */
    /* < 0: failures */
    GSMCAL_E_ARG = -1,
    GSMCAL_E_HIP = -2,
    GSMCAL_E_NO_DEVICE = -3,
    GSMCAL_E_CAPACITY = -4,       /* an output buffer capacity argument is too small             */
    GSMCAL_E_INDEX = -5,          /* MATLAB would raise "index exceeds matrix dimensions"         */
    GSMCAL_E_UNSUPPORTED = -6
};

#define GSMCAL_MAX_HITS 24          /* capacity for FCCH/SCH hits per stream (ceil(len/1562.5)) */
#define GSMCAL_MAX_POS_ROWS (6 * GSMCAL_MAX_HITS)
#define GSMCAL_TABLE_COLS 10
#define GSMCAL_DEMOD_COLS (4 + 3 * GSMCAL_MAX_HITS)   /* one row of gsmcal_fcch_demod_batch[_dev]: 76 doubles */
#define GSMCAL_MAX_BCCH (4 * GSMCAL_MAX_HITS)         /* BCCH bursts (type-2 rows of pos_info) gsmcal_bcch_demod_batch evaluates */
#define GSMCAL_BCCH_COLS (6 + 4 * GSMCAL_MAX_BCCH)    /* one row of gsmcal_bcch_demod_batch[_dev]: 390 doubles */
#define GSMCAL_SCH_COLS (8 + 7 * GSMCAL_MAX_HITS)      /* one row of gsmcal_sch_decode_batch[_dev]: 176 doubles */
#define GSMCAL_SI_COLS (4 + 7 * GSMCAL_MAX_HITS)       /* one row of gsmcal_bcch_decode_batch[_dev]: 172 doubles */
#define GSMCAL_BLOCK_OCTETS 23                         /* octets of one BCCH block (GSMCAL_SI_OCTETS of gsmcal_si.h) */
#define GSMCAL_BLOCK_CODED 456                         /* coded bits of one BCCH block */
#define GSMCAL_MAX_PAIR_BURSTS (GSMCAL_MAX_HITS + GSMCAL_MAX_BCCH)   /* type-1 and type-2 rows gsmcal_pair_coherence_batch evaluates: 120 */
#define GSMCAL_PAIR_COLS (16 + 6 * GSMCAL_MAX_PAIR_BURSTS)           /* one row of gsmcal_pair_coherence_batch[_dev]: 736 doubles */
#define GSMCAL_MAX_ALIGN_MEMBERS 64                    /* members of one gsmcal_pair_align_batch[_dev] call */
#define GSMCAL_ALIGN_PARAMS 6                          /* one member's row: delay, slope_ppm, carrier_hz, phase, anchor, weight */
#define GSMCAL_ALIGN_INFO_COLS 4                       /* one row of the info table of gsmcal_pair_align_batch[_dev] */
#define GSMCAL_ALIGN_TAPS 16                           /* taps of the interpolator, k = -7 .. 8 */
#define GSMCAL_MAX_COV_WINDOWS 256                     /* windows of one gsmcal_array_covariance_batch[_dev] call */
#define GSMCAL_COV_CHUNK 512                           /* samples of one partial sum of gsmcal_array_covariance_batch[_dev], counted from the window's start */
#define GSMCAL_MAX_BEAMS 16                            /* weight vectors of one gsmcal_array_combine_batch[_dev] call */
#define GSMCAL_WEIGHTS_INFO_COLS 4                     /* info of gsmcal_combine_weights: status, lambda_1, lambda_2, sweeps */

/* columns of one row of the calibration table (doubles; this row is what ranks all-gather) */
enum {
    GSMCAL_T_SAMPLING_PPM_FCCH = 0, /* FCCH_fine_correction sampling_ppm      (gsm_sync_demod.m:118) */
    GSMCAL_T_SAMPLING_PPM_SCH = 1,  /* SCH_corr_rate_correction sampling_ppm  (:119)                 */
    GSMCAL_T_CARRIER_PPM_FCCH = 2,  /* FCCH_fine_correction carrier_ppm       (:118)                 */
    GSMCAL_T_CARRIER_PPM_POST = 3,  /* carrier_correct_post_SCH carrier_ppm   (:120)                 */
    GSMCAL_T_TOTAL_SAMPLING_PPM = 4,/* total_ppm_calculation                  (:123)                 */
    GSMCAL_T_TOTAL_CARRIER_PPM = 5, /* total_ppm_calculation                  (:124)                 */
    GSMCAL_T_N_FCCH = 6,            /* length(FCCH_pos) after FCCH_fine_correction (1 if sentinel)   */
    GSMCAL_T_N_POS_ROWS = 7,        /* rows of pos_info (1 if sentinel)                              */
    GSMCAL_T_FIRST_FCCH_POS = 8,    /* pos_info(1,1) or -1                                           */
    GSMCAL_T_STATUS = 9             /* first non-zero status code met along the chain               */
};

/* columns of one row of the FCCH_demod table (doubles) */
enum {
    GSMCAL_D_NUM_FCCH = 0,                          /* type-0 rows of pos_info                    FCCH_demod.m:20 */
    GSMCAL_D_MEAN_FREQ = 1,                         /* mean(freq), NaN without a burst            :44             */
    GSMCAL_D_CARRIER_PPM = 2,                       /* 1e6*(mean_freq - symbol_rate/4)/carrier    :47-48          */
    GSMCAL_D_STATUS = 3,                            /* 0, GSMCAL_S_POST_NO_POS, GSMCAL_E_CAPACITY or GSMCAL_E_INDEX */
    GSMCAL_D_FREQ = 4,                              /* [GSMCAL_MAX_HITS] tone frequency per burst :42             */
    GSMCAL_D_SNR = 4 + GSMCAL_MAX_HITS,             /* [GSMCAL_MAX_HITS] in-band SNR, dB          :62             */
    GSMCAL_D_MAX_IDX = 4 + 2 * GSMCAL_MAX_HITS      /* [GSMCAL_MAX_HITS] max_idx - (fft_len/2+1)  :66             */
};

/* columns of one row of the BCCH_demod table (doubles) */
enum {
    GSMCAL_B_NUM_BCCH = 0,                          /* type-2 rows of pos_info (0 at GSMCAL_S_POST_NO_POS)    BCCH_demod.m:13  */
    GSMCAL_B_TSC_IDX = 1,                           /* normal_training_sequence_idx: 1..8, or -1              :102             */
    GSMCAL_B_MEAN_FO = 2,                           /* mean(fo) of the FCCH bursts, NaN without one           :70              */
    GSMCAL_B_CARRIER_PPM = 3,                       /* 1e6*(fo - symbol_rate/4)/carrier_freq                  :71              */
    GSMCAL_B_STATUS = 4,                            /* 0, GSMCAL_S_POST_NO_POS, _S_POST_FEW_BCCH, _S_BCCH_TSC_MIXED, _E_CAPACITY, _E_INDEX */
    GSMCAL_B_NUM_AGREE = 5,                         /* evaluated bursts whose idx equals the first burst's                     */
    GSMCAL_B_IDX = 6,                               /* [GSMCAL_MAX_BCCH] first maximum of |corr_val| per burst, 1..8  :99      */
    GSMCAL_B_PEAK = 6 + GSMCAL_MAX_BCCH,            /* [GSMCAL_MAX_BCCH] |corr_val| of the winner                              */
    GSMCAL_B_RUNNER_UP = 6 + 2 * GSMCAL_MAX_BCCH,   /* [GSMCAL_MAX_BCCH] the second largest |corr_val|                         */
    GSMCAL_B_PHASE = 6 + 3 * GSMCAL_MAX_BCCH        /* [GSMCAL_MAX_BCCH] angle of the winning correlation                      */
};

/* columns of one row of the SCH_decode table (doubles) */
enum {
    GSMCAL_C_NUM_SCH = 0,                           /* type-1 rows of pos_info (0 at GSMCAL_S_POST_NO_POS)                     */
    GSMCAL_C_NUM_OK = 1,                            /* bursts whose decoded word passes every check                            */
    GSMCAL_C_NUM_CONSISTENT = 2,                    /* c_anchor: ok bursts that agree with the anchor on BSIC and frame count  */
    GSMCAL_C_BSIC = 3,                              /* the cell's BSIC (0..63; the low three bits are the colour code), or -1  */
    GSMCAL_C_FN_ANCHOR = 4,                         /* GSM frame number of the anchor burst, or -1                             */
    GSMCAL_C_POS_ANCHOR = 5,                        /* 1-based start sample of the anchor burst, or -1                         */
    GSMCAL_C_STATUS = 6,                            /* 0, GSMCAL_S_POST_NO_POS, GSMCAL_S_SCH_NO_DECODE, GSMCAL_E_CAPACITY      */
    GSMCAL_C_MEAN_SLOPE = 7,                        /* mean of slope[] over the ok bursts (rad/symbol), NaN without one        */
    GSMCAL_C_OK = 8,                                /* [GSMCAL_MAX_HITS] 1 / 0; NaN: the burst was not evaluated               */
    GSMCAL_C_BSIC_B = 8 + GSMCAL_MAX_HITS,          /* [GSMCAL_MAX_HITS] BSIC of an ok burst, NaN otherwise                    */
    GSMCAL_C_FN = 8 + 2 * GSMCAL_MAX_HITS,          /* [GSMCAL_MAX_HITS] frame number of an ok burst, NaN otherwise            */
    GSMCAL_C_TS_ERR = 8 + 3 * GSMCAL_MAX_HITS,      /* [GSMCAL_MAX_HITS] hard errors in the 64 training bits                   */
    GSMCAL_C_CORRECTED = 8 + 4 * GSMCAL_MAX_HITS,   /* [GSMCAL_MAX_HITS] hard channel bits that differ from the re-encoded word */
    GSMCAL_C_SLOPE = 8 + 5 * GSMCAL_MAX_HITS,       /* [GSMCAL_MAX_HITS] phase slope across the burst, rad/symbol              */
    GSMCAL_C_AMP = 8 + 6 * GSMCAL_MAX_HITS          /* [GSMCAL_MAX_HITS] |h| / 64                                              */
};

/* columns of one row of the BCCH_decode table (doubles) */
enum {
    GSMCAL_I_NUM_BLOCKS = 0,                        /* type-1 rows of pos_info that four type-2 rows follow (0 at GSMCAL_S_POST_NO_POS) */
    GSMCAL_I_NUM_OK = 1,                            /* blocks whose decoded word passes the Fire code and the tail check       */
    GSMCAL_I_STATUS = 2,                            /* 0, GSMCAL_S_POST_NO_POS, GSMCAL_S_BCCH_NO_DECODE, GSMCAL_E_CAPACITY     */
    GSMCAL_I_FIRST_OK = 3,                          /* 1-based index of the first ok block, -1 without one                     */
    GSMCAL_I_OK = 4,                                /* [GSMCAL_MAX_HITS] 1 / 0; NaN: the block was not evaluated               */
    GSMCAL_I_POS = 4 + GSMCAL_MAX_HITS,             /* [GSMCAL_MAX_HITS] 1-based start sample of the block's first burst       */
    GSMCAL_I_CORRECTED = 4 + 2 * GSMCAL_MAX_HITS,   /* [GSMCAL_MAX_HITS] hard channel bits (of 456) that differ from the re-encoded word */
    GSMCAL_I_TS_ERR = 4 + 3 * GSMCAL_MAX_HITS,      /* [GSMCAL_MAX_HITS] hard errors in the 4 x 26 mid-amble bits              */
    GSMCAL_I_STEAL = 4 + 4 * GSMCAL_MAX_HITS,       /* [GSMCAL_MAX_HITS] stealing flags read as one, 0..8 (a BCCH block: 8)    */
    GSMCAL_I_MEAN_SLOPE = 4 + 5 * GSMCAL_MAX_HITS,  /* [GSMCAL_MAX_HITS] mean phase slope of the four bursts, rad/symbol       */
    GSMCAL_I_AMP = 4 + 6 * GSMCAL_MAX_HITS          /* [GSMCAL_MAX_HITS] mean of the four bursts' |h| / 26                     */
};

/* columns of one row of the pair_coherence table (doubles) */
#define GSMCAL_P_STATUS 0               /* 0, GSMCAL_S_POST_NO_POS, GSMCAL_S_PAIR_FEW, GSMCAL_E_CAPACITY                         */
#define GSMCAL_P_NUM_BURSTS 1           /* type-1 and type-2 rows of a's pos_info (0 at GSMCAL_S_POST_NO_POS)                    */
#define GSMCAL_P_NUM_EVAL 2             /* bursts whose two windows lie inside the streams                                       */
#define GSMCAL_P_NUM_USED 3             /* evaluated, not at the edge of the lag range, coherence >= min_coherence               */
#define GSMCAL_P_NUM_ADJACENT 4         /* steps between consecutive used bursts at most 1.5 frames apart                        */
#define GSMCAL_P_LAG0 5                 /* the pair's lag0, as given                                                             */
#define GSMCAL_P_DELAY0 6               /* delay of b against a at the first used burst, samples (the fitted line at t = 0)      */
#define GSMCAL_P_REL_SAMPLING_PPM 7     /* 1e6 * slope of that line                                                              */
#define GSMCAL_P_DELAY_RMS 8            /* rms of the delays about the line, samples                                             */
#define GSMCAL_P_REL_CARRIER_HZ 9       /* carrier of b against a: burst_carrier_hz refined by the adjacent phase steps          */
#define GSMCAL_P_BURST_CARRIER_HZ 10    /* mean of freq[] over the used bursts                                                   */
#define GSMCAL_P_PHASE0 11              /* phase of b against a at the centre of the first used burst, rad                       */
#define GSMCAL_P_PHASE_RMS 12           /* rms of the used bursts' phases about phase0 + 2 pi rel_carrier_hz t / fs, rad         */
#define GSMCAL_P_MEAN_COHERENCE 13      /* mean of coherence[] over the used bursts                                              */
#define GSMCAL_P_MIN_COHERENCE_SEEN 14  /* ... and the smallest                                                                  */
#define GSMCAL_P_MAX_LAG 15             /* M, as used                                                                            */
#define GSMCAL_P_POS 16                                     /* [GSMCAL_MAX_PAIR_BURSTS] the burst's row of a's table, 1-based    */
#define GSMCAL_P_DELAY (16 + GSMCAL_MAX_PAIR_BURSTS)        /* [..] lag0 + m* + the parabola's offset, samples                  */
#define GSMCAL_P_PHASE (16 + 2 * GSMCAL_MAX_PAIR_BURSTS)    /* [..] phase of b against a at the burst's centre, rad             */
#define GSMCAL_P_FREQ (16 + 3 * GSMCAL_MAX_PAIR_BURSTS)     /* [..] segment-to-segment phase step as a frequency, Hz            */
#define GSMCAL_P_COH (16 + 4 * GSMCAL_MAX_PAIR_BURSTS)      /* [..] sum |c_k| / sqrt(sum Ea sum Eb), <= 1                       */
#define GSMCAL_P_EDGE (16 + 5 * GSMCAL_MAX_PAIR_BURSTS)     /* [..] 1: the maximum sits at -M or +M (delay .. coherence NaN); 0 */

/* columns of one member's parameter row of pair_align (doubles) */
#define GSMCAL_A_DELAY 0                /* position of output sample `anchor` in the member's stream minus anchor, samples        */
#define GSMCAL_A_SLOPE_PPM 1            /* 1e6 * how much faster than the output index the position advances, |.| <= 1000          */
#define GSMCAL_A_CARRIER_HZ 2           /* carrier to take out, Hz of the OUTPUT time base                                         */
#define GSMCAL_A_PHASE 3                /* carrier phase to take out at output sample `anchor`, rad                                */
#define GSMCAL_A_ANCHOR 4               /* output index the drift and the carrier are counted from                                 */
#define GSMCAL_A_WEIGHT 5               /* the member's weight in the sum                                                          */
/* columns of the info table of pair_align (doubles): rows 0 .. G-1 the members, row G the sum */
#define GSMCAL_AI_STATUS 0              /* member: 0, GSMCAL_S_POST_NO_POS, GSMCAL_S_ALIGN_SKIPPED      sum: members with status 0  */
#define GSMCAL_AI_FIRST_VALID 1         /* member: first valid output index (0 with none)               sum: the largest of them    */
#define GSMCAL_AI_END_VALID 2           /* member: one past the last valid output index (0 with none)   sum: the smallest, >= first */
#define GSMCAL_AI_NUM_VALID 3           /* member: end_valid - first_valid                              sum: sum of the used weights */

/* ---- algorithm thresholds (the constants the reference hard-codes inside its functions) ---------- */
/* Defaults = the reference's literals.  gsmcal_set_params() takes effect from the next call on (calls in flight finish with the
 * values they were made under; a captured graph is never replayed across a change); the fields marked "geometry" size windows
 * and launch shapes and must keep their default (any other value: GSMCAL_E_UNSUPPORTED).
 * Accepted ranges (anything else: GSMCAL_E_ARG, and the context keeps the values it had):
 *   min_hits        2 .. GSMCAL_MAX_HITS (24)
 *   scan_min_hits   >= 1.  At 1 a capture in which nothing was found is accepted as the reference's rule would accept it: its
 *                   FCCH_pos = FCCH_snr = -1 is one element with no gap to refuse, so snr = -1 and num_hit = 1
 *   post_min_bcch   >= 0 (0: the :15 exit is never taken)
 *   coarse_th_db, fine_max_ppm, fine_gate_snr_db, sch_max_ppm, scan_spacing, scan_spacing_idle, scan_tol
 *                   any double but NaN, infinities included (every comparison with NaN is false: refused, not defined).
 *                   Comparisons are the reference's strict ones: hit iff snr - avg > coarse_th_db; a gap is in a spacing class
 *                   iff |gap - 10 or 11 frames| < floor(frames * max_ppm * 1e-6); gate iff snr < fine_gate_snr_db; a scanner gap
 *                   is refused iff |gap - spacing| > scan_tol.  coarse_th_db below -989 lets the first window hit (the moving
 *                   average is seeded with 999 dB): the fine stage then answers GSMCAL_E_INDEX, as MATLAB would stop.
 *                   fine_max_ppm / sch_max_ppm above 47 619 let one gap pass both class tests: it counts twice at :95 / :106,
 *                   and where the count still fits the eleven-frame class wins (:129-130).
 *                   Raising them does not widen what the resampling stages can follow: their tile and window buffers are sized for
 *                   the reference's bounds plus a tenth, and a measured stretch above +4400 ppm (FCCH_fine_correction.m:113) or
 *                   +440 ppm (SCH_corr_rate_correction.m:116) is answered with GSMCAL_E_UNSUPPORTED -- in the table's status
 *                   column for a batch row -- instead of the reference's resampled stream.  From raw bytes the search windows
 *                   themselves keep the error far below that; hand-given positions can exceed it. */
typedef struct gsmcal_params {
    double coarse_th_db;        /* FCCH_coarse_position.m:21          th = 10            hit iff snr - avg > th            */
    int coarse_mv_factor;       /* FCCH_coarse_position.m:22          mv_len = 10*fft_len                     (geometry)  */
    int coarse_max_offset;      /* FCCH_coarse_position.m:45          max_offset = 5                          (geometry)  */
    int min_hits;               /* FCCH_fine_correction.m:12,69,142; SCH_corr_rate_correction.m:11,84        5            */
    int fine_max_offset;        /* FCCH_fine_correction.m:30          max_offset = 64 symbols                 (geometry)  */
    double fine_max_ppm;        /* FCCH_fine_correction.m:83          max_ppm = 4000     spacing classes                  */
    double fine_gate_snr_db;    /* FCCH_fine_correction.m:192         FCCH_snr < 5  ->  FCCH_pos = -1                     */
    double fine_noise_bw_hz;    /* FCCH_fine_correction.m:22          200e3: half_noise_len                   (geometry)  */
    int sch_max_offset;         /* SCH_corr_rate_correction.m:36      max_offset = 8 symbols                  (geometry)  */
    double sch_max_ppm;         /* SCH_corr_rate_correction.m:94      max_ppm = 400                                       */
    int post_min_bcch;          /* carrier_correct_post_SCH.m:15      fewer than 4 BCCH rows -> r = -1                    */
    int scan_min_hits;          /* multi_rtl_sdr_gsm_FCCH_scanner.m:169  at least 3 hits                                  */
    double scan_spacing;        /* ..FCCH_scanner.m:171               12500 (1x symbols between FCCH bursts)              */
    double scan_spacing_idle;   /* ..FCCH_scanner.m:176               12500 + 1250 across the idle frame                  */
    double scan_tol;            /* ..FCCH_scanner.m:171,176           50                                                  */
} gsmcal_params;
void gsmcal_params_default(gsmcal_params* p);
int gsmcal_set_params(gsmcal_ctx* ctx, const gsmcal_params* p);
int gsmcal_get_params(gsmcal_ctx* ctx, gsmcal_params* p);

/* ---- context --------------------------------------------------------------------------------- */
/* Creates a context on GPU `device_id` with its own non-blocking HIP stream. */
int gsmcal_ctx_create(int device_id, gsmcal_ctx** out);
/* Same, but enqueue on an existing hipStream_t (passed as void*; 0 = the default stream). */
int gsmcal_ctx_create_on_stream(int device_id, void* hip_stream, gsmcal_ctx** out);
void gsmcal_ctx_destroy(gsmcal_ctx* ctx);
int gsmcal_sync(gsmcal_ctx* ctx);
const char* gsmcal_last_error(gsmcal_ctx* ctx);
/* The reference's console diagnostics.  The .m files disp() their intermediate results -- "FCCH coarse: hit successive
 * 10 FCCH. pos ...", "FCCH fine: first round diff ...", "FCCH fine: FCCH freq ...", "SCH: sampling error ppm ...", the warnings of
 * every early exit (FCCH_coarse_position.m:6,28,92-94, FCCH_fine_correction.m:6,13,66,96-99,116,156-161,190-193,
 * SCH_corr_rate_correction.m:6,12,60,80,107-110,118, carrier_correct_post_SCH.m:6,11,17,73-79) -- and a MEX file that shadows one
 * would otherwise run silent.  After gsmcal_FCCH_coarse_position / _FCCH_fine_correction / _SCH_corr_rate_correction /
 * _carrier_correct_post_SCH this returns the lines that call's .m file would have printed, '\n'-separated, numbers formatted as
 * MATLAB's num2str formats them (gsmcal_num2str: the same formatter, for row vectors).  gsmcal_FCCH_demod, gsmcal_BCCH_demod, gsmcal_SCH_decode and gsmcal_BCCH_decode leave their lines too.  buf may be NULL; the return value is the
 * text's length without the terminator.  The gateway mexPrintf()s it; the Python mirror prints it when GSMCAL_VERBOSE=1. */
long gsmcal_last_call_report(gsmcal_ctx* ctx, char* buf, size_t cap);
long gsmcal_num2str(const double* x, int n, char* buf, size_t cap);
const char* gsmcal_version(void);
/* Bytes of LDS the coarse scan keeps for itself in front of its len + mv_len + 128 window SNRs (the size of the per-stream state
 * is in it): what bounds len + mv_len in the three coarse-detector entry points below. */
long gsmcal_coarse_scan_lds_fixed(void);
/* Pipelined batch calls (round 6).  gsm_sync_demod.m:107-124 is a serial chain per batch of dongles; a service that calibrates batch
 * after batch does not need batch i finished before batch i+1 starts.  With depth D > 1, up to D consecutive
 * gsmcal_calibrate_batch_dev calls that run on one lane (up to 127 streams) are in flight at once: call i runs on internal HIP
 * stream i mod D, in workspace i mod D, with the four-launch tail (whose kernels never wait for each other), and the kernels of the
 * calls in flight interleave on the GPU -- 64 streams x 1 020 000: 0.177 ms per call at depth 1, 0.148 at 3, 0.138 at 4 (the device
 * schedules four hardware queues: more gain nothing; with r_correct written calls in flight are supported and gain nothing).  The
 * same holds for single-stage gsmcal_fcch_scan_batch_dev calls (fewer than 1 200 captures; multi_rtl_sdr_gsm_FCCH_scanner.m:132-135,
 * 163-186 over consecutive sweeps): the detector of call i runs under the front kernel of call i+1 -- 200 captures 0.086 -> 0.068 ms.
 *   depth 1 (default): every call is complete in the context's stream order when it returns: the semantics of every earlier release.
 *   depth D = 2..8: the outputs of call i (table, pos_info, r_len) are complete in the context's stream order at the start of call
 *     i+D, or after gsmcal_sync(), or after ANY other entry point of this context (they all join the calls in flight first).  The
 *     raw bytes and output buffers of call i must stay untouched until then: give D consecutive calls distinct output buffers.
 *     Each call starts behind whatever the context's stream held when it was made (its input is ordered like at depth 1).
 *     (Inside call i+D the library first hands the context's stream position to the internal stream and only then makes the
 *     context's stream wait for the end of call i: call i+D follows call i on the same in-order internal stream anyway, so its
 *     first kernel does not wait for that join, and the outputs of call i are complete in the context's stream order when call
 *     i+D RETURNS -- work the caller enqueues on the context's stream after that sees them.)
 *     gsmcal_allgather_table[_async] right behind a pipelined call is enqueued behind THAT call (the gathered table completes where
 *     the call's own outputs do).  gsmcal_last_batch_details describes the most recent call.
 * Results are identical at every depth (same kernels, same order per call).  Returns GSMCAL_E_ARG for depth < 1 or > 8.
 * (The staged forms of the first design -- a call cut into front end | fine search | fused tail on stage streams -- measured no gain
 * and are not in the library: profiles/experiments_r06/staged_pipeline_and_side_fused.patch, profiles/NOTES_r06.md.) */
int gsmcal_ctx_set_pipeline_depth(gsmcal_ctx* ctx, int depth);
int gsmcal_ctx_get_pipeline_depth(gsmcal_ctx* ctx);
/* How many internal streams the context has SEEN running side by side (= hardware queues its calls in flight are spread over; the
 * runtime hands out four): 0 before the first call in flight.  The context creates a dozen candidate streams at that call, keeps
 * those that pass a 200-us pairwise probe and maps slot s to kept stream s mod that number -- which streams share a hardware queue
 * depends on every stream the process created before (under PyTorch four streams created in a row landed on three queues). */
int gsmcal_ctx_pipeline_queues(gsmcal_ctx* ctx);
/* Diagnostics of the batch path's fused tail (one launch for everything behind the fine search's chunk sweep: its workgroups
 * exchange results inside the launch).  Several contexts may drive one GPU from several host threads; the library lets only one
 * such launch of the process be in flight per device and gives the later caller the four-launch tail (same results).
 * fused_launches: batch calls of this context that took the fused tail; gate_fallbacks: calls that would have but found
 * another context's fused tail unfinished (or ran inside the caller's own stream capture, where replays cannot be gated). */
int gsmcal_fused_tail_stats(gsmcal_ctx* ctx, unsigned long long* fused_launches, unsigned long long* gate_fallbacks);
/* The gate above is per process.  A fused tail stalled by ANOTHER process's fused tail on the same GPU gives up after
 * GSMCAL_FUSED_POLL_S seconds (default 3) and reports it through a pinned host word; gsmcal_sync() and the host-buffer entry
 * points then run the affected calls again with the four-launch tail (same inputs -- which the caller leaves untouched until it
 * has synchronised -- same outputs) and return 0: the time-out costs seconds, not the call.  A caller that synchronises its
 * stream without gsmcal_sync() sees GSMCAL_E_HIP in the status column of the affected rows instead.  Returns how often that
 * happened on this context (test hook: GSMCAL_TEST_FUSED_STALL=<stage 1..4> makes one workgroup never publish). */
long long gsmcal_fused_tail_reruns(gsmcal_ctx* ctx);
/* device memory helpers so a host program needs no HIP headers */
int gsmcal_dev_alloc(gsmcal_ctx* ctx, size_t bytes, void** dptr);
int gsmcal_dev_free(gsmcal_ctx* ctx, void* dptr);
int gsmcal_memcpy_h2d(gsmcal_ctx* ctx, void* dst, const void* src, size_t bytes);
int gsmcal_memcpy_d2h(gsmcal_ctx* ctx, void* dst, const void* src, size_t bytes);
/* Per-kernel timing with HIP events on the context's stream.  enable=1 brackets every kernel launch
 * with events (serialises nothing, adds two event records per launch).  Stats accumulate until reset. */
int gsmcal_profile_enable(gsmcal_ctx* ctx, int enable);
int gsmcal_profile_reset(gsmcal_ctx* ctx);
/* Restrict the bracketing to kernels whose name contains `substr` (NULL or "" = every kernel), so a
 * timed region can carry events for one kernel only. */
int gsmcal_profile_filter(gsmcal_ctx* ctx, const char* substr);
/* Returns the number of distinct kernels seen; fills up to `cap` entries (name pointers stay valid
 * for the life of the library). total_ms[i] is the summed duration, launches[i] the launch count. */
int gsmcal_profile_get(gsmcal_ctx* ctx, int cap, const char** names, double* total_ms, long* launches);

/* ---- the nine reference functions, MATLAB signatures (host pointers, synchronous) -------------- */

/* b = raw2iq(a)                                                     raw2iq.m:5-8
 * a: 2N x D doubles holding byte values (column-major); b: N x D complex. */
int gsmcal_raw2iq(gsmcal_ctx* ctx, const double* a, long rows_2n, int d, double* b);
/* same with the bytes as they come off the wire (fread(...,'uint8') before MATLAB widens them) */
int gsmcal_raw2iq_u8(gsmcal_ctx* ctx, const uint8_t* a, long rows_2n, int d, double* b);

/* r = chn_filter_8x_4x(s)                                           chn_filter_8x_4x.m:5-15
 * s: N x D complex; r: ceil(N/2) x D complex.  `num`/`ntaps`: the numerator the reference loads
 * from gsm_chn_filter_8x.mat (:9-10); pass NULL/0 to use the built-in 60 taps of
 * gsm_chn_filter_8x.fda. */
int gsmcal_chn_filter_8x_4x(gsmcal_ctx* ctx, const double* s, long n, int d,
                            const double* num, int ntaps, double* r);
/* r = chn_filter_4x(s)                                              chn_filter_4x.m:5-13
 * Single-rate channel filter at 4x oversampling: s, r: N x D complex.  `num`/`ntaps`: the numerator the
 * reference loads from gsm_chn_filter_4x.mat (:8-9); NULL/0 = the built-in 30 taps of gsm_chn_filter_4x.fda. */
int gsmcal_chn_filter_4x(gsmcal_ctx* ctx, const double* s, long n, int d, const double* num, int ntaps, double* r);
/* r = filter(coef, 1, s) column-wise (gsm_sync_demod.m:110, multi_rtl_sdr_gsm_FCCH_scanner.m:133);
 * keep every `decim`-th row starting with row 1 (decim = 1: all rows; the drivers' r(1:64:end,i)).
 * Any ntaps >= 1, decim >= 1, n >= 1 (n below ntaps or decim included): r has ceil(n/decim) rows; nothing is staged, so there is
 * no upper limit on decim. */
int gsmcal_filter(gsmcal_ctx* ctx, const double* coef, int ntaps, const double* s, long n, int d,
                  int decim, double* r);

/* [hit_flag,hit_idx,hit_avg_snr,hit_snr] = move_fft_snr_runtime_avg(s,mv_len,fft_len,th)
 *                                                                    move_fft_snr_runtime_avg.m:5-50
 * Supported geometry of the three coarse-detector entry points (tests/test_gpu_geometry.py pins it):
 *   fft_len 2 .. 64 (16: the radix-2 kernels; any other length: direct DFTs); fft_len < 2 is GSMCAL_E_ARG, fft_len > 64
 *   GSMCAL_E_UNSUPPORTED.  At fft_len = 2 the reference's three "signal" bins count the other bin twice, the SNR is NaN and
 *   nothing hits; at fft_len = 3 all bins are signal bins and noise_power is a rounding residue (0 or an ulp either side): the
 *   call returns cleanly, which windows hit is not defined by the reference.
 *   mv_len >= 1, len >= 1 (fewer than fft_len samples: no window, no hit).  The scan keeps len + mv_len + 128 SNRs in LDS
 *   behind gsmcal_coarse_scan_lds_fixed() = 11 344 bytes of its own, 159 KiB in all: up to len + mv_len = 18 806
 *   (GSMCAL_E_UNSUPPORTED beyond).
 *   gsmcal_FCCH_coarse_position derives fft_len = 2^floor(log2(148/decimation_ratio)) itself: decimation_ratio 2 .. 74 is
 *   served (fft_len 64 .. 2; 5, 6, 7 and 8 give the 16-point kernels), 1 (128-point windows) and 75 and above (windows of one
 *   sample) are GSMCAL_E_UNSUPPORTED.  Fewer than ceil(28750/decimation_ratio) samples: GSMCAL_E_INDEX (s(1:n_first), :25).
 * GSMCAL_E_UNSUPPORTED is decided on the host before anything is uploaded; no output has been written. */
int gsmcal_move_fft_snr_runtime_avg(gsmcal_ctx* ctx, const double* s, long len, int mv_len, int fft_len,
                                    double th, int* hit_flag, double* hit_idx, double* hit_avg_snr,
                                    double* hit_snr);
/* [hit_flag,hit_idx,hit_snr] = specific_fft_snr_fix_avg(s,target_set,fft_len,th,avg_snr)
 *                                                                    specific_fft_snr_fix_avg.m:5-34 */
int gsmcal_specific_fft_snr_fix_avg(gsmcal_ctx* ctx, const double* s, long len, const double target_set[2],
                                    int fft_len, double th, double avg_snr, int* hit_flag,
                                    double* hit_idx, double* hit_snr);
/* [position,snr] = FCCH_coarse_position(s,decimation_ratio)         FCCH_coarse_position.m:5-94
 * position/snr: capacity `cap` doubles; *count = number of hits (sentinel: *count = 1, both -1). */
int gsmcal_FCCH_coarse_position(gsmcal_ctx* ctx, const double* s, long len, int decimation_ratio,
                                double* position, double* snr, int cap, int* count);

/* [FCCH_pos,r,sampling_ppm,carrier_ppm] = FCCH_fine_correction(s,base_position,ov,carrier_freq)
 *                                                                    FCCH_fine_correction.m:5-197
 * r: capacity cap_r complex samples; *len_r = samples written (sentinel r = -1: *len_r = -1 and
 * nothing written).  r may be NULL (cap_r = 0) when only positions/ppm are wanted.
 * oversampling_ratio (this function, gsmcal_SCH_corr_rate_correction and gsmcal_carrier_correct_post_SCH share one range):
 * 1 (148-point spectra, two 64-shift chunks) to 30, odd ratios included; held to the oracle at 1, 2, 3, 4, 5, 6, 8, 12, 16 and
 * 30.  The burst kernels keep two 148*ov-sample buffers, the window's samples and their tables in LDS; from 31 on that
 * passes 159 KiB (the chunk sweep follows at 34): GSMCAL_E_UNSUPPORTED, decided on the host before anything is uploaded or
 * launched, nothing written.  (Behind it, 128 and above would pass the 255 chunks of 64 shifts a work item can name.) */
int gsmcal_FCCH_fine_correction(gsmcal_ctx* ctx, const double* s, long len, const double* base_position,
                                int num_base, int oversampling_ratio, double carrier_freq,
                                double* fcch_pos, int cap_pos, int* num_pos,
                                double* r, long cap_r, long* len_r,
                                double* sampling_ppm, double* carrier_ppm);

/* [pos_info,r,sampling_ppm] = SCH_corr_rate_correction(s,FCCH_pos,sch_training_sequence,ov)
 *                                                                    SCH_corr_rate_correction.m:5-181
 * pos_info: cap_rows x 2 doubles, column-major with leading dimension cap_rows; *num_rows rows valid
 * (sentinel: *num_rows = 1, row = [-1 -1]). */
int gsmcal_SCH_corr_rate_correction(gsmcal_ctx* ctx, const double* s, long len, const double* fcch_pos,
                                    int num_fcch, const double* sch_training_sequence, int len_ts,
                                    int oversampling_ratio, double* pos_info, int cap_rows, int* num_rows,
                                    double* r, long cap_r, long* len_r, double* sampling_ppm);

/* [r,carrier_ppm] = carrier_correct_post_SCH(s,pos_info,ov,carrier_freq)
 *                                                                    carrier_correct_post_SCH.m:5-83
 * pos_info: rows x 2 column-major, leading dimension `ld`. */
int gsmcal_carrier_correct_post_SCH(gsmcal_ctx* ctx, const double* s, long len, const double* pos_info,
                                    int rows, int ld, int oversampling_ratio, double carrier_freq,
                                    double* r, long cap_r, long* len_r, double* carrier_ppm);

/* Front end of SCH_demod(s,pos_info,training_sequence,ov)                SCH_demod.m:53-59,79-90
 * Per SCH row of pos_info (type 1): the burst with 8 symbols either side and the traceback depth behind it
 * (len_fde_ov = 194*ov samples), its frequency-domain channel estimate against the training sequence and the equalised
 * burst x_eq = ifft(fft(x) ./ (fft(x_training) ./ fft(training))).  The Viterbi GMSK demodulator that follows in the
 * reference (Communications Toolbox, output discarded) is not part of this library.
 * x_eq: cap_bursts x len_fde_ov complex, burst-major; *num_bursts SCH bursts written, *len_fde_ov their length.
 * pos_info all -1 (:8-11): returns GSMCAL_S_POST_NO_POS with *num_bursts = 0.
 * oversampling_ratio 1 .. 12: a burst's three 194*ov-point buffers and the 97 x (2*ov + 1) matrix of its transform live in
 * LDS; 13 and above pass 159 KiB: GSMCAL_E_UNSUPPORTED, nothing written. */
int gsmcal_SCH_equalise(gsmcal_ctx* ctx, const double* s, long len, const double* pos_info, int rows, int ld,
                        const double* sch_training_sequence, int len_ts, int oversampling_ratio,
                        double* x_eq, int cap_bursts, int* num_bursts, int* len_fde_ov);

/* FCCH_demod(s,pos_info,ov,carrier_freq)                            FCCH_demod.m:5-66
 * The check behind the calibration (gsm_sync_demod.m:144): per FCCH row of pos_info (type 0, start sp) the window
 * s(sp : sp+148*ov-1), the first maximum of its power spectrum in fftshift order, the tone frequency from the integer-bin
 * rotation and the mean phase step of the unit phasors (:28-42), and the SNR of :51-63 -- the five bins at the peak against the
 * rest of the 110 bins around the centre.  freq, snr, max_idx: capacity `cap` doubles, *num_fcch written; max_idx holds the
 * offset max_idx - (fft_len/2+1) the reference prints (:66).  *mean_freq = mean(freq), *carrier_ppm the carrier error still left
 * (:44-48); both NaN when pos_info has no type-0 row (MATLAB's mean([])).
 * snr: where noise_power < 0 (peak outside the band) MATLAB's log10 yields a complex number: NaN here; noise_power == 0: +Inf.
 * pos_info all -1 (:8-11): returns GSMCAL_S_POST_NO_POS with *num_fcch = 0.  More than GSMCAL_MAX_HITS type-0 rows (or than
 * `cap`): GSMCAL_E_CAPACITY.  A window that leaves the stream: GSMCAL_E_INDEX, decided before a sample is read.
 * gsmcal_last_call_report then returns the lines the .m file prints (:6,9,43,45,49,65,66).
 * oversampling_ratio 1 .. 33 (tested at 1, 2, 3, 4, 8 and 16): the window and its 37 x (4*ov + 1) transform matrix live in LDS
 * and pass 159 KiB at 34, GSMCAL_E_UNSUPPORTED from there on. */
int gsmcal_FCCH_demod(gsmcal_ctx* ctx, const double* s, long len, const double* pos_info, int rows, int ld,
                      int oversampling_ratio, double carrier_freq, double* freq, double* snr, double* max_idx, int cap,
                      int* num_fcch, double* mean_freq, double* carrier_ppm);

/* [normal_training_sequence_idx, r, carrier_ppm] = BCCH_demod(s,pos_info,normal_training_sequence,ov,carrier_freq)   BCCH_demod.m
 * Which of the eight GSM normal training sequences the BCCH bursts carry -- the cell's base-station colour code.  The .m file uses
 * two names it does not define: carrier_freq (:71), the argument every sibling function takes and the fifth one here, and
 * normal_training_sequence (:97), its third parameter: 26*ov x 8 complex as gsm_normal_training_sequence_gen returns it, passed
 * column by column ([8][len_ts] complex, len_ts = 26*ov; any other len_ts: GSMCAL_E_ARG, MATLAB's inner dimensions would disagree).
 * :49-72 the tone estimate of every FCCH row (type 0), fo = mean, carrier_ppm -- the estimator of gsmcal_FCCH_demod; :74-76
 * r = s .* exp(1i*(0:len-1)'*comp_phase_rotate); :84-97 for the first four BCCH rows (type 2, start p) the window r(p+61*ov :
 * p+87*ov-1) against the conjugated templates; :99-106 the first maximum of |corr_val| per burst: all four equal gives *idx = 1..8
 * and status 0, otherwise *idx = -1 and GSMCAL_S_BCCH_TSC_MIXED -- r and carrier_ppm are valid then, the .m file has them by :76.
 * pos_info all -1 (:9): GSMCAL_S_POST_NO_POS; fewer than 4 type-2 rows (:14): GSMCAL_S_POST_FEW_BCCH -- the literal 4 of :14 and
 * :80, not gsmcal_params.post_min_bcch: num_bcch_used = 4 rows are read unconditionally afterwards.  Both leave *idx = -1,
 * *len_r = -1 and *carrier_ppm = -1, the values of :6-8.  No type-0 row: mean([]) = NaN, r, corr_val and carrier_ppm are NaN and
 * *idx = -1 with GSMCAL_S_BCCH_TSC_MIXED (MATLAB's max over an all-NaN column answers 1, a number without a meaning).
 * An FCCH window or one of the four BCCH windows outside the stream: GSMCAL_E_INDEX, decided before a sample is read.
 * r (may be NULL): cap_r complex, *len_r = len written; must not overlap s (GSMCAL_E_ARG).  corr_val (may be NULL): the 8 x 4
 * matrix of :97, column-major.  table_row (may be NULL): GSMCAL_BCCH_COLS doubles, the row gsmcal_bcch_demod_batch writes for
 * this stream -- every type-2 row evaluated, not only four.  gsmcal_last_call_report then returns the lines of :15, :69, :72 and
 * :101 or :104.  oversampling_ratio as for gsmcal_FCCH_demod. */
int gsmcal_BCCH_demod(gsmcal_ctx* ctx, const double* s, long len, const double* pos_info, int rows, int ld,
                      const double* normal_training_sequence, int len_ts, int oversampling_ratio, double carrier_freq,
                      int* idx, double* r, long cap_r, long* len_r, double* carrier_ppm, double* corr_val, double* table_row);

/* SCH_decode(s, pos_info, sch_training_sequence, ov): the payload of the SCH bursts that pos_info marks (type 1) -- the cell's BSIC
 * and the GSM frame number of every burst.  The project's own function, NOT a port of SCH_demod.m, which has
 * no outputs and demodulates with Communications Toolbox code.  Per burst with 1-based start p, ov in {2, 4, 8} (anything else:
 * GSMCAL_E_UNSUPPORTED), delta = (5*ov - 1) div 2:
 *   y_k = s(p + k*ov + delta) * (-j)^k for the symbols k = 3..144 -- one sample per symbol; a burst whose reads leave the stream, or
 *   whose p is NaN or < 1, is not evaluated (NaN columns, no error);  h1, h2 = the correlations of y_42..73 and y_74..105 with the
 *   two halves of the 64 training bits (1 - 2 bit), h = h1 + h2, slope = angle(h2 conj(h1)) / 32, amp = |h| / 64;
 *   soft_k = Re(y_k conj(h)/|h| exp(-j slope (k - 73.5))), positive = bit 0;  a 16-state soft-decision Viterbi decoder (GSM 05.03
 *   4.7: c(2k) = u(k)+u(k-3)+u(k-4), c(2k+1) = u(k)+u(k-1)+u(k-3)+u(k-4); burst bits 3..41 and 106..144) from state 0 to state 0;
 *   ok = the 10-bit CRC leaves all ones, the four tail bits are zero, T3' <= 4 and T2 <= 25;  FN = 1326 T1 + 51 ((T3 - T2) mod 26) + T3.
 * Per stream: the ok bursts that agree on the BSIC and whose frame numbers differ by what their positions say (1250*ov samples per
 * frame, modulo the hyperframe of 2 715 648 frames) are counted per burst; the first burst with the largest count c is the anchor;
 * status 0 needs c >= 2 (one pass of a 10-bit CRC is not evidence), otherwise GSMCAL_S_SCH_NO_DECODE and *bsic, *fn_anchor,
 * *pos_anchor = -1.  pos_info all -1: GSMCAL_S_POST_NO_POS.  More than GSMCAL_MAX_HITS type-1 rows: GSMCAL_E_CAPACITY.
 * sch_training_sequence: the template gsmcal_SCH_corr_rate_correction takes; the decoder works on the 64 training BITS, so only
 * len_ts is looked at: len_ts != 64*ov is GSMCAL_E_ARG.  The bit map of the 25 information bits is unpinned against a real capture.
 * table_row (may be NULL): GSMCAL_SCH_COLS doubles (GSMCAL_C_*), the row gsmcal_sch_decode_batch writes for this stream.  soft (may
 * be NULL): [GSMCAL_MAX_HITS][148] doubles, NaN outside 3..144 and for bursts not evaluated.  u (may be NULL): [GSMCAL_MAX_HITS][39]
 * bytes, the decoded words (25 information, 10 parity, 4 tail bits), 255 for bursts not evaluated.  gsmcal_last_call_report then
 * returns "SCH bursts N decoded N consistent N" and "BSIC b frame number f at sample p" or "Fail to decode the SCH bursts."
 * (nothing at GSMCAL_S_POST_NO_POS).  Returns the status. */
int gsmcal_SCH_decode(gsmcal_ctx* ctx, const double* s, long len, const double* pos_info, int rows, int ld,
                      const double* sch_training_sequence, int len_ts, int oversampling_ratio, int* bsic, long* fn_anchor,
                      long* pos_anchor, double* table_row, double* soft, unsigned char* u);

/* BCCH_decode(s, pos_info, tsc, ov): the system information in the BCCH blocks that pos_info marks -- which cell this is.  The
 * project's own function, NOT a port: BCCH_demod.m stops at the training sequence index.  A block is four
 * type-2 rows of pos_info directly behind a type-1 row (rows i+1..i+4; a shorter run is no block).  Per burst with 1-based start
 * p, tsc in 0..7 (anything else: GSMCAL_E_ARG), ov in {2, 4, 8} (anything else: GSMCAL_E_UNSUPPORTED), delta = (5*ov - 1) div 2:
 *   y_k = s(p + k*ov + delta) * (-j)^k for k = 3..144; if any of the block's four bursts would read outside the stream, or has p
 *   NaN or < 1, the block is not evaluated (NaN columns, zero octets, no error);  pass 0: h = the correlation of y_61..86 with the
 *   26 training bits of code tsc (1 - 2 bit), amp = |h| / 26, soft_k = Re(y_k conj(h)/|h|);  two decision-directed refinements:
 *   b_k = sign(soft_k) (+1 at zero; the training bits inside the mid-amble), g1, g2 = the sums of y_k b_k over k = 3..73 and
 *   74..144, g = g1 + g2, slope = angle(g2 conj(g1)) / 71, soft_k = Re(y_k conj(g)/|g| exp(-j slope (k - 73.5))), positive = bit 0;
 *   the 4 x 114 data values are de-interleaved to c(0..455) (GSM 05.03 4.1.4: c(k) in burst k mod 4 at position 2 ((49 k) mod 57) +
 *   ((k mod 8) div 4)); the stealing flags are counted, not used;  the 16-state soft-decision Viterbi decoder of gsmcal_SCH_decode
 *   (the same generators) over 228 steps from state 0 to state 0;  ok = the remainder of u(0..223) by the Fire code's g(D) =
 *   D^40 + D^26 + D^23 + D^17 + D^3 + 1 is all ones and u(224..227) = 0 -- detection only, no burst-error correction.
 * Octet n of the block has d(8n + k) as its bit k (LSB first); unpinned against a real capture.
 * Per stream: status 0 iff at least one block is ok (a 40-bit code is evidence on its own), otherwise GSMCAL_S_BCCH_NO_DECODE.
 * pos_info all -1: GSMCAL_S_POST_NO_POS.  More than GSMCAL_MAX_HITS blocks: GSMCAL_E_CAPACITY.
 * octets (required): [GSMCAL_MAX_HITS][23] bytes, the decoded blocks, zeros unless ok.  table_row (may be NULL): GSMCAL_SI_COLS
 * doubles (GSMCAL_I_*), the row gsmcal_bcch_decode_batch writes for this stream.  soft (may be NULL): [GSMCAL_MAX_HITS][456]
 * doubles, the de-interleaved soft values, NaN for blocks not evaluated.  first (may be NULL): what gsmcal_si_fields (gsmcal_si.h)
 * reads in the first ok block (valid = 0 without one).  gsmcal_last_call_report then returns "BCCH blocks N decoded N" and
 * "System information type T cell identity c LAI mcc-mnc-lac" or "Fail to decode the BCCH blocks." (nothing at
 * GSMCAL_S_POST_NO_POS).  Returns the status. */
int gsmcal_BCCH_decode(gsmcal_ctx* ctx, const double* s, long len, const double* pos_info, int rows, int ld, int tsc,
                       int oversampling_ratio, unsigned char* octets, double* table_row, double* soft, gsmcal_si_info* first);

/* pair_coherence(s_a, s_b, pos_info_a, ov, lag0, max_lag, min_coherence) -- the project's own function: the
 * reference names the goal, dongles that "work together coherently", and has no code for it beyond a difference of integer burst
 * positions (gsm_sync_demod.m:149-158).  How far apart two corrected streams are in time, to a fraction of a sample, and in carrier
 * phase; how coherent they are; how fast they still drift.  ov 2, 4 or 8 (anything else GSMCAL_E_UNSUPPORTED); lag0: the expected
 * offset of b's content against a's, samples; max_lag M, 1 <= M <= 4*ov (0 selects 2*ov); min_coherence in [0, 1].
 * With L = 148*ov, Ls = 37*ov, fs = (1625e3/6)*ov, per type-1 or type-2 row of a's pos_info, in table order (1-based start pos,
 * p = round(pos) - 1; FCCH rows are left out, a tone has no delay):
 *   evaluated iff 0 <= p, p + L <= len_a, 0 <= p + lag0 - M and p + lag0 + M + L <= len_b (otherwise every column NaN, no error);
 *   c[m][k] = sum_{n<Ls} b[p + lag0 + m + k*Ls + n] conj(a[p + k*Ls + n]) for m = -M..M, k = 0..3, Ea[k] and Eb[m][k] the energies
 *   of the same samples;  y[m] = sum_k |c[m][k]|^2, m* its first maximum;  m* = -M or +M: edge = 1, the burst is not used;
 *   delay = lag0 + m* + 0.5 (y[m*-1] - y[m*+1]) / (y[m*-1] - 2 y[m*] + y[m*+1]);
 *   theta = arg sum_{k<3} c[m*][k+1] conj(c[m*][k]), freq = theta fs / (2 pi Ls) (unambiguous to +-fs/(2 Ls) = 3.66 kHz);
 *   phase = arg sum_k c[m*][k] exp(-j theta (k - 1.5));  coherence = sum_k |c[m*][k]| / sqrt(sum Ea sum Eb[m*]) (NaN at 0 / 0).
 * Per pair, over the used bursts (evaluated, not edge, coherence >= min_coherence), t = p - p of the first used burst: delay0,
 * rel_sampling_ppm and delay_rms from the least-squares line of delay on t; burst_carrier_hz = mean freq; rel_carrier_hz refines it
 * by the phase steps between consecutive used bursts at most 1875*ov samples apart (with none it equals burst_carrier_hz); phase0
 * and phase_rms of the phases rotated back by rel_carrier_hz.  Fewer than two used bursts: GSMCAL_S_PAIR_FEW, the summaries NaN.
 * Either stream empty or a pos_info all -1: GSMCAL_S_POST_NO_POS.  More than GSMCAL_MAX_PAIR_BURSTS rows: GSMCAL_E_CAPACITY.
 * table_row (required): GSMCAL_PAIR_COLS doubles (GSMCAL_P_*), the row gsmcal_pair_coherence_batch writes for the pair.  corr (may
 * be NULL): [GSMCAL_MAX_PAIR_BURSTS][2M+1][4] complex, c[m][k], NaN for bursts not evaluated.  gsmcal_last_call_report then returns
 * the summary lines.  Returns the status. */
int gsmcal_pair_coherence(gsmcal_ctx* ctx, const double* s_a, long len_a, const double* s_b, long len_b, const double* pos_info,
                          int rows, int ld, int oversampling_ratio, int lag0, int max_lag, double min_coherence, double* table_row,
                          double* corr);

/* pair_align(s, ov, params_row, out_len) -- the project's own function: what pair_coherence measures, this
 * acts on.  One stream is resampled onto another dongle's time base by a fractional delay that may drift, and a carrier is taken out.
 * ov 2, 4 or 8 (anything else GSMCAL_E_UNSUPPORTED), fs = (1625e3/6)*ov; params_row: GSMCAL_ALIGN_PARAMS doubles {delay, slope_ppm,
 * carrier_hz, phase, anchor, weight} (GSMCAL_A_*), |slope_ppm| <= 1000 (beyond: GSMCAL_E_ARG); out_len >= 1.  For n = 0 .. out_len-1,
 * in fp64, every operation rounded on its own:
 *   x = (n + delay) + (slope_ppm*1e-6)*(n - anchor),  base = floor(x),  mu = x - base;
 *   valid iff 0 <= base - 7 and base + 8 < len (decided before a sample is read);
 *   out[n] = exp(-j (phase + (2 pi carrier_hz / fs) (n - anchor))) sum_{k=-7..8} h(k - mu) s[base + k] where valid, exactly 0 + 0j
 *   where not;  h(u) = sinc(u) (0.42 + 0.5 cos(2 pi u/16) + 0.08 cos(4 pi u/16)), sinc(u) = sin(pi u)/(pi u), h(0) = 1 exactly.
 * The window is zero at |u| = 8, so h is continuous: a floor() that lands on the other side of an integer x changes a sample by
 * rounding only.  x increases with n, so the valid samples are one interval [first_valid, end_valid).
 * info_row (required): GSMCAL_ALIGN_INFO_COLS doubles {status, first_valid, end_valid, num_valid} (GSMCAL_AI_*), 0 0 0 with no
 * valid sample.  status (also the return value): 0; GSMCAL_S_POST_NO_POS: len < 1 (s may then be NULL); GSMCAL_S_ALIGN_SKIPPED: a
 * value of params_row is not finite -- out is all zero in both cases.  out: out_len complex; it must not overlap s.
 * gsmcal_last_call_report then returns the member's line. */
int gsmcal_pair_align(gsmcal_ctx* ctx, const double* s, long len, int oversampling_ratio, const double* params_row, long out_len,
                      double* out, double* info_row);

/* One row of the pair_coherence table -> the parameter row that aligns stream b of that pair onto stream a (pure host arithmetic; no
 * context needed).  pair_row: GSMCAL_PAIR_COLS doubles; min_coherence: the threshold the row was made with (the row does not carry
 * it; it decides which burst is the first USED one: pos not NaN, edge 0, coherence >= min_coherence); weight: copied.  With
 * L = 148*ov, s = 1e-6 rel_sampling_ppm, p0 = round(pos) - 1 of the first used burst:
 *   anchor = p0 + (L-1)/2;  delay = delay0 + s (L-1)/2;  slope_ppm = rel_sampling_ppm;  carrier_hz = rel_carrier_hz (1 + s);
 *   phase = phase0
 * (pair_coherence's phase is that of b against a at the burst's centre IN b's INDEX, its delay0 sits at the burst's START: at output
 * index n the position in b is n + delay0 + s (n - p0), and the carrier seen there, rel_carrier_hz per second of a's samples counted
 * in b's index, turns (1 + s) times as fast per output sample).  A row whose status is not 0, or without a used burst: every value
 * NaN but the weight (gsmcal_pair_align_batch then skips the member); returns GSMCAL_S_ALIGN_SKIPPED then, otherwise 0.  The
 * reference stream itself is the row {0, 0, 0, 0, 0, weight}. */
int gsmcal_pair_align_params(const double* pair_row, int oversampling_ratio, double min_coherence, double weight, double* params_row);

/* ppm_out = total_ppm_calculation(ppm_in)                           total_ppm_calculation.m:5-21
 * (pure host arithmetic; no context needed) */
int gsmcal_total_ppm_calculation(const double* ppm_in, int n, double* ppm_out);

/* ---- batched hot path (what the drivers' loops become) ----------------------------------------- */

/* Front end of both drivers for D captures at once: raw2iq + filter(coef,1,.) + r(1:decim:end)
 * (gsm_sync_demod.m:107,110,117; multi_rtl_sdr_gsm_FCCH_scanner.m:132-135).
 * raw: D x 2N bytes (capture-major: capture d starts at raw + d*2N). out: D x ceil(N/decim) complex.
 * Any N >= 1 (N below ntaps or decim included; 2N need not be a multiple of 16: captures may start anywhere), ntaps >= 1.
 * decim: a workgroup stages the 256*decim + ntaps raw samples of its 256 outputs in LDS -- 1 .. 282 for one tap, 281 for 47,
 * 277 for 300 taps; beyond that GSMCAL_E_UNSUPPORTED with nothing written (gsmcal_filter on raw2iq's output has no limit). */
int gsmcal_frontend_batch(gsmcal_ctx* ctx, const uint8_t* raw, int d, long n, const double* coef,
                          int ntaps, int decim, double* out);
int gsmcal_frontend_batch_dev(gsmcal_ctx* ctx, const uint8_t* d_raw, int d, long n, const double* coef,
                              int ntaps, int decim, double* d_out);

/* Band power of D captures: power[d] = mean(abs(filter(coef,1,raw2iq(s_d))(1:decim:end)).^2)
 * (multi_rtl_sdr_split_scanner.m:154-156, multi_rtl_sdr_diversity_scanner.m:156-158; coef = [1], decim = 1:
 * scan_band_power_spectrum.m:80-84).  raw: D x 2N bytes, capture-major as above.  power: [D] doubles.
 * 1 <= ntaps <= 1024, decim >= 1, anything else GSMCAL_E_ARG.  The DC of raw2iq.m:8 is removed as exact integer sums, so a
 * constant capture gives exactly 0; a capture's result is bit-identical at any position in a batch of any size.  The calls
 * use workspaces of their own: gsmcal_last_batch_details / _snr and gsmcal_last_call_report keep answering for the call
 * before.  _dev: enqueues on the context's stream only; d_power may be device or pinned host memory. */
int gsmcal_band_power_batch(gsmcal_ctx* ctx, const uint8_t* raw, int d, long n, const double* coef,
                            int ntaps, int decim, double* power);
int gsmcal_band_power_batch_dev(gsmcal_ctx* ctx, const uint8_t* d_raw, int d, long n, const double* coef,
                                int ntaps, int decim, double* d_power);

/* Several sub-band powers per capture (multi_rtl_sdr_diversity_scanner_another_bak.m:186-210, the multi-channel diversity
 * scanner: every grid point that falls inside a capture is taken out of that one capture):
 *   power[c][j] = mean(abs(filter(coef,1, raw2iq(s_c).*exp(1i*(1:N)'*phase_rotate[c][j]))(1:decim:end)).^2)
 * raw: D x 2N bytes, capture-major; phase_rotate: HOST memory [D][nsub] in both forms (radians per sample, :195, taken
 * verbatim: the sign is the caller's), NaN = unused slot (its power is NaN, nothing is computed for it); power: [D][nsub].
 * decim = 1 is the script (:203); decim > 1 keeps rows 1:decim:end as multi_rtl_sdr_diversity_scanner.m:156-158 does.
 * 1 <= ntaps <= 128 (:52-53), 1 <= nsub <= GSMCAL_MAX_SUBBANDS, decim >= 1, d >= 1, n >= 1, no NULL pointer, no infinite
 * phase_rotate: anything else GSMCAL_E_ARG, decided before anything is enqueued.  The mixer is folded into the taps
 * (h_k = coef_k e^{-jwk}, built on the host in double): no phase ramp over n is formed.  DC as in gsmcal_band_power_batch:
 * a constant capture gives exactly 0 in every sub-band.  A (capture, phase) pair gives the same bits in any slot, beside any
 * other sub-bands, at any position in a batch of any size.  Workspaces of their own: gsmcal_last_batch_details / _snr and
 * gsmcal_last_call_report keep answering for the call before.  _dev: enqueues on the context's stream only; d_power may be
 * device or pinned host memory. */
#define GSMCAL_MAX_SUBBANDS 16
int gsmcal_subband_power_batch(gsmcal_ctx* ctx, const uint8_t* raw, int d, long n, const double* coef, int ntaps, int decim,
                               const double* phase_rotate, int nsub, double* power);
int gsmcal_subband_power_batch_dev(gsmcal_ctx* ctx, const uint8_t* d_raw, int d, long n, const double* coef, int ntaps,
                                   int decim, const double* phase_rotate, int nsub, double* d_power);

/* CW sample-loss check (CW_check.m:6-8; check_CW_samples_loss_tcp.m:70,89-90 without the plots).  Per capture
 *   s = raw2iq(bytes);  q_n = s(n+1)./s(n), n = 1..N-1;  phase_rotate = angle(mean(q));  r_n = angle(q_n) - phase_rotate
 * with MATLAB's scaled complex division and r NOT wrapped (the reference does not wrap it: values lie in (-2pi, 2pi)).  A lost
 * run of k samples shows as ONE spike of k*phase_rotate mod 2pi at the ratio behind which the samples are missing; a loss with
 * k*phase_rotate mod 2pi below thr is invisible, so the CW offset is the operator's to choose.
 * raw: D x 2N bytes, capture-major.  summary: [D][GSMCAL_CW_COLS] doubles, row =
 *   [0] phase_rotate   [1] count of n with |r_n| > thr (strictly; it goes on past the capacity of the list)   [2] max |r_n|
 *   [3] 1-based n of the first maximum (MATLAB's max)   [4] status
 *   [5..] GSMCAL_CW_MAX_EVENTS pairs (1-based n, r_n) of the first exceeds in index order, NaN in unused slots.
 * r: NULL (summary only) or D rows of r_stride >= N-1 doubles, N-1 written per row, the padding left alone.
 * status GSMCAL_CW_OK; GSMCAL_CW_SHORT: N < 2, no ratio exists -- columns 0, 2, 3 and the events NaN, count 0, r untouched;
 * GSMCAL_CW_ZERO: some s(n), n <= N-1, is exactly 0+0i (a sample equal to the capture's mean, or a constant capture).  The
 * reference then computes with Inf and NaN and what comes out depends on the platform's complex division; that is NOT
 * reproduced: columns 0, 2, 3 and the events are NaN, the count is 0 and every r_n of that capture is NaN.
 * A phase_rotate of exactly +-pi sits on atan2's branch cut and r is then defined modulo 2pi only; a byte capture of N = 2 always
 * is such a case (raw2iq makes s(2) = -s(1), the one ratio is -1).
 * thr must be finite and > 0, d >= 1, n >= 1, no NULL raw / summary: anything else GSMCAL_E_ARG with a message, decided before
 * anything is enqueued.  No atomics and a tiling that depends on N only (GSMCAL_CW_TILE ratios per workgroup): a capture's row
 * and residuals are bit-identical at any position in a batch of any size, with or without r.  Workspaces of their own:
 * gsmcal_last_batch_details / _snr and gsmcal_last_call_report keep answering for the call before.  _dev: enqueues on the
 * context's stream only; d_summary and d_r may be device or pinned host memory.
 * gsmcal_CW_check is the MATLAB signature r = CW_check(s) on a complex array (len >= 2; r: len-1 doubles; *phase_rotate too
 * unless NULL): the same kernels behind another load stage, so CW_check(raw2iq(bytes)) equals the batch r bit for bit.  A zero
 * sample among s(1..len-1) gives NaN in every r_n and in *phase_rotate, as above. */
#define GSMCAL_CW_MAX_EVENTS 16
#define GSMCAL_CW_COLS (5 + 2 * GSMCAL_CW_MAX_EVENTS)     /* 37 doubles per stream */
#define GSMCAL_CW_TILE 2048
#define GSMCAL_CW_OK 0
#define GSMCAL_CW_SHORT 1
#define GSMCAL_CW_ZERO 2
int gsmcal_CW_check(gsmcal_ctx* ctx, const double* s, long len, double* r, double* phase_rotate);
int gsmcal_cw_check_batch(gsmcal_ctx* ctx, const uint8_t* raw, int d, long n, double thr, double* summary, double* r,
                          long r_stride);
int gsmcal_cw_check_batch_dev(gsmcal_ctx* ctx, const uint8_t* d_raw, int d, long n, double thr, double* d_summary,
                              double* d_r, long r_stride);

/* I/Q imbalance and clipping check of the analogue front end (the reference's TODO item 4.5; no .m file exists for it).  Model: the
 * dongle delivers I = x_I, Q = g*(x_Q cos(phi) + x_I sin(phi)) of a circular x (equal variance on both rails, uncorrelated: any
 * signal that sits off 0 Hz for the length of a capture), so var_Q/var_I = g^2 and cov_IQ/sqrt(var_I var_Q) = sin(phi).
 * Raw form, per capture of N samples with I bytes a_n and Q bytes b_n (raw2iq.m:6), raw: D x 2N bytes, capture-major:
 *   S_I = sum a, S_Q = sum b, S_II = sum a^2, S_QQ = sum b^2, S_IQ = sum a b, per rail min, max and clip = bytes equal to 0 or 255;
 *   A_I = N S_II - S_I^2, A_Q = N S_QQ - S_Q^2, C = N S_IQ - S_I S_Q as exact signed 64-bit integers (N <= 2^23 keeps them below
 *   2^62; a larger n is GSMCAL_E_UNSUPPORTED, decided before anything is enqueued); then in fp64, each integer converted once:
 *   dc_I = S_I/N, dc_Q = S_Q/N, var_I = A_I/(N*N), var_Q = A_Q/(N*N), gain = sqrt(A_Q/A_I),
 *   s = C/(sqrt(A_I)*sqrt(A_Q)) clamped to [-1, 1], c = sqrt(1 - s*s), phase_deg = asin(s)*180/pi,
 *   level_dbfs = 10 log10((var_I + var_Q)/(2*127.5^2)) (-Inf for two constant rails),
 *   irr_db = 10 log10(((gain+1)^2 - k)/((gain-1)^2 + k)) with k = 2*gain*s*s/(1 + c): |K1|^2/|K2|^2 of K1 = (1 + g e^{j phi})/2,
 *   K2 = (1 - g e^{-j phi})/2, written so that g ~ 1, phi ~ 0 does not cancel; a zero denominator gives +Inf.
 * table: [D][GSMCAL_IQ_COLS] doubles, row = the GSMCAL_Q_* columns below; every integer column is below 2^53.
 * status GSMCAL_IQ_OK; GSMCAL_IQ_SHORT: N < 2 -- the integer columns and dc are written, var_I .. level_dbfs are NaN;
 * GSMCAL_IQ_FLAT: A_I == 0 or A_Q == 0 (a constant rail) -- gain, sin_phase, phase_deg and irr_db are NaN, the rest is written.
 * The sums are integers: a row depends on the capture's bytes alone, whatever the batch, its position in it or the alignment.
 * d >= 1, n >= 1, no NULL pointer, raw 2-byte aligned in the _dev form: anything else GSMCAL_E_ARG with a message.  Workspaces of
 * their own: gsmcal_last_batch_details / _snr and gsmcal_last_call_report keep answering for the call before.  _dev: enqueues on
 * the context's stream only; d_table may be device or pinned host memory.
 * gsmcal_IQ_imbalance is the complex form on one stream s (len complex samples, 1 <= len <= 2^23: raw2iq's output, r_correct):
 * the same five sums and the min / max of the real and imaginary parts in fp64, the clip columns NaN, A_I, A_Q and C formed in
 * fp64 -- a DC far above the signal cancels there (raw2iq's output has none); a rail whose A is not positive is GSMCAL_IQ_FLAT.
 * GSMCAL_IQ_TILE samples per workgroup, one fixed reduction order that depends on len only, no float atomics: a row is
 * bit-identical from call to call and at any address.  It leaves in gsmcal_last_call_report one line
 * "I/Q gain g phase p deg image rejection r dB DC i q", or "I/Q imbalance undefined: constant rail." /
 * "I/Q imbalance undefined: fewer than two samples.".
 * gsmcal_iq_correct removes a measured imbalance from d complex streams of len samples each (s: [d][len], host), with the
 * per-stream host arrays gain[d] and sin_phase[d] of their rows: out_I = I, out_Q = (Q/g - I*s)/c, c = sqrt(1 - s*s), which makes
 * the sample moments of the output balanced.  out may equal s exactly; any partial overlap, a non-finite or non-positive gain or
 * |sin_phase| >= 1 (or not finite) is GSMCAL_E_ARG.  The output is a complex stream for the per-function entry points. */
#define GSMCAL_IQ_COLS 22
#define GSMCAL_IQ_TILE 16384
#define GSMCAL_IQ_MAX_N (1L << 23)
#define GSMCAL_IQ_OK 0
#define GSMCAL_IQ_SHORT 1
#define GSMCAL_IQ_FLAT 2
#define GSMCAL_Q_N 0
#define GSMCAL_Q_S_I 1
#define GSMCAL_Q_S_Q 2
#define GSMCAL_Q_S_II 3
#define GSMCAL_Q_S_QQ 4
#define GSMCAL_Q_S_IQ 5
#define GSMCAL_Q_MIN_I 6
#define GSMCAL_Q_MAX_I 7
#define GSMCAL_Q_MIN_Q 8
#define GSMCAL_Q_MAX_Q 9
#define GSMCAL_Q_CLIP_I 10
#define GSMCAL_Q_CLIP_Q 11
#define GSMCAL_Q_DC_I 12
#define GSMCAL_Q_DC_Q 13
#define GSMCAL_Q_VAR_I 14
#define GSMCAL_Q_VAR_Q 15
#define GSMCAL_Q_GAIN 16
#define GSMCAL_Q_SIN_PHASE 17
#define GSMCAL_Q_PHASE_DEG 18
#define GSMCAL_Q_IRR_DB 19
#define GSMCAL_Q_LEVEL_DBFS 20
#define GSMCAL_Q_STATUS 21
int gsmcal_IQ_imbalance(gsmcal_ctx* ctx, const double* s, long len, double* table_row);
int gsmcal_iq_imbalance_batch(gsmcal_ctx* ctx, const uint8_t* raw, int d, long n, double* table);
int gsmcal_iq_imbalance_batch_dev(gsmcal_ctx* ctx, const uint8_t* d_raw, int d, long n, double* d_table);
int gsmcal_iq_correct(gsmcal_ctx* ctx, const double* s, long len, int d, const double* gain, const double* sin_phase, double* out);

/* Scanner detect loop for D captures (multi_rtl_sdr_gsm_FCCH_scanner.m:132-135 front end,
 * :164 FCCH_coarse_position, :168-185 acceptance).  Outputs per capture: snr, num_hit (as the
 * driver's arrays), optional positions/snrs [D][GSMCAL_MAX_HITS] and counts [D] (NULL to skip). */
int gsmcal_fcch_scan_batch(gsmcal_ctx* ctx, const uint8_t* raw, int d, long n, const double* coef,
                           int ntaps, double* snr, double* num_hit, double* positions,
                           double* pos_snr, int* counts);
int gsmcal_fcch_scan_batch_dev(gsmcal_ctx* ctx, const uint8_t* d_raw, int d, long n, const double* coef,
                               int ntaps, double* d_snr_numhit /* [D][2] */, double* d_positions,
                               double* d_pos_snr, int* d_counts);

/* Per-dongle body of gsm_sync_demod.m:107-124 for D streams at once, from raw bytes to the
 * calibration table.  carrier_freq: [D].  table: [D][GSMCAL_TABLE_COLS].
 * Optional outputs (NULL to skip): pos_info [D][2][GSMCAL_MAX_POS_ROWS] (per stream column-major,
 * ld = GSMCAL_MAX_POS_ROWS); r_correct [D][N] complex + r_len [D] (the corrected stream the
 * reference hands to SCH_demod; r_len = -1 where the reference returns r = -1). */
int gsmcal_calibrate_batch(gsmcal_ctx* ctx, const uint8_t* raw, int d, long n, const double* coef,
                           int ntaps, const double* sch_training_sequence, int len_ts,
                           const double* carrier_freq, double* table, double* pos_info,
                           double* r_correct, long* r_len);
/* The d_* outputs of the *_dev entry points may be any memory the GPU can store to, in particular pinned host memory
 * (hipHostMalloc): the kernels that finish a batch then write the table / (snr, num_hit) rows where the host reads them
 * after synchronising the stream, and no device-to-host copy has to be queued behind the batch (bench.py does this). */
int gsmcal_calibrate_batch_dev(gsmcal_ctx* ctx, const uint8_t* d_raw, int d, long n, const double* coef,
                               int ntaps, const double* sch_training_sequence, int len_ts,
                               const double* carrier_freq, double* d_table, double* d_pos_info,
                               double* d_r_correct, long* d_r_len);

/* FCCH_demod for D streams, on exactly the optional outputs of gsmcal_calibrate_batch[_dev]: r [D][stride] complex, r_len [D]
 * (-1 where the reference returns r = -1), pos_info [D][2][GSMCAL_MAX_POS_ROWS] with -1 padding; carrier_freq: host [D].
 * out: [D][GSMCAL_DEMOD_COLS], row = {num_fcch, mean_freq, carrier_ppm, status, freq[], snr[], max_idx[]} (GSMCAL_D_*), unused
 * entries NaN.  Per-row outcomes go in the status column, not the return value: r_len = -1 or an all -1 pos_info gives
 * GSMCAL_S_POST_NO_POS (num_fcch 0, the rest NaN); GSMCAL_E_CAPACITY / GSMCAL_E_INDEX as above (num_fcch = the type-0 rows,
 * the rest NaN).  A burst's figures do not depend on the batch it is in: a row is bit-identical alone, at any position, and
 * equal to what gsmcal_FCCH_demod returns.  _dev: device pointers, only enqueues on the context's stream -- directly behind a
 * calibrate call, no host synchronisation in between; d_out may be device or pinned host memory.  The calls use a workspace of
 * their own: gsmcal_last_batch_details / _snr and gsmcal_last_call_report keep answering for the call before. */
int gsmcal_fcch_demod_batch(gsmcal_ctx* ctx, const double* r, long stride, const long* r_len, const double* pos_info, int d,
                            int oversampling_ratio, const double* carrier_freq, double* out);
int gsmcal_fcch_demod_batch_dev(gsmcal_ctx* ctx, const double* d_r, long stride, const long* d_r_len, const double* d_pos_info,
                                int d, int oversampling_ratio, const double* carrier_freq, double* d_out);

/* BCCH_demod for D streams, on the same inputs as gsmcal_fcch_demod_batch[_dev] plus the templates (host, [8][len_ts] complex,
 * len_ts = 26*ov) and carrier_freq (host [D]).  out: [D][GSMCAL_BCCH_COLS], row = {num_bcch, tsc_idx, mean_fo, carrier_ppm, status,
 * num_agree, idx[], peak[], runner_up[], phase[]} (GSMCAL_B_*): EVERY type-2 row is evaluated, up to GSMCAL_MAX_BCCH, the decision
 * is the reference's on the first four; num_agree counts the evaluated rows whose idx equals the first row's; unused entries NaN.
 * A row beyond the fourth whose window leaves the stream is NaN and no error: the reference never reads it.  Per-row outcomes go
 * in the status column: GSMCAL_S_POST_NO_POS (r_len = -1 or an all -1 pos_info; num_bcch 0), GSMCAL_S_POST_FEW_BCCH,
 * GSMCAL_S_BCCH_TSC_MIXED (mean_fo and carrier_ppm valid), GSMCAL_E_CAPACITY (more than GSMCAL_MAX_BCCH type-2 or GSMCAL_MAX_HITS
 * type-0 rows), GSMCAL_E_INDEX; in all but MIXED tsc_idx is -1 and mean_fo, carrier_ppm, num_agree are NaN.
 * Optional outputs (NULL to skip): corr [D][GSMCAL_MAX_BCCH][8] complex, the correlations of :97 (NaN where none was formed);
 * r_out [D][stride] complex with r_len_out [D] (both or neither): the rotated stream of :76 and its length, -1 wherever the
 * reference leaves r = -1 or stops (the _dev form leaves those rows of r_out untouched, the host form returns them as zeros).  r_out must not overlap r: GSMCAL_E_ARG.
 * A row is bit-identical alone, at any position of a batch, and equal to what gsmcal_BCCH_demod returns.  _dev: device pointers,
 * only enqueues on the context's stream; the calls share gsmcal_fcch_demod_batch's workspace and leave the lanes and every answer
 * about the calibrate / scan call before untouched. */
int gsmcal_bcch_demod_batch(gsmcal_ctx* ctx, const double* r, long stride, const long* r_len, const double* pos_info, int d,
                            int oversampling_ratio, const double* normal_training_sequence, int len_ts,
                            const double* carrier_freq, double* out, double* corr, double* r_out, long* r_len_out);
int gsmcal_bcch_demod_batch_dev(gsmcal_ctx* ctx, const double* d_r, long stride, const long* d_r_len, const double* d_pos_info,
                                int d, int oversampling_ratio, const double* normal_training_sequence, int len_ts,
                                const double* carrier_freq, double* d_out, double* d_corr, double* d_r_out, long* d_r_len_out);

/* SCH_decode for D streams, on the same inputs as gsmcal_bcch_demod_batch[_dev] with the SCH template (host, len_ts = 64*ov complex;
 * only its length is looked at) in place of the normal templates and no carrier_freq.  out: [D][GSMCAL_SCH_COLS], row = {num_sch,
 * num_ok, num_consistent, bsic, fn_anchor, pos_anchor, status, mean_slope, ok[], bsic[], fn[], ts_err[], corrected[], slope[], amp[]}
 * (GSMCAL_C_*); unused entries and bursts that were not evaluated NaN.  Per-row outcomes go in the status column: 0,
 * GSMCAL_S_POST_NO_POS (r_len = -1 or an all -1 pos_info; num_sch 0), GSMCAL_S_SCH_NO_DECODE, GSMCAL_E_CAPACITY (more than
 * GSMCAL_MAX_HITS type-1 rows; nothing evaluated).  Optional outputs (NULL to skip): soft [D][GSMCAL_MAX_HITS][148] doubles, u
 * [D][GSMCAL_MAX_HITS][39] bytes, as for gsmcal_SCH_decode.  ov other than 2, 4, 8: GSMCAL_E_UNSUPPORTED; len_ts != 64*ov:
 * GSMCAL_E_ARG.  A row is bit-identical alone, at any position of a batch, and equal to what gsmcal_SCH_decode returns.  _dev:
 * device pointers, only enqueues on the context's stream; the lanes and every answer about the calibrate / scan call before stay
 * untouched. */
int gsmcal_sch_decode_batch(gsmcal_ctx* ctx, const double* r, long stride, const long* r_len, const double* pos_info, int d,
                            int oversampling_ratio, const double* sch_training_sequence, int len_ts, double* out, double* soft,
                            unsigned char* u);
int gsmcal_sch_decode_batch_dev(gsmcal_ctx* ctx, const double* d_r, long stride, const long* d_r_len, const double* d_pos_info,
                                int d, int oversampling_ratio, const double* sch_training_sequence, int len_ts, double* d_out,
                                double* d_soft, unsigned char* d_u);

/* BCCH_decode for D streams, on the same inputs as gsmcal_sch_decode_batch[_dev] with one training sequence code per stream (host,
 * tsc[D], each 0..7: anything else GSMCAL_E_ARG) in place of the SCH template.  out: [D][GSMCAL_SI_COLS], row = {num_blocks, num_ok,
 * status, first_ok, ok[], pos[], corrected[], ts_err[], steal[], mean_slope[], amp[]} (GSMCAL_I_*); unused entries and blocks that
 * were not evaluated NaN.  Per-row outcomes go in the status column: 0, GSMCAL_S_POST_NO_POS (r_len = -1 or an all -1 pos_info;
 * num_blocks 0), GSMCAL_S_BCCH_NO_DECODE, GSMCAL_E_CAPACITY (more than GSMCAL_MAX_HITS blocks; nothing evaluated).  octets
 * (required): [D][GSMCAL_MAX_HITS][23] bytes, zeros unless the block is ok.  soft (NULL to skip): [D][GSMCAL_MAX_HITS][456] doubles,
 * NaN where the block was not evaluated.  ov other than 2, 4, 8: GSMCAL_E_UNSUPPORTED.  A row is bit-identical alone, at any
 * position of a batch, and equal to what gsmcal_BCCH_decode returns.  _dev: device pointers (tsc stays a host array), only enqueues
 * on the context's stream; the lanes and every answer about the calibrate / scan call before stay untouched. */
int gsmcal_bcch_decode_batch(gsmcal_ctx* ctx, const double* r, long stride, const long* r_len, const double* pos_info, int d,
                             int oversampling_ratio, const int* tsc, double* out, unsigned char* octets, double* soft);
int gsmcal_bcch_decode_batch_dev(gsmcal_ctx* ctx, const double* d_r, long stride, const long* d_r_len, const double* d_pos_info,
                                 int d, int oversampling_ratio, const int* tsc, double* d_out, unsigned char* d_octets,
                                 double* d_soft);

/* pair_coherence for P pairs of D streams, on the same inputs as gsmcal_sch_decode_batch[_dev].  pairs (host): [P][2] stream indices
 * (a, b), each in [0, D): anything else GSMCAL_E_ARG, decided before anything is enqueued; lag0 (host): [P].  The bursts of a pair are
 * the rows of a's table.  out: [P][GSMCAL_PAIR_COLS], row = {status, num_bursts, num_eval, num_used, num_adjacent, lag0, delay0,
 * rel_sampling_ppm, delay_rms, rel_carrier_hz, burst_carrier_hz, phase0, phase_rms, mean_coherence, min_coherence_seen, max_lag,
 * pos[], delay[], phase[], freq[], coherence[], edge[]} (GSMCAL_P_*), as gsmcal_pair_coherence defines them; per-row outcomes go in
 * the status column.  corr (NULL to skip): [P][GSMCAL_MAX_PAIR_BURSTS][2M+1][4] complex.  A row is bit-identical alone, at any
 * position of a batch of any size, from call to call, and equal to what gsmcal_pair_coherence returns.  _dev: device pointers (pairs
 * and lag0 stay host arrays), only enqueues on the context's stream; the lanes and every answer about the calibrate / scan call
 * before stay untouched. */
int gsmcal_pair_coherence_batch(gsmcal_ctx* ctx, const double* r, long stride, const long* r_len, const double* pos_info, int d,
                                int oversampling_ratio, const int* pairs, const int* lag0, int num_pairs, int max_lag,
                                double min_coherence, double* out, double* corr);
int gsmcal_pair_coherence_batch_dev(gsmcal_ctx* ctx, const double* d_r, long stride, const long* d_r_len, const double* d_pos_info,
                                    int d, int oversampling_ratio, const int* pairs, const int* lag0, int num_pairs, int max_lag,
                                    double min_coherence, double* d_out, double* d_corr);

/* pair_align for G members of D streams, (r, stride, r_len) as gsmcal_sch_decode_batch[_dev] takes them, and their weighted sum.
 * members (host): [G] stream indices, each in [0, D); params (host): [G][GSMCAL_ALIGN_PARAMS], rows as gsmcal_pair_align defines
 * them; 1 <= G <= GSMCAL_MAX_ALIGN_MEMBERS; a stream may be named more than once.  len of a member = min(r_len, stride) of its stream.
 * aligned (may be NULL): [G][out_len] complex, row g = gsmcal_pair_align of member g.  combined (may be NULL, not both):
 * [out_len] complex, combined[n] = sum_g weight_g aligned_g[n] in list order over the members valid at n (0 with none).
 * info (required): [G + 1][GSMCAL_ALIGN_INFO_COLS]: member rows {status, first_valid, end_valid, num_valid}, then the sum's
 * {members_used, combined_first, combined_end, sum of the used members' weights}: [combined_first, combined_end) is where every
 * member with status 0 is valid (empty: end = first).  Per-member outcomes go in the status column and the call succeeds: a member
 * with len < 1 (GSMCAL_S_POST_NO_POS) or with a value in its row that is not finite (GSMCAL_S_ALIGN_SKIPPED: the NaN summaries of a
 * failed pair_coherence row pass straight through gsmcal_pair_align_params) has an all-zero aligned row and is left out of the sum.
 * Decided before anything is enqueued: GSMCAL_E_ARG for a stream index outside [0, D), G outside 1 .. 64, out_len < 1,
 * |slope_ppm| > 1000, both outputs NULL; GSMCAL_E_UNSUPPORTED for ov not in {2, 4, 8}.  An output that overlaps r is not supported.
 * An aligned row is the same bits alone, at any place of any list, with or without `combined`, from call to call and from
 * gsmcal_pair_align; combined is the same bits from call to call and between the two forms.  The host form leaves the report lines
 * (one per member, one for the sum) with gsmcal_last_call_report.  _dev: device pointers (members and params stay host arrays), only
 * enqueues on the context's stream; the lanes and every answer about the calibrate / scan call before stay untouched. */
int gsmcal_pair_align_batch(gsmcal_ctx* ctx, const double* r, long stride, const long* r_len, int d, int oversampling_ratio,
                            const int* members, const double* params, int G, long out_len, double* aligned, double* combined,
                            double* info);
int gsmcal_pair_align_batch_dev(gsmcal_ctx* ctx, const double* d_r, long stride, const long* d_r_len, int d, int oversampling_ratio,
                                const int* members, const double* params, int G, long out_len, double* d_aligned, double* d_combined,
                                double* d_info);

/* ---- optimal combining: covariance of the aligned streams, the weights, the beams -------------------------
 * The project's own functions.  x: [d][stride] complex (the `aligned` rows of gsmcal_pair_align_batch, or any streams on one time
 * base); rows (host): [G] indices into it, each in [0, d), 1 <= G <= GSMCAL_MAX_ALIGN_MEMBERS; a row may be named twice.
 *
 * gsmcal_array_covariance_batch[_dev]: windows (host): [W][2] longs {start, len}, 1 <= W <= GSMCAL_MAX_COV_WINDOWS; cov: [W][G][G]
 * complex, row-major:  cov[w][i][j] = sum_{n = start}^{start + len - 1} x_i[n] conj(x_j[n])  in fp64, not divided by len; len = 0
 * gives an all-zero matrix.  cov[w][j][i] is the exact conjugate of cov[w][i][j] (one triangle is computed and mirrored) and the
 * imaginary part of the diagonal is exactly +0.  The order of the sum is fixed: every window is cut into chunks of GSMCAL_COV_CHUNK
 * samples counted from its own start, a chunk is added sample after sample with fused multiply-adds, the chunks' sums are added in
 * chunk order (no atomics).  So a window's matrix is the same bits from call to call, between the two forms, alone or at any
 * place of any window list, whatever other windows overlap it.  NaN and Inf propagate; nothing is screened.
 * Decided before anything is enqueued: GSMCAL_E_ARG for a row index outside [0, d), G or W outside its range, start < 0, len < 0,
 * start + len > stride, d < 1, stride < 1 or a NULL pointer.  _dev: x and cov are device pointers (rows and windows stay host
 * arrays); only enqueues on the context's stream. */
int gsmcal_array_covariance_batch(gsmcal_ctx* ctx, const double* x, long stride, int d, const int* rows, int G, const long* windows, int W,
                                  double* cov);
int gsmcal_array_covariance_batch_dev(gsmcal_ctx* ctx, const double* d_x, long stride, int d, const int* rows, int G, const long* windows,
                                      int W, double* d_cov);

/* The combining weights from covariances (pure host arithmetic; no context needed).  cov_signal, cov_noise: [G][G] complex as
 * gsmcal_array_covariance_batch writes them; only the upper triangle (i <= j) and the real part of the diagonal are read.
 * cov_noise NULL: w = the eigenvector of the largest eigenvalue of cov_signal (largest SNR when the noise is white and equal).
 * cov_noise given: w = the dominant generalised eigenvector of  Rs w = lambda Rn w  (largest SINR), through Rn = L L^H, the Hermitian
 * eigenproblem of L^-1 Rs L^-H (cyclic complex Jacobi) and w = L^-H u.  Either way |w|_2 = 1 and w[ref] is real and >= 0 (left as
 * found when it is exactly 0).  weights: [G] complex.  info: GSMCAL_WEIGHTS_INFO_COLS doubles {status, lambda_1, lambda_2, sweeps}
 * (lambda_2 NaN at G = 1).  Returns the status: 0, or GSMCAL_S_WEIGHTS_SINGULAR -- a value read that is not finite, a Cholesky pivot
 * <= 0 or not finite, lambda_1 <= 0 -- with every weight NaN.  GSMCAL_E_ARG: G outside 1 .. 64, ref outside [0, G), a NULL
 * cov_signal, weights or info. */
int gsmcal_combine_weights(const double* cov_signal, const double* cov_noise, int G, int ref, double* weights, double* info);

/* gsmcal_array_combine_batch[_dev]: weights (host): [B][G] complex, 1 <= B <= GSMCAL_MAX_BEAMS; out: [B][out_len] complex,
 * 1 <= out_len <= stride:  out[b][n] = sum_g conj(weights[b][g]) x_{rows[g]}[n]  (w^H x), g in list order, every term two fused
 * multiply-adds per part.  x is read once for all beams; a beam's row is the same bits alone or among other beams, from call to
 * call and between the two forms.  GSMCAL_E_ARG as above, and for B or out_len outside its range.  An output that overlaps x is
 * not supported.  _dev: x and out are device pointers (rows and weights stay host arrays); only enqueues on the context's stream. */
int gsmcal_array_combine_batch(gsmcal_ctx* ctx, const double* x, long stride, int d, const int* rows, int G, const double* weights, int B,
                               long out_len, double* out);
int gsmcal_array_combine_batch_dev(gsmcal_ctx* ctx, const double* d_x, long stride, int d, const int* rows, int G, const double* weights,
                                   int B, long out_len, double* d_out);

/* ---- apply a calibration to any capture: raw bytes resampled and de-rotated ---------------------------------
 * The project's own function: what the calibration chain measures on the GSM carrier (GSMCAL_T_TOTAL_SAMPLING_PPM, _CARRIER_PPM),
 * this takes out of a capture of the same dongle at any centre frequency and sample rate.  raw: [d][2n] bytes, capture-major, I / Q
 * interleaved (raw2iq.m:6); sample_rate > 0 and finite, Hz; params (host): [d][GSMCAL_APPLY_PARAMS] doubles, one row per capture
 * {delay, slope_ppm, carrier_hz, phase, anchor, scale, dc_i, dc_q, gain, sin_phase} (GSMCAL_AP_*); out_len >= 1, out_stride >= out_len.
 * With a_m, b_m the I and Q bytes of sample m, c = sqrt(1 - sin_phase^2) and h the interpolator of gsmcal_pair_align (GSMCAL_ALIGN_TAPS
 * taps, the Blackman-windowed sinc), for n = 0 .. out_len-1, in fp64:
 *   z[m] = (a_m - dc_i) + j ((b_m - dc_q)/gain - (a_m - dc_i) sin_phase)/c         (raw2iq's DC removal, then gsmcal_iq_correct's form)
 *   x = (n + delay) + (slope_ppm 1e-6) (n - anchor),  base = floor(x),  mu = x - base   (every operation rounded on its own)
 *   valid iff 0 <= base - 7 and base + 8 < n_samples
 *   out[n] = scale exp(-j (phase + (2 pi carrier_hz / sample_rate) (n - anchor))) sum_{k=-7..8} h(k - mu) z[base + k]   where valid,
 *   exactly 0 + 0j elsewhere.
 * out: [d][out_stride] complex; the elements at and beyond out_len of a row are not touched.  info: [d][GSMCAL_APPLY_INFO_COLS]
 * doubles {status, first_valid, end_valid, num_valid} (the GSMCAL_AI_* columns), 0 0 0 with no valid sample.  A row with a value
 * that is not finite has status GSMCAL_S_ALIGN_SKIPPED and an all-zero output row: a dongle whose calibration failed (total ppm =
 * Inf, an all-NaN row of gsmcal_apply_params) passes through a batch this way, and the call succeeds.
 * GSMCAL_E_ARG, decided before anything is enqueued and with the outputs untouched: a NULL pointer; d < 1, n < 1, out_len < 1 or
 * out_stride < out_len; sample_rate not finite or <= 0; in a row whose values are all finite |slope_ppm| > 1000, gain <= 0 or
 * |sin_phase| >= 1; raw not 2-byte aligned in the resident form.  An output that overlaps raw is not supported.
 * A capture's output row and info row depend on its bytes, its parameter row, n, sample_rate and out_len alone: they are the same
 * bits alone, at any position of any batch, from call to call and between the two forms.  No float atomics; the call keeps no state
 * between calls (the parameter rows are uploaded by every call).  The output rows are streams on one nominal time base, as
 * gsmcal_array_covariance_batch and gsmcal_array_combine_batch take them.
 * _resident: d_raw, d_out and d_info are device pointers (the outputs may be pinned host memory), params stays a host array; it
 * only enqueues on the context's stream, behind whatever wrote d_raw there; the lanes and every answer about the calibrate / scan
 * call before stay untouched. */
#define GSMCAL_APPLY_PARAMS 10          /* one capture's parameter row of gsmcal_apply_calibration_batch */
#define GSMCAL_APPLY_INFO_COLS 4        /* one row of its info table */
#define GSMCAL_AP_DELAY 0               /* position of output sample `anchor` in the capture minus anchor, samples                */
#define GSMCAL_AP_SLOPE_PPM 1           /* 1e6 * how much faster than the output index the position advances, |.| <= 1000          */
#define GSMCAL_AP_CARRIER_HZ 2          /* carrier to take out, Hz of the OUTPUT time base                                         */
#define GSMCAL_AP_PHASE 3               /* carrier phase to take out at output sample `anchor`, rad                                */
#define GSMCAL_AP_ANCHOR 4              /* output index the drift and the carrier are counted from                                 */
#define GSMCAL_AP_SCALE 5               /* real factor on the output                                                               */
#define GSMCAL_AP_DC_I 6                /* DC of the I bytes (127.5: raw2iq's)                                                     */
#define GSMCAL_AP_DC_Q 7                /* DC of the Q bytes                                                                       */
#define GSMCAL_AP_GAIN 8                /* Q / I gain ratio to remove, > 0 (GSMCAL_Q_GAIN)                                         */
#define GSMCAL_AP_SIN_PHASE 9           /* sine of the quadrature skew to remove, |.| < 1 (GSMCAL_Q_SIN_PHASE)                     */
int gsmcal_apply_calibration_batch(gsmcal_ctx* ctx, const uint8_t* raw, int d, long n, double sample_rate, const double* params,
                                   long out_len, long out_stride, double* out, double* info);
int gsmcal_apply_calibration_batch_resident(gsmcal_ctx* ctx, const uint8_t* d_raw, int d, long n, double sample_rate,
                                            const double* params, long out_len, long out_stride, double* d_out, double* d_info);

/* One row of the calibration table -> the parameter row that undoes it on a capture tuned to tuned_freq Hz (pure host arithmetic;
 * no context needed).  With e = 1e-6 TOTAL_SAMPLING_PPM and f_off = 1e-6 TOTAL_CARRIER_PPM tuned_freq:
 *   slope_ppm = TOTAL_SAMPLING_PPM,  anchor = 0,  carrier_hz = f_off (1 + e),  delay, phase and scale as given.
 * Why: the dongle samples at ideal time k/(1 + e) (in nominal sample periods) and its carrier error turns its sample k by
 * 2 pi f_off k / sample_rate; output sample n of the nominal time base therefore sits at dongle index n (1 + e), and the angle to
 * take out there is 2 pi f_off n (1 + e) / sample_rate (the reasoning of gsmcal_pair_align_params).
 * iq_row (may be NULL): a GSMCAL_IQ_COLS row of gsmcal_iq_imbalance_batch taken on the capture to correct: dc_i, dc_q from
 * GSMCAL_Q_DC_I / _DC_Q, gain and sin_phase from their columns, 1 and 0 at GSMCAL_IQ_FLAT / GSMCAL_IQ_SHORT.  Without it dc_i =
 * dc_q = 127.5, gain = 1, sin_phase = 0.  A table row whose GSMCAL_T_STATUS is not 0, or whose totals are not finite, gives an
 * all-NaN row (gsmcal_apply_calibration_batch then skips the capture) and the return value GSMCAL_S_ALIGN_SKIPPED; otherwise 0.
 * GSMCAL_E_ARG: a NULL table_row or params_row. */
int gsmcal_apply_params(const double* table_row, double tuned_freq, const double* iq_row, double delay, double phase, double scale,
                        double* params_row);

/* ---- row_coherence: delay, phase and drift between any rows on one nominal time base -----------------------
 * The project's own function: gsmcal_pair_coherence's estimator without the GSM carrier -- on any rows x: [d][stride] complex (the
 * output rows of gsmcal_apply_calibration_batch, for instance), over a caller's list of windows of one length.  valid (host, may be
 * NULL): [d][2] longs {first, end} per row, NULL = [0, stride) -- the first_valid, end_valid of apply_calibration's info table:
 * outside them a row is exact zeros and is not correlated.  pairs (host): [P][2] row indices (a, b); lag0 (host): [P] ints, the
 * expected offset of b's content against a's; starts (host): [W] longs, window starts in a's index, >= 0 and strictly ascending,
 * 1 <= W <= GSMCAL_MAX_ROW_WINDOWS; 16 <= win_len <= 65536, Ls = floor(win_len / 4), K = 4: the 4 Ls first samples of a window
 * are used; 1 <= max_lag M <= GSMCAL_MAX_ROW_LAG; min_coherence in [0, 1]; max_gap >= 0, samples; sample_rate fs finite and > 0.
 * Per (pair, window), p = the window's start:
 *   evaluated iff first_a <= p, p + 4 Ls <= end_a, first_b <= p + lag0 - M and p + lag0 + M + 4 Ls <= end_b (decided before a sample
 *   is read; otherwise every column of the window is NaN, no error);
 *   c[m][k], Ea[k], Eb[m][k], y[m], m*, edge, delay, theta, freq = theta fs / (2 pi Ls), phase and coherence: gsmcal_pair_coherence's
 *   formulas with this Ls and this fs.
 * Per pair, over the used windows (evaluated, not edge, coherence >= min_coherence), t = start - start of the first used window:
 * gsmcal_pair_coherence's summaries, the phase steps taken between consecutive used windows at most max_gap samples apart.  Fewer
 * than two used windows: GSMCAL_S_PAIR_FEW, the summaries NaN.
 * out: [P][GSMCAL_ROW_COLS] doubles: columns 0..15 with the meaning of GSMCAL_P_* (column 1 is W), then win_len, sample_rate,
 * min_coherence, max_gap, then GSMCAL_MAX_ROW_WINDOWS entries each of start, delay, phase, freq, coherence, edge (GSMCAL_R_*); entries
 * at and beyond W are NaN.  corr (NULL to skip): [P][W][2M+1][4] complex, NaN where not evaluated.
 * Order of the sums: a segment is cut into chunks of GSMCAL_ROW_CHUNK samples counted from its start; inside a chunk four interleaved
 * partial sums over the samples = 0, 1, 2, 3 mod 4, each ascending with explicit fused multiply-adds, combined (s0 + s1) + (s2 + s3);
 * the chunk sums are added in chunk order.  No atomics.  For Ls <= GSMCAL_ROW_CHUNK this is gsmcal_pair_coherence's own order: at
 * win_len = 148 ov the correlations are its correlations bit for bit.
 * A pair's row and corr block depend on its two rows, their valid intervals and the arguments alone: the same bits alone, at any
 * place of any pair list (also when the pair is listed twice), from call to call, with or without corr and between the two forms.
 * GSMCAL_E_ARG, decided before anything is enqueued and with the outputs untouched: a NULL required pointer; d, P, W, stride, win_len,
 * M or sample_rate outside its range; a pair index outside [0, d); starts negative or not strictly ascending; a valid row with
 * first < 0, end > stride or first > end; min_coherence outside [0, 1]; max_gap < 0 (or NaN).  The call keeps no state between calls
 * (pairs, starts and valid are uploaded by every call).
 * _resident: d_x, d_out and d_corr are device pointers (the outputs may be pinned host memory), everything else is a host array; it
 * only enqueues on the context's stream; the lanes and every answer about the calibrate / scan call before stay untouched. */
#define GSMCAL_MAX_ROW_WINDOWS 128      /* windows of one gsmcal_row_coherence_batch call */
#define GSMCAL_MAX_ROW_LAG 64           /* its largest max_lag */
#define GSMCAL_ROW_CHUNK 512            /* samples of one partial sum of a segment */
#define GSMCAL_ROW_COLS (20 + 6 * GSMCAL_MAX_ROW_WINDOWS)   /* one row of gsmcal_row_coherence_batch[_resident]: 788 doubles */
#define GSMCAL_R_STATUS 0               /* 0 or GSMCAL_S_PAIR_FEW                                                                  */
#define GSMCAL_R_NUM_WINDOWS 1          /* W                                                                                       */
#define GSMCAL_R_NUM_EVAL 2             /* windows both of whose spans lie inside the rows' valid intervals                        */
#define GSMCAL_R_NUM_USED 3             /* evaluated, not at the edge of the lag range, coherence >= min_coherence                 */
#define GSMCAL_R_NUM_ADJACENT 4         /* steps between consecutive used windows at most max_gap samples apart                    */
#define GSMCAL_R_LAG0 5                 /* the pair's lag0, as given                                                               */
#define GSMCAL_R_DELAY0 6               /* delay of b against a at the first used window, samples (the fitted line at t = 0)       */
#define GSMCAL_R_REL_SAMPLING_PPM 7     /* 1e6 * slope of that line                                                                */
#define GSMCAL_R_DELAY_RMS 8            /* rms of the delays about the line, samples                                               */
#define GSMCAL_R_REL_CARRIER_HZ 9       /* carrier of b against a: window_carrier_hz refined by the adjacent phase steps           */
#define GSMCAL_R_WINDOW_CARRIER_HZ 10   /* mean of freq[] over the used windows                                                    */
#define GSMCAL_R_PHASE0 11              /* phase of b against a at the centre of the first used window, rad                        */
#define GSMCAL_R_PHASE_RMS 12           /* rms of the used windows' phases about phase0 + 2 pi rel_carrier_hz t / fs, rad          */
#define GSMCAL_R_MEAN_COHERENCE 13      /* mean of coherence[] over the used windows                                               */
#define GSMCAL_R_MIN_COHERENCE_SEEN 14  /* ... and the smallest                                                                    */
#define GSMCAL_R_MAX_LAG 15             /* M, as given                                                                             */
#define GSMCAL_R_WIN_LEN 16             /* win_len, as given                                                                       */
#define GSMCAL_R_SAMPLE_RATE 17         /* sample_rate, as given                                                                   */
#define GSMCAL_R_MIN_COHERENCE 18       /* min_coherence, as given                                                                 */
#define GSMCAL_R_MAX_GAP 19             /* max_gap, as given                                                                       */
#define GSMCAL_R_START 20                                   /* [GSMCAL_MAX_ROW_WINDOWS] the window's start (NaN: not evaluated)    */
#define GSMCAL_R_DELAY (20 + GSMCAL_MAX_ROW_WINDOWS)        /* [..] lag0 + m* + the parabola's offset, samples                     */
#define GSMCAL_R_PHASE (20 + 2 * GSMCAL_MAX_ROW_WINDOWS)    /* [..] phase of b against a at the centre of the 4 Ls samples, rad    */
#define GSMCAL_R_FREQ (20 + 3 * GSMCAL_MAX_ROW_WINDOWS)     /* [..] segment-to-segment phase step as a frequency, Hz               */
#define GSMCAL_R_COH (20 + 4 * GSMCAL_MAX_ROW_WINDOWS)      /* [..] sum |c_k| / sqrt(sum Ea sum Eb), <= 1                          */
#define GSMCAL_R_EDGE (20 + 5 * GSMCAL_MAX_ROW_WINDOWS)     /* [..] 1: the maximum sits at -M or +M (delay .. coherence NaN); 0    */
int gsmcal_row_coherence_batch(gsmcal_ctx* ctx, const double* x, long stride, int d, const long* valid, const int* pairs, const int* lag0,
                               int P, const long* starts, int W, int win_len, int max_lag, double min_coherence, double max_gap,
                               double sample_rate, double* out, double* corr);
int gsmcal_row_coherence_batch_resident(gsmcal_ctx* ctx, const double* d_x, long stride, int d, const long* valid, const int* pairs,
                                        const int* lag0, int P, const long* starts, int W, int win_len, int max_lag, double min_coherence,
                                        double max_gap, double sample_rate, double* d_out, double* d_corr);

/* One row of the row_coherence table of the pair (reference, b), measured on the output rows of a first gsmcal_apply_calibration_batch
 * pass, composed into the parameter row that produced row b: a second pass over the same bytes with params_out lands on the
 * reference row's time base, carrier and phase (pure host arithmetic; no context needed).  With d1, s1 = 1e-6 slope_ppm, f1, phi1,
 * A1 = delay, slope, carrier_hz, phase, anchor of params_in; s = 1e-6 rel_sampling_ppm, f = rel_carrier_hz, fs, Ls of coh_row; p0 =
 * the start of its first used window (start not NaN, edge 0, coherence >= the row's min_coherence), n_c = p0 + (4 Ls - 1)/2 and
 * Du = delay0 + s (A1 - p0):
 *   delay' = d1 + Du (1 + s1),  slope_ppm' = 1e6 (s + s1 + s s1),  anchor' = A1,  carrier_hz' = (f1 + f)(1 + s),
 *   phase' = phi1 + (2 pi f1 / fs) Du + phase0 + (2 pi f (1 + s) / fs)(A1 - n_c);  scale, dc and imbalance copied.
 * (The second pass reads the capture at x1(u(n)), u(n) = n + delay0 + s (n - p0) the position in the first pass's row that belongs
 * at n: the composition of two affine maps; the first pass's carrier was taken out at u, not at n, hence the term f1 Du; the
 * (1 + s) is gsmcal_pair_align_params' reasoning.)  A coh_row whose status is not 0 or without a used window, or a value of
 * params_in that is not finite: every value of params_out NaN but the copied scale, returns GSMCAL_S_ALIGN_SKIPPED; otherwise 0.
 * GSMCAL_E_ARG: a NULL pointer, or |slope_ppm'| > 1000 (params_out is then all NaN but the scale). */
int gsmcal_apply_params_refine(const double* coh_row, const double* params_in, double* params_out);

/* ---- multi-GPU: one process per GPU, ONE collective ---------------------------------------------------------------
 * The reference has no distributed layer; units (dongle streams, ARFCN captures) are independent (gsm_sync_demod.m:112,
 * multi_rtl_sdr_gsm_FCCH_scanner.m:60-65,163), so ranks shard them block-contiguously and exchange only the result
 * table every rank needs for the inter-dongle comparison (gsm_sync_demod.m:151-158).  RCCL (librccl.so, loaded on first
 * use) over xGMI; the all-gather is enqueued on the context's stream right behind the kernels that fill the table.
 * Bootstrap: rank 0 obtains a 128-byte id and hands it to the other ranks by any means (gsmcal_comm_init_rank), or all
 * ranks name the same file on a shared filesystem (gsmcal_comm_init_file: rank 0 writes the id, the others wait for it). */
typedef struct gsmcal_comm gsmcal_comm;
#define GSMCAL_COMM_ID_BYTES 128
int gsmcal_comm_get_unique_id(void* id_out /* GSMCAL_COMM_ID_BYTES */);
int gsmcal_comm_init_rank(gsmcal_ctx* ctx, const void* id, int world, int rank, gsmcal_comm** out);
int gsmcal_comm_init_file(gsmcal_ctx* ctx, const char* path, int world, int rank, gsmcal_comm** out);
/* The id file is run-specific: it carries a magic word and a 64-bit nonce next to the id.  Rank 0 removes whatever sits at
 * `path` before it generates the id, publishes the new file by an atomic rename, and removes it again once the communicator
 * is up (ncclCommInitRank returns only after every rank has joined), so a file survives only a crashed bootstrap.  Readers
 * accept nothing but a complete file with the right magic AND the caller's nonce; with nonce 0 ("none") they instead
 * refuse files older than GSMCAL_COMM_STALE_S seconds (default 120) -- unsafe for a relaunch inside that window, which
 * would accept the dead launch's id.  Give every launch its own nonce (job id, launcher pid, start time).
 * gsmcal_comm_init_file derives one itself: GSMCAL_COMM_NONCE if set, else a hash of the launcher's run / job id
 * (TORCHELASTIC_RUN_ID unless it is torchrun's literal default "none", TORCHELASTIC_RESTART_COUNT, SLURM_JOB_ID,
 * SLURM_STEP_ID, PBS_JOBID, LSB_JOBID) and MASTER_ADDR:MASTER_PORT; 0 only if none of these exist.  A nonce DERIVED this way
 * may repeat from launch to launch (plain `torchrun`: RUN_ID "none", 127.0.0.1:29500 every time), so gsmcal_comm_init_file
 * keeps the age test on for it: a record is accepted only with the right nonce AND younger than the stale window.  Only a
 * nonce the caller chose (GSMCAL_COMM_NONCE, gsmcal_comm_init_file_nonce with nonce != 0) switches the age test off. */
int gsmcal_comm_init_file_nonce(gsmcal_ctx* ctx, const char* path, unsigned long long nonce, int world, int rank,
                                gsmcal_comm** out);
/* The nonce gsmcal_comm_init_file derives from the environment (see above); 0 = the environment identifies no launch. */
unsigned long long gsmcal_comm_default_nonce(void);
/* The file protocol alone (no GPU, no RCCL; what the two functions above run before ncclCommInitRank): rank 0 publishes
 * id_inout, the other ranks wait up to timeout_s seconds for it and receive it in id_inout.  GSMCAL_E_ARG on time-out.
 * gsmcal_comm_id_file_remove: rank 0's clean-up after the communicator is up. */
int gsmcal_comm_id_file_exchange(const char* path, unsigned long long nonce, int world, int rank,
                                 void* id_inout /* GSMCAL_COMM_ID_BYTES */, double timeout_s);
/* ... with the age test on whatever the nonce (what gsmcal_comm_init_file runs for a nonce derived from the environment). */
int gsmcal_comm_id_file_exchange_aged(const char* path, unsigned long long nonce, int world, int rank,
                                      void* id_inout /* GSMCAL_COMM_ID_BYTES */, double timeout_s);
int gsmcal_comm_id_file_remove(const char* path);
void gsmcal_comm_destroy(gsmcal_comm* comm);
/* d_all[r][i][c] = rank r's d_local[i][c]: rows_per_rank x cols doubles per rank (ranks with fewer units pad their block,
 * e.g. with NaN); device pointers; enqueued on the context's stream (gsmcal_sync() before reading d_all on the host). */
int gsmcal_allgather_table(gsmcal_ctx* ctx, gsmcal_comm* comm, const double* d_local, int rows_per_rank, int cols,
                           double* d_all);

/* The same collective off the critical path of the caller's stream: RCCL runs on a side stream of the context, behind an event
 * recorded on the context's stream at the time of the call; the context's stream does NOT wait for it, so the kernels of the
 * next batch start at once and the gather of batch i travels under the kernels of batch i+1 (gsm_sync_demod.m:151-158 only
 * needs the gathered table after the per-dongle loop).  `slot` (0..3) names the buffer pair in flight:
 *   gsmcal_allgather_wait(ctx, slot)  the context's stream waits -- on the GPU -- for that slot's collective: call it before
 *                                     enqueueing whatever overwrites d_local or reads d_all of the slot (no-op for a slot never posted);
 *   gsmcal_allgather_sync(ctx, slot)  blocks the host until that slot's collective has finished. */
int gsmcal_allgather_table_async(gsmcal_ctx* ctx, gsmcal_comm* comm, const double* d_local, int rows_per_rank, int cols,
                                 double* d_all, int slot);
int gsmcal_allgather_wait(gsmcal_ctx* ctx, int slot);
int gsmcal_allgather_sync(gsmcal_ctx* ctx, int slot);

/* ---- ingest ring: rtl_tcp bytes -> pinned host ring -> asynchronous H2D ----------------------------------
 * The reference reads every capture with fread(tcp_obj, 2*num_sample, 'uint8') into MATLAB memory and processes it in
 * place (gsm_sync_demod.m:94-104, multi_rtl_sdr_gsm_FCCH_scanner.m:117-131).  Here the socket reader writes straight into
 * a pinned host slot, the slot goes to its device twin on a copy stream, and the copy of batch k+1 runs under the kernels
 * of batch k.  A ring has `slots` (>= 2) slots of `batch_bytes`; per slot the cycle is
 *     host = gsmcal_ring_host(ring, s)          the producer fills it (recv() target, zero copy)
 *     gsmcal_ring_submit(ring, s)               async H2D on the ring's copy stream (waits, on the GPU, for the
 *                                               consumer's previous use of the slot)
 *     dev = gsmcal_ring_acquire(ring, s)        the context's stream waits (on the GPU) for that copy; returns the
 *                                               device buffer to hand to a *_dev entry point
 *     gsmcal_ring_release(ring, s)              after enqueueing the consumer: the slot may be overwritten once it is done
 *     gsmcal_ring_host_ready(ring, s)           host-side wait until the slot's H2D has finished, i.e. until the pinned
 *                                               host buffer may be refilled
 * No call blocks the host except gsmcal_ring_host_ready. */
typedef struct gsmcal_ring gsmcal_ring;
int gsmcal_ring_create(gsmcal_ctx* ctx, size_t batch_bytes, int slots, gsmcal_ring** out);
void gsmcal_ring_destroy(gsmcal_ring* ring);
void* gsmcal_ring_host(gsmcal_ring* ring, int slot);
int gsmcal_ring_submit(gsmcal_ring* ring, int slot, size_t bytes);
void* gsmcal_ring_acquire(gsmcal_ring* ring, int slot);
int gsmcal_ring_release(gsmcal_ring* ring, int slot);
int gsmcal_ring_host_ready(gsmcal_ring* ring, int slot);

/* Synthetic-input utility for benchmarks and tests (NOT part of the reference's path; SURVEY 8d: the 131 GB scanner
 * configuration is generated on the device).  Expands k seeded base captures (d_base: [k][2n] bytes) into d distinct
 * captures d_out: [d][2n]: capture first_unit+j = base[(first_unit+j) mod k] rotated by a per-capture number of
 * samples, every byte dithered by -1/0/+1 from a counter-based hash of (seed, unit, sample), clipped to 0..255.
 * multi-rtl-sdr-calibration_amd/synth.py:expand_capture() is the bit-identical host twin. */
int gsmcal_synth_expand_dev(gsmcal_ctx* ctx, const uint8_t* d_base, int k, long n, uint8_t* d_out, long d,
                            long first_unit, unsigned long long seed);

/* Debug/parity taps into the last calibrate/scan batch: copies per-stream intermediates to host.
 * coarse_pos/coarse_snr/fine_first/fcch_pos/sch_first: [D][GSMCAL_MAX_HITS]; counts: [D][5]
 * (n_coarse, n_fine_first, n_fcch, n_sch_first, n_pos_rows).  Any pointer may be NULL. */
int gsmcal_last_batch_details(gsmcal_ctx* ctx, int d, double* coarse_pos, double* coarse_snr,
                              double* fine_first, double* fcch_pos, double* sch_first, int* counts);

/* Parity tap: the per-window SNR table (move_fft_snr_runtime_avg.m:18-27, 1-based window i at index i-1) the coarse detector of
 * the last batch call built for `stream`.  *n_moving entries are the moving search's windows (every one computed in full);
 * entries beyond them (latency path only, up to *n_table) serve the hop walk and hold -inf where a window was proved to be
 * below the screening level.  The decisions snr - avg > th are taken on these values: the parity suite measures how far they
 * sit from the oracle's (the implementation noise the certified scan's 1e-6 dB margin has to cover).
 * Batches of more than 128 streams per internal lane keep no table (the scan kernel computes the values in LDS):
 * GSMCAL_E_UNSUPPORTED unless the context was created under GSMCAL_SNR_INLINE_KEEP=1. */
int gsmcal_last_batch_snr(gsmcal_ctx* ctx, int stream, double* snr, long cap, long* n_table, long* n_moving);

#ifdef __cplusplus
}
#endif
#endif /* GSMCAL_H */
