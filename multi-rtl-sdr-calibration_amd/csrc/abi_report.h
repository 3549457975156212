// abi_report.h -- the reference's console diagnostics (FCCH_coarse_position.m:6,28,92-94, FCCH_fine_correction.m:6,13,66,
// 96-99,116,156-161,190-193, SCH_corr_rate_correction.m:6,12,60,80,107-110,118, carrier_correct_post_SCH.m:6,11,17,73-79, FCCH_demod.m:6,9,43-49,65-66,
// BCCH_demod.m:15,69,72,101,104; gsmcal_SCH_decode's and gsmcal_BCCH_decode's own three lines each) as TEXT:
// the per-function entry points of abi_calls.h have the stream's state on the host anyway and leave the lines the .m file would
// have disp()ed in the context; gsmcal_last_call_report() hands them to the MEX gateway (mexPrintf) or the Python mirror.
// Included by gsmcal.hip ahead of abi_calls.h (host code only).
#pragma once
namespace {

// MATLAB's num2str for a real row vector: integers as %{w}d with w = digits + 2 (+ 1 if any is negative), everything else as
// %{d+7}.{d}g with d = max(floor(log10(max|x|)) + 5, 5) capped at 16; the pieces are concatenated and the result trimmed.
std::string rep_num2str(const double* x, int n) {
    if (n <= 0) return std::string();
    bool ints = true, neg = false;
    double mx = 0.0;
    for (int i = 0; i < n; ++i) {
        if (x[i] != floor(x[i]) || !std::isfinite(x[i])) ints = false;
        if (x[i] < 0.0) neg = true;
        if (std::isfinite(x[i]) && fabs(x[i]) > mx) mx = fabs(x[i]);
    }
    char fmt[32], buf[64];
    std::string out;
    const int lg = mx > 0.0 ? (int)floor(log10(mx)) : 0;
    if (ints) {
        const int w = (lg > 0 ? lg : 0) + (neg ? 1 : 0) + 3;
        snprintf(fmt, sizeof(fmt), "%%%d.0f", w);
    } else {
        int d = lg + 5;
        if (d < 5) d = 5;
        if (d > 16) d = 16;
        snprintf(fmt, sizeof(fmt), "%%%d.%dg", d + 7 + (neg ? 1 : 0), d);
    }
    for (int i = 0; i < n; ++i) {
        if (std::isnan(x[i])) snprintf(buf, sizeof(buf), "%*s", ints ? 5 : 12, "NaN");
        else if (std::isinf(x[i])) snprintf(buf, sizeof(buf), "%*s", ints ? 5 : 12, x[i] > 0 ? "Inf" : "-Inf");
        else snprintf(buf, sizeof(buf), fmt, x[i]);
        out += buf;
    }
    const size_t a = out.find_first_not_of(' ');
    const size_t b = out.find_last_not_of(' ');
    return a == std::string::npos ? std::string() : out.substr(a, b - a + 1);
}
std::string rep_num2str(double v) { return rep_num2str(&v, 1); }
std::string rep_diff(const double* x, int n) {
    std::vector<double> d(n > 1 ? n - 1 : 0);
    for (int i = 0; i + 1 < n; ++i) d[i] = x[i + 1] - x[i];
    return rep_num2str(d.data(), (int)d.size());
}

// the "Kinds of pos diff more than 2" block (FCCH_fine_correction.m:96-99 / SCH_corr_rate_correction.m:107-110)
void rep_spacing(std::string& r, const char* who, const double* pos, int n, int ov, double max_ppm) {
    const double d = 10.0 * 1250.0 * ov, d1 = 11.0 * 1250.0 * ov;
    const double max_th = floor(d * max_ppm * 1e-6), max_th1 = floor(d1 * max_ppm * 1e-6);
    std::vector<double> a(n > 1 ? n - 1 : 0), b(a.size());
    double na = 0, nb = 0;
    for (int i = 0; i + 1 < n; ++i) {
        a[i] = fabs(pos[i + 1] - pos[i] - d); b[i] = fabs(pos[i + 1] - pos[i] - d1);
        na += a[i] < max_th; nb += b[i] < max_th1;
    }
    const double cnt[2] = {na, nb};
    r += std::string(who) + " Warning! Kinds of pos diff more than 2!\n";
    r += "Expected len " + rep_num2str((double)(n - 1)) + ". Actual " + rep_num2str(cnt, 2) + "\n";
    r += "diff intra multiframe max th " + rep_num2str(max_th) + " actual " + rep_num2str(a.data(), (int)a.size()) + "\n";
    r += "diff inter multiframe max th " + rep_num2str(max_th1) + " actual " + rep_num2str(b.data(), (int)b.size()) + "\n";
}

// the tone estimates of nb bursts (FCCH_fine_correction.m:156-161 / carrier_correct_post_SCH.m:73-79)
void rep_tone(std::string& r, const char* who, const double* fo, int nb, double carrier_ppm) {
    double m = 0.0;
    for (int i = 0; i < nb; ++i) m += fo[i];
    m /= (double)nb;
    r += std::string(who) + " FCCH freq " + rep_num2str(fo, nb) + "\n";
    r += std::string(who) + " mean FCCH freq " + rep_num2str(m) + "\n";
    r += std::string(who) + " carrier error ppm " + rep_num2str(carrier_ppm) + "\n";
}

std::string report_coarse(const StreamState& st) {
    std::string r = " \n";
    if (st.n_coarse == 0) return r + "FCCH coarse: No FCCH found!\n";
    r += "FCCH coarse: hit successive " + rep_num2str((double)st.n_coarse) + " FCCH. pos " + rep_num2str(st.coarse_pos, st.n_coarse) + "\n";
    r += "FCCH coarse: pos diff " + rep_diff(st.coarse_pos, st.n_coarse) + "\n";
    r += "FCCH coarse: SNR " + rep_num2str(st.coarse_snr, st.n_coarse) + "\n";
    return r;
}

std::string report_fine(const StreamState& st, int ov, double max_ppm, double gate_db) {
    std::string r = " \n";
    const int code = st.stage_status[0];
    if (code == GSMCAL_S_FEW_HITS) return r + "FCCH fine: Warning! Length of hits is smaller than 5!\n";
    r += "FCCH fine: first round diff " + rep_diff(st.fine_first, st.n_fine) + "\n";
    if (code == GSMCAL_S_FINE_FEW) return r;
    if (code == GSMCAL_S_FINE_SPACING) { rep_spacing(r, "FCCH fine:", st.fine_first, st.n_fine, ov, max_ppm); return r; }
    r += "FCCH fine: sampling error ppm " + rep_num2str(st.sampling_ppm1) + "\n";
    if (st.r1_kind != 3) return r;                               // fewer than 5 bursts left: the carrier block is skipped (:142)
    int nb = st.fcch_is_sentinel ? 0 : st.n_fcch;
    if (nb == 0) for (nb = 0; nb < st.n_fine && nb < MAXH && st.fo_burst[nb] != 0.0; ++nb) {}     // (the gate zeroed n_fcch: the bursts that were estimated)
    rep_tone(r, "FCCH fine:", st.fo_burst, nb, st.carrier_ppm1);
    r += "FCCH fine: SNR " + rep_num2str(st.snr_burst, nb) + "\n";
    bool low = false;
    for (int i = 0; i < nb; ++i) low = low || st.snr_burst[i] < gate_db;
    if (low) r += "FCCH fine: Warning! Some FCCH SNR seems pretty low!\n";
    return r;
}

std::string report_sch(const StreamState& st, int ov, double max_ppm) {
    std::string r = " \n";
    const int code = st.stage_status[1];
    if (code == GSMCAL_S_FEW_HITS) return r + "SCH: Warning! Length of hits is smaller than 5!\n";
    if (code == GSMCAL_S_SCH_EDGE) return r + "SCH:  Warning! No peak around base position is found!\n";
    r += "SCH: first round diff " + rep_diff(st.sch_first, st.n_sch_first) + "\n";
    if (code == GSMCAL_S_SCH_FEW) return r;
    if (code == GSMCAL_S_SCH_SPACING) { rep_spacing(r, "SCH:", st.sch_first, st.n_sch_first, ov, max_ppm); return r; }
    r += "SCH: sampling error ppm " + rep_num2str(st.sampling_ppm2) + "\n";
    return r;
}

std::string report_post(const StreamState& st) {
    std::string r = " \n";
    const int code = st.stage_status[2];
    if (code == GSMCAL_S_POST_NO_POS) return r + "post SCH: Warning! No valid position information!\n";
    if (code == GSMCAL_S_POST_FEW_BCCH) return r + "post SCH: Warning! The number of BCCH bursts is less than 4!\n";
    if (st.r3_kind != 3) return r;
    int nb = 0;
    for (int i = 0; i < st.n_rows && i < MAXROWS; ++i) nb += st.pos_info[MAXROWS + i] == 0.0;
    if (nb > MAXH) nb = MAXH;
    if (nb > 0) rep_tone(r, "post SCH:", st.fo_burst, nb, st.carrier_ppm2);
    return r;
}

// FCCH_demod.m:6,9,43,45,49,65,66.  row: one row of the FCCH_demod table (GSMCAL_D_*), status 0 or GSMCAL_S_POST_NO_POS.
std::string report_fcch_demod(const double* row) {
    std::string r = " \n";
    if ((int)row[GSMCAL_D_STATUS] == GSMCAL_S_POST_NO_POS) return r + "FCCH demod: Warning! No valid position information!\n";
    const int nb = (int)row[GSMCAL_D_NUM_FCCH];
    r += "FCCH demod: FCCH freq " + rep_num2str(row + GSMCAL_D_FREQ, nb) + "\n";
    r += "FCCH demod: mean FCCH freq " + rep_num2str(row[GSMCAL_D_MEAN_FREQ]) + "\n";
    r += "FCCH demod: carrier error ppm " + rep_num2str(row[GSMCAL_D_CARRIER_PPM]) + "\n";
    r += "FCCH demod: SNR " + rep_num2str(row + GSMCAL_D_SNR, nb) + "\n";
    r += "FCCH demod: max idx " + rep_num2str(row + GSMCAL_D_MAX_IDX, nb) + "\n";
    return r;
}

// BCCH_demod.m:15,69,72,101,104.  row: one row of the BCCH_demod table (GSMCAL_B_*), status 0, GSMCAL_S_POST_FEW_BCCH or
// GSMCAL_S_BCCH_TSC_MIXED (the .m file prints nothing at the :9 exit, and no blank line first); fo: the n0 per-burst frequencies.
std::string report_bcch_demod(const double* row, const double* fo, int n0) {
    const int status = (int)row[GSMCAL_B_STATUS];
    if (status == GSMCAL_S_POST_FEW_BCCH) return "The number of BCCH bursts is less than 4!\n";
    std::string r = "post SCH freq " + rep_num2str(fo, n0) + "\n";
    const double both[2] = {row[GSMCAL_B_CARRIER_PPM], row[GSMCAL_B_MEAN_FO]};
    r += "carrier ppm and mean fo " + rep_num2str(both, 2) + "\n";
    if (status == 0) r += "Normal training sequence idx (BCCH) " + rep_num2str(row[GSMCAL_B_TSC_IDX]) + "\n";
    else r += "Fail to identity normal training sequence idx (BCCH).\n";
    return r;
}

// gsmcal_SCH_decode (the project's own lines; SCH_demod.m prints nothing of the kind).  row: one row of the SCH_decode table
// (GSMCAL_C_*), status 0 or GSMCAL_S_SCH_NO_DECODE.
std::string report_sch_decode(const double* row) {
    char buf[160];
    snprintf(buf, sizeof buf, "SCH bursts %d decoded %d consistent %d\n", (int)row[GSMCAL_C_NUM_SCH], (int)row[GSMCAL_C_NUM_OK],
             (int)row[GSMCAL_C_NUM_CONSISTENT]);
    std::string r = buf;
    if ((int)row[GSMCAL_C_STATUS] != 0) return r + "Fail to decode the SCH bursts.\n";
    snprintf(buf, sizeof buf, "BSIC %d frame number %ld at sample %ld\n", (int)row[GSMCAL_C_BSIC], (long)row[GSMCAL_C_FN_ANCHOR],
             (long)row[GSMCAL_C_POS_ANCHOR]);
    return r + buf;
}

// gsmcal_BCCH_decode (the project's own lines).  row: one row of the BCCH_decode table (GSMCAL_I_*), status 0 or
// GSMCAL_S_BCCH_NO_DECODE; si: what gsmcal_si_fields reads in the first ok block.
std::string report_bcch_decode(const double* row, const gsmcal_si_info& si) {
    char buf[160];
    snprintf(buf, sizeof buf, "BCCH blocks %d decoded %d\n", (int)row[GSMCAL_I_NUM_BLOCKS], (int)row[GSMCAL_I_NUM_OK]);
    std::string r = buf;
    if ((int)row[GSMCAL_I_STATUS] != 0) return r + "Fail to decode the BCCH blocks.\n";
    snprintf(buf, sizeof buf, "System information type %d cell identity %d LAI %d-%d-%d\n", si.si_type, si.cell_id, si.mcc, si.mnc, si.lac);
    return r + buf;
}

// gsmcal_IQ_imbalance (the project's own line).  row: one row of the I/Q table (GSMCAL_Q_*).
std::string report_iq_imbalance(const double* row) {
    const int status = (int)row[GSMCAL_Q_STATUS];
    if (status == GSMCAL_IQ_SHORT) return "I/Q imbalance undefined: fewer than two samples.\n";
    if (status == GSMCAL_IQ_FLAT) return "I/Q imbalance undefined: constant rail.\n";
    return "I/Q gain " + rep_num2str(row[GSMCAL_Q_GAIN]) + " phase " + rep_num2str(row[GSMCAL_Q_PHASE_DEG]) + " deg image rejection " +
           rep_num2str(row[GSMCAL_Q_IRR_DB]) + " dB DC " + rep_num2str(row + GSMCAL_Q_DC_I, 2) + "\n";
}

// gsmcal_pair_coherence (the project's own lines).  row: one row of the pair_coherence table (GSMCAL_P_*), status 0 or
// GSMCAL_S_PAIR_FEW.
std::string report_pair_coherence(const double* row) {
    char buf[200];
    snprintf(buf, sizeof buf, "pair bursts %d evaluated %d used %d adjacent %d\n", (int)row[GSMCAL_P_NUM_BURSTS], (int)row[GSMCAL_P_NUM_EVAL],
             (int)row[GSMCAL_P_NUM_USED], (int)row[GSMCAL_P_NUM_ADJACENT]);
    std::string r = buf;
    if ((int)row[GSMCAL_P_STATUS] != 0) return r + "Fewer than two bursts to compare the streams on.\n";
    r += "pair delay " + rep_num2str(row[GSMCAL_P_DELAY0]) + " samples drift " + rep_num2str(row[GSMCAL_P_REL_SAMPLING_PPM]) + " ppm rms " +
         rep_num2str(row[GSMCAL_P_DELAY_RMS]) + "\n";
    r += "pair carrier " + rep_num2str(row[GSMCAL_P_REL_CARRIER_HZ]) + " Hz phase " + rep_num2str(row[GSMCAL_P_PHASE0]) + " rad rms " +
         rep_num2str(row[GSMCAL_P_PHASE_RMS]) + "\n";
    r += "pair coherence mean " + rep_num2str(row[GSMCAL_P_MEAN_COHERENCE]) + " min " + rep_num2str(row[GSMCAL_P_MIN_COHERENCE_SEEN]) + "\n";
    return r;
}

// gsmcal_pair_align / gsmcal_pair_align_batch (the project's own lines).  info: [G + 1][GSMCAL_ALIGN_INFO_COLS]; one line per member
// (status, valid interval), one for the sum.
std::string report_pair_align(const int* members, const double* info, int G, bool with_sum) {
    char buf[200];
    std::string r;
    for (int g = 0; g < G; ++g) {
        const double* o = info + (size_t)g * GSMCAL_ALIGN_INFO_COLS;
        snprintf(buf, sizeof buf, "align member %d stream %d status %d valid [%ld, %ld) %ld samples\n", g, members[g], (int)o[GSMCAL_AI_STATUS],
                 (long)o[GSMCAL_AI_FIRST_VALID], (long)o[GSMCAL_AI_END_VALID], (long)o[GSMCAL_AI_NUM_VALID]);
        r += buf;
    }
    if (with_sum) {
        const double* o = info + (size_t)G * GSMCAL_ALIGN_INFO_COLS;
        snprintf(buf, sizeof buf, "align sum of %d members valid [%ld, %ld) weights ", (int)o[GSMCAL_AI_STATUS], (long)o[GSMCAL_AI_FIRST_VALID],
                 (long)o[GSMCAL_AI_END_VALID]);
        r += buf + rep_num2str(o[GSMCAL_AI_NUM_VALID]) + "\n";
    }
    return r;
}

}  // namespace
