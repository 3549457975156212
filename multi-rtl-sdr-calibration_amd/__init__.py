"""gsmcal -- MI355X-native GSM FCCH+SCH calibration chain (package dir: multi-rtl-sdr-calibration_amd/).

Import it as `import gsmcal` (the top-level gsmcal.py aliases this directory, whose name is not a
valid Python identifier).  Sub-modules:
    api    -- host mirror of the reference's MATLAB functions + batched entry points (ctypes -> HIP)
    synth  -- seeded synthetic GSM IQ, GMSK modulator, fir1
    dist   -- multi-GPU sharding + all-gather of the calibration table (torch.distributed, RCCL)
    ingest -- rtl_tcp framing (command packets, flush, capture reads) + the pinned ring / async H2D of the C ABI
    build  -- hipcc build of csrc/ -> lib/libgsmcal.so
"""
from . import build, ingest, synth  # noqa: F401
from ._lib import GsmcalError, MAX_HITS, MAX_POS_ROWS, MAX_SUBBANDS, TABLE_COLS, DEMOD_COLS, MAX_BCCH, BCCH_COLS, SCH_COLS, SI_COLS, BLOCK_OCTETS, BLOCK_CODED, MAX_PAIR_BURSTS, PAIR_COLS, S_PAIR_FEW, MAX_ALIGN_MEMBERS, ALIGN_PARAMS, ALIGN_INFO_COLS, S_ALIGN_SKIPPED, MAX_COV_WINDOWS, COV_CHUNK, MAX_BEAMS, WEIGHTS_INFO_COLS, S_WEIGHTS_SINGULAR, APPLY_PARAMS, APPLY_INFO_COLS, ROW_COLS, MAX_ROW_WINDOWS, MAX_ROW_LAG, ROW_CHUNK, HYPERFRAME, CW_MAX_EVENTS, CW_COLS, CW_TILE, CW_OK, CW_SHORT, CW_ZERO, IQ_COLS, IQ_TILE, IQ_MAX_N, IQ_OK, IQ_SHORT, IQ_FLAT, SIGNATURES, lib_path, load  # noqa: F401
from .api import (  # noqa: F401
    Context, default_context, raw2iq, filter, chn_filter_8x_4x, chn_filter_4x, move_fft_snr_runtime_avg,
    specific_fft_snr_fix_avg, FCCH_coarse_position, FCCH_fine_correction, SCH_corr_rate_correction,
    carrier_correct_post_SCH, total_ppm_calculation, SCH_equalise, frontend_batch, frontend_batch_dev, fcch_scan_batch, calibrate_batch,
    last_batch_details, last_batch_snr, TABLE_FIELDS, fcch_scan_batch_dev, calibrate_batch_dev, synth_expand_dev,
    set_verbose, last_call_report, num2str, band_power_batch, band_power_batch_dev, split_spectrum_scan,
    diversity_spectrum_scan, FCCH_demod, fcch_demod_batch, fcch_demod_batch_dev, demod_rows, DEMOD_FIELDS,
    subband_power_batch, subband_power_batch_dev, multichannel_spectrum_scan, CW_check, cw_check_batch, cw_check_batch_dev,
    cw_rows, CW_FIELDS, BCCH_demod, bcch_demod_batch, bcch_demod_batch_dev, bcch_rows, BCCH_FIELDS,
    SCH_decode, sch_decode_batch, sch_decode_batch_dev, sch_rows, SCH_FIELDS, sch_alignment,
    BCCH_decode, bcch_decode_batch, bcch_decode_batch_dev, si_rows, SI_FIELDS, SI_BLOCK_FIELDS, si_fields,
    IQ_imbalance, iq_imbalance_batch, iq_imbalance_batch_dev, iq_correct, iq_rows, IQ_FIELDS,
    pair_coherence, pair_coherence_batch, pair_coherence_batch_dev, pair_rows, pair_lag0, PAIR_FIELDS, PAIR_BURST_FIELDS,
    pair_align, pair_align_batch, pair_align_batch_dev, pair_align_params, align_rows, coherent_combine, ALIGN_PARAM_FIELDS,
    ALIGN_INFO_FIELDS, array_covariance, array_covariance_dev, combine_weights, array_combine, array_combine_dev, burst_windows,
    WEIGHTS_INFO_FIELDS, apply_params, apply_calibration, apply_calibration_resident, apply_rows, APPLY_PARAM_FIELDS,
    row_coherence, row_coherence_resident, row_rows, ROW_FIELDS, ROW_WINDOW_FIELDS, valid_of, apply_params_refine, row_lag_search,
    retune_align,
)
