"""Host-side mirror of the reference's MATLAB interface for the calibration path, over libgsmcal.so.

MATLAB is not available in the build image, so the host layer above the C ABI is Python.  Each
function keeps the reference function's name, argument order/meaning, 1-based positions and
sentinel returns (scalar -1.0 / inf, pos_info = [[-1, -1]]) so that tests read like calls of the
.m files:

    b = raw2iq(a)                                                   raw2iq.m:5
    r = chn_filter_8x_4x(s)                                         chn_filter_8x_4x.m:5
    r = chn_filter_4x(s)                                            chn_filter_4x.m:5
    [hit_flag,hit_idx,hit_avg_snr,hit_snr] = move_fft_snr_runtime_avg(s,mv_len,fft_len,th)
    [hit_flag,hit_idx,hit_snr] = specific_fft_snr_fix_avg(s,target_set,fft_len,th,avg_snr)
    [position,snr] = FCCH_coarse_position(s,decimation_ratio)
    [FCCH_pos,r,sampling_ppm,carrier_ppm] = FCCH_fine_correction(s,base_position,ov,carrier_freq)
    [pos_info,r,sampling_ppm] = SCH_corr_rate_correction(s,FCCH_pos,sch_training_sequence,ov)
    [r,carrier_ppm] = carrier_correct_post_SCH(s,pos_info,ov,carrier_freq)
    FCCH_demod(s,pos_info,ov,carrier_freq)                           FCCH_demod.m:5 (what it prints, returned as a dict)
    [idx,r,carrier_ppm] = BCCH_demod(s,pos_info,normal_training_sequence,ov,carrier_freq)     BCCH_demod.m:5 (a dict)
    ppm_out = total_ppm_calculation(ppm_in)
and, without a counterpart in the reference (its SCH_demod.m returns nothing, its BCCH_demod.m stops at the training sequence index):
SCH_decode(s,pos_info,sch_training_sequence,ov) and BCCH_decode(s,pos_info,tsc,ov); pair_coherence(s_a,s_b,pos_info_a,ov,lag0)
and pair_align(s,ov,params,out_len) / coherent_combine(...) for the goal its README names, dongles that work together coherently
(measure how far apart two streams are; put them on one time base and add them up); and IQ_imbalance(s) / iq_correct(s,gain,sin_phase)
for the I/Q imbalance its TODO item 4.5 asks about.

Everything computes on the GPU through the C ABI; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _lib
from ._lib import BCCH_COLS, SCH_COLS, SI_COLS, PAIR_COLS, MAX_PAIR_BURSTS, ALIGN_PARAMS, ALIGN_INFO_COLS, APPLY_PARAMS, APPLY_INFO_COLS, ROW_COLS, MAX_ROW_WINDOWS, BLOCK_OCTETS, BLOCK_CODED, CW_COLS, CW_MAX_EVENTS, IQ_COLS, DEMOD_COLS, MAX_BCCH, MAX_HITS, MAX_POS_ROWS, TABLE_COLS, GsmcalError

_CTX = {}


_VERBOSE = [os.environ.get("GSMCAL_VERBOSE") == "1"]


def set_verbose(on=True):
    """Print the reference's console diagnostics (FCCH_coarse_position.m:92-94, FCCH_fine_correction.m:66,116,156-161,190, ...:
    gsmcal_last_call_report) after every per-function call, as the .m files do.  Also switched on by GSMCAL_VERBOSE=1."""
    _VERBOSE[0] = bool(on)


def last_call_report(ctx=None):
    """The lines the .m file of the most recent per-function call would have disp()ed (a str, '\\n'-separated)."""
    ctx = ctx or default_context()
    n = ctx.lib.gsmcal_last_call_report(ctx.h, None, 0)
    if n <= 0:
        return ""
    buf = C.create_string_buffer(int(n) + 1)
    ctx.lib.gsmcal_last_call_report(ctx.h, buf, len(buf))
    return buf.value.decode()


def num2str(x):
    """MATLAB's num2str for a scalar / row vector, as the library formats its diagnostics (gsmcal_num2str)."""
    v = np.ascontiguousarray(np.atleast_1d(np.asarray(x, dtype=np.float64)).ravel())
    lib = _lib.load()
    n = lib.gsmcal_num2str(_dp(v), len(v), None, 0)
    buf = C.create_string_buffer(int(n) + 1)
    lib.gsmcal_num2str(_dp(v), len(v), buf, len(buf))
    return buf.value.decode()


def _say(ctx):
    if _VERBOSE[0]:
        txt = last_call_report(ctx)
        if txt:
            print(txt, end="")


class Context:
    """One GPU + one HIP stream (gsmcal_ctx)."""

    def __init__(self, device=0, stream=None):
        self.lib = _lib.load()
        h = C.c_void_p()
        if stream is None:
            rc = self.lib.gsmcal_ctx_create(int(device), C.byref(h))
        else:
            rc = self.lib.gsmcal_ctx_create_on_stream(int(device), C.c_void_p(int(stream)), C.byref(h))
        if rc != 0:
            raise GsmcalError(f"gsmcal_ctx_create(device={device}) failed with {rc}: no usable gfx950 GPU "
                              f"(this package has no CPU fallback)")
        self.h = h
        self.device = device
        self.stream_handle = None if stream is None else int(stream)   # the caller's HIP stream (None: the context's own)

    def close(self):
        if getattr(self, "h", None):
            self.lib.gsmcal_ctx_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    _E_NAMES = {-1: "GSMCAL_E_ARG (an argument is null, zero or out of its documented range: include/gsmcal.h)", -2: "GSMCAL_E_HIP",
                -3: "GSMCAL_E_NO_DEVICE", -4: "GSMCAL_E_CAPACITY (an output buffer's capacity argument is too small)",
                -5: "GSMCAL_E_INDEX (MATLAB would raise 'index exceeds matrix dimensions')", -6: "GSMCAL_E_UNSUPPORTED"}

    def check(self, rc, what):
        if rc < 0:
            msg = self.lib.gsmcal_last_error(self.h)
            text = msg.decode() if msg else ""
            raise GsmcalError(f"{what} failed with {rc} = {self._E_NAMES.get(rc, '?')}" + (f": {text}" if text else ""))
        return rc

    def sync(self):
        self.check(self.lib.gsmcal_sync(self.h), "gsmcal_sync")

    def set_pipeline_depth(self, depth):
        """gsmcal_ctx_set_pipeline_depth: up to `depth` consecutive single-lane calibrate_batch_dev calls in flight (the front
        end of call i+1 under the tail of call i); outputs of call i complete at call i+depth or sync().  1 = off."""
        self.check(self.lib.gsmcal_ctx_set_pipeline_depth(self.h, int(depth)), "gsmcal_ctx_set_pipeline_depth")

    def pipeline_depth(self):
        return int(self.lib.gsmcal_ctx_get_pipeline_depth(self.h))

    def pipeline_queues(self):
        """gsmcal_ctx_pipeline_queues: internal streams seen running side by side (0 before the first call in flight)"""
        return int(self.lib.gsmcal_ctx_pipeline_queues(self.h))

    def fused_tail_reruns(self):
        """how often gsmcal_sync / a host-buffer call re-ran calls with the four-launch tail after a fused tail timed out"""
        return int(self.lib.gsmcal_fused_tail_reruns(self.h))

    def fused_tail_stats(self):
        """(batch calls that took the fused tail, calls the one-fused-tail-per-device gate sent to the four-launch tail)"""
        a, b = C.c_ulonglong(0), C.c_ulonglong(0)
        self.check(self.lib.gsmcal_fused_tail_stats(self.h, C.byref(a), C.byref(b)), "gsmcal_fused_tail_stats")
        return int(a.value), int(b.value)

    # ---- thresholds (gsmcal_params: the constants the reference hard-codes) ----
    def get_params(self):
        p = _lib.Params()
        self.check(self.lib.gsmcal_get_params(self.h, C.byref(p)), "gsmcal_get_params")
        return p

    def set_params(self, **kw):
        p = self.get_params()
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(f"gsmcal_params has no field {k}")
            setattr(p, k, v)
        self.check(self.lib.gsmcal_set_params(self.h, C.byref(p)), "gsmcal_set_params")

    # ---- device memory ----
    def alloc(self, nbytes):
        p = C.c_void_p()
        self.check(self.lib.gsmcal_dev_alloc(self.h, int(nbytes), C.byref(p)), "gsmcal_dev_alloc")
        return p.value

    def free(self, ptr):
        self.check(self.lib.gsmcal_dev_free(self.h, C.c_void_p(ptr)), "gsmcal_dev_free")

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self.check(self.lib.gsmcal_memcpy_h2d(self.h, C.c_void_p(dptr), arr.ctypes.data_as(C.c_void_p), arr.nbytes),
                   "gsmcal_memcpy_h2d")

    def d2h(self, arr, dptr):
        assert arr.flags.c_contiguous
        self.check(self.lib.gsmcal_memcpy_d2h(self.h, arr.ctypes.data_as(C.c_void_p), C.c_void_p(dptr), arr.nbytes),
                   "gsmcal_memcpy_d2h")

    # ---- profiling ----
    def profile_enable(self, on=True):
        self.check(self.lib.gsmcal_profile_enable(self.h, 1 if on else 0), "gsmcal_profile_enable")

    def profile_filter(self, substr=None):
        self.check(self.lib.gsmcal_profile_filter(self.h, substr.encode() if substr else None), "gsmcal_profile_filter")

    def profile_reset(self):
        self.check(self.lib.gsmcal_profile_reset(self.h), "gsmcal_profile_reset")

    def profile_get(self):
        cap = 64
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        n = (C.c_long * cap)()
        k = self.check(self.lib.gsmcal_profile_get(self.h, cap, names, ms, n), "gsmcal_profile_get")
        return {names[i].decode(): (ms[i], n[i]) for i in range(min(k, cap))}


def default_context(device=0):
    if device not in _CTX:
        _CTX[device] = Context(device)
    return _CTX[device]


def _dp(a):
    return a.ctypes.data_as(_lib.c_double_p)


def _cplx_in(s):
    """complex (n,) or (n,d) -> contiguous column-major interleaved doubles, returns (buf, n, d)."""
    s = np.asarray(s)
    if s.ndim == 1:
        s = s[:, None]
    n, d = s.shape
    buf = np.ascontiguousarray(s.T.astype(np.complex128))  # (d, n): each column contiguous
    return buf, n, d


# ------------------------------------------------------------------------------------------------
def raw2iq(a, ctx=None):
    """b = raw2iq(a) -- raw2iq.m:5-8.  a: (2N,) or (2N,D) byte values (uint8 or doubles)."""
    ctx = ctx or default_context()
    a = np.asarray(a)
    squeeze = a.ndim == 1
    if squeeze:
        a = a[:, None]
    rows, d = a.shape
    out = np.empty((d, rows // 2), dtype=np.complex128)
    if a.dtype == np.uint8:
        buf = np.ascontiguousarray(a.T)
        rc = ctx.lib.gsmcal_raw2iq_u8(ctx.h, buf.ctypes.data_as(_lib.c_u8_p), rows, d, _dp(out))
    else:
        buf = np.ascontiguousarray(a.T.astype(np.float64))
        rc = ctx.lib.gsmcal_raw2iq(ctx.h, _dp(buf), rows, d, _dp(out))
    ctx.check(rc, "raw2iq")
    return out[0] if squeeze else out.T


def filter(coef, s, decim=1, ctx=None):  # noqa: A001 - mirrors MATLAB's filter(coef,1,s)
    """r = filter(coef,1,s) column-wise (gsm_sync_demod.m:110), optionally r(1:decim:end,:)."""
    ctx = ctx or default_context()
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    squeeze = np.asarray(s).ndim == 1
    buf, n, d = _cplx_in(s)
    nd = (n + decim - 1) // decim
    out = np.empty((d, nd), dtype=np.complex128)
    ctx.check(ctx.lib.gsmcal_filter(ctx.h, _dp(coef), len(coef), _dp(buf), n, d, decim, _dp(out)), "filter")
    return out[0] if squeeze else out.T


def chn_filter_8x_4x(s, num=None, ctx=None):
    """r = chn_filter_8x_4x(s) -- chn_filter_8x_4x.m:5-15 (60 built-in taps unless `num` is given)."""
    ctx = ctx or default_context()
    squeeze = np.asarray(s).ndim == 1
    buf, n, d = _cplx_in(s)
    out = np.empty((d, (n + 1) // 2), dtype=np.complex128)
    if num is None:
        rc = ctx.lib.gsmcal_chn_filter_8x_4x(ctx.h, _dp(buf), n, d, None, 0, _dp(out))
    else:
        num = np.ascontiguousarray(num, dtype=np.float64)
        rc = ctx.lib.gsmcal_chn_filter_8x_4x(ctx.h, _dp(buf), n, d, _dp(num), len(num), _dp(out))
    ctx.check(rc, "chn_filter_8x_4x")
    return out[0] if squeeze else out.T


def chn_filter_4x(s, num=None, ctx=None):
    """r = chn_filter_4x(s) -- chn_filter_4x.m:5-13 (30 built-in taps of gsm_chn_filter_4x.fda unless `num` is given)."""
    ctx = ctx or default_context()
    squeeze = np.asarray(s).ndim == 1
    buf, n, d = _cplx_in(s)
    out = np.empty((d, n), dtype=np.complex128)
    if num is None:
        rc = ctx.lib.gsmcal_chn_filter_4x(ctx.h, _dp(buf), n, d, None, 0, _dp(out))
    else:
        num = np.ascontiguousarray(num, dtype=np.float64)
        rc = ctx.lib.gsmcal_chn_filter_4x(ctx.h, _dp(buf), n, d, _dp(num), len(num), _dp(out))
    ctx.check(rc, "chn_filter_4x")
    return out[0] if squeeze else out.T


def move_fft_snr_runtime_avg(s, mv_len, fft_len, th, ctx=None):
    ctx = ctx or default_context()
    buf, n, _ = _cplx_in(np.asarray(s).ravel())
    hf = C.c_int()
    hi, ha, hs = C.c_double(), C.c_double(), C.c_double()
    ctx.check(ctx.lib.gsmcal_move_fft_snr_runtime_avg(ctx.h, _dp(buf), n, int(mv_len), int(fft_len), float(th),
                                                      C.byref(hf), C.byref(hi), C.byref(ha), C.byref(hs)),
              "move_fft_snr_runtime_avg")
    return bool(hf.value), (int(hi.value) if hf.value else -1), ha.value, hs.value


def specific_fft_snr_fix_avg(s, target_set, fft_len, th, avg_snr, ctx=None):
    ctx = ctx or default_context()
    buf, n, _ = _cplx_in(np.asarray(s).ravel())
    ts = (C.c_double * 2)(float(target_set[0]), float(target_set[1]))
    hf = C.c_int()
    hi, hs = C.c_double(), C.c_double()
    ctx.check(ctx.lib.gsmcal_specific_fft_snr_fix_avg(ctx.h, _dp(buf), n, ts, int(fft_len), float(th),
                                                      float(avg_snr), C.byref(hf), C.byref(hi), C.byref(hs)),
              "specific_fft_snr_fix_avg")
    return bool(hf.value), (int(hi.value) if hf.value else -1), hs.value


def FCCH_coarse_position(s, decimation_ratio, ctx=None):
    """[position, snr] = FCCH_coarse_position(s, decimation_ratio); (-1.0, -1.0) when nothing found."""
    ctx = ctx or default_context()
    buf, n, _ = _cplx_in(np.asarray(s).ravel())
    pos = np.zeros(MAX_HITS)
    snr = np.zeros(MAX_HITS)
    cnt = C.c_int()
    rc = ctx.check(ctx.lib.gsmcal_FCCH_coarse_position(ctx.h, _dp(buf), n, int(decimation_ratio), _dp(pos),
                                                       _dp(snr), MAX_HITS, C.byref(cnt)), "FCCH_coarse_position")
    _say(ctx)
    if rc == 1:
        return -1.0, -1.0
    return pos[:cnt.value].copy(), snr[:cnt.value].copy()


def _r_in(s):
    """A stream argument that may be the reference's r = -1 sentinel."""
    if np.ndim(s) == 0:
        return None, 0
    buf, n, _ = _cplx_in(np.asarray(s).ravel())
    return buf, n


def FCCH_fine_correction(s, base_position, oversampling_ratio, carrier_freq, ctx=None, want_r=True):
    """[FCCH_pos, r, sampling_ppm, carrier_ppm] = FCCH_fine_correction(...) -- FCCH_fine_correction.m:5."""
    ctx = ctx or default_context()
    buf, n = _r_in(s)
    bp = np.ascontiguousarray(np.atleast_1d(np.asarray(base_position, dtype=np.float64)))
    pos = np.zeros(MAX_HITS)
    npos = C.c_int()
    r = np.empty(n if want_r else 0, dtype=np.complex128)
    lr = C.c_long()
    sp, cp = C.c_double(), C.c_double()
    ctx.check(ctx.lib.gsmcal_FCCH_fine_correction(ctx.h, _dp(buf), n, _dp(bp), len(bp), int(oversampling_ratio),
                                                  float(carrier_freq), _dp(pos), MAX_HITS, C.byref(npos),
                                                  _dp(r) if want_r else None, len(r), C.byref(lr),
                                                  C.byref(sp), C.byref(cp)), "FCCH_fine_correction")
    _say(ctx)
    fpos = pos[:npos.value].copy()
    if npos.value == 1 and fpos[0] == -1.0:
        fpos = -1.0
    rr = -1.0 if lr.value < 0 else (r[:lr.value] if want_r else lr.value)
    return fpos, rr, sp.value, cp.value


def SCH_corr_rate_correction(s, FCCH_pos, sch_training_sequence, oversampling_ratio, ctx=None, want_r=True):
    """[pos_info, r, sampling_ppm] = SCH_corr_rate_correction(...) -- SCH_corr_rate_correction.m:5."""
    ctx = ctx or default_context()
    buf, n = _r_in(s)
    fp = np.ascontiguousarray(np.atleast_1d(np.asarray(FCCH_pos, dtype=np.float64)))
    ts = np.ascontiguousarray(np.asarray(sch_training_sequence, dtype=np.complex128).ravel())
    pi = np.zeros((2, MAX_POS_ROWS))
    nrows = C.c_int()
    r = np.empty(n if want_r else 0, dtype=np.complex128)
    lr = C.c_long()
    sp = C.c_double()
    ctx.check(ctx.lib.gsmcal_SCH_corr_rate_correction(ctx.h, _dp(buf) if buf is not None else None, n, _dp(fp),
                                                      len(fp), _dp(ts), len(ts), int(oversampling_ratio), _dp(pi),
                                                      MAX_POS_ROWS, C.byref(nrows), _dp(r) if want_r else None,
                                                      len(r), C.byref(lr), C.byref(sp)), "SCH_corr_rate_correction")
    _say(ctx)
    pos_info = pi[:, :nrows.value].T.copy()
    rr = -1.0 if lr.value < 0 else (r[:lr.value] if want_r else lr.value)
    return pos_info, rr, sp.value


def _pos_info_in(pos_info):
    """pos_info as a MATLAB-signature wrapper takes it -> (the (rows, 2) table, rows, its column-major copy with ld = rows)"""
    pi = np.atleast_2d(np.asarray(pos_info, dtype=np.float64))
    return pi, pi.shape[0], np.ascontiguousarray(pi.T)


def carrier_correct_post_SCH(s, pos_info, oversampling_ratio, carrier_freq, ctx=None, want_r=True):
    """[r, carrier_ppm] = carrier_correct_post_SCH(...) -- carrier_correct_post_SCH.m:5."""
    ctx = ctx or default_context()
    buf, n = _r_in(s)
    pi, rows, pic = _pos_info_in(pos_info)
    r = np.empty(n if want_r else 0, dtype=np.complex128)
    lr = C.c_long()
    cp = C.c_double()
    ctx.check(ctx.lib.gsmcal_carrier_correct_post_SCH(ctx.h, _dp(buf) if buf is not None else None, n, _dp(pic),
                                                      rows, rows, int(oversampling_ratio), float(carrier_freq),
                                                      _dp(r) if want_r else None, len(r), C.byref(lr), C.byref(cp)),
              "carrier_correct_post_SCH")
    _say(ctx)
    rr = -1.0 if lr.value < 0 else (r[:lr.value] if want_r else lr.value)
    return rr, cp.value


def SCH_equalise(s, pos_info, training_sequence, oversampling_ratio, ctx=None):
    """Front end of SCH_demod(s, pos_info, training_sequence, ov) -- SCH_demod.m:53-59,79-90: the equalised burst of
    every SCH row of pos_info, shape (num_sch, 194*ov).  pos_info all -1 (:8-11) -> None."""
    ctx = ctx or default_context()
    buf, n = _r_in(s)
    pi, rows, pic = _pos_info_in(pos_info)
    ts = np.ascontiguousarray(np.asarray(training_sequence, dtype=np.complex128).ravel())
    L = 194 * int(oversampling_ratio)
    cap = int(np.sum(pi[:, 1] == 1)) if pi.shape[1] > 1 else 0
    out = np.empty((max(cap, 1), L), dtype=np.complex128)
    nb, lf = C.c_int(), C.c_int()
    rc = ctx.check(ctx.lib.gsmcal_SCH_equalise(ctx.h, _dp(buf) if buf is not None else None, n, _dp(pic), rows, rows, _dp(ts),
                                               len(ts), int(oversampling_ratio), _dp(out), cap, C.byref(nb), C.byref(lf)),
                   "SCH_equalise")
    if rc == 10:
        return None
    return out[:nb.value]


def FCCH_demod(s, pos_info, oversampling_ratio, carrier_freq, ctx=None):
    """FCCH_demod(s, pos_info, ov, carrier_freq) -- FCCH_demod.m:5-66, the check behind the calibration: per FCCH burst of
    pos_info the tone frequency `freq`, the in-band SNR `snr` (dB; NaN where the reference's noise_power is negative) and the
    offset of the spectrum's peak `max_idx` (max_idx - (fft_len/2+1), :66); `mean_freq` and the carrier error still left,
    `carrier_ppm`.  Returns a dict of these, or None at the :8 exit (pos_info all -1)."""
    ctx = ctx or default_context()
    buf, n = _r_in(s)
    pi, rows, pic = _pos_info_in(pos_info)
    cap = int(np.sum(pi[:, 1] == 0)) if pi.shape[1] > 1 else 0
    freq, snr, idx = (np.full(max(cap, 1), np.nan) for _ in range(3))
    nb = C.c_int()
    mf, cp = C.c_double(), C.c_double()
    rc = ctx.check(ctx.lib.gsmcal_FCCH_demod(ctx.h, _dp(buf) if buf is not None else None, n, _dp(pic), rows, rows,
                                             int(oversampling_ratio), float(carrier_freq), _dp(freq), _dp(snr), _dp(idx), cap,
                                             C.byref(nb), C.byref(mf), C.byref(cp)), "FCCH_demod")
    _say(ctx)
    if rc == 10:
        return None
    k = nb.value
    return {"freq": freq[:k], "snr": snr[:k], "max_idx": idx[:k].astype(np.int64), "mean_freq": mf.value, "carrier_ppm": cp.value}


def _templates_in(normal_training_sequence, oversampling_ratio):
    """(len_ts, 8) complex as gsm_normal_training_sequence_gen returns it -> (buf, len_ts): the columns one after the other"""
    t = np.asarray(normal_training_sequence, dtype=np.complex128)
    if t.ndim != 2 or t.shape[1] != 8:
        raise ValueError("normal_training_sequence must be (26*oversampling_ratio, 8)")
    return np.ascontiguousarray(t.T), t.shape[0]


def BCCH_demod(s, pos_info, normal_training_sequence, oversampling_ratio, carrier_freq, ctx=None, want_r=True):
    """[normal_training_sequence_idx, r, carrier_ppm] = BCCH_demod(s, pos_info, normal_training_sequence, ov, carrier_freq) --
    BCCH_demod.m with the two names it leaves undefined as arguments (include/gsmcal.h): which of the eight normal training
    sequences (synth.normal_training_sequences(ov), (26*ov, 8)) the BCCH bursts of pos_info carry.  Returns None at the :9 exit
    (pos_info all -1), otherwise a dict: `idx` (1..8, or -1), `r` (the stream rotated at :76; -1.0 where the .m file leaves it, or
    with want_r=False), `carrier_ppm`, `status` (0, 11 = fewer than 4 BCCH bursts, 13 = the first four disagree), `corr_val` (8, 4)
    -- and, for every type-2 row, not only four: `num_bcch`, `mean_fo`, `num_agree`, `max_idx`, `peak`, `runner_up`, `phase`;
    `row` is the (BCCH_COLS,) table row bcch_demod_batch holds for this stream."""
    ctx = ctx or default_context()
    buf, n = _r_in(s)
    pi, rows, pic = _pos_info_in(pos_info)
    ts, len_ts = _templates_in(normal_training_sequence, oversampling_ratio)
    r = np.empty(n, dtype=np.complex128) if want_r and n > 0 else None
    idx, lr, cp = C.c_int(), C.c_long(), C.c_double()
    corr = np.full((4, 8), np.nan + 0j)
    row = np.full(BCCH_COLS, np.nan)
    rc = ctx.check(ctx.lib.gsmcal_BCCH_demod(ctx.h, _dp(buf) if buf is not None else None, n, _dp(pic), rows, rows, _dp(ts), len_ts,
                                             int(oversampling_ratio), float(carrier_freq), C.byref(idx), _dp(r) if r is not None else None,
                                             n, C.byref(lr), C.byref(cp), _dp(corr), _dp(row)), "BCCH_demod")
    _say(ctx)
    if rc == _lib.S_POST_NO_POS:
        return None
    out = {"idx": idx.value, "r": r if r is not None and lr.value > 0 else -1.0, "carrier_ppm": cp.value, "status": rc,
           "corr_val": corr.T.copy() if rc != _lib.S_POST_FEW_BCCH else None}
    t = bcch_rows(row)
    k = int(t["num_bcch"][0])
    out.update(num_bcch=k, mean_fo=float(t["mean_fo"][0]), num_agree=t["num_agree"][0], row=row)
    for name in ("max_idx", "peak", "runner_up", "phase"):
        out[name] = t[name][0, :min(k, MAX_BCCH)].copy()
    return out


def _sch_template_in(sch_training_sequence):
    t = np.ascontiguousarray(np.asarray(sch_training_sequence, dtype=np.complex128).ravel())
    return t, len(t)


def SCH_decode(s, pos_info, sch_training_sequence, oversampling_ratio, ctx=None, want_soft=False):
    """SCH_decode(s, pos_info, sch_training_sequence, ov) -- the project's own function (include/gsmcal.h; not a
    port of SCH_demod.m): the BSIC and the GSM frame number the SCH bursts of pos_info carry.  ov 2, 4 or 8.  Returns None when
    pos_info is all -1, otherwise a dict: `status` (0, or 14 = fewer than two bursts decode consistently), `bsic`, `fn_anchor`,
    `pos_anchor` (-1 at status 14), `num_sch`, `num_ok`, `num_consistent`, `mean_slope`, per SCH burst `ok`, `bsic_b`, `fn`,
    `ts_err`, `corrected`, `slope`, `amp` (NaN for a burst that was not evaluated), `u` (num_sch, 39) uint8 -- the decoded words
    -- and with want_soft `soft` (num_sch, 148); `row` is the (SCH_COLS,) table row sch_decode_batch holds for this stream."""
    ctx = ctx or default_context()
    buf, n = _r_in(s)
    pi, rows, pic = _pos_info_in(pos_info)
    ts, len_ts = _sch_template_in(sch_training_sequence)
    bsic, fn, pos = C.c_int(), C.c_long(), C.c_long()
    row = np.full(SCH_COLS, np.nan)
    soft = np.empty((MAX_HITS, 148)) if want_soft else None
    u = np.empty((MAX_HITS, 39), dtype=np.uint8)
    rc = ctx.check(ctx.lib.gsmcal_SCH_decode(ctx.h, _dp(buf) if buf is not None else None, n, _dp(pic), rows, rows, _dp(ts), len_ts,
                                             int(oversampling_ratio), C.byref(bsic), C.byref(fn), C.byref(pos), _dp(row),
                                             _dp(soft) if want_soft else None, u.ctypes.data_as(_lib.c_u8_p)), "SCH_decode")
    _say(ctx)
    if rc == _lib.S_POST_NO_POS:
        return None
    t = sch_rows(row)
    k = min(int(t["num_sch"][0]), MAX_HITS) if rc >= 0 else 0
    out = {"status": rc, "bsic": bsic.value, "fn_anchor": fn.value, "pos_anchor": pos.value, "num_sch": int(t["num_sch"][0]),
           "num_ok": int(t["num_ok"][0]), "num_consistent": int(t["num_consistent"][0]), "mean_slope": float(t["mean_slope"][0]),
           "u": u[:k].copy(), "row": row}
    for name in ("ok", "bsic_b", "fn", "ts_err", "corrected", "slope", "amp"):
        out[name] = t[name][0, :k].copy()
    if want_soft:
        out["soft"] = soft[:k].copy()
    return out


class _SiInfo(C.Structure):
    _fields_ = [(name, C.c_int) for name in ("valid", "msg_type", "si_type", "cell_id", "mcc", "mnc", "mnc_digits", "lac")]


def _si_dict(info):
    return {name: int(getattr(info, name)) for name, _ in _SiInfo._fields_}


def si_fields(octets):
    """What a decoded BCCH block says about the cell: gsmcal_si_fields (include/gsmcal_si.h, plain C, the definition libgsmcal.so
    exports) on 23 octets -> dict(valid, msg_type, si_type, cell_id, mcc, mnc, mnc_digits, lac); fields a message does not carry
    are -1, valid is 0 for anything the parser does not recognise.  Needs no context and no GPU."""
    o = np.ascontiguousarray(np.asarray(octets, dtype=np.uint8).ravel())
    if o.shape != (BLOCK_OCTETS,):
        raise ValueError("si_fields: 23 octets")
    fn = _lib.load().gsmcal_si_fields
    fn.restype, fn.argtypes = C.c_int, [_lib.c_u8_p, C.POINTER(_SiInfo)]
    info = _SiInfo()
    fn(o.ctypes.data_as(_lib.c_u8_p), C.byref(info))
    return _si_dict(info)


def BCCH_decode(s, pos_info, tsc, oversampling_ratio, ctx=None, want_soft=False):
    """BCCH_decode(s, pos_info, tsc, ov) -- the project's own function (include/gsmcal.h; BCCH_demod.m stops at
    the training sequence index): the system information the BCCH blocks of pos_info carry.  A block is four type-2 rows directly
    behind a type-1 row; tsc 0..7 is the cell's training sequence code (what BCCH_demod finds, minus one); ov 2, 4 or 8.  Returns
    None when pos_info is all -1, otherwise a dict: `status` (0, or 15 = no block passes the Fire code), `num_blocks`, `num_ok`,
    `first_ok` (1-based, -1 without one), per block `ok`, `pos`, `corrected`, `ts_err`, `steal`, `mean_slope`, `amp` (NaN for a
    block that was not evaluated), `octets` (num_blocks, 23) uint8 -- zeros unless ok --, `si`: si_fields of the first ok block
    (valid 0 without one), and with want_soft `soft` (num_blocks, 456); `row` is the (SI_COLS,) table row bcch_decode_batch holds
    for this stream."""
    ctx = ctx or default_context()
    buf, n = _r_in(s)
    pi, rows, pic = _pos_info_in(pos_info)
    row = np.full(SI_COLS, np.nan)
    octets = np.zeros((MAX_HITS, BLOCK_OCTETS), dtype=np.uint8)
    soft = np.empty((MAX_HITS, BLOCK_CODED)) if want_soft else None
    info = _SiInfo()
    rc = ctx.check(ctx.lib.gsmcal_BCCH_decode(ctx.h, _dp(buf) if buf is not None else None, n, _dp(pic), rows, rows, int(tsc),
                                              int(oversampling_ratio), octets.ctypes.data_as(_lib.c_u8_p), _dp(row),
                                              _dp(soft) if want_soft else None, C.c_void_p(C.addressof(info))), "BCCH_decode")
    _say(ctx)
    if rc == _lib.S_POST_NO_POS:
        return None
    t = si_rows(row)
    k = min(int(t["num_blocks"][0]), MAX_HITS) if rc >= 0 else 0
    out = {"status": rc, "num_blocks": int(t["num_blocks"][0]), "num_ok": int(t["num_ok"][0]), "first_ok": int(t["first_ok"][0]),
           "octets": octets[:k].copy(), "si": _si_dict(info), "row": row}
    for name in SI_BLOCK_FIELDS:
        out[name] = t[name][0, :k].copy()
    if want_soft:
        out["soft"] = soft[:k].copy()
    return out


def total_ppm_calculation(ppm_in):
    lib = _lib.load()
    p = np.ascontiguousarray(np.atleast_1d(np.asarray(ppm_in, dtype=np.float64)))
    out = C.c_double()
    rc = lib.gsmcal_total_ppm_calculation(_dp(p), len(p), C.byref(out))
    if rc < 0:
        raise GsmcalError(f"total_ppm_calculation failed with {rc}")
    if rc == 12 and _VERBOSE[0]:
        print("total PPM calculation: No valid PPM input!")          # total_ppm_calculation.m:8
    return out.value


# ------------------------------------------------------------------------------------------------
# batched hot path
# ------------------------------------------------------------------------------------------------
TABLE_FIELDS = ("sampling_ppm_fcch", "sampling_ppm_sch", "carrier_ppm_fcch", "carrier_ppm_post",
                "total_sampling_ppm", "total_carrier_ppm", "n_fcch", "n_pos_rows", "first_fcch_pos", "status")


def frontend_batch(raw, coef, decim, ctx=None):
    """raw: (D, 2N) uint8 -> (D, ceil(N/decim)) complex: raw2iq + filter + r(1:decim:end)."""
    ctx = ctx or default_context()
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    d, two_n = raw.shape
    n = two_n // 2
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    out = np.empty((d, (n + decim - 1) // decim), dtype=np.complex128)
    ctx.check(ctx.lib.gsmcal_frontend_batch(ctx.h, raw.ctypes.data_as(_lib.c_u8_p), d, n, _dp(coef), len(coef),
                                            int(decim), _dp(out)), "frontend_batch")
    return out


def frontend_batch_dev(d_raw, d, n, coef, decim, d_out, ctx=None):
    """Device-pointer form of frontend_batch: only enqueues on the context's stream (ctx.sync() before reading).
    d_raw: [d][2n] bytes; d_out: [d][ceil(n/decim)] complex."""
    ctx = ctx or default_context()
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    ctx.check(ctx.lib.gsmcal_frontend_batch_dev(ctx.h, C.c_void_p(d_raw), int(d), int(n), _dp(coef), len(coef), int(decim),
                                                C.c_void_p(d_out)), "frontend_batch_dev")


def band_power_batch(raw, coef, decim, ctx=None):
    """raw: (D, 2N) uint8 -> (D,) linear band power mean(abs(filter(coef,1,raw2iq(s))(1:decim:end)).^2)
    (multi_rtl_sdr_split_scanner.m:154-156; coef = [1], decim = 1: scan_band_power_spectrum.m:80-84)."""
    ctx = ctx or default_context()
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    if raw.ndim != 2 or raw.shape[1] % 2:
        raise ValueError("raw must be (D, 2N) bytes")
    d, two_n = raw.shape
    coef = np.ascontiguousarray(np.atleast_1d(np.asarray(coef, dtype=np.float64)).ravel())
    out = np.empty(d)
    ctx.check(ctx.lib.gsmcal_band_power_batch(ctx.h, raw.ctypes.data_as(_lib.c_u8_p), d, two_n // 2, _dp(coef), len(coef),
                                              int(decim), _dp(out)), "band_power_batch")
    return out


def band_power_batch_dev(d_raw, d, n, coef, decim, d_power, ctx=None):
    """Device-pointer form of band_power_batch: only enqueues on the context's stream (ctx.sync() before reading).
    d_raw: [d][2n] bytes; d_power: [d] doubles in device or pinned host memory."""
    ctx = ctx or default_context()
    coef = np.ascontiguousarray(np.atleast_1d(np.asarray(coef, dtype=np.float64)).ravel())
    ctx.check(ctx.lib.gsmcal_band_power_batch_dev(ctx.h, C.c_void_p(d_raw), int(d), int(n), _dp(coef), len(coef), int(decim),
                                                  C.c_void_p(d_power)), "band_power_batch_dev")


def _subband_args(coef, phase_rotate, d):
    coef = np.ascontiguousarray(np.atleast_1d(np.asarray(coef, dtype=np.float64)).ravel())
    w = np.ascontiguousarray(np.atleast_2d(np.asarray(phase_rotate, dtype=np.float64)))
    if w.ndim != 2 or w.shape[0] != d:
        raise ValueError("phase_rotate must be (D, J): one row of sub-band phases per capture")
    return coef, w


def subband_power_batch(raw, coef, phase_rotate, decim=1, ctx=None):
    """raw: (D, 2N) uint8, phase_rotate: (D, J) radians per sample (NaN = unused slot) -> (D, J) linear powers
    mean(abs(filter(coef,1, raw2iq(s).*exp(1i*(1:N)'*phase_rotate[c][j]))(1:decim:end)).^2)
    (multi_rtl_sdr_diversity_scanner_another_bak.m:194-203; decim = 1 is the script).  NaN slots return NaN."""
    ctx = ctx or default_context()
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    if raw.ndim != 2 or raw.shape[1] % 2:
        raise ValueError("raw must be (D, 2N) bytes")
    d, two_n = raw.shape
    coef, w = _subband_args(coef, phase_rotate, d)
    out = np.empty(w.shape)
    ctx.check(ctx.lib.gsmcal_subband_power_batch(ctx.h, raw.ctypes.data_as(_lib.c_u8_p), d, two_n // 2, _dp(coef), len(coef),
                                                 int(decim), _dp(w), w.shape[1], _dp(out)), "subband_power_batch")
    return out


def subband_power_batch_dev(d_raw, d, n, coef, phase_rotate, d_power, decim=1, ctx=None):
    """Device-pointer form of subband_power_batch: only enqueues on the context's stream (ctx.sync() before reading).
    d_raw: [d][2n] bytes; phase_rotate: (d, J) on the host; d_power: [d][J] doubles in device or pinned host memory."""
    ctx = ctx or default_context()
    coef, w = _subband_args(coef, phase_rotate, int(d))
    ctx.check(ctx.lib.gsmcal_subband_power_batch_dev(ctx.h, C.c_void_p(d_raw), int(d), int(n), _dp(coef), len(coef), int(decim),
                                                     _dp(w), w.shape[1], C.c_void_p(d_power)), "subband_power_batch_dev")


CW_FIELDS = ("phase_rotate", "count", "max_abs", "max_n", "status")   # columns 0..4 of a CW-check row; then the (n, r_n) pairs


def cw_rows(table):
    """(D, CW_COLS) summary of cw_check_batch[_dev] -> one dict per capture: the CW_FIELDS (count, max_n and status as ints,
    max_n None where it is NaN) and "events", the listed (1-based n, r_n) pairs of the first exceeds."""
    rows = []
    for t in np.asarray(table, dtype=np.float64).reshape(-1, CW_COLS):
        ev = t[5:].reshape(CW_MAX_EVENTS, 2)
        ev = ev[~np.isnan(ev[:, 0])]
        rows.append({"phase_rotate": float(t[0]), "count": int(t[1]), "max_abs": float(t[2]),
                     "max_n": None if np.isnan(t[3]) else int(t[3]), "status": int(t[4]),
                     "events": [(int(n), float(v)) for n, v in ev]})
    return rows


def CW_check(s, ctx=None):
    """r = CW_check(s) -- CW_check.m:6-8: angle(s(2:end)./s(1:end-1)) minus the angle of the mean ratio, not wrapped.  s: complex
    (N,), N >= 2 -> (N-1,) doubles.  A sample among s(1..N-1) that is exactly 0 gives NaN everywhere (include/gsmcal.h)."""
    ctx = ctx or default_context()
    buf, n, _ = _cplx_in(np.asarray(s).ravel())
    r = np.empty(max(n - 1, 0))
    ctx.check(ctx.lib.gsmcal_CW_check(ctx.h, _dp(buf), n, _dp(r), None), "CW_check")
    return r


def cw_check_batch(raw, thr, want_r=False, ctx=None):
    """raw: (D, 2N) uint8 -> the (D, CW_COLS) summary of the CW sample-loss check (cw_rows names its columns): phase_rotate, the
    count of |r_n| > thr, max |r_n| and where, a status, the first CW_MAX_EVENTS exceeds.  want_r: returns (summary, r) with r
    (D, N-1), the residuals CW_check(raw2iq(.)) of every capture."""
    ctx = ctx or default_context()
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    if raw.ndim != 2 or raw.shape[1] % 2:
        raise ValueError("raw must be (D, 2N) bytes")
    d, two_n = raw.shape
    n = two_n // 2
    out = np.empty((d, CW_COLS))
    r = np.empty((d, max(n - 1, 0))) if want_r else None
    ctx.check(ctx.lib.gsmcal_cw_check_batch(ctx.h, raw.ctypes.data_as(_lib.c_u8_p), d, n, float(thr), _dp(out),
                                            _dp(r) if want_r else None, max(n - 1, 0)), "cw_check_batch")
    return (out, r) if want_r else out


def cw_check_batch_dev(d_raw, d, n, thr, d_summary, d_r=None, r_stride=0, ctx=None):
    """Device-pointer form of cw_check_batch: only enqueues on the context's stream (ctx.sync() before reading).  d_raw: [d][2n]
    bytes; d_summary: [d][CW_COLS] doubles; d_r: None (summary only) or d rows of r_stride >= n-1 doubles (n-1 written per row);
    device or pinned host memory."""
    ctx = ctx or default_context()
    ctx.check(ctx.lib.gsmcal_cw_check_batch_dev(ctx.h, C.c_void_p(d_raw), int(d), int(n), float(thr), C.c_void_p(d_summary),
                                                C.c_void_p(d_r) if d_r else None, int(r_stride)), "cw_check_batch_dev")


# columns of a row of iq_imbalance_batch[_dev] / IQ_imbalance, in order (GSMCAL_Q_*)
IQ_FIELDS = ("n", "S_I", "S_Q", "S_II", "S_QQ", "S_IQ", "min_I", "max_I", "min_Q", "max_Q", "clip_I", "clip_Q", "dc_I", "dc_Q",
             "var_I", "var_Q", "gain", "sin_phase", "phase_deg", "irr_db", "level_dbfs", "status")
_IQ_INT_FIELDS = ("n", "clip_I", "clip_Q", "status")


def iq_rows(table):
    """(D, IQ_COLS) table of iq_imbalance_batch[_dev] / one row of IQ_imbalance -> one dict per capture keyed by IQ_FIELDS: n and
    status as ints, the clip counts as ints or None where they are NaN (the complex form), everything else as floats."""
    rows = []
    for t in np.asarray(table, dtype=np.float64).reshape(-1, IQ_COLS):
        row = {k: float(v) for k, v in zip(IQ_FIELDS, t)}
        for k in _IQ_INT_FIELDS:
            row[k] = None if np.isnan(row[k]) else int(row[k])
        rows.append(row)
    return rows


def iq_imbalance_batch(raw, ctx=None):
    """raw: (D, 2N) uint8 -> the (D, IQ_COLS) table of the I/Q imbalance and clipping check (IQ_FIELDS / iq_rows name its columns):
    the exact byte sums, min, max and clip count per rail, DC, variance, gain ratio, quadrature skew, image rejection, level."""
    ctx = ctx or default_context()
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    if raw.ndim != 2 or raw.shape[1] % 2:
        raise ValueError("raw must be (D, 2N) bytes")
    d, two_n = raw.shape
    out = np.empty((d, IQ_COLS))
    ctx.check(ctx.lib.gsmcal_iq_imbalance_batch(ctx.h, raw.ctypes.data_as(_lib.c_u8_p), d, two_n // 2, _dp(out)), "iq_imbalance_batch")
    return out


def iq_imbalance_batch_dev(d_raw, d, n, d_table, ctx=None):
    """Device-pointer form of iq_imbalance_batch: only enqueues on the context's stream (ctx.sync() before reading).  d_raw: [d][2n]
    bytes, 2-byte aligned; d_table: [d][IQ_COLS] doubles in device or pinned host memory."""
    ctx = ctx or default_context()
    ctx.check(ctx.lib.gsmcal_iq_imbalance_batch_dev(ctx.h, C.c_void_p(d_raw), int(d), int(n), C.c_void_p(d_table)), "iq_imbalance_batch_dev")


def IQ_imbalance(s, ctx=None):
    """The I/Q check of one complex stream s (N,) (raw2iq's output, r_correct) -> one (IQ_COLS,) row, the clip columns NaN."""
    ctx = ctx or default_context()
    buf, n, _ = _cplx_in(np.asarray(s).ravel())
    row = np.empty(IQ_COLS)
    ctx.check(ctx.lib.gsmcal_IQ_imbalance(ctx.h, _dp(buf.view(np.float64)), n, _dp(row)), "IQ_imbalance")
    _say(ctx)
    return row


def iq_correct(s, gain, sin_phase, ctx=None):
    """Removes a measured imbalance: s complex (N,) or (N, D) (one stream per column, as the per-function entry points take them),
    gain and sin_phase scalars or (D,) from the streams' rows -> the same shape with Q replaced by (Q/g - I*s)/sqrt(1 - s*s)."""
    ctx = ctx or default_context()
    s = np.asarray(s)
    buf, n, d = _cplx_in(s)
    g = np.ascontiguousarray(np.broadcast_to(np.asarray(gain, dtype=np.float64).ravel(), (d,)))
    sp = np.ascontiguousarray(np.broadcast_to(np.asarray(sin_phase, dtype=np.float64).ravel(), (d,)))
    out = np.empty_like(buf)
    ctx.check(ctx.lib.gsmcal_iq_correct(ctx.h, _dp(buf.view(np.float64)), n, d, _dp(g), _dp(sp), _dp(out.view(np.float64))), "iq_correct")
    return out[0] if s.ndim == 1 else np.ascontiguousarray(out.T)


def _opt(p):
    """an optional device pointer"""
    return C.c_void_p(p) if p else None


def _post_batch_in(r_correct, r_len, pos_info_raw):
    """What calibrate_batch(..., want_r=True) returns, as the *_batch wrappers of the demod family pass it on -> r (D, N), D, N,
    r_len (D,) int64, pos_info (D, 2, MAX_POS_ROWS)"""
    r = np.ascontiguousarray(np.atleast_2d(np.asarray(r_correct, dtype=np.complex128)))
    d, stride = r.shape
    rl = np.ascontiguousarray(np.asarray(r_len, dtype=np.int64).ravel())
    pi = np.ascontiguousarray(np.asarray(pos_info_raw, dtype=np.float64).reshape(d, 2, MAX_POS_ROWS))
    if len(rl) != d:
        raise ValueError("r_len must have one entry per stream")
    return r, d, stride, rl, pi


def _table_rows(table, cols, head_fields, block_fields, width):
    """(D, cols) table -> dict of its columns: the head fields one column each, then `width` columns per block field"""
    t = np.asarray(table).reshape(-1, cols)
    out = {k: t[:, i] for i, k in enumerate(head_fields)}
    n = len(head_fields)
    for j, name in enumerate(block_fields):
        out[name] = t[:, n + j * width: n + (j + 1) * width]
    return out


DEMOD_FIELDS = ("num_fcch", "mean_freq", "carrier_ppm", "status")      # columns 0..3 of a demod row; then freq | snr | max_idx


def demod_rows(table):
    """(D, DEMOD_COLS) table of fcch_demod_batch[_dev] -> dict of its columns (freq, snr, max_idx: (D, MAX_HITS), NaN unused)."""
    return _table_rows(table, DEMOD_COLS, DEMOD_FIELDS, ("freq", "snr", "max_idx"), MAX_HITS)


def fcch_demod_batch(r_correct, r_len, pos_info_raw, oversampling_ratio, carrier_freq, ctx=None):
    """FCCH_demod.m:5-66 for D streams, on what calibrate_batch(..., want_r=True) returns: r_correct (D, N) complex, r_len (D,)
    (-1 where the reference returns r = -1), pos_info_raw (D, 2, MAX_POS_ROWS).  Returns the (D, DEMOD_COLS) table (demod_rows
    names its columns); per-row outcomes are in its status column."""
    ctx = ctx or default_context()
    r, d, stride, rl, pi = _post_batch_in(r_correct, r_len, pos_info_raw)
    cf = np.ascontiguousarray(np.broadcast_to(np.asarray(carrier_freq, dtype=np.float64), (d,)))
    out = np.empty((d, DEMOD_COLS))
    ctx.check(ctx.lib.gsmcal_fcch_demod_batch(ctx.h, _dp(r), stride, rl.ctypes.data_as(_lib.c_long_p), _dp(pi), d,
                                              int(oversampling_ratio), _dp(cf), _dp(out)), "fcch_demod_batch")
    return out


def fcch_demod_batch_dev(d_r, stride, d_r_len, d_pos_info, d, oversampling_ratio, carrier_freq, d_out, ctx=None):
    """Device-pointer form of fcch_demod_batch: only enqueues on the context's stream, e.g. directly behind calibrate_batch_dev
    on its d_r_correct / d_r_len / d_pos_info (ctx.sync() before reading).  d_out: [d][DEMOD_COLS] doubles, device or pinned."""
    ctx = ctx or default_context()
    cf = np.ascontiguousarray(np.broadcast_to(np.asarray(carrier_freq, dtype=np.float64), (int(d),)))
    ctx.check(ctx.lib.gsmcal_fcch_demod_batch_dev(ctx.h, C.c_void_p(d_r), int(stride), C.c_void_p(d_r_len), C.c_void_p(d_pos_info),
                                                  int(d), int(oversampling_ratio), _dp(cf), C.c_void_p(d_out)),
              "fcch_demod_batch_dev")


BCCH_FIELDS = ("num_bcch", "tsc_idx", "mean_fo", "carrier_ppm", "status", "num_agree")   # columns 0..5 of a BCCH_demod row


def bcch_rows(table):
    """(D, BCCH_COLS) table of bcch_demod_batch[_dev] -> dict of its columns (max_idx, peak, runner_up, phase: (D, MAX_BCCH), NaN
    unused; max_idx is the 1-based winning template per burst)."""
    return _table_rows(table, BCCH_COLS, BCCH_FIELDS, ("max_idx", "peak", "runner_up", "phase"), MAX_BCCH)


def bcch_demod_batch(r_correct, r_len, pos_info_raw, oversampling_ratio, normal_training_sequence, carrier_freq, ctx=None,
                     want_corr=False, want_r=False):
    """BCCH_demod.m for D streams, on what calibrate_batch(..., want_r=True) returns (as fcch_demod_batch) plus the (26*ov, 8)
    templates.  Returns the (D, BCCH_COLS) table (bcch_rows names its columns; per-row outcomes are in its status column) -- or,
    with want_corr / want_r, a dict: "table", "corr" (D, MAX_BCCH, 8) complex, "r" (D, N) complex and "r_len" (D,), -1 where the
    reference leaves r = -1 (those rows of "r" are zeros)."""
    ctx = ctx or default_context()
    r, d, stride, rl, pi = _post_batch_in(r_correct, r_len, pos_info_raw)
    ts, len_ts = _templates_in(normal_training_sequence, oversampling_ratio)
    cf = np.ascontiguousarray(np.broadcast_to(np.asarray(carrier_freq, dtype=np.float64), (d,)))
    out = np.empty((d, BCCH_COLS))
    corr = np.empty((d, MAX_BCCH, 8), dtype=np.complex128) if want_corr else None
    ro = np.empty((d, stride), dtype=np.complex128) if want_r else None
    rlo = np.empty(d, dtype=np.int64) if want_r else None
    ctx.check(ctx.lib.gsmcal_bcch_demod_batch(ctx.h, _dp(r), stride, rl.ctypes.data_as(_lib.c_long_p), _dp(pi), d,
                                              int(oversampling_ratio), _dp(ts), len_ts, _dp(cf), _dp(out),
                                              _dp(corr) if want_corr else None, _dp(ro) if want_r else None,
                                              rlo.ctypes.data_as(_lib.c_long_p) if want_r else None), "bcch_demod_batch")
    if not (want_corr or want_r):
        return out
    return {"table": out, "corr": corr, "r": ro, "r_len": rlo}


def bcch_demod_batch_dev(d_r, stride, d_r_len, d_pos_info, d, oversampling_ratio, normal_training_sequence, carrier_freq, d_out,
                         d_corr=None, d_r_out=None, d_r_len_out=None, ctx=None):
    """Device-pointer form of bcch_demod_batch: only enqueues on the context's stream, e.g. directly behind calibrate_batch_dev on
    its d_r_correct / d_r_len / d_pos_info (ctx.sync() before reading).  d_out: [d][BCCH_COLS] doubles; optional d_corr:
    [d][MAX_BCCH][8] complex; d_r_out [d][stride] complex with d_r_len_out [d] int64 (both or neither; d_r_out must not overlap
    d_r).  Device or pinned host memory."""
    ctx = ctx or default_context()
    ts, len_ts = _templates_in(normal_training_sequence, oversampling_ratio)
    cf = np.ascontiguousarray(np.broadcast_to(np.asarray(carrier_freq, dtype=np.float64), (int(d),)))
    ctx.check(ctx.lib.gsmcal_bcch_demod_batch_dev(ctx.h, C.c_void_p(d_r), int(stride), C.c_void_p(d_r_len), C.c_void_p(d_pos_info),
                                                  int(d), int(oversampling_ratio), _dp(ts), len_ts, _dp(cf), C.c_void_p(d_out),
                                                  _opt(d_corr), _opt(d_r_out), _opt(d_r_len_out)), "bcch_demod_batch_dev")


SCH_FIELDS = ("num_sch", "num_ok", "num_consistent", "bsic", "fn_anchor", "pos_anchor", "status", "mean_slope")   # columns 0..7


def sch_rows(table):
    """(D, SCH_COLS) table of sch_decode_batch[_dev] -> dict of its columns (ok, bsic_b, fn, ts_err, corrected, slope, amp:
    (D, MAX_HITS), NaN for unused entries and for bursts that were not evaluated)."""
    return _table_rows(table, SCH_COLS, SCH_FIELDS, ("ok", "bsic_b", "fn", "ts_err", "corrected", "slope", "amp"), MAX_HITS)


def sch_alignment(rows, oversampling_ratio, ref=0):
    """Per stream of an SCH_decode table (or of sch_rows' dict), the sample offset of its frame clock against stream `ref` at a
    common frame number: pos_anchor[d] - pos_anchor[ref] - wrap(fn_anchor[d] - fn_anchor[ref]) * 1250 * ov, the frame difference
    wrapped into +-half a hyperframe.  NaN for a stream whose status is not 0 (for all of them when `ref`'s is not)."""
    t = rows if isinstance(rows, dict) else sch_rows(rows)
    good = t["status"] == 0
    out = np.full(len(good), np.nan)
    if not good[ref]:
        return out
    half = _lib.HYPERFRAME // 2
    dfn = (t["fn_anchor"][good] - t["fn_anchor"][ref] + half) % _lib.HYPERFRAME - half
    out[good] = t["pos_anchor"][good] - t["pos_anchor"][ref] - dfn * 1250.0 * oversampling_ratio
    return out


def sch_decode_batch(r_correct, r_len, pos_info_raw, oversampling_ratio, sch_training_sequence, ctx=None, want_soft=False,
                     want_u=False):
    """SCH_decode for D streams, on what calibrate_batch(..., want_r=True) returns (as bcch_demod_batch) plus the SCH template
    (64*ov samples; only its length is looked at).  Returns the (D, SCH_COLS) table (sch_rows names its columns; per-row outcomes
    are in its status column) -- or, with want_soft / want_u, a dict: "table", "soft" (D, MAX_HITS, 148), "u" (D, MAX_HITS, 39)
    uint8 (255 where no burst was evaluated)."""
    ctx = ctx or default_context()
    r, d, stride, rl, pi = _post_batch_in(r_correct, r_len, pos_info_raw)
    ts, len_ts = _sch_template_in(sch_training_sequence)
    out = np.empty((d, SCH_COLS))
    soft = np.empty((d, MAX_HITS, 148)) if want_soft else None
    u = np.empty((d, MAX_HITS, 39), dtype=np.uint8) if want_u else None
    ctx.check(ctx.lib.gsmcal_sch_decode_batch(ctx.h, _dp(r), stride, rl.ctypes.data_as(_lib.c_long_p), _dp(pi), d,
                                              int(oversampling_ratio), _dp(ts), len_ts, _dp(out), _dp(soft) if want_soft else None,
                                              u.ctypes.data_as(_lib.c_u8_p) if want_u else None), "sch_decode_batch")
    if not (want_soft or want_u):
        return out
    return {"table": out, "soft": soft, "u": u}


def sch_decode_batch_dev(d_r, stride, d_r_len, d_pos_info, d, oversampling_ratio, sch_training_sequence, d_out, d_soft=None,
                         d_u=None, ctx=None):
    """Device-pointer form of sch_decode_batch: only enqueues on the context's stream, e.g. directly behind calibrate_batch_dev on
    its d_r_correct / d_r_len / d_pos_info (ctx.sync() before reading).  d_out: [d][SCH_COLS] doubles; optional d_soft:
    [d][MAX_HITS][148] doubles, d_u: [d][MAX_HITS][39] bytes.  Device or pinned host memory."""
    ctx = ctx or default_context()
    ts, len_ts = _sch_template_in(sch_training_sequence)
    ctx.check(ctx.lib.gsmcal_sch_decode_batch_dev(ctx.h, C.c_void_p(d_r), int(stride), C.c_void_p(d_r_len), C.c_void_p(d_pos_info),
                                                  int(d), int(oversampling_ratio), _dp(ts), len_ts, C.c_void_p(d_out), _opt(d_soft),
                                                  _opt(d_u)), "sch_decode_batch_dev")


SI_FIELDS = ("num_blocks", "num_ok", "status", "first_ok")          # columns 0..3
SI_BLOCK_FIELDS = ("ok", "pos", "corrected", "ts_err", "steal", "mean_slope", "amp")


def si_rows(table):
    """(D, SI_COLS) table of bcch_decode_batch[_dev] -> dict of its columns (ok, pos, corrected, ts_err, steal, mean_slope, amp:
    (D, MAX_HITS), NaN for unused entries and for blocks that were not evaluated)."""
    return _table_rows(table, SI_COLS, SI_FIELDS, SI_BLOCK_FIELDS, MAX_HITS)


def _tsc_in(tsc, d):
    t = np.asarray(tsc, dtype=np.int32).ravel()
    t = np.ascontiguousarray(np.broadcast_to(t, (d,)) if t.size == 1 else t)
    if len(t) != d:
        raise ValueError("tsc must be one code or one per stream")
    return t


def bcch_decode_batch(r_correct, r_len, pos_info_raw, oversampling_ratio, tsc, ctx=None, want_soft=False):
    """BCCH_decode for D streams, on what calibrate_batch(..., want_r=True) returns (as sch_decode_batch) plus the training
    sequence code: one int for all streams or one per stream.  Returns a dict: "table" (D, SI_COLS) (si_rows names its columns;
    per-row outcomes are in its status column), "octets" (D, MAX_HITS, 23) uint8, zeros unless the block is ok, and with want_soft
    "soft" (D, MAX_HITS, 456)."""
    ctx = ctx or default_context()
    r, d, stride, rl, pi = _post_batch_in(r_correct, r_len, pos_info_raw)
    codes = _tsc_in(tsc, d)
    out = np.empty((d, SI_COLS))
    octets = np.empty((d, MAX_HITS, BLOCK_OCTETS), dtype=np.uint8)
    soft = np.empty((d, MAX_HITS, BLOCK_CODED)) if want_soft else None
    ctx.check(ctx.lib.gsmcal_bcch_decode_batch(ctx.h, _dp(r), stride, rl.ctypes.data_as(_lib.c_long_p), _dp(pi), d,
                                               int(oversampling_ratio), codes.ctypes.data_as(_lib.c_int_p), _dp(out),
                                               octets.ctypes.data_as(_lib.c_u8_p), _dp(soft) if want_soft else None),
              "bcch_decode_batch")
    res = {"table": out, "octets": octets}
    if want_soft:
        res["soft"] = soft
    return res


def bcch_decode_batch_dev(d_r, stride, d_r_len, d_pos_info, d, oversampling_ratio, tsc, d_out, d_octets, d_soft=None, ctx=None):
    """Device-pointer form of bcch_decode_batch: only enqueues on the context's stream, e.g. directly behind calibrate_batch_dev on
    its d_r_correct / d_r_len / d_pos_info (ctx.sync() before reading).  tsc: one int or one per stream (host).  d_out:
    [d][SI_COLS] doubles; d_octets: [d][MAX_HITS][23] bytes; optional d_soft: [d][MAX_HITS][456] doubles.  Device or pinned host
    memory."""
    ctx = ctx or default_context()
    codes = _tsc_in(tsc, int(d))
    ctx.check(ctx.lib.gsmcal_bcch_decode_batch_dev(ctx.h, C.c_void_p(d_r), int(stride), C.c_void_p(d_r_len), C.c_void_p(d_pos_info),
                                                   int(d), int(oversampling_ratio), codes.ctypes.data_as(_lib.c_int_p),
                                                   C.c_void_p(d_out), C.c_void_p(d_octets), _opt(d_soft)),
              "bcch_decode_batch_dev")


PAIR_FIELDS = ("status", "num_bursts", "num_eval", "num_used", "num_adjacent", "lag0", "delay0", "rel_sampling_ppm", "delay_rms",
               "rel_carrier_hz", "burst_carrier_hz", "phase0", "phase_rms", "mean_coherence", "min_coherence_seen", "max_lag")   # columns 0..15
PAIR_BURST_FIELDS = ("pos", "delay", "phase", "freq", "coherence", "edge")


def pair_rows(table):
    """(P, PAIR_COLS) table of pair_coherence_batch[_dev] -> dict of its columns (pos, delay, phase, freq, coherence, edge:
    (P, MAX_PAIR_BURSTS), NaN for unused entries and for bursts that were not evaluated)."""
    return _table_rows(table, PAIR_COLS, PAIR_FIELDS, PAIR_BURST_FIELDS, MAX_PAIR_BURSTS)


def pair_lag0(sch_table_or_rows, pairs, oversampling_ratio):
    """The expected offset of b's content against a's for every pair (a, b), from an SCH_decode table (or sch_rows' dict):
    round(alignment[b] - alignment[a]) of sch_alignment -> (P,) int32.  Raises ValueError where a stream of a pair has no
    alignment (its SCH bursts did not decode)."""
    al = sch_alignment(sch_table_or_rows, oversampling_ratio)
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    diff = al[pr[:, 1]] - al[pr[:, 0]]
    if np.isnan(diff).any():
        raise ValueError("pair_lag0: a stream of a pair has no SCH alignment")
    return (np.sign(diff) * np.floor(np.abs(diff) + 0.5)).astype(np.int32)


def _pairs_in(pairs, lag0, d):
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    lg = np.asarray(lag0, dtype=np.int32).ravel()
    lg = np.ascontiguousarray(np.broadcast_to(lg, (len(pr),)) if lg.size == 1 else lg)
    if len(pr) < 1 or len(lg) != len(pr):
        raise ValueError("pairs must be (P, 2) stream indices with one lag0 per pair")
    return pr, lg, len(pr)


def _max_lag_in(max_lag, oversampling_ratio):
    return 2 * int(oversampling_ratio) if max_lag is None else int(max_lag)


def pair_coherence(s_a, s_b, pos_info, oversampling_ratio, lag0=0, max_lag=None, min_coherence=0.5, ctx=None, want_corr=False):
    """pair_coherence(s_a, s_b, pos_info_a, ov, lag0) -- the project's own function (include/gsmcal.h): the
    delay of stream b against stream a to a fraction of a sample, their carrier phase and frequency difference, their coherence
    and the drift of the delay, measured on the SCH and BCCH bursts of a's pos_info.  lag0: the expected offset of b's content
    against a's (pair_lag0); max_lag M in 1..4*ov (default 2*ov); ov 2, 4 or 8.  Returns None when pos_info is all -1, otherwise a
    dict: the PAIR_FIELDS as scalars (`status` 0, or 16 = fewer than two used bursts), per burst `pos`, `delay`, `phase`, `freq`,
    `coherence`, `edge` (NaN for a burst that was not evaluated), with want_corr `corr` (num_bursts, 2M+1, 4) complex; `row` is the
    (PAIR_COLS,) table row pair_coherence_batch holds for this pair."""
    ctx = ctx or default_context()
    ba, na = _r_in(s_a)
    bb, nb = _r_in(s_b)
    pi, rows, pic = _pos_info_in(pos_info)
    m = _max_lag_in(max_lag, oversampling_ratio)
    row = np.full(PAIR_COLS, np.nan)
    corr = np.empty((MAX_PAIR_BURSTS, 2 * max(m, 0) + 1, 4), dtype=np.complex128) if want_corr else None
    rc = ctx.check(ctx.lib.gsmcal_pair_coherence(ctx.h, _dp(ba) if ba is not None else None, na, _dp(bb) if bb is not None else None, nb,
                                                 _dp(pic), rows, rows, int(oversampling_ratio), int(lag0), m, float(min_coherence),
                                                 _dp(row), _dp(corr) if want_corr else None), "pair_coherence")
    _say(ctx)
    if rc == _lib.S_POST_NO_POS:
        return None
    t = pair_rows(row)
    k = min(int(t["num_bursts"][0]), MAX_PAIR_BURSTS) if rc >= 0 else 0
    out = {name: (int(t[name][0]) if name in ("status", "num_bursts", "num_eval", "num_used", "num_adjacent", "lag0", "max_lag")
                  else float(t[name][0])) for name in PAIR_FIELDS}
    for name in PAIR_BURST_FIELDS:
        out[name] = t[name][0, :k].copy()
    out["row"] = row
    if want_corr:
        out["corr"] = corr[:k].copy()
    return out


def pair_coherence_batch(r_correct, r_len, pos_info_raw, oversampling_ratio, pairs, lag0, max_lag=None, min_coherence=0.5, ctx=None,
                         want_corr=False):
    """pair_coherence for P pairs of D streams, on what calibrate_batch(..., want_r=True) returns (as sch_decode_batch).  pairs:
    (P, 2) stream indices (a, b); the bursts of a pair are the rows of a's table.  lag0: one int or one per pair (pair_lag0).
    Returns the (P, PAIR_COLS) table (pair_rows names its columns; per-row outcomes are in its status column) -- or, with
    want_corr, a dict: "table", "corr" (P, MAX_PAIR_BURSTS, 2M+1, 4) complex, NaN where no burst was evaluated."""
    ctx = ctx or default_context()
    r, d, stride, rl, pi = _post_batch_in(r_correct, r_len, pos_info_raw)
    pr, lg, npairs = _pairs_in(pairs, lag0, d)
    m = _max_lag_in(max_lag, oversampling_ratio)
    out = np.empty((npairs, PAIR_COLS))
    corr = np.empty((npairs, MAX_PAIR_BURSTS, 2 * max(m, 0) + 1, 4), dtype=np.complex128) if want_corr else None
    ctx.check(ctx.lib.gsmcal_pair_coherence_batch(ctx.h, _dp(r), stride, rl.ctypes.data_as(_lib.c_long_p), _dp(pi), d,
                                                  int(oversampling_ratio), pr.ctypes.data_as(_lib.c_int_p),
                                                  lg.ctypes.data_as(_lib.c_int_p), npairs, m, float(min_coherence), _dp(out),
                                                  _dp(corr) if want_corr else None), "pair_coherence_batch")
    if not want_corr:
        return out
    return {"table": out, "corr": corr}


def pair_coherence_batch_dev(d_r, stride, d_r_len, d_pos_info, d, oversampling_ratio, pairs, lag0, d_out, max_lag=None,
                             min_coherence=0.5, d_corr=None, ctx=None):
    """Device-pointer form of pair_coherence_batch: only enqueues on the context's stream, e.g. directly behind calibrate_batch_dev on
    its d_r_correct / d_r_len / d_pos_info (ctx.sync() before reading).  pairs, lag0: host arrays.  d_out: [P][PAIR_COLS] doubles;
    optional d_corr: [P][MAX_PAIR_BURSTS][2M+1][4] complex.  Device or pinned host memory."""
    ctx = ctx or default_context()
    pr, lg, npairs = _pairs_in(pairs, lag0, int(d))
    ctx.check(ctx.lib.gsmcal_pair_coherence_batch_dev(ctx.h, C.c_void_p(d_r), int(stride), C.c_void_p(d_r_len), C.c_void_p(d_pos_info),
                                                      int(d), int(oversampling_ratio), pr.ctypes.data_as(_lib.c_int_p),
                                                      lg.ctypes.data_as(_lib.c_int_p), npairs, _max_lag_in(max_lag, oversampling_ratio),
                                                      float(min_coherence), C.c_void_p(d_out), _opt(d_corr)), "pair_coherence_batch_dev")


ALIGN_PARAM_FIELDS = ("delay", "slope_ppm", "carrier_hz", "phase", "anchor", "weight")        # one member's row of pair_align_batch
ALIGN_INFO_FIELDS = ("status", "first_valid", "end_valid", "num_valid")                     # one member's row of the info table
ALIGN_SUM_FIELDS = ("members_used", "combined_first", "combined_end", "weight_sum")          # ... and its last row, for the sum


def align_rows(info):
    """(G + 1, ALIGN_INFO_COLS) info table of pair_align_batch[_dev] -> dict: the ALIGN_INFO_FIELDS as (G,) columns of the members
    (status 0, 10 = the stream is empty, 17 = a parameter is not finite; [first_valid, end_valid) the output samples every tap of
    which lies inside the stream) and the ALIGN_SUM_FIELDS as scalars of the sum ([combined_first, combined_end): where every member
    with status 0 is valid)."""
    t = np.asarray(info, dtype=np.float64).reshape(-1, ALIGN_INFO_COLS)
    out = {k: t[:-1, i] for i, k in enumerate(ALIGN_INFO_FIELDS)}
    out.update({k: (float(t[-1, i]) if k == "weight_sum" else int(t[-1, i])) for i, k in enumerate(ALIGN_SUM_FIELDS)})
    return out


def pair_align_params(pair_table, oversampling_ratio, weights=None, min_coherence=0.5):
    """Rows of a pair_coherence table (pairs (a, b)) -> (P, ALIGN_PARAMS) parameter rows {delay, slope_ppm, carrier_hz, phase, anchor,
    weight} that put stream b of each pair on stream a's time base and take its carrier out (gsmcal_pair_align_params; pure host
    arithmetic, no context).  With L = 148 ov, s = 1e-6 rel_sampling_ppm and p0 = round(pos) - 1 of the first USED burst:
        anchor = p0 + (L-1)/2,  delay = delay0 + s (L-1)/2,  slope_ppm = rel_sampling_ppm,
        carrier_hz = rel_carrier_hz (1 + s),  phase = phase0.
    Why: pair_coherence fits delay(t) = delay0 + s t with t counted from the START of the first used burst, so output sample n of
    a's time base sits at n + delay0 + s (n - p0) in b -- which is (n + delay) + s (n - anchor) with the two values above.  Its
    phase0 is the phase of b against a at that burst's CENTRE, the sample p0 + (L-1)/2 of a: the anchor.  Its rel_carrier_hz is
    measured per sample of a as the burst is walked in b's index, and one output sample advances b's index by 1 + s: the carrier to
    take out per output sample is (1 + s) times as large.
    A burst is used when its pos is not NaN, its edge is 0 and its coherence >= min_coherence: the row does not carry the threshold
    pair_coherence was run with, so it is an argument here (default 0.5, pair_coherence's own default) -- pass the same value.
    weights: one per row (default 1 / (P + 1): equal gain for the P members and the reference stream, whose own row is
    {0, 0, 0, 0, 0, w}).  A row whose status is not 0 gives NaN parameters; pair_align_batch then skips that member."""
    lib = _lib.load()
    tab = np.ascontiguousarray(np.asarray(pair_table, dtype=np.float64).reshape(-1, PAIR_COLS))
    w = np.full(len(tab), 1.0 / (len(tab) + 1)) if weights is None else np.broadcast_to(np.asarray(weights, dtype=np.float64), (len(tab),))
    out = np.empty((len(tab), ALIGN_PARAMS))
    for i in range(len(tab)):
        rc = lib.gsmcal_pair_align_params(_dp(tab[i]), int(oversampling_ratio), float(min_coherence), float(w[i]), _dp(out[i]))
        if rc < 0:
            raise GsmcalError(f"pair_align_params failed with {rc}")
    return out


def _members_in(members, params):
    mb = np.ascontiguousarray(np.asarray(members, dtype=np.int32).ravel())
    pr = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1, ALIGN_PARAMS))
    if len(mb) != len(pr):
        raise ValueError("one parameter row per member")
    return mb, pr, len(mb)


def pair_align(s, oversampling_ratio, params_row, out_len=None, ctx=None):
    """pair_align(s, ov, params_row, out_len) -- the project's own function (include/gsmcal.h): stream s
    resampled at x(n) = (n + delay) + 1e-6 slope_ppm (n - anchor) by a 16-tap Blackman-windowed sinc and turned by
    exp(-j (phase + 2 pi carrier_hz (n - anchor) / fs)), n = 0 .. out_len-1 (default len(s)); samples a tap of which would fall
    outside s are exactly 0.  ov 2, 4 or 8; |slope_ppm| <= 1000.  Returns (out, info): out (out_len,) complex, info a dict of the
    ALIGN_INFO_FIELDS (status 0, 10 for an empty s, 17 for a parameter that is not finite)."""
    ctx = ctx or default_context()
    buf, n = _r_in(s)
    out_len = n if out_len is None else int(out_len)
    pr = np.ascontiguousarray(np.asarray(params_row, dtype=np.float64).ravel())
    if len(pr) != ALIGN_PARAMS:
        raise ValueError("params_row: delay, slope_ppm, carrier_hz, phase, anchor, weight")
    out = np.empty(max(out_len, 0), dtype=np.complex128)
    info = np.empty(ALIGN_INFO_COLS)
    ctx.check(ctx.lib.gsmcal_pair_align(ctx.h, _dp(buf) if buf is not None else None, n, int(oversampling_ratio), _dp(pr), out_len,
                                        _dp(out), _dp(info)), "pair_align")
    _say(ctx)
    return out, {k: int(info[i]) for i, k in enumerate(ALIGN_INFO_FIELDS)}


def pair_align_batch(r_correct, r_len, oversampling_ratio, members, params, out_len=None, ctx=None, want_aligned=True, want_combined=True):
    """pair_align for G members of D streams (r_correct, r_len as calibrate_batch(..., want_r=True) returns them) and their weighted
    sum.  members: (G,) stream indices; params: (G, ALIGN_PARAMS) rows (pair_align_params; the reference stream is {0, 0, 0, 0, 0, w});
    out_len defaults to the streams' row length.  Returns a dict: "aligned" (G, out_len) complex (with want_aligned), "combined"
    (out_len,) complex = sum_g weight_g aligned_g in list order over the members valid at each sample (with want_combined), "info"
    the (G + 1, ALIGN_INFO_COLS) table (align_rows names its columns; per-member outcomes are in its status column)."""
    ctx = ctx or default_context()
    r = np.ascontiguousarray(np.atleast_2d(np.asarray(r_correct, dtype=np.complex128)))
    d, stride = r.shape
    rl = np.ascontiguousarray(np.asarray(r_len, dtype=np.int64).ravel())
    if len(rl) != d:
        raise ValueError("r_len must have one entry per stream")
    mb, pr, g = _members_in(members, params)
    out_len = stride if out_len is None else int(out_len)
    al = np.empty((g, max(out_len, 0)), dtype=np.complex128) if want_aligned else None
    cb = np.empty(max(out_len, 0), dtype=np.complex128) if want_combined else None
    info = np.empty((g + 1, ALIGN_INFO_COLS))
    ctx.check(ctx.lib.gsmcal_pair_align_batch(ctx.h, _dp(r), stride, rl.ctypes.data_as(_lib.c_long_p), d, int(oversampling_ratio),
                                              mb.ctypes.data_as(_lib.c_int_p), _dp(pr), g, out_len, _dp(al) if want_aligned else None,
                                              _dp(cb) if want_combined else None, _dp(info)), "pair_align_batch")
    out = {"info": info}
    if want_aligned:
        out["aligned"] = al
    if want_combined:
        out["combined"] = cb
    return out


def pair_align_batch_dev(d_r, stride, d_r_len, d, oversampling_ratio, members, params, out_len, d_info, d_aligned=None, d_combined=None,
                         ctx=None):
    """Device-pointer form of pair_align_batch: only enqueues on the context's stream (ctx.sync() before reading).  members, params:
    host arrays.  d_info: [G + 1][ALIGN_INFO_COLS] doubles; d_aligned: [G][out_len] complex and d_combined: [out_len] complex, either
    may be left out, not both; neither may overlap d_r.  Device or pinned host memory."""
    ctx = ctx or default_context()
    mb, pr, g = _members_in(members, params)
    ctx.check(ctx.lib.gsmcal_pair_align_batch_dev(ctx.h, C.c_void_p(d_r), int(stride), C.c_void_p(d_r_len), int(d), int(oversampling_ratio),
                                                  mb.ctypes.data_as(_lib.c_int_p), _dp(pr), g, int(out_len), _opt(d_aligned), _opt(d_combined),
                                                  C.c_void_p(d_info)), "pair_align_batch_dev")


WEIGHTS_INFO_FIELDS = ("status", "lambda_1", "lambda_2", "sweeps")                          # info of combine_weights


def _rows_in(rows):
    rw = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).ravel())
    return rw, len(rw)


def _windows_in(windows):
    return np.ascontiguousarray(np.asarray(windows, dtype=np.int64).reshape(-1, 2))


def array_covariance(x, rows, windows, ctx=None):
    """The spatial covariance of streams on one time base (include/gsmcal.h).  x: (D, N) complex, e.g. the
    "aligned" rows of pair_align_batch; rows: (G,) indices into it, 1 .. 64 of them; windows: (W, 2) {start, len}, 1 .. 256 of them.
    Returns (W, G, G) complex: cov[w, i, j] = sum over the window of x_i conj(x_j), in fp64, not divided by len -- exactly Hermitian,
    the diagonal exactly real, the same bits for a window wherever it stands in whatever list."""
    ctx = ctx or default_context()
    xa = np.ascontiguousarray(np.atleast_2d(np.asarray(x, dtype=np.complex128)))
    d, stride = xa.shape
    rw, g = _rows_in(rows)
    wn = _windows_in(windows)
    cov = np.empty((len(wn), g, g), dtype=np.complex128)
    ctx.check(ctx.lib.gsmcal_array_covariance_batch(ctx.h, _dp(xa), stride, d, rw.ctypes.data_as(_lib.c_int_p), g,
                                                    wn.ctypes.data_as(_lib.c_long_p), len(wn), _dp(cov)), "array_covariance")
    return cov


def array_covariance_dev(d_x, stride, d, rows, windows, d_cov, ctx=None):
    """Device-pointer form of array_covariance: only enqueues on the context's stream (ctx.sync() before reading).  rows, windows: host
    arrays.  d_cov: [W][G][G] complex.  Device or pinned host memory."""
    ctx = ctx or default_context()
    rw, g = _rows_in(rows)
    wn = _windows_in(windows)
    ctx.check(ctx.lib.gsmcal_array_covariance_batch_dev(ctx.h, C.c_void_p(d_x), int(stride), int(d), rw.ctypes.data_as(_lib.c_int_p), g,
                                                        wn.ctypes.data_as(_lib.c_long_p), len(wn), C.c_void_p(d_cov)), "array_covariance_dev")


def combine_weights(cov_signal, cov_noise=None, ref=0):
    """The weights w of the beam w^H x (gsmcal_combine_weights; pure host arithmetic, no context).  cov_signal: (G, G) Hermitian, of
    which the upper triangle is read.  Without cov_noise: the eigenvector of its largest eigenvalue.  With cov_noise (a covariance
    of windows without the wanted signal): the dominant generalised eigenvector of Rs w = lambda Rn w, the weights of the largest
    SINR.  |w| = 1, w[ref] real and >= 0.  Returns (weights (G,) complex, info dict of the WEIGHTS_INFO_FIELDS): status 0, or 18
    (S_WEIGHTS_SINGULAR: a value that is not finite, cov_noise not positive definite, lambda_1 <= 0) with every weight NaN."""
    lib = _lib.load()
    rs = np.ascontiguousarray(np.asarray(cov_signal, dtype=np.complex128))
    if rs.ndim != 2 or rs.shape[0] != rs.shape[1]:
        raise ValueError("cov_signal must be (G, G)")
    g = rs.shape[0]
    rn = None
    if cov_noise is not None:
        rn = np.ascontiguousarray(np.asarray(cov_noise, dtype=np.complex128))
        if rn.shape != rs.shape:
            raise ValueError("cov_noise must have the shape of cov_signal")
    w = np.empty(max(g, 1), dtype=np.complex128)
    info = np.empty(_lib.WEIGHTS_INFO_COLS)
    rc = lib.gsmcal_combine_weights(_dp(rs), _dp(rn) if rn is not None else None, g, int(ref), _dp(w), _dp(info))
    if rc < 0:
        raise GsmcalError(f"combine_weights failed with {rc} ")
    out = {k: float(info[i]) for i, k in enumerate(WEIGHTS_INFO_FIELDS)}
    out["status"], out["sweeps"] = int(info[0]), int(info[3])
    return w[:g], out


def _weights_in(weights, g):
    w = np.ascontiguousarray(np.atleast_2d(np.asarray(weights, dtype=np.complex128)))
    if w.shape[1] != g:
        raise ValueError("one weight per row and beam: (B, G) or (G,)")
    return w, w.shape[0]


def array_combine(x, rows, weights, out_len=None, ctx=None):
    """The beams out[b, n] = sum_g conj(weights[b, g]) x[rows[g], n] (w^H x; include/gsmcal.h).  weights: (G,)
    for one beam -> (out_len,), or (B, G) for 1 .. 16 beams -> (B, out_len); out_len defaults to the row length.  x is read once for
    all beams, and a beam's row is the same bits alone or among others."""
    ctx = ctx or default_context()
    xa = np.ascontiguousarray(np.atleast_2d(np.asarray(x, dtype=np.complex128)))
    d, stride = xa.shape
    rw, g = _rows_in(rows)
    w, b = _weights_in(weights, g)
    out_len = stride if out_len is None else int(out_len)
    out = np.empty((b, max(out_len, 0)), dtype=np.complex128)
    ctx.check(ctx.lib.gsmcal_array_combine_batch(ctx.h, _dp(xa), stride, d, rw.ctypes.data_as(_lib.c_int_p), g, _dp(w), b, out_len, _dp(out)),
              "array_combine")
    return out[0] if np.ndim(weights) == 1 else out


def array_combine_dev(d_x, stride, d, rows, weights, out_len, d_out, ctx=None):
    """Device-pointer form of array_combine: only enqueues on the context's stream.  rows, weights ((B, G) or (G,)): host arrays.
    d_out: [B][out_len] complex; it must not overlap d_x."""
    ctx = ctx or default_context()
    rw, g = _rows_in(rows)
    w, b = _weights_in(weights, g)
    ctx.check(ctx.lib.gsmcal_array_combine_batch_dev(ctx.h, C.c_void_p(d_x), int(stride), int(d), rw.ctypes.data_as(_lib.c_int_p), g, _dp(w), b,
                                                     int(out_len), C.c_void_p(d_out)), "array_combine_dev")


def burst_windows(pos_info_raw_of_ref, oversampling_ratio, align_info, kinds=(1, 2)):
    """The windows {round(pos) - 1, 148 ov} of the reference stream's SCH (kind 1) and BCCH (kind 2) rows that lie wholly inside
    [combined_first, combined_end) of a pair_align info table: where every used member is valid, so a covariance over them sees
    every stream.  pos_info_raw_of_ref: the (2, MAX_POS_ROWS) table of the reference stream.  Returns (W, 2) int64 (W may be 0)."""
    pi = np.asarray(pos_info_raw_of_ref, dtype=np.float64).reshape(2, MAX_POS_ROWS)
    t = align_rows(align_info)
    first, end, L = t["combined_first"], t["combined_end"], 148 * int(oversampling_ratio)
    out = []
    for i in range(MAX_POS_ROWS):
        pos = pi[0, i]
        if pi[1, i] not in [float(k) for k in kinds] or not (pos == pos) or abs(pos) > 2.0 ** 52:
            continue
        p = int(np.floor(pos + 0.5)) - 1
        if first <= p and p + L <= end:
            out.append((p, L))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def coherent_combine(r_correct, r_len, pos_info_raw, oversampling_ratio, sch_table, ref=0, members=None, max_lag=None, min_coherence=0.5,
                     want_aligned=False, ctx=None, weights=None):
    """One stream out of several calibrated dongles on one cell: pair_lag0 -> pair_coherence_batch for the pairs (ref, m) ->
    pair_align_params -> pair_align_batch, on what calibrate_batch(..., want_r=True) and sch_decode_batch returned.  members: the
    streams to put on ref's time base (default: every other stream).  The sum has equal weights 1 / (1 + len(members)) and ref
    itself as its first member; a member whose pair row has a status other than 0 is skipped (info says so).  Returns a dict:
    "combined" (N,) complex, "info" (align_rows names its columns; row 0 is ref), "pair_table" (len(members), PAIR_COLS), "params"
    (1 + len(members), ALIGN_PARAMS), "members" (ref first), with want_aligned "aligned" (1 + len(members), N).  The combined stream
    has the shape the demod family takes: SCH_decode and the others read it with ref's pos_info.
    weights="max_ratio": the members are aligned as above, their covariance is summed over burst_windows (ref's SCH and BCCH bursts
    inside the interval where every used member is valid), combine_weights(ref=0) gives its dominant eigenvector and "combined" is
    array_combine with it over the members of status 0.  The dict then also holds "weights" (1 + len(members),) complex, NaN for a
    skipped member, and "cov" (used, used) complex."""
    ctx = ctx or default_context()
    r, d, stride, rl, pi = _post_batch_in(r_correct, r_len, pos_info_raw)
    ms = [m for m in range(d) if m != ref] if members is None else [int(m) for m in members]
    pairs = [(int(ref), m) for m in ms]
    lag0 = pair_lag0(sch_table, pairs, oversampling_ratio)
    table = pair_coherence_batch(r, rl, pi, oversampling_ratio, pairs, lag0, max_lag, min_coherence, ctx=ctx)
    w = 1.0 / (1 + len(ms))
    params = np.vstack([[0.0, 0.0, 0.0, 0.0, 0.0, w], pair_align_params(table, oversampling_ratio, w, min_coherence)])
    if weights is None:
        out = pair_align_batch(r, rl, oversampling_ratio, [int(ref)] + ms, params, ctx=ctx, want_aligned=want_aligned)
    elif weights == "max_ratio":
        out = pair_align_batch(r, rl, oversampling_ratio, [int(ref)] + ms, params, ctx=ctx, want_aligned=True, want_combined=False)
        used = np.flatnonzero(align_rows(out["info"])["status"] == 0)
        wins = burst_windows(pi[int(ref)], oversampling_ratio, out["info"])
        if len(wins) == 0 or len(used) == 0 or used[0] != 0:
            raise GsmcalError("coherent_combine: no burst of the reference stream lies inside the interval every member covers")
        cov = array_covariance(out["aligned"], used, wins, ctx=ctx).sum(axis=0)
        w, winfo = combine_weights(cov, ref=0)
        if winfo["status"] != 0:
            raise GsmcalError(f"coherent_combine: combine_weights ended with status {winfo['status']}")
        out["combined"] = array_combine(out["aligned"], used, w, ctx=ctx)
        out["weights"] = np.full(1 + len(ms), np.nan + 1j * np.nan)
        out["weights"][used] = w
        out["cov"] = cov
        if not want_aligned:
            del out["aligned"]
    else:
        raise ValueError('weights: None or "max_ratio"')
    out.update({"pair_table": table, "params": params, "members": np.array([int(ref)] + ms)})
    return out


APPLY_PARAM_FIELDS = ("delay", "slope_ppm", "carrier_hz", "phase", "anchor", "scale", "dc_i", "dc_q", "gain", "sin_phase")     # one capture's row of apply_calibration


def apply_rows(info):
    """(D, APPLY_INFO_COLS) info table of apply_calibration[_resident] -> dict of the ALIGN_INFO_FIELDS as (D,) columns: status 0,
    or 17 = a value of the capture's parameter row is not finite (its output row is all zero); [first_valid, end_valid) the output
    samples every tap of which lies inside the capture."""
    t = np.asarray(info, dtype=np.float64).reshape(-1, APPLY_INFO_COLS)
    return {k: t[:, i] for i, k in enumerate(ALIGN_INFO_FIELDS)}


def apply_params(table, tuned_freq, iq_table=None, delay=0.0, phase=0.0, scale=1.0):
    """Rows of a calibration table (calibrate_batch) -> (D, APPLY_PARAMS) parameter rows {delay, slope_ppm, carrier_hz, phase, anchor,
    scale, dc_i, dc_q, gain, sin_phase} that undo each dongle's sampling clock error and carrier error on a capture tuned to
    tuned_freq Hz (gsmcal_apply_params; pure host arithmetic, no context).  With e = 1e-6 total_sampling_ppm and f_off = 1e-6
    total_carrier_ppm tuned_freq:
        slope_ppm = total_sampling_ppm,  anchor = 0,  carrier_hz = f_off (1 + e);  delay, phase and scale as given.
    Why: the dongle samples at ideal time k / (1 + e) and its carrier error turns its sample k by 2 pi f_off k / fs, so output sample
    n of the nominal time base sits at dongle index n (1 + e) and the angle to take out there is 2 pi f_off n (1 + e) / fs.
    iq_table: the (D, IQ_COLS) table of iq_imbalance_batch ON THE CAPTURE TO CORRECT (DC and imbalance change with the tuning): DC,
    gain and sin_phase come from it (gain 1, sin_phase 0 where its status is not 0); without it DC = 127.5, 127.5 (raw2iq's) and no
    I/Q correction.  tuned_freq, delay, phase and scale: scalars or one value per dongle.  A row whose status is not 0, or whose
    totals are not finite, gives an all-NaN row; apply_calibration then skips that capture (status 17, zeros)."""
    lib = _lib.load()
    tab = np.ascontiguousarray(np.asarray(table, dtype=np.float64).reshape(-1, TABLE_COLS))
    d = len(tab)
    iq = None if iq_table is None else np.ascontiguousarray(np.asarray(iq_table, dtype=np.float64).reshape(-1, IQ_COLS))
    if iq is not None and len(iq) != d:
        raise ValueError("iq_table must have one row per row of table")
    per = [np.broadcast_to(np.asarray(v, dtype=np.float64).ravel(), (d,)) for v in (tuned_freq, delay, phase, scale)]
    out = np.empty((d, APPLY_PARAMS))
    for i in range(d):
        rc = lib.gsmcal_apply_params(_dp(tab[i]), float(per[0][i]), _dp(iq[i]) if iq is not None else None, float(per[1][i]),
                                     float(per[2][i]), float(per[3][i]), _dp(out[i]))
        if rc < 0:
            raise GsmcalError(f"apply_params failed with {rc}")
    return out


def _apply_params_in(params, d):
    pr = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1, APPLY_PARAMS))
    if len(pr) != d:
        raise ValueError("one parameter row per capture")
    return pr


def apply_calibration(raw, params, sample_rate, out_len=None, ctx=None):
    """The project's own function (include/gsmcal.h): raw (D, 2N) uint8 captures of calibrated dongles at any
    centre frequency and sample_rate -> (out, info): out (D, out_len) complex (default out_len = N), every capture with its DC and
    I/Q imbalance removed, resampled at x(n) = (n + delay) + 1e-6 slope_ppm (n - anchor) by pair_align's 16-tap interpolator, turned
    by exp(-j (phase + 2 pi carrier_hz (n - anchor) / sample_rate)) and scaled; samples a tap of which would fall outside the capture
    are exactly 0.  params: (D, APPLY_PARAMS) rows (apply_params).  info: apply_rows of the (D, APPLY_INFO_COLS) table.  The rows
    are streams on one nominal time base: array_covariance and array_combine take them as they are."""
    ctx = ctx or default_context()
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    if raw.ndim != 2 or raw.shape[1] % 2:
        raise ValueError("raw must be (D, 2N) bytes")
    d, two_n = raw.shape
    n = two_n // 2
    out_len = n if out_len is None else int(out_len)
    pr = _apply_params_in(params, d)
    out = np.empty((d, max(out_len, 0)), dtype=np.complex128)
    info = np.empty((d, APPLY_INFO_COLS))
    ctx.check(ctx.lib.gsmcal_apply_calibration_batch(ctx.h, raw.ctypes.data_as(_lib.c_u8_p), d, n, float(sample_rate), _dp(pr), out_len,
                                                     out_len, _dp(out.view(np.float64)), _dp(info)), "apply_calibration_batch")
    return out, apply_rows(info)


def apply_calibration_resident(d_raw, d, n, params, sample_rate, out_len, out_stride, d_out, d_info, ctx=None):
    """Device-pointer form of apply_calibration: only enqueues on the context's stream (ctx.sync() before reading), behind whatever
    wrote d_raw there.  d_raw: [d][2n] bytes, 2-byte aligned; params: host rows; d_out: [d][out_stride] complex, out_stride >=
    out_len, the tail of every row is not touched; d_info: [d][APPLY_INFO_COLS] doubles; the outputs in device or pinned host memory,
    not overlapping d_raw."""
    ctx = ctx or default_context()
    pr = _apply_params_in(params, int(d))
    ctx.check(ctx.lib.gsmcal_apply_calibration_batch_resident(ctx.h, C.c_void_p(d_raw), int(d), int(n), float(sample_rate), _dp(pr),
                                                              int(out_len), int(out_stride), C.c_void_p(d_out), C.c_void_p(d_info)),
              "apply_calibration_batch_resident")


ROW_FIELDS = ("status", "num_windows", "num_eval", "num_used", "num_adjacent", "lag0", "delay0", "rel_sampling_ppm", "delay_rms",
              "rel_carrier_hz", "window_carrier_hz", "phase0", "phase_rms", "mean_coherence", "min_coherence_seen", "max_lag",
              "win_len", "sample_rate", "min_coherence", "max_gap")                                   # columns 0..19 (GSMCAL_R_*)
ROW_WINDOW_FIELDS = ("start", "delay", "phase", "freq", "coherence", "edge")


def row_rows(table):
    """(P, ROW_COLS) table of row_coherence[_resident] -> dict of its columns (start, delay, phase, freq, coherence, edge:
    (P, MAX_ROW_WINDOWS), NaN at and beyond W and for windows that were not evaluated)."""
    return _table_rows(table, ROW_COLS, ROW_FIELDS, ROW_WINDOW_FIELDS, MAX_ROW_WINDOWS)


def _row_args_in(pairs, lag0, starts, win_len, max_gap, valid, d):
    pr, lg, npairs = _pairs_in(pairs, lag0, d)
    st = np.ascontiguousarray(np.asarray(starts, dtype=np.int64).ravel())
    if len(st) < 1:
        raise ValueError("starts must hold at least one window start")
    gap = 8.0 * int(win_len) if max_gap is None else float(max_gap)
    va = None
    if valid is not None:
        va = np.ascontiguousarray(np.asarray(valid, dtype=np.int64).reshape(-1, 2))
        if len(va) != d:
            raise ValueError("valid must be (D, 2): {first, end} per row")
    return pr, lg, npairs, st, gap, va


def valid_of(info):
    """apply_calibration's info (apply_rows' dict or the (D, APPLY_INFO_COLS) table) -> the (D, 2) int64 {first_valid, end_valid} that
    row_coherence takes as `valid`"""
    t = info if isinstance(info, dict) else apply_rows(info)
    return np.stack([t["first_valid"], t["end_valid"]], axis=1).astype(np.int64)


def row_coherence(x, pairs, starts, win_len, sample_rate, lag0=0, max_lag=16, min_coherence=0.5, max_gap=None, valid=None, want_corr=False,
                  ctx=None):
    """row_coherence -- the project's own function (include/gsmcal.h): pair_coherence's estimator on any rows
    x (D, N) complex on one nominal time base (apply_calibration's output rows), over the windows starts (W,), 1 .. 128 of them,
    ascending, each win_len samples (16 .. 65536) of which the 4 floor(win_len / 4) first are used.  pairs: (P, 2) row indices (a, b);
    lag0: one int or one per pair, the expected offset of b's content against a's; max_lag M in 1 .. 64; max_gap (default 8 win_len):
    the phase steps between consecutive used windows at most this many samples apart refine the carrier; valid: (D, 2) {first, end}
    per row (valid_of(info) of apply_calibration), None = whole rows.  Returns the (P, ROW_COLS) table (row_rows names its columns;
    status 0, or 16 = fewer than two used windows) -- or, with want_corr, a dict: "table", "corr" (P, W, 2M+1, 4) complex, NaN
    where a window was not evaluated."""
    ctx = ctx or default_context()
    xa = np.ascontiguousarray(np.atleast_2d(np.asarray(x, dtype=np.complex128)))
    d, stride = xa.shape
    pr, lg, npairs, st, gap, va = _row_args_in(pairs, lag0, starts, win_len, max_gap, valid, d)
    m = int(max_lag)
    out = np.empty((npairs, ROW_COLS))
    corr = np.empty((npairs, len(st), 2 * max(m, 0) + 1, 4), dtype=np.complex128) if want_corr else None
    ctx.check(ctx.lib.gsmcal_row_coherence_batch(ctx.h, _dp(xa), stride, d, va.ctypes.data_as(_lib.c_long_p) if va is not None else None,
                                                 pr.ctypes.data_as(_lib.c_int_p), lg.ctypes.data_as(_lib.c_int_p), npairs,
                                                 st.ctypes.data_as(_lib.c_long_p), len(st), int(win_len), m, float(min_coherence), gap,
                                                 float(sample_rate), _dp(out), _dp(corr) if want_corr else None), "row_coherence_batch")
    if not want_corr:
        return out
    return {"table": out, "corr": corr}


def row_coherence_resident(d_x, stride, d, pairs, starts, win_len, sample_rate, d_out, lag0=0, max_lag=16, min_coherence=0.5, max_gap=None,
                           valid=None, d_corr=None, ctx=None):
    """Device-pointer form of row_coherence: only enqueues on the context's stream, e.g. directly behind apply_calibration_resident on
    its d_out (ctx.sync() before reading).  pairs, lag0, starts, valid: host arrays.  d_out: [P][ROW_COLS] doubles; optional d_corr:
    [P][W][2M+1][4] complex.  Device or pinned host memory."""
    ctx = ctx or default_context()
    pr, lg, npairs, st, gap, va = _row_args_in(pairs, lag0, starts, win_len, max_gap, valid, int(d))
    ctx.check(ctx.lib.gsmcal_row_coherence_batch_resident(ctx.h, C.c_void_p(d_x), int(stride), int(d),
                                                          va.ctypes.data_as(_lib.c_long_p) if va is not None else None,
                                                          pr.ctypes.data_as(_lib.c_int_p), lg.ctypes.data_as(_lib.c_int_p), npairs,
                                                          st.ctypes.data_as(_lib.c_long_p), len(st), int(win_len), int(max_lag),
                                                          float(min_coherence), gap, float(sample_rate), C.c_void_p(d_out), _opt(d_corr)),
              "row_coherence_batch_resident")


def apply_params_refine(coh_table, params):
    """Rows of a row_coherence table of the pairs (reference, b), measured on the output rows of a first apply_calibration pass,
    composed into the parameter rows that produced the rows b (gsmcal_apply_params_refine; pure host arithmetic, no context): a second
    pass over the same bytes with the returned rows lands on the reference's time base, carrier and phase.  coh_table: (D, ROW_COLS),
    params: (D, APPLY_PARAMS), row for row.  A coherence row whose status is not 0 gives an all-NaN row but the scale
    (apply_calibration then skips that capture).  The reference's own row is refined by a coherence row of (ref, ref), which leaves it
    unchanged up to rounding -- or keep its first-pass row."""
    lib = _lib.load()
    coh = np.ascontiguousarray(np.asarray(coh_table, dtype=np.float64).reshape(-1, ROW_COLS))
    pr = _apply_params_in(params, len(coh))
    out = np.empty_like(pr)
    for i in range(len(coh)):
        rc = lib.gsmcal_apply_params_refine(_dp(coh[i]), _dp(pr[i]), _dp(out[i]))
        if rc < 0:
            raise GsmcalError(f"apply_params_refine failed with {rc} ")
    return out


def row_lag_search(x, a, b, starts, win_len, sample_rate, lo, hi, max_lag=64, min_coherence=0.5, valid=None, ctx=None):
    """The whole-sample offset of row b's content against row a's, searched over [lo, hi] by ONE row_coherence call: the pair (a, b)
    repeated with lag0 tiled in steps of 2 max_lag - 1 (a maximum on a tile's edge lag is not used, so neighbouring tiles share their
    edge lags).  Returns round(delay0) of the status-0 tile with the largest mean coherence, or None when no tile has status 0."""
    m = int(max_lag)
    lo, hi = int(lo), int(hi)
    if hi < lo:
        raise ValueError("row_lag_search: hi must be at least lo")
    step = max(2 * m - 1, 1)
    lags = np.arange(lo + m - 1, hi + m, step, dtype=np.int64)       # tile j covers the inner lags lag0 - (M - 1) .. lag0 + (M - 1)
    t = row_rows(row_coherence(x, [(int(a), int(b))] * len(lags), starts, win_len, sample_rate, lag0=lags, max_lag=m,
                               min_coherence=min_coherence, valid=valid, ctx=ctx))
    ok = t["status"] == 0
    if not ok.any():
        return None
    best = int(np.argmax(np.where(ok, t["mean_coherence"], -1.0)))
    return int(np.floor(t["delay0"][best] + 0.5))


def retune_align(raw, params, sample_rate, ref, starts, win_len, lag0=0, max_lag=16, min_coherence=0.5, max_gap=None, out_len=None, ctx=None):
    """After a retune: apply_calibration(raw, params) -> row_coherence of every row against row `ref` over the windows `starts` ->
    apply_params_refine -> apply_calibration again with the refined rows.  Returns (out, info, refined params, coherence table): out
    and info of the second pass, the rows on ref's time base, carrier and phase; the coherence table (D, ROW_COLS) is the first
    pass's, row i for the pair (ref, i).  The reference keeps its first-pass parameter row.  A row whose coherence status is not 0
    is skipped by the second pass (info status 17, zeros)."""
    ctx = ctx or default_context()
    out, info = apply_calibration(raw, params, sample_rate, out_len=out_len, ctx=ctx)
    d = out.shape[0]
    table = row_coherence(out, [(int(ref), i) for i in range(d)], starts, win_len, sample_rate, lag0=lag0, max_lag=max_lag,
                          min_coherence=min_coherence, max_gap=max_gap, valid=valid_of(info), ctx=ctx)
    refined = apply_params_refine(table, params)
    refined[int(ref)] = _apply_params_in(params, d)[int(ref)]
    out2, info2 = apply_calibration(raw, refined, sample_rate, out_len=out_len, ctx=ctx)
    return out2, info2, refined, table


def split_spectrum_scan(s_all, start_freq, end_freq, freq_step, num_dongle, gain=0, observe_time=0.1, sample_rate=2.048e6,
                        ctx=None):
    """multi_rtl_sdr_split_scanner.m:150-177 after the captures: s_all is the script's (2*num_samples, num_dongle *
    num_freq_per_sub_band) uint8 matrix (column = capture, units in dist.scan_frequency_plan's order).  Returns the fields
    the script saves (dist.split_spectrum_record), power_spectrum linear."""
    from . import dist
    _, coef, decim, num_samples = dist.spectrum_filter(sample_rate, freq_step, observe_time)
    s_all = np.asarray(s_all, dtype=np.uint8)
    if s_all.ndim != 2 or s_all.shape[0] != 2 * num_samples:
        raise ValueError("s_all must be (2*num_samples, units)")
    power = band_power_batch(s_all.T, coef, decim, ctx=ctx)
    return dist.split_spectrum_record(power, start_freq, end_freq, freq_step, num_dongle, gain, observe_time, sample_rate)


def diversity_spectrum_scan(s_all, start_freq, end_freq, freq_step, gain=0, observe_time=0.1, sample_rate=2.048e6, ctx=None):
    """multi_rtl_sdr_diversity_scanner.m:150-180 after the captures: s_all is the script's (2*num_samples, length(freq),
    num_dongle) uint8 array.  All num_dongle*length(freq) captures go to the GPU in one call.  Returns the fields the
    script saves (dist.diversity_spectrum_record): power_spectrum (num_dongle x length(freq)) and its linear mean over
    dongles, power_spectrum_combine."""
    from . import dist
    _, coef, decim, num_samples = dist.spectrum_filter(sample_rate, freq_step, observe_time)
    s_all = np.asarray(s_all, dtype=np.uint8)
    if s_all.ndim == 2:
        s_all = s_all[:, :, None]
    if s_all.ndim != 3 or s_all.shape[0] != 2 * num_samples:
        raise ValueError("s_all must be (2*num_samples, length(freq), num_dongle)")
    num_dongle, nf = s_all.shape[2], s_all.shape[1]
    raw = s_all.transpose(2, 1, 0).reshape(num_dongle * nf, 2 * num_samples)     # capture (dongle i, point j) = row i*nf + j
    power = band_power_batch(raw, coef, decim, ctx=ctx).reshape(num_dongle, nf)
    return dist.diversity_spectrum_record(power, start_freq, end_freq, freq_step, num_dongle, gain, observe_time,
                                          sample_rate)


def multichannel_spectrum_scan(r_all_raw, start_freq, end_freq, freq_step, gain=0, observe_time=0.2, sample_rate=2.048e6,
                               shift_sign=-1, decim=1, ctx=None):
    """multi_rtl_sdr_diversity_scanner_another_bak.m:186-231 after the captures: r_all_raw is (2*num_samples, num_dongle,
    length(real_freq)) uint8, the script's s per real_freq_idx (:155-176) before raw2iq.  All num_dongle*length(real_freq)
    captures go to the GPU in one call, every grid point of a capture is taken out of it (dist.multichannel_frequency_plan).
    shift_sign: the sign of the mixer's phase.  -1 (default) does what the comment at :193 says, the sub-frequency goes to 0 Hz
    and power_spectrum[:, i] belongs to freq[i]; +1 is the script's literal line :195-196, which measures the point mirrored
    about the capture's centre.  decim = 1 is the script (:203).  Returns dist.multichannel_spectrum_record's fields."""
    from . import dist
    if shift_sign not in (-1, 1):
        raise ValueError("shift_sign must be -1 or +1")
    _, coef, _, num_samples = dist.spectrum_filter(sample_rate, freq_step, observe_time)
    plan = dist.multichannel_frequency_plan(start_freq, end_freq, freq_step, sample_rate)
    r = np.asarray(r_all_raw, dtype=np.uint8)
    ncap = len(plan["real_freq"])
    if r.ndim != 3 or r.shape[0] != 2 * num_samples or r.shape[2] != ncap:
        raise ValueError("r_all_raw must be (2*num_samples, num_dongle, length(real_freq))")
    num_dongle = r.shape[1]
    nsub = max(len(v) for v in plan["freq_set"])
    if nsub > _lib.MAX_SUBBANDS:
        raise ValueError("a capture holds %d grid points: more than %d" % (nsub, _lib.MAX_SUBBANDS))
    w = np.full((ncap, nsub), np.nan)
    for c, rel in enumerate(plan["relative_sub_freq_set"]):
        w[c, :len(rel)] = shift_sign * rel * 2 * np.pi / sample_rate                          # :195
    raw = r.transpose(1, 2, 0).reshape(num_dongle * ncap, 2 * num_samples)      # capture (dongle i, real_freq c) = row i*ncap + c
    power = subband_power_batch(raw, coef, np.tile(w, (num_dongle, 1)), decim=decim, ctx=ctx).reshape(num_dongle, ncap, nsub)
    ps = np.empty((num_dongle, len(plan["freq"])))
    for c, fs in enumerate(plan["freq_set"]):
        ps[:, fs] = power[:, c, :len(fs)]                                       # idx of :186-210, capture by capture
    return dist.multichannel_spectrum_record(ps, start_freq, end_freq, freq_step, num_dongle, gain, observe_time, sample_rate)


def fcch_scan_batch(raw, coef, ctx=None):
    """Scanner detect loop for D captures -> dict(snr, num_hit, positions, pos_snr, counts)."""
    ctx = ctx or default_context()
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    d, two_n = raw.shape
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    snr = np.zeros(d)
    nh = np.zeros(d)
    pos = np.zeros((d, MAX_HITS))
    psnr = np.zeros((d, MAX_HITS))
    cnt = np.zeros(d, dtype=np.int32)
    ctx.check(ctx.lib.gsmcal_fcch_scan_batch(ctx.h, raw.ctypes.data_as(_lib.c_u8_p), d, two_n // 2, _dp(coef),
                                             len(coef), _dp(snr), _dp(nh), _dp(pos), _dp(psnr),
                                             cnt.ctypes.data_as(_lib.c_int_p)), "fcch_scan_batch")
    return {"snr": snr, "num_hit": nh, "positions": pos, "pos_snr": psnr, "counts": cnt}


def calibrate_batch(raw, coef, sch_training_sequence, carrier_freq, want_r=False, ctx=None):
    """gsm_sync_demod.m:107-124 for D streams: raw (D, 2N) uint8 -> dict(table, pos_info, r_correct, r_len)."""
    ctx = ctx or default_context()
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    d, two_n = raw.shape
    n = two_n // 2
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    ts = np.ascontiguousarray(np.asarray(sch_training_sequence, dtype=np.complex128).ravel())
    cf = np.ascontiguousarray(np.broadcast_to(np.asarray(carrier_freq, dtype=np.float64), (d,)))
    table = np.zeros((d, TABLE_COLS))
    pos_info = np.zeros((d, 2, MAX_POS_ROWS))
    r_len = np.zeros(d, dtype=np.int64)
    r = np.empty((d, n), dtype=np.complex128) if want_r else None
    ctx.check(ctx.lib.gsmcal_calibrate_batch(ctx.h, raw.ctypes.data_as(_lib.c_u8_p), d, n, _dp(coef), len(coef),
                                             _dp(ts), len(ts), _dp(cf), _dp(table), _dp(pos_info),
                                             _dp(r) if want_r else None, r_len.ctypes.data_as(_lib.c_long_p)),
              "calibrate_batch")
    out = {"table": table, "pos_info_raw": pos_info, "r_len": r_len, "r_correct": r}
    rows = []
    for i in range(d):
        k = int(table[i, 7])
        if table[i, 8] == -1.0:
            # the reference's all -1 sentinel, in the shape of the exit taken: [-1 -1] (SCH_corr_rate_correction.m:9,:61) or
            # the -ones(3*num_fcch_hit,2) pre-allocation of :32 returned by the :84 / :106-112 exits
            rows.append(-np.ones((k, 2)))
        else:
            rows.append(pos_info[i, :, :k].T.copy())
    out["pos_info"] = rows
    return out


def calibrate_batch_dev(d_raw, d, n, coef, sch_training_sequence, carrier_freq, d_table, d_pos_info=None, d_r_correct=None,
                        d_r_len=None, ctx=None):
    """Device-pointer form of calibrate_batch: only enqueues on the context's stream (ctx.sync() before reading the outputs).
    d_raw: [d][2n] bytes; d_table: [d][TABLE_COLS] doubles in any memory the GPU can store to (device or pinned host);
    optional d_pos_info [d][2][MAX_POS_ROWS], d_r_correct [d][n] complex, d_r_len [d] int64.  carrier_freq: scalar or [d]."""
    ctx = ctx or default_context()
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    ts = np.ascontiguousarray(np.asarray(sch_training_sequence, dtype=np.complex128).ravel())
    cf = np.ascontiguousarray(np.broadcast_to(np.asarray(carrier_freq, dtype=np.float64), (int(d),)))
    vp = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx.check(ctx.lib.gsmcal_calibrate_batch_dev(ctx.h, C.c_void_p(d_raw), int(d), int(n), _dp(coef), len(coef),
                                                 _dp(ts), len(ts), _dp(cf),
                                                 C.c_void_p(d_table), vp(d_pos_info), vp(d_r_correct), vp(d_r_len)),
              "calibrate_batch_dev")


def fcch_scan_batch_dev(d_raw, d, n, coef, d_snr_numhit, d_positions=None, d_pos_snr=None, d_counts=None, ctx=None):
    """Device-pointer form of fcch_scan_batch: only enqueues (call ctx.sync() before reading the outputs).
    d_raw: [d][2n] bytes; d_snr_numhit: [d][2] doubles; optional [d][MAX_HITS] doubles x2 and [d] ints."""
    ctx = ctx or default_context()
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    vp = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx.check(ctx.lib.gsmcal_fcch_scan_batch_dev(ctx.h, C.c_void_p(d_raw), int(d), int(n), _dp(coef), len(coef),
                                                 C.c_void_p(d_snr_numhit), vp(d_positions), vp(d_pos_snr), vp(d_counts)),
              "fcch_scan_batch_dev")


def synth_expand_dev(d_base, k, n, d_out, d, first_unit=0, seed=20260101, ctx=None):
    """Synthetic-input utility: expand k base captures on the device into d distinct ones (see include/gsmcal.h;
    synth.expand_capture is the host twin)."""
    ctx = ctx or default_context()
    ctx.check(ctx.lib.gsmcal_synth_expand_dev(ctx.h, C.c_void_p(d_base), int(k), int(n), C.c_void_p(d_out), int(d),
                                              int(first_unit), int(seed)), "synth_expand_dev")


def last_batch_snr(stream, ctx=None):
    """Parity tap: (snr table of `stream` from the last batch call, number of moving-search windows at its head)."""
    ctx = ctx or default_context()
    buf = np.zeros(1 << 16)
    n_tab, n_mov = C.c_long(0), C.c_long(0)
    ctx.check(ctx.lib.gsmcal_last_batch_snr(ctx.h, int(stream), _dp(buf), len(buf), C.byref(n_tab), C.byref(n_mov)),
              "last_batch_snr")
    return buf[: min(n_tab.value, len(buf))].copy(), int(n_mov.value)


def last_batch_details(d, ctx=None):
    """Intermediates of the last batch call (coarse/fine/SCH positions per stream) for parity tests."""
    ctx = ctx or default_context()
    arrs = [np.zeros((d, MAX_HITS)) for _ in range(5)]
    counts = np.zeros((d, 5), dtype=np.int32)
    ctx.check(ctx.lib.gsmcal_last_batch_details(ctx.h, d, *[_dp(a) for a in arrs],
                                                counts.ctypes.data_as(_lib.c_int_p)), "last_batch_details")
    names = ("coarse_pos", "coarse_snr", "fine_first", "fcch_pos", "sch_first")
    out = {k: a for k, a in zip(names, arrs)}
    out["counts"] = counts
    return out
