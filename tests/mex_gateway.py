"""Builds and drives mex/gsmcal_mex.c without MATLAB: one shared object per (target, storage mode, backend), made of the gateway,
the working mxArray stand-in tests/mex_stub/mxstub.c and either the recording fake of the ABI (tests/mex_stub/fake_gsmcal.c) or
libgsmcal.so itself, loaded with ctypes.  numpy arrays go in and come out in Fortran order, as MATLAB holds them.

Everything in an object is compiled with hidden visibility except the harness (mxh_*) and the fake's controls (fake_*): each
object binds its own stub, its own mexFunction and its own g_ctx, however many of them one process holds."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "mex_stub")
SOURCE = os.path.join(ROOT, "mex", "gsmcal_mex.c")

TARGETS = ("raw2iq", "chn_filter_8x_4x", "chn_filter_4x", "move_fft_snr_runtime_avg", "specific_fft_snr_fix_avg",
           "FCCH_coarse_position", "FCCH_fine_correction", "SCH_corr_rate_correction", "carrier_correct_post_SCH", "FCCH_demod",
           "BCCH_demod", "SCH_decode", "BCCH_decode", "CW_check", "IQ_imbalance", "pair_coherence", "pair_align",
           "total_ppm_calculation", "gsmcal_calibrate", "gsmcal_fcch_scan", "gsmcal_band_power", "gsmcal_subband_power")
MODES = ("interleaved", "split")
MAX_OUT = 8
CLS_DOUBLE, CLS_UINT8, CLS_LOGICAL, CLS_CELL = range(4)

_TMP = []
_CACHE = {}


def compiler():
    """cc / gcc where present, ROCm's clang otherwise; none at all is an error (a test that needs it fails, it does not skip)."""
    for name in ("cc", "gcc"):
        p = shutil.which(name)
        if p:
            return p
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for p in (os.path.join(rocm, "llvm", "bin", "clang"), os.path.join(rocm, "lib", "llvm", "bin", "clang"), shutil.which("clang")):
        if p and os.path.exists(p):
            return p
    raise RuntimeError("no C compiler (cc, gcc or ROCm's clang) to build the MEX gateway with")


def _tmpdir():
    if not _TMP:
        _TMP.append(tempfile.mkdtemp(prefix="gsmcal_mex_"))
        atexit.register(shutil.rmtree, _TMP[0], ignore_errors=True)
    return _TMP[0]


def build(target, mode, backend="fake", source=SOURCE, defines=("MATLAB_MEX_FILE",)):
    """Compiles one gateway object and returns its path.  backend "fake": the recording ABI; "lib": libgsmcal.so (the file the
    package loads; it must exist).  source: another gateway source (the stub's own tests).  defines: -D flags; MATLAB_MEX_FILE is
    what `mex` itself defines, so the gateway takes the paths it takes under MATLAB (defines=() builds it as the -fsyntax-only
    checks see it, against the reduced mex.h)."""
    assert mode in MODES and backend in ("fake", "lib")
    tag = "%s_%s_%s_%d" % (target, mode, backend, len(os.listdir(_tmpdir())))
    out = os.path.join(_tmpdir(), tag + ".so")
    cmd = [compiler(), "-std=c99", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-Wall", "-Wextra", "-Wno-unused-function",
           "-Werror", "-DGSMCAL_FN_" + target] + ["-D" + d for d in defines]
    if mode == "split":
        cmd.append("-DGSMCAL_STUB_SPLIT")
    cmd += ["-I" + os.path.join(ROOT, "include"), "-I" + STUB, source, os.path.join(STUB, "mxstub.c")]
    if backend == "fake":
        cmd.append(os.path.join(STUB, "fake_gsmcal.c"))
    else:
        import gsmcal
        lib = gsmcal.lib_path()
        if not os.path.exists(lib):
            raise RuntimeError(lib + " is missing: build the library first")
        cmd += [lib, "-Wl,-rpath," + os.path.dirname(lib)]
    cmd += ["-lm", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building the gateway failed:\n" + " ".join(cmd) + "\n" + r.stderr)
    return out


class Result:
    """One call: out (list of numpy arrays / lists for cells, None where plhs[i] was not set), err ((id, text) or None), printed,
    failures (what the stub recorded: guard words, invalid mxFree, ...; "" when clean), released (mxMalloc blocks left to MATLAB)."""

    def __init__(self, out, err, printed, failures, released):
        self.out, self.err, self.printed, self.failures, self.released = out, err, printed, failures, released

    @property
    def set_mask(self):
        return [o is not None for o in self.out]


class Gateway:
    def __init__(self, target, mode, backend="fake", source=SOURCE, defines=("MATLAB_MEX_FILE",)):
        self.target, self.mode, self.backend = target, mode, backend
        if backend == "lib":
            import gsmcal
            gsmcal.load()                                     # the gateway object then binds the instance the package uses
        self.path = build(target, mode, backend, source, defines)
        h = self.h = C.CDLL(self.path)
        h.mxh_create.restype = C.c_void_p
        h.mxh_create.argtypes = [C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p]
        h.mxh_destroy.argtypes = [C.c_void_p]
        h.mxh_info.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        h.mxh_read.argtypes = [C.c_void_p, C.c_void_p]
        h.mxh_cell.restype = C.c_void_p
        h.mxh_cell.argtypes = [C.c_void_p, C.c_size_t]
        h.mxh_out.restype = C.c_void_p
        h.mxh_out.argtypes = [C.c_int]
        h.mxh_call.argtypes = [C.c_int, C.c_int, C.c_void_p]
        for name in ("mxh_err_id", "mxh_err_msg", "mxh_printed", "mxh_failures"):
            getattr(h, name).restype = C.c_char_p
        assert bool(h.mxh_interleaved()) == (mode == "interleaved")
        if backend == "fake":
            h.fake_log.restype = C.c_char_p
            h.fake_preset.argtypes = [C.c_int, C.c_int, C.c_long, C.c_int]
            self.preset()

    # ---- numpy <-> mxArray ----
    def to_mx(self, x):
        a = np.asarray(x)
        if a.ndim == 0:
            a = a.reshape(1, 1)
        if a.ndim != 2:
            raise ValueError("MATLAB arrays are matrices: give a row or a column (2-D)")
        if a.dtype == np.uint8:
            cls, cplx = CLS_UINT8, 0
        elif a.dtype == np.bool_:
            cls, cplx, a = CLS_LOGICAL, 0, a.astype(np.uint8)
        elif np.iscomplexobj(a):
            cls, cplx, a = CLS_DOUBLE, 1, a.astype(np.complex128)
        else:
            cls, cplx, a = CLS_DOUBLE, 0, a.astype(np.float64)
        buf = np.asfortranarray(a)
        return self.h.mxh_create(cls, cplx, a.shape[0], a.shape[1], buf.ctypes.data_as(C.c_void_p))

    def from_mx(self, p):
        cls, cplx, m, n = C.c_int(), C.c_int(), C.c_size_t(), C.c_size_t()
        self.h.mxh_info(p, C.byref(cls), C.byref(cplx), C.byref(m), C.byref(n))
        shape = (m.value, n.value)
        if cls.value == CLS_CELL:
            cells = [self.h.mxh_cell(p, i) for i in range(m.value * n.value)]
            return {"shape": shape, "cells": [None if c is None else self.from_mx(c) for c in cells]}
        dt = np.complex128 if cplx.value else {CLS_DOUBLE: np.float64, CLS_UINT8: np.uint8, CLS_LOGICAL: np.uint8}[cls.value]
        a = np.zeros(shape, dtype=dt, order="F")
        if a.size:
            self.h.mxh_read(p, a.ctypes.data_as(C.c_void_p))
        return a.astype(np.bool_) if cls.value == CLS_LOGICAL else a

    # ---- a call ----
    def call(self, *args, nlhs=1):
        h = self.h
        ins = [self.to_mx(a) for a in args]
        arr = (C.c_void_p * MAX_OUT)(*ins)                     # the slots behind nrhs stay NULL
        rc = h.mxh_call(int(nlhs), len(ins), arr)
        out = [None] * MAX_OUT
        for i in range(MAX_OUT):
            p = h.mxh_out(i)
            if p:
                out[i] = self.from_mx(p)
        printed, released = h.mxh_printed().decode(), h.mxh_released()
        failures = h.mxh_failures().decode()
        err = (h.mxh_err_id().decode(), h.mxh_err_msg().decode()) if rc else None
        for p in ins:
            h.mxh_destroy(p)
        failures += h.mxh_failures().decode()[len(failures):]   # guard words behind the inputs are looked at when they go
        return Result(out, err, printed, failures, released)

    def run_atexit(self):
        """Runs the hooks the gateway gave mexAtExit, as MATLAB does when the MEX file is cleared; returns how many ran."""
        return self.h.mxh_run_atexit()

    def num_hooks(self):
        return self.h.mxh_num_hooks()

    # ---- the fake's controls ----
    def preset(self, status=0, count=3, len_r=5, create_rc=0):
        self.h.fake_preset(status, count, len_r, create_rc)
        self.h.fake_reset()

    def calls(self):
        return self.h.fake_calls()

    def created(self):
        return self.h.fake_created()

    def destroyed(self):
        return self.h.fake_destroyed()

    def log(self):
        """The fake's record: one dict per call, {"fn": name, key: text, ..., "hash": hex}."""
        recs = []
        for line in self.h.fake_log().decode().splitlines():
            parts = line.split("|")
            d = {"fn": parts[0]}
            d.update(p.split("=", 1) for p in parts[1:])
            recs.append(d)
        return recs


def gateway(target, mode, backend="fake"):
    """The cached object of (target, mode, backend): built once per process."""
    key = (target, mode, backend)
    if key not in _CACHE:
        _CACHE[key] = Gateway(target, mode, backend)
    return _CACHE[key]


def fnv(*arrays):
    """The fake's hash of what it read: FNV-1a over the bytes of the given arrays, each in Fortran order, one after the other."""
    h = 0xcbf29ce484222325
    for a in arrays:
        a = np.asarray(a)
        if np.iscomplexobj(a):
            a = a.astype(np.complex128)
        elif a.dtype != np.uint8:
            a = a.astype(np.float64)
        for b in a.tobytes(order="F"):
            h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h
