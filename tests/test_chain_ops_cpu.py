"""CPU-only: csrc/chain_ops.h, the one text of the resampling chain's per-sample arithmetic, held to literal copies of the
spellings it replaced by a host program run directly (tests/chain_ops_main.cpp, its own main), like tests/test_fc_banks_cpu.py:
nothing of it touches a GPU and nothing is loaded into Python.  The program checks the source range of a LERP level against the
three former spellings, the interp1 index and weight against the 64-bit-index and the double-index spelling (bit for bit), the
cover of a raw span by 16-byte chunks against the three former counts, ffast_chunk on a heap buffer of exactly the stream's
bytes (the sanitizer sees any read outside it) and the slots of the window rotator table."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-rtl-sdr-calibration_amd", "csrc")


def test_chain_ops_equal_the_spellings_they_replaced(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = tmp_path / "chain_ops"
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        "-pthread", "-I" + CSRC, os.path.join(ROOT, "tests", "chain_ops_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "chain_ops ok" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def test_kernels_spell_no_chain_arithmetic_themselves():
    """The kernels read chain_ops.h: no second definition of its functions and none of the expressions they replaced."""
    for name in ("kernels_frontend.h", "kernels_estim.h", "kernels_detect.h"):
        src = open(os.path.join(CSRC, name)).read()
        for gone in ("st_rot(", "ST_FIR_TAP", "uintptr_t)base >> 1", "1 + GC_ROT_A + (", "uint4 ffast_chunk(", "long raw_first_al(",
                     "void fir4_lds(", "double lerp_pos("):
            assert gone not in src, (name, gone)
        assert src.count("lerp_pos(") == 0, name                  # interp1 goes through lerp_tap / lerp_at
