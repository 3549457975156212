"""CPU-only: csrc/combine_weights.h, the host arithmetic of gsmcal_combine_weights, on its own under the
address and undefined-behaviour sanitizers.  A host program run directly, like tests/test_asan_cpu.py: nothing of it touches a GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_solver_header_stands_alone_under_the_sanitizers(tmp_path):
    """csrc/combine_weights.h includes nothing of HIP: a plain C++ main (tests/array_solver_main.cpp) is built with
    -fsanitize=address,undefined and run directly on the G = 1 and G = 64 cases.  A host program; nothing is preloaded anywhere."""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = tmp_path / "array_solver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "multi-rtl-sdr-calibration_amd", "csrc"), os.path.join(ROOT, "tests", "array_solver_main.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "solver ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    src = open(os.path.join(ROOT, "multi-rtl-sdr-calibration_amd", "csrc", "combine_weights.h")).read()
    includes = [ln for ln in src.splitlines() if ln.startswith("#include")]
    assert includes and all(ln.split()[1] in ("<cmath>", "<complex>", "<vector>") for ln in includes), includes
