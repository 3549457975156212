"""CPU-only: csrc/apply_refine.h, the host arithmetic of gsmcal_apply_params_refine, on its own under the
address and undefined-behaviour sanitizers.  A host program run directly, like tests/test_apply_params_cpu.py: nothing of it touches
a GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_helper_header_stands_alone_under_the_sanitizers(tmp_path):
    """csrc/apply_refine.h includes nothing of HIP: a plain C++ main (tests/apply_refine_main.cpp) is built with
    -fsanitize=address,undefined and run directly.  A host program; nothing is preloaded anywhere."""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = tmp_path / "apply_refine"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "multi-rtl-sdr-calibration_amd", "csrc"), os.path.join(ROOT, "tests", "apply_refine_main.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "apply_refine ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    src = open(os.path.join(ROOT, "multi-rtl-sdr-calibration_amd", "csrc", "apply_refine.h")).read()
    includes = [ln for ln in src.splitlines() if ln.startswith("#include")]
    assert includes and all(ln.split()[1] in ("<cmath>", "<limits>") for ln in includes), includes
