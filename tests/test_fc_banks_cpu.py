"""CPU-only: csrc/fc_layout.h, k_fine_cert's LDS carve and the lane maps of its slide phase and E/C scans, checked against the LDS
bank rule of gfx950 by a host program run directly (tests/fc_banks_main.cpp), like tests/test_apply_params_cpu.py: nothing of it
touches a GPU.  For the reference geometry every read and store of the two phases must be 1-way; for 1 .. 16 samples per symbol
every chunk and every shift is visited exactly once and no index leaves its region of the carve."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slides_and_scans_are_conflict_free_and_stay_inside_the_carve(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = tmp_path / "fc_banks"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "multi-rtl-sdr-calibration_amd", "csrc"), os.path.join(ROOT, "tests", "fc_banks_main.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "fc_banks ok" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    # the kernel reads the same text: kernels_detect.h defines no padding of its own
    src = open(os.path.join(ROOT, "multi-rtl-sdr-calibration_amd", "csrc", "kernels_detect.h")).read()
    assert "#define FC_XP" not in src
