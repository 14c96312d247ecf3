"""CPU checks of the device-array argument checker (csrc/wr_args.h, DESIGN.md
12) by itself: tests/native/args_check.cpp, compiled here with g++ from the
product's header, drives it with a fake pointer classifier over an address map
of two device-0 blocks, a device-1 block, a host and a pinned block, and
asserts each rule -- null and empty arguments, alignment, the two addresses
classified per array, foreign and host memory, overlaps, and the order in which
the rules report.  What the library's calls do around the checker is checked on
the GPU (the refusal tests of test_gpu_device_rays.py, test_gpu_shading.py and
test_gpu_points.py)."""
import os
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "winmad-s-raytracer-v1.0_amd", "csrc")


def test_the_checker_alone_compiles_without_hip_and_keeps_its_rules():
    out = os.path.join(tempfile.mkdtemp(prefix="wr_args_"), "args_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "native", "args_check.cpp"),
                    "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr


def test_the_header_names_no_hip():
    with open(os.path.join(CSRC, "wr_args.h")) as f:
        text = f.read()
    assert "#include <hip" not in text and "#include \"hip" not in text
    assert "hipPointerGetAttributes(" not in text and "hipGetLastError(" not in text
