"""Builds and runs the stand-alone check of the resident solve's line-per-lane plan (tests/host/resident_lanes_main.cpp over
neutfem_amd/csrc/nf_resident_lanes.h): plain C++, no device.  The same program is meant to be built with -fsanitize=address,undefined by hand;
here it is compiled plainly so that it cannot rot."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_resident_lanes_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "the build needs a host C++ compiler anyway"
    exe = str(tmp_path / "resident_lanes")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(HERE, "host", "resident_lanes_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ok   24 meshes" in r.stdout and "FAIL" not in r.stderr
