"""Builds and runs the stand-alone check of the outer step (tests/host/outer_main.cpp over neutfem_amd/csrc/nf_outer.h): the Chebyshev
schedule over 40 steps and its coefficients, the table against the cosh formulas, outer_step and the stop test on hand-computed inputs,
the element update per mode; plain C++, no device.  The same program is meant to be built with -fsanitize=address,undefined by hand; here
it is compiled plainly so that it cannot rot."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_outer_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "the build needs a host C++ compiler anyway"
    exe = str(tmp_path / "outer")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(HERE, "host", "outer_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count("ok ") == 7 and "FAIL" not in r.stderr
