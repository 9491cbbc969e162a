"""Builds and runs the stand-alone check of the fingerprint grouping (tests/host/line_groups_main.cpp over
neutfem_amd/csrc/nf_line_groups.h): plain C++, no device.  The same program is meant to be built with
-fsanitize=address,undefined by hand; here it is compiled plainly so that it cannot rot."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_line_groups_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "the build needs a host C++ compiler anyway"
    exe = str(tmp_path / "line_groups")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(HERE, "host", "line_groups_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count("ok ") == 9 and "FAIL" not in r.stderr
