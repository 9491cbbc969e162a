"""Builds and runs the stand-alone checks of the direction ring behind the batched x_sol update (tests/host/xsol_ring_main.cpp over
neutfem_amd/csrc/nf_xsol_ring.h) and of its option (tests/host/xsol_option_main.cpp over nf_options.h): plain C++, no device.  The same programs are meant to be built with
-fsanitize=address,undefined by hand; here they are compiled plainly so that they cannot rot."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_xsol_ring_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "the build needs a host C++ compiler anyway"
    exe = str(tmp_path / "xsol_ring")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(HERE, "host", "xsol_ring_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ok   " in r.stdout and "FAIL" not in r.stderr


def test_xsol_option_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "the build needs a host C++ compiler anyway"
    exe = str(tmp_path / "xsol_option")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(HERE, "host", "xsol_option_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count("ok ") == 3 and "FAIL" not in r.stderr
