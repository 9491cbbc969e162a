"""Builds and runs the stand-alone check of the option table (tests/host/options_main.cpp over neutfem_amd/csrc/nf_options.h): every
key's normaliser, default, effects and copy class against values written out by hand; plain C++, no device.  The same program is meant
to be built with -fsanitize=address,undefined by hand; here it is compiled plainly so that it cannot rot."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_options_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "the build needs a host C++ compiler anyway"
    exe = str(tmp_path / "options")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(HERE, "host", "options_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count("ok ") == 8 and "FAIL" not in r.stderr
