"""The block-id placement of the weight-gradient GEMM (csrc/inr_dw_place.h) on the host: tools/probes/dw_place_check.cpp
includes nothing but that header, is built here with the host C++ compiler and checks, for every grid size 1..4096, that
the map is a permutation of the block ids and that the ids sharing an XCD (b, b + 8, ...) get consecutive logical ids;
for the graded launch (250 workgroups, 10 per chunk) that at least 18 of the 25 chunks sit under one label."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mri-implicit-neural-representations_amd", "csrc")
SRC = os.path.join(ROOT, "tools", "probes", "dw_place_check.cpp")


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_dw_place_check(tmp_path):
    cxx = _host_compiler()
    assert cxx is not None, "no host C++ compiler (c++, g++, clang++ or $CXX)"
    exe = str(tmp_path / "dw_place_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout
    assert "chunks under one label" in run.stdout
