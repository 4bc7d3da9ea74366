"""The C/D index map of barc4dip_amd/csrc/b4d_mfma.hpp as host code: tools/host_check/check_mfma_map.cpp, a stand-alone C++
program with its own main, built against the host stand-in for <hip/hip_runtime.h> (tools/host_check/hip).  No GPU, nothing
loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def map_program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("mfma_map_host") / "check_mfma_map"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "tools", "host_check"), "-I", os.path.join(ROOT, "barc4dip_amd", "csrc"),
           os.path.join(ROOT, "tools", "host_check", "check_mfma_map.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:      # a compiler without the sanitizer runtimes still checks the map
        r = subprocess.run([c for c in cmd if not c.startswith("-fsanitize") and not c.startswith("-fno-sanitize")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def test_mfma_walker_covers_the_tile_once(map_program):
    """Over 256 lanes x 2 x 2 tiles x 16 registers the walker's (row, col) pairs cover the 128 x 128 tile exactly once, in
    sub-tile and register order, and equal col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) offset by the
    wave's 64 and the sub-tile's 32 (and by the tile corner)."""
    r = subprocess.run([map_program], capture_output=True, text=True)
    assert r.returncode == 0 and "TOTAL BAD 0" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
