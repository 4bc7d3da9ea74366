"""The walk of csrc/b4d_tile.hpp (tile_walk, tile_step: which (row, group-of-four) pairs of a tile each of the 256 lanes of a
workgroup takes), run as host code by a small C++ program in two forms: rounds of U = 4 groups until the lane has left the tile
(`stage` of b4d_window.hpp: separable filters, local statistics, SSIM), and one round of U = 6 or 7 over a lane's whole share (the form
of a fully unrolled fill; no kernel runs the walk that way yet: `fill_tile` of b4d_rankfilt.hip still divides per group).  Every
pair of the tile must be visited exactly once and nothing else.  The border rule of the same header is covered by
tests/test_rank_filter_host.py (test_border_index_equals_numpy_pad)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WALK_PROGRAM = r"""
// For ng in 1 .. 140, nrows in {1, 2, 7, 9, 38, 46, 264, 767} and U in {4, 6, 7}: the walk of all 256 lanes, as a tile fill runs it.
// U = 4 takes rounds while the lane is inside the tile; U = 6, 7 take one round and are run where nrows * ng <= 256 * U.
// Prints "combinations <n>" and exits 0, or the first fault and exits 1.
#include <cstdio>
#include <vector>

#include "b4d_tile.hpp"
using namespace b4d;

static int run(int ng, int nrows, int U, bool once) {
    std::vector<int> seen((size_t)nrows * ng, 0);
    for (int t = 0; t < 256; ++t) {
        TileWalk w = tile_walk(t, ng);
        while (once || w.j < nrows) {
            for (int u = 0; u < U; ++u) {
                if (w.j < nrows) {
                    if (w.j < 0 || w.g < 0 || w.g >= ng) {
                        std::printf("ng %d nrows %d U %d lane %d: pair (%d, %d) outside the tile\n", ng, nrows, U, t, w.j, w.g);
                        return 1;
                    }
                    ++seen[(size_t)w.j * ng + w.g];
                }
                tile_step(w);
            }
            if (once) break;
        }
    }
    for (int j = 0; j < nrows; ++j)
        for (int g = 0; g < ng; ++g)
            if (seen[(size_t)j * ng + g] != 1) {
                std::printf("ng %d nrows %d U %d: pair (%d, %d) visited %d times\n", ng, nrows, U, j, g, seen[(size_t)j * ng + g]);
                return 1;
            }
    return 0;
}

int main() {
    const int rows[8] = {1, 2, 7, 9, 38, 46, 264, 767}, us[3] = {4, 6, 7};
    int n = 0;
    for (int ng = 1; ng <= 140; ++ng)
        for (int nrows : rows)
            for (int U : us) {
                const bool once = U != 4;
                if (once && nrows * ng > 256 * U) continue;
                if (run(ng, nrows, U, once)) return 1;
                ++n;
            }
    std::printf("combinations %d\n", n);
    return 0;
}
"""


@pytest.fixture(scope="module")
def walk_program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("tile_walk")
    src, exe = d / "walk.cpp", d / "walk"
    src.write_text(WALK_PROGRAM)
    # a stand-alone program with its own main: the sanitizers are linked in the ordinary way
    cmd = [cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "barc4dip_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:      # a compiler without the sanitizer runtimes still checks the walk
        r = subprocess.run([c for c in cmd if not c.startswith("-fsanitize") and not c.startswith("-fno-sanitize")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def test_every_pair_of_the_tile_is_visited_once(walk_program):
    r = subprocess.run([walk_program], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    # U = 4: all 140 * 8 tiles; one round of U: the tiles with nrows * ng <= 256 * U
    rows = (1, 2, 7, 9, 38, 46, 264, 767)
    want = 140 * 8 + sum(1 for ng in range(1, 141) for n in rows for u in (6, 7) if n * ng <= 256 * u)
    assert r.stdout.split() == ["combinations", str(want)]
