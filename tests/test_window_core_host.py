"""The windowed-moments core of csrc/b4d_window.hpp (k_local_stats of b4d_smooth.hip, k_ssim of b4d_perceptual.hip), run as host
code by a small C++ program: the LDS layout for every window 1 .. 63 x 1 .. 63 in both kernels' configurations (plane offsets
aligned and disjoint, checked in the program; the byte counts printed and compared here with perceptual.lds_bytes and with the
local-statistics formula; the constants by value), and the row and column passes on a 9 x 11 tile pair against a plainly written
double loop in the order include/b4d.h states, bit for bit.  The walk of the stager is covered by tests/test_tile_walk_host.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
// "layout": prints "constants WIN_T WIN_MAX WIN_PAIR_LANES WIN_LDS_LIMIT", then "sy sx bytes(1 plane, 2 sums, 0 extra) bytes(2 planes,
// 5 sums, the pair kernel's extra doubles)" for every window, after checking each layout.  "passes": prints "passes <n>".
// Exits 1 with the first fault.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "b4d_window.hpp"
using namespace b4d;

static int check_layout(int planes, int sums, int sy, int sx, int extra, const WindowLayout& l) {
    const long rows = WIN_T + sy - 1;
    bool ok = l.rows == rows && l.pitch >= WIN_T + sx - 1 && l.pitch % 4 == 0;
    ok = ok && l.plane >= rows * l.pitch && l.plane % 4 == 0;                  // float planes: disjoint, each on 16 bytes
    ok = ok && l.sums >= planes * l.plane && l.sums % 4 == 0;                  // the float64 part: behind them, on 16 bytes
    ok = ok && l.sum_plane >= rows * WIN_T;                                    // planes of row sums: disjoint
    ok = ok && l.bytes == 4 * (size_t)l.sums + 8 * ((size_t)sums * l.sum_plane + extra);
    if (!ok) std::printf("layout (%d planes, %d sums, %d x %d, %d extra) is inconsistent\n", planes, sums, sy, sx, extra);
    return ok ? 0 : 1;
}
static int layout() {
    std::printf("constants %d %d %d %zu\n", WIN_T, WIN_MAX, WIN_PAIR_LANES, WIN_LDS_LIMIT);
    const int extra = 2 * (WIN_PAIR_LANES / 64);
    for (int sy = 1; sy <= WIN_MAX; ++sy)
        for (int sx = 1; sx <= WIN_MAX; ++sx) {
            const WindowLayout a = window_layout(1, 2, sy, sx, 0), b = window_layout(2, 5, sy, sx, extra);
            if (check_layout(1, 2, sy, sx, 0, a) || check_layout(2, 5, sy, sx, extra, b)) return 1;
            std::printf("%d %d %zu %zu\n", sy, sx, a.bytes, b.bytes);
        }
    return 0;
}

constexpr int TH = 9, TW = 11;   // the staged tile: halo included
static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

// the contract, plainly: sum q of output (oy, ox), rows first, taps ascending; a box window adds, a weighted one fuses the tap
static double moment(int q, int np, float r, float x) {
    const double u = r, v = x;
    if (np == 1) return q == 0 ? u : u * u;
    return q == 0 ? u : q == 1 ? v : q == 2 ? u * u : q == 3 ? v * v : u * v;
}
static double plain(int q, int np, const float* R, const float* X, int oy, int ox, const WindowTaps& t) {
    double S = 0.0;
    for (int j = 0; j < t.sy; ++j) {
        double row = 0.0;
        for (int k = 0; k < t.sx; ++k) {
            const double m = moment(q, np, R[(oy + j) * TW + ox + k], X[(oy + j) * TW + ox + k]);
            row = t.box ? row + m : std::fma(t.wx[k], m, row);
        }
        S = t.box ? S + row : std::fma(t.wy[j], row, S);
    }
    return S;
}

template <int NP, int ROWS>
static int run(const WindowTaps& t, const std::vector<float>& tiles, int plane) {
    constexpr int NS = window_sums(NP);
    const int ow = TW - t.sx + 1, oh = TH - t.sy + 1;              // outputs of the tile
    const int sum_plane = (TH + 1) * WIN_T;                         // one row more: ROWS = 2 reads it below the last odd row
    std::vector<double> B((size_t)NS * sum_plane, 0.0);
    for (int r = 0; r < TH; ++r)
        for (int c = 0; c < ow; ++c) {
            double s[NS] = {};
            window_row_sums<NP>(tiles.data() + r * TW + c, plane, t, s);
            for (int q = 0; q < NS; ++q) B[(size_t)q * sum_plane + r * WIN_T + c] = s[q];
        }
    for (int ly = 0; ly < oh; ly += ROWS)
        for (int c = 0; c < ow; ++c) {
            const WindowSums<NS, ROWS> got = window_col_sums<NS, ROWS>(B.data() + ly * WIN_T + c, sum_plane, t);
            for (int i = 0; i < ROWS && ly + i < oh; ++i)
                for (int q = 0; q < NS; ++q) {
                    const double want = plain(q, NP, tiles.data(), tiles.data() + plane, ly + i, c, t);
                    if (!same(got.s[i][q], want)) {
                        std::printf("planes %d rows %d window %d x %d box %d: sum %d of output (%d, %d) is %a, the plain loop gives %a\n", NP, ROWS,
                                    t.sy, t.sx, t.box, q, ly + i, c, got.s[i][q], want);
                        return 1;
                    }
                }
        }
    return 0;
}

static int passes() {
    const int plane = up4(TH * TW);
    std::vector<float> tiles(2 * plane, 0.f);
    unsigned s = 12345u;
    for (int p = 0; p < 2; ++p)
        for (int i = 0; i < TH * TW; ++i) {          // mixed sign, magnitudes from 1e-6 to 1e+6
            s = s * 1664525u + 1013904223u;
            const float mant = (float)((s >> 8) & 0xffff) / 65536.f + 0.5f;
            tiles[p * plane + i] = std::ldexp((s & 0x80) ? -mant : mant, (int)((s >> 24) % 41) - 20);
        }
    tiles[plane + 4 * TW + 6] = std::nanf("");       // one NaN, in the second tile: it reaches x, x x and r x, not r and r r
    const int wins[4][2] = {{1, 1}, {2, 4}, {3, 5}, {7, 7}};
    double wy[WIN_MAX], wx[WIN_MAX];
    for (int k = 0; k < WIN_MAX; ++k) {
        wy[k] = 0.3 + 0.17 * k;
        wx[k] = 1.0 / (k + 3);
    }
    int n = 0;
    for (const auto& w : wins)
        for (int box = 0; box < 2; ++box) {
            const WindowTaps t = fill_window_taps(w[0], w[1], box ? nullptr : wy, box ? nullptr : wx);
            double W = 0.0, sx = 0.0;               // W as the first moment of a frame of ones
            for (int k = 0; k < t.sx; ++k) sx = box ? sx + 1.0 : std::fma(t.wx[k], 1.0, sx);
            for (int j = 0; j < t.sy; ++j) W = box ? W + sx : std::fma(t.wy[j], sx, W);
            if (t.box != box || !same(window_weight(t), W)) {
                std::printf("window %d x %d box %d: weight %a, the plain loop gives %a\n", t.sy, t.sx, box, window_weight(t), W);
                return 1;
            }
            if (run<1, 1>(t, tiles, plane) || run<1, 2>(t, tiles, plane) || run<2, 1>(t, tiles, plane) || run<2, 2>(t, tiles, plane)) return 1;
            n += 4;
        }
    std::printf("passes %d\n", n);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "layout")) return layout();
    if (argc == 2 && !std::strcmp(argv[1], "passes")) return passes();
    return 2;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("window_core")
    src, exe = d / "window.cpp", d / "window"
    src.write_text(PROGRAM)
    # a stand-alone program with its own main: the sanitizers are linked in the ordinary way.  No contraction: the plain loop's
    # s + u * u must stay a product and a sum (the header's own sums are explicit fma() calls or exact either way)
    cmd = [cxx, "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "barc4dip_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:      # a compiler without the sanitizer runtimes still checks the core
        r = subprocess.run([c for c in cmd if not c.startswith("-fsanitize") and not c.startswith("-fno-sanitize")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def test_layout_equals_the_python_formula_and_the_constants(program):
    from barc4dip_amd.metrics import perceptual as P

    r = subprocess.run([program, "layout"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert lines[0].split() == ["constants", "32", "63", "512", str(160 * 1024)] and P.LDS_LIMIT == 160 * 1024
    up4 = lambda n: (n + 3) & ~3  # noqa: E731
    table = [tuple(int(v) for v in ln.split()) for ln in lines[1:]]
    assert [(sy, sx) for sy, sx, _, _ in table] == [(sy, sx) for sy in range(1, 64) for sx in range(1, 64)]
    for sy, sx, stats, pair in table:
        rows = 31 + sy
        assert stats == 4 * up4(rows * up4(31 + sx)) + 16 * rows * 32, (sy, sx)
        assert pair == P.lds_bytes(sy, sx), (sy, sx)


def test_row_and_column_pass_equal_the_plain_double_loop(program):
    r = subprocess.run([program, "passes"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    # 4 windows x box / weighted x {one plane, two} x {one output row per call, two}
    assert r.stdout.split() == ["passes", "32"]
