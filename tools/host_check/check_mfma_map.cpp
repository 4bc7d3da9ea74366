// The C/D index map of b4d_mfma.hpp on the host: the (row, col) pairs that for_each hands out over a 256-lane workgroup, 2 x 2
// tiles per wave and 16 registers per tile must cover the 128 x 128 tile exactly once and equal the map of
// v_mfma_f32_32x32x2_f32 (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) offset by the wave's 64 and the
// sub-tile's 32.  Build: c++ -std=c++17 -Itools/host_check -Ibarc4dip_amd/csrc tools/host_check/check_mfma_map.cpp
#include <cstdio>
#include <vector>

#include "b4d_mfma.hpp"

struct Regs {   // stands in for f32x16: entry r holds its own (sub-tile, register) as 16 (2 i + j) + r
    float v[16];
    float operator[](int r) const { return v[r]; }
};

int main() {
    long bad = 0;
    const int m0 = 384, n0 = 640;   // any tile corner
    std::vector<int> seen(128 * 128, 0);
    Regs acc[2][2];
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j)
            for (int r = 0; r < 16; ++r) acc[i][j].v[r] = (float)(16 * (2 * i + j) + r);
    for (int tid = 0; tid < 256; ++tid) {
        const int lane = tid & 63, wave = tid >> 6;
        const b4d::WaveTile t = b4d::wave_tile(tid);
        if (t.wr != wave / 2 || t.wc != wave % 2 || t.li != (lane & 31) || t.lk != (lane >> 5)) ++bad;
        int calls = 0;
        b4d::for_each(acc, t, m0, n0, [&](int row, int col, float v) {
            const int id = (int)v, r = id & 15, i = id >> 5, j = (id >> 4) & 1;
            const int want_row = 64 * (wave >> 1) + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const int want_col = 64 * (wave & 1) + 32 * j + (lane & 31);
            if (row != m0 + want_row || col != n0 + want_col) ++bad;
            if (id != calls) ++bad;   // sub-tiles (0,0) (0,1) (1,0) (1,1), registers in order
            ++calls;
            const int rr = row - m0, cc = col - n0;
            if (rr < 0 || rr >= 128 || cc < 0 || cc >= 128) ++bad;
            else ++seen[rr * 128 + cc];
        });
        if (calls != 64) ++bad;
    }
    for (int e = 0; e < 128 * 128; ++e)
        if (seen[e] != 1) ++bad;
    for (int r = 0; r < 16; ++r)   // the single-tile form, with and without a base
        for (int lk = 0; lk < 2; ++lk)
            if (b4d::mfma_row(r, lk) != (r & 3) + 8 * (r >> 2) + 4 * lk || b4d::mfma_row(r, lk, 96) != 96 + b4d::mfma_row(r, lk)) ++bad;
    for (int li = 0; li < 32; ++li)
        if (b4d::mfma_col(li) != li) ++bad;
    std::printf("TOTAL BAD %ld\n", bad);
    return bad ? 1 : 0;
}
