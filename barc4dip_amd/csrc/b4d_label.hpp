// b4d_label.hpp -- the union-find core of connected-component labelling (b4d_label.hip).  Everything here is
// __host__ __device__ over a small memory concept and free of HIP types, so a plain C++ program can run the whole algorithm
// serially with a tile of its own choice (tests/test_labels_host.py).
//
// The forest.  A frame's label array holds, per pixel, LB_BACKGROUND or a LINK: the frame-relative raster index (y * nx + x) of
// another pixel of the same set, never a larger one than the pixel's own.  A pixel that links to itself is a root, and because
// links only ever decrease, the root of a set is its smallest raster index: the first pixel of the component in raster order,
// whatever the order in which concurrent lanes won their fetch_min.
//
// Termination (every loop below ends by construction, and carries a bound anyway):
//   uf_find   follows links; each step goes to a strictly smaller index, so it takes at most `bound` = (cells of the array) steps.
//   uf_unite  each round takes the roots a > b of both sides and lowers the word of a to b with fetch_min.  Either the word still
//             held a (done: a now links to b), or it held old < a (another lane linked a first): the round is repeated with
//             (old, b), both smaller than a.  The larger index of the pair strictly decreases, so at most `bound` rounds.
//   A stale read only returns an older link, which is still a member of the same set and not smaller than the current one:
//   the round then fails its fetch_min test and is repeated from a smaller index; no link is ever lost, because a round that
//   lowers a word whose previous value was not a carries that previous value into the next round.
// Reaching a bound sets `tripped`; the kernels pass it to an error word (include/b4d.h: n_regions = B4D_ELOOP).
//
// Mem: int load(int i) const; int fetch_min(int i, int v) (returns the previous word); void store(int i, int v).
#pragma once
#include <cstdint>

#include "b4d_keys.hpp"   // B4D_HD

namespace b4d {

// tile of the first pass (one workgroup of LB_THREADS lanes; TY * TX links of LDS); pixels per block of the numbering scan;
// the area of a region's box up to which one wave measures it (above: one workgroup); columns of b4d_region_properties
constexpr int LB_TY = 32, LB_TX = 64, LB_THREADS = 256;
constexpr int LB_SCAN = 2048;
constexpr int RP_WAVE_AREA = 4096, RP_NQ = 20;
constexpr int LB_BACKGROUND = -1;

struct SerialMem {   // a plain array, one thread
    int* p;
    int load(int i) const { return p[i]; }
    int fetch_min(int i, int v) {
        const int o = p[i];
        if (v < o) p[i] = v;
        return o;
    }
    void store(int i, int v) { p[i] = v; }
};

template <class Mem>
B4D_HD int uf_find(const Mem& m, int i, unsigned bound, int& tripped) {
    for (unsigned k = 0; k <= bound; ++k) {
        const int p = m.load(i);
        if (p == i) return i;
        i = p;
    }
    tripped = 1;
    return i;
}

template <class Mem>
B4D_HD void uf_unite(Mem& m, int a, int b, unsigned bound, int& tripped) {
    for (unsigned k = 0; k <= bound; ++k) {
        a = uf_find(m, a, bound, tripped);
        b = uf_find(m, b, bound, tripped);
        if (a == b || tripped) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = m.fetch_min(a, b);
        if (old == a) return;
        a = old;
    }
    tripped = 1;
}

// First pass, one pixel (ly, lx) of a tile whose links are tile-local indices ly * pitch + lx: unite with the foreground
// neighbours that precede it in raster order inside the tile (W, N; connectivity 2: NW, NE too).  tw: valid columns of the tile.
template <class Mem>
B4D_HD void lb_tile_pixel(Mem& m, int ly, int lx, int tw, int pitch, int conn, unsigned bound, int& tripped) {
    const int l = ly * pitch + lx;
    if (m.load(l) < 0) return;
    if (lx > 0 && m.load(l - 1) >= 0) uf_unite(m, l, l - 1, bound, tripped);
    if (ly > 0) {
        if (m.load(l - pitch) >= 0) uf_unite(m, l, l - pitch, bound, tripped);
        if (conn == 2) {
            if (lx > 0 && m.load(l - pitch - 1) >= 0) uf_unite(m, l, l - pitch - 1, bound, tripped);
            if (lx + 1 < tw && m.load(l - pitch + 1) >= 0) uf_unite(m, l, l - pitch + 1, bound, tripped);
        }
    }
}

// Second pass, one pixel (y, x) on a seam of the frame-wide links.  row_seam: y is the first row of a tile and the pixel is united
// with its neighbours in row y - 1; otherwise x is the first column of a tile and the neighbours are those in column x - 1
// (rows y - 1, y, y + 1).  Every pair of neighbouring pixels in different tiles has one pixel in a first row or first column with
// the other in the row above or the column to the left, so the two kinds of seam pixel cover every contact, the diagonal
// contacts at tile corners included.
template <class Mem>
B4D_HD void lb_seam_pixel(Mem& m, int y, int x, int ny, int nx, int conn, bool row_seam, unsigned bound, int& tripped) {
    const int p = y * nx + x;
    if (m.load(p) < 0) return;
    for (int d = -1; d <= 1; ++d) {
        if (d != 0 && conn != 2) continue;
        const int qy = row_seam ? y - 1 : y + d, qx = row_seam ? x + d : x - 1;
        if (qy < 0 || qy >= ny || qx < 0 || qx >= nx) continue;
        const int q = qy * nx + qx;
        if (m.load(q) >= 0) uf_unite(m, p, q, bound, tripped);
    }
}

// Numbering.  After the flatten pass every foreground pixel links to its root.  Roots are counted per scan block, the counts are
// scanned, and root number k (1-based, raster order) is first written as the CODE -(k + 1) <= -2 over the root's own link; a
// pixel then reads its root's word, which is that code or, once the root's own lane has finished, k itself: told apart by sign.
B4D_HD int lb_code(int k) { return -(k + 1); }
B4D_HD int lb_number(int word) { return word < 0 ? -(word + 1) : word; }   // of a root's word: LB_BACKGROUND -> 0
// the final label of pixel p from its own word v (a link, a code or LB_BACKGROUND)
template <class Mem>
B4D_HD int lb_final(const Mem& m, int v) {
    return v < 0 ? lb_number(v) : lb_number(m.load(v));
}

// The whole algorithm, serially, with tiles of ty x tx: fg (ny * nx) bytes -> labels (ny * nx), returns the region count or -1
// for a tripped bound.  The passes, their helpers and their order are those of the kernels.
inline int label_frame_serial(const uint8_t* fg, int ny, int nx, int conn, int ty, int tx, int scan, int* labels, int* tile_links) {
    int tripped = 0;
    const unsigned npix = (unsigned)(ny * nx);
    for (int y0 = 0; y0 < ny; y0 += ty)
        for (int x0 = 0; x0 < nx; x0 += tx) {
            const int th = ny - y0 < ty ? ny - y0 : ty, tw = nx - x0 < tx ? nx - x0 : tx;
            SerialMem t{tile_links};
            for (int ly = 0; ly < th; ++ly)
                for (int lx = 0; lx < tw; ++lx) t.store(ly * tx + lx, fg[(y0 + ly) * nx + x0 + lx] ? ly * tx + lx : LB_BACKGROUND);
            for (int ly = 0; ly < th; ++ly)
                for (int lx = 0; lx < tw; ++lx) lb_tile_pixel(t, ly, lx, tw, tx, conn, (unsigned)(ty * tx), tripped);
            for (int ly = 0; ly < th; ++ly)
                for (int lx = 0; lx < tw; ++lx) {
                    const int l = ly * tx + lx;
                    int g = LB_BACKGROUND;
                    if (t.load(l) >= 0) {
                        const int r = uf_find(t, l, (unsigned)(ty * tx), tripped);
                        g = (y0 + r / tx) * nx + x0 + r % tx;
                    }
                    labels[(y0 + ly) * nx + x0 + lx] = g;
                }
        }
    SerialMem m{labels};
    for (int y = ty; y < ny; y += ty)
        for (int x = 0; x < nx; ++x) lb_seam_pixel(m, y, x, ny, nx, conn, true, npix, tripped);
    for (int x = tx; x < nx; x += tx)
        for (int y = 0; y < ny; ++y) lb_seam_pixel(m, y, x, ny, nx, conn, false, npix, tripped);
    for (int p = 0; p < ny * nx; ++p)
        if (m.load(p) >= 0) m.store(p, uf_find(m, p, npix, tripped));
    int n = 0;
    for (int b0 = 0; b0 < ny * nx; b0 += scan) {     // count and scan fall together in a serial run
        const int b1 = b0 + scan < ny * nx ? b0 + scan : ny * nx;
        for (int p = b0; p < b1; ++p)
            if (m.load(p) == p) m.store(p, lb_code(++n));
    }
    for (int p = 0; p < ny * nx; ++p) m.store(p, lb_final(m, m.load(p)));
    return tripped ? -1 : n;
}

}  // namespace b4d
