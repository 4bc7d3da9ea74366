"""The column-set tile layout of the "colsets" option, stated in NumPy: where the forward row pass stores a bin
(k_row_r2c<.., CS>, b4d_fft2d.hpp) and where the column pass loads a register from (k_col<.., CS>).  No GPU: the two index maps are
written out as the kernels compute them and checked against each other and against the layout's definition

    tile[n][e][cp][h]   complex64,  n < 512, e < 2, cp < 16, h < 2   <->   column 2 cp + e, tile row n + 512 h

for every nx the route accepts (ny = 2048; nx = 4096 runs one row transform per workgroup and keeps the plain tiles)."""
import numpy as np
import pytest

NY = 2048
H = NY // 2          # rows of a parity tile
CW = 32              # columns of a parity tile
TILE = H * CW        # complex elements of a tile
NXS = [64, 128, 256, 512, 1024, 2048]


def row_seq(n):
    """transforms per workgroup of the row passes (b4d_fft2d.hpp)"""
    return 1 if n == 4096 else (32 if n == 64 else 256 // (n // 16))


def k1_store_map(nx):
    """(tile, element offset in the tile) -> (column of the tile, tile row): every 16-byte store of the forward row pass, for the even
    tile set of one frame (the odd set is the same map, one tile set further)"""
    seq, t = row_seq(nx), nx // 16
    half, lanes, nt = seq // 2, 2 * t, (nx // 2) // CW
    assert seq % 2 == 0 and (H // 2) % half == 0 and (nx // 2) // lanes == 4
    where = {}
    nblocks = (NY // 2) // seq
    for block in range(nblocks):
        bx = block
        if seq == 2 and nblocks % 16 == 0:             # one couple per workgroup: blocks b and b + 8 take adjacent couples
            bx = (block & ~15) + 2 * (block & 7) + ((block >> 3) & 1)
        for s in range(seq):
            sq, hi = s % half, s // half
            q = bx * half + sq                         # the couple's pairs are q and q + 512
            for u in range(t):
                m0 = u + t * hi                        # lane of the couple
                for i in range(4):
                    m = m0 + lanes * i                 # slot (tile, e, cp) of the lane
                    k = (m & ~(CW - 1)) + 2 * (m & 15) + ((m >> 4) & 1)   # the bin it splits
                    tile, off = m // CW, q * 2 * CW + 2 * (m & (CW - 1))
                    for h in range(2):                 # 16 bytes: transform q (h = 0) and q + 512 (h = 1)
                        key = (tile, off + h)
                        assert key not in where, "two stores to one element"
                        where[key] = (k, q + (NY // 4) * h)
    assert len(where) == nt * TILE
    return where, nt


def k2_load_map():
    """element offset in the tile -> (column of the tile, tile row): every 16-byte load of the column pass; lane (u, cp), set s,
    load j < 8 fills v[s][j] (row u + 64 j) and v[s][j + 8] (row u + 64 (j + 8))"""
    where = {}
    for u in range(64):
        for cp in range(16):
            for s in range(2):
                for j in range(8):
                    off = (64 * j * 2 * CW + s * CW) + (u * 2 * CW + 2 * cp)
                    for h in range(2):
                        assert off + h not in where, "two loads of one element"
                        where[off + h] = (2 * cp + s, u + 64 * (j + 8 * h))
    return where


def layout(off):
    """the definition: offset ((n 2 + e) 16 + cp) 2 + h"""
    h, cp, e, n = off % 2, (off // 2) % 16, (off // 32) % 2, off // 64
    return 2 * cp + e, n + 512 * h


def test_column_pass_loads_are_a_bijection_of_the_tile():
    loads = k2_load_map()
    assert sorted(loads) == list(range(TILE))
    assert sorted(loads.values()) == [(c, r) for c in range(CW) for r in range(H)]
    for off, cr in loads.items():
        assert cr == layout(off)


@pytest.mark.parametrize("nx", NXS)
def test_row_pass_stores_match_the_loads(nx):
    stores, nt = k1_store_map(nx)
    loads = k2_load_map()
    seen = np.zeros((nx // 2, H), dtype=np.int32)
    for (tile, off), (k, row) in stores.items():
        assert 0 <= off < TILE and 0 <= tile < nt
        assert k // CW == tile                          # the bin lands in its own column tile ...
        assert (k % CW, row) == loads[off] == layout(off)   # ... where the column pass reads that column and row from
        seen[k, row] += 1
    assert np.all(seen == 1)                            # every bin of every row pair, once


@pytest.mark.parametrize("nx", NXS)
def test_sixteen_lanes_store_one_run(nx):
    """lanes m0 .. m0 + 15 of a couple (m0 a multiple of 16) write 256 contiguous bytes: one (n, e) run"""
    t = nx // 16
    lanes = 2 * t
    for i in range(4):
        for m0 in range(0, lanes, 16):
            offs = [2 * ((m0 + d + lanes * i) & (CW - 1)) for d in range(min(16, lanes))]
            assert offs == list(range(offs[0], offs[0] + 2 * len(offs), 2))
