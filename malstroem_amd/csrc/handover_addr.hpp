// handover_addr.hpp -- address arithmetic of the fused first visit (noflat_geo.hip: ng_handover_kernel), which computes the plain
// fill F of its 64 x 64 window from the flood's dem + basin slots + final level table instead of reading it back.  Plain C++ with
// nothing but <cstdint>: the kernel includes it, and so does tools/handover_addr_check.cpp, a host program that walks every
// window of a list of raster shapes and asserts that every index generated here lies inside its array and that every cell of the
// raster is stored exactly once.  (The one GPU fault in this project's record came from a window load on a ragged raster.)
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MH_HD __host__ __device__
#else
#define MH_HD
#endif

namespace mh {
namespace ho {

constexpr int WN = 64;        // window edge (tile + ring)
constexpr int TI = 62;        // tile edge
constexpr int NBMAX = 1024;   // basins per tile of the flood's level table (pflood.hip)

// The windows of tile (ti, tj): origin (ti * TI, tj * TI).  Interior cell (r, c) of the raster belongs to tile ((r - 1) / TI,
// (c - 1) / TI) -- of the flood and of the transform alike.
struct Win {
    int64_t H, W;
    int ntr, ntc, ti, tj;
    int64_t r0, c0;
    int last_row;      // last window row inside the raster (rows behind it read that row again)
    int border_row;    // window row of the raster's last row (2 * WN: beyond the window)
    int tib, tjb;      // first tile row / column of the 3 x 3 tiles the window's cells belong to, clamped into the tile grid
};

MH_HD inline Win window(int64_t H, int64_t W, int ntr, int ntc, int ti, int tj)
{
    Win w;
    w.H = H; w.W = W; w.ntr = ntr; w.ntc = ntc; w.ti = ti; w.tj = tj;
    w.r0 = (int64_t)ti * TI;
    w.c0 = (int64_t)tj * TI;
    w.last_row = (int)(H - 1 - w.r0 < WN - 1 ? H - 1 - w.r0 : WN - 1);
    w.border_row = (int)(H - 1 - w.r0 < 2 * WN ? H - 1 - w.r0 : 2 * WN);
    w.tib = ti > 0 ? ti - 1 : 0;
    w.tjb = tj > 0 ? tj - 1 : 0;
    return w;
}

// ---- loads: window cell (r, lane) reads raster cell (row_of, col_of); a row / column outside the raster reads the raster's last
// row / column again (a raster border cell: its F is its elevation, whatever the basin slot says)
MH_HD inline int row_of(const Win &w, int r) { return r < w.last_row ? r : w.last_row; }                          // window row that is read
MH_HD inline int col_of(const Win &w, int lane) { return w.c0 + lane < w.W ? lane : (int)(w.W - 1 - w.c0); }      // window column that is read
MH_HD inline int64_t cell_index(const Win &w, int r, int lane) { return (w.r0 + row_of(w, r)) * w.W + w.c0 + col_of(w, lane); }

// a raster border cell (or the copy of one that a clamped load returns)
// (bitwise operators on purpose, here and below: the kernel wants selects, not branches on per-lane values)
MH_HD inline bool border_row(const Win &w, int r) { return ((w.ti == 0) & (r == 0)) | (r >= w.border_row); }
MH_HD inline bool border_col(const Win &w, int lane) { return ((w.tj == 0) & (lane == 0)) | (w.c0 + lane >= w.W - 1); }

// ---- the level table: tile of window cell (r, lane).  Row 0 / 63 and lane 0 / 63 are the ring: cells of the neighbouring tiles.
// Clamped into the tile grid: where the clamp bites the cell is a raster border cell and its level is not used.
MH_HD inline int tile_row(const Win &w, int r)
{
    const int t = w.ti + (r == WN - 1 ? 1 : 0) - (r == 0 ? 1 : 0);
    return t < 0 ? 0 : (t > w.ntr - 1 ? w.ntr - 1 : t);
}
MH_HD inline int tile_col(const Win &w, int lane)
{
    const int t = w.tj + (lane == WN - 1 ? 1 : 0) - (lane == 0 ? 1 : 0);
    return t < 0 ? 0 : (t > w.ntc - 1 ? w.ntc - 1 : t);
}
// the table is addressed from the entry of tile (tib, tjb): a word offset per row (scalar) + one per lane + the slot
MH_HD inline int64_t tab_origin(const Win &w) { return ((int64_t)w.tib * w.ntc + w.tjb) * NBMAX; }
MH_HD inline uint32_t tab_row_words(const Win &w, int r) { return (uint32_t)(tile_row(w, r) - w.tib) * (uint32_t)w.ntc * (uint32_t)NBMAX; }
MH_HD inline uint32_t tab_lane_words(const Win &w, int lane) { return (uint32_t)(tile_col(w, lane) - w.tjb) * (uint32_t)NBMAX; }
// the slot of a border cell was never written by the flood: selected away, and every slot stays inside its tile's entries
MH_HD inline uint32_t tab_slot(uint32_t slot, bool border) { return border ? 0u : (slot < (uint32_t)NBMAX - 1u ? slot : (uint32_t)NBMAX - 1u); }
MH_HD inline int64_t tab_index(const Win &w, int r, int lane, uint32_t slot, bool border)
{
    return tab_origin(w) + tab_row_words(w, r) + tab_lane_words(w, lane) + tab_slot(slot, border);
}
MH_HD inline int64_t tab_words_behind_origin(const Win &w) { return (int64_t)w.ntr * w.ntc * NBMAX - tab_origin(w); }

// ---- stores of F and depths: the tile's own 62 x 62 cells and the raster border cells inside the window; every cell of the
// raster has exactly one owner.  (The raster's last row / column lies in the last tile row / column only, at window row / lane
// >= 2: the window in front of it would hold it at 64.)
MH_HD inline bool own_row(const Win &w, int r) { return ((r >= 1) & (r <= TI) & (r <= w.last_row)) | ((w.ti == 0) & (r == 0)) | (r == w.border_row); }
MH_HD inline bool own_col(const Win &w, int lane)
{
    const int64_t c = w.c0 + lane;
    return (c < w.W) & (((lane >= 1) & (lane <= TI)) | ((w.tj == 0) & (lane == 0)) | (c == w.W - 1));
}
MH_HD inline int64_t store_index(const Win &w, int r, int lane) { return (w.r0 + r) * w.W + w.c0 + lane; }

// ---- the wet bits: "F > dem" of a window column as one 64-bit word (bit r = window row r), kept per (tile row, raster column):
// word ti * W + c, written by the one tile that owns column c in tile row ti (own_col).  Lane = column in the visit that writes
// the words and in both kernels that read them (ng_finish_kernel, ccl_tile_kernel), so every access is a coalesced 8-byte word a
// lane.  A reader takes the bit of raster row R from the word of the tile row that OWNS R -- (R - 1) / TI, bit R - ti * TI, in
// 1 .. TI -- never from the copy a neighbouring window holds of it (rows 0 and 63), and takes a raster border cell as dry without
// looking: there F is the elevation bit for bit.
MH_HD inline int64_t wet_words(int64_t W, int ntr) { return (int64_t)ntr * W; }
MH_HD inline int64_t wet_index(const Win &w, int lane) { return (int64_t)w.ti * w.W + w.c0 + lane; }
// bytes of tile row ti's words from column c0 on: the records of the buffer the visit stores through (a lane behind them is dropped)
MH_HD inline int64_t wet_bytes_behind(const Win &w) { return (w.W - w.c0) * 8; }
MH_HD inline int wet_tile_row(int64_t R, int ntr)      // of any row: clamped into the tile grid (the clamp bites on border rows only)
{
    const int64_t t = (R < 1 ? 0 : R - 1) / TI;
    return (int)(t < ntr - 1 ? t : ntr - 1);
}
// The bits of the rows R0 .. R0 + 63 of one column (bit i = row R0 + i), from the words of the tile rows t0 = wet_tile_row(R0), t0 + 1
// and t0 + 2 (clamped like wet_tile_row; a reader of 32 rows passes anything for w2 and uses the low half).  Rows outside 1 .. H - 2 are dry.
MH_HD inline uint64_t wet_rows64(uint64_t w0, uint64_t w1, uint64_t w2, int64_t R0, int64_t H, int ntr)
{
    const int t0 = wet_tile_row(R0, ntr);
    const int s = (int)(R0 - (int64_t)t0 * TI);                  // bit of row R0 in w0: 0 (R0 == 0) .. TI
    const int n0 = TI - s;                                      // rows 0 .. n0 of the 64 are w0's
    const uint64_t lo0 = (2ull << n0) - 1ull;                   // (n0 <= 62)
    const uint64_t lo1 = n0 + TI >= 63 ? ~0ull : (2ull << (n0 + TI)) - 1ull;      // rows n0 + 1 .. n0 + TI are w1's
    const uint64_t p2 = n0 + TI < 64 ? w2 << ((n0 + TI) & 63) : 0ull;             // the rest (n0 <= 1 only) w2's
    uint64_t m = ((w0 >> s) & lo0) | ((w1 << n0) & ~lo0 & lo1) | (p2 & ~lo1);
    const int64_t inner = H - 1 - R0;                           // rows R0 .. H - 2
    m &= inner >= 64 ? ~0ull : (inner <= 0 ? 0ull : (1ull << inner) - 1ull);
    return R0 == 0 ? m & ~1ull : m;
}

}  // namespace ho
}  // namespace mh
