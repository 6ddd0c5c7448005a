// handover_addr_check.cpp -- host check of the fused first visit's address arithmetic (malstroem_amd/csrc/handover_addr.hpp).
// Walks every window of every raster shape the GPU tests use (and a few more ragged ones) and asserts that
//   - every load index of dem / basin slots lies inside the raster,
//   - every index into the flood's level table lies inside the table -- for ANY 16-bit slot value on an interior cell (the slots
//     of border cells are poison), and equals the flood's own (tile of the cell) * NBMAX + slot for slots the flood can write,
//   - a cell is treated as a raster border cell exactly when the cell that is read is one,
//   - every cell of the raster is stored exactly once,
//   - every wet-bit word (tile row, raster column) is stored exactly once, inside its buffer and inside the records of the buffer
//     resource the visit stores through,
//   - the readers of the words (ng_finish_kernel: 32 rows from a multiple of 32; ccl_tile_kernel: 64 rows from a multiple of 64)
//     fetch inside the buffer and get, for every interior cell, the bit its OWNER stored -- the copies in the ring rows of the
//     neighbouring windows hold the opposite here -- and a clear bit for every raster border cell and every row behind the raster.
// Build and run (no GPU, no HIP):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I malstroem_amd/csrc tools/handover_addr_check.cpp -o build/handover_addr_check
//   build/handover_addr_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "handover_addr.hpp"

using namespace mh::ho;

static long long g_checks = 0;
#define REQUIRE(cond, ...)                                  \
    do {                                                    \
        ++g_checks;                                         \
        if (!(cond)) {                                      \
            std::fprintf(stderr, "FAILED %s: ", #cond);     \
            std::fprintf(stderr, __VA_ARGS__);              \
            std::fprintf(stderr, "\n");                     \
            std::exit(1);                                   \
        }                                                   \
    } while (0)

// what the bit of raster cell (R, c) is in this walk: any function that tells neighbours apart
static bool wet_pattern(int64_t R, int64_t c) { return (((R * 7 + c * 13) ^ (R >> 2) ^ (c >> 1)) & 3) != 0; }

static void walk_wet(int64_t H, int64_t W, int ntr, int ntc)
{
    const int64_t nw = wet_words(W, ntr);
    std::vector<uint64_t> wet((size_t)nw, 0ull);
    std::vector<int> stored((size_t)nw, 0);
    for (int ti = 0; ti < ntr; ++ti)
        for (int tj = 0; tj < ntc; ++tj) {
            const Win w = window(H, W, ntr, ntc, ti, tj);
            REQUIRE(wet_index(w, 0) >= 0 && wet_index(w, 0) < nw, "wet origin");
            for (int lane = 0; lane < WN; ++lane) {
                if (!own_col(w, lane)) continue;
                const int64_t k = wet_index(w, lane);
                REQUIRE(k >= 0 && k < nw, "%lldx%lld tile %d,%d lane %d: wet word %lld of %lld", (long long)H, (long long)W, ti, tj, lane, (long long)k, (long long)nw);
                REQUIRE((int64_t)lane * 8 + 8 <= wet_bytes_behind(w), "behind the wet buffer's records");
                REQUIRE(k == (int64_t)ti * W + w.c0 + lane && w.c0 + lane < W, "wet word of another column");
                uint64_t word = 0ull;
                for (int r = 0; r < WN; ++r) {
                    const int64_t R = w.r0 + row_of(w, r);                       // the row the visit reads
                    const bool border = border_row(w, r) || border_col(w, lane);
                    const bool mine = r >= 1 && r <= TI;                         // rows whose bit a reader may take from this word
                    const bool bit = border ? false : (mine ? wet_pattern(R, w.c0 + lane) : !wet_pattern(R, w.c0 + lane));
                    word |= bit ? 1ull << r : 0ull;
                }
                wet[(size_t)k] = word;
                ++stored[(size_t)k];
            }
        }
    for (int64_t k = 0; k < nw; ++k) REQUIRE(stored[(size_t)k] == 1, "%lldx%lld: wet word %lld stored %d times", (long long)H, (long long)W, (long long)k, stored[(size_t)k]);
    for (int rows : {32, 64})
        for (int64_t R0 = 0; R0 < H; R0 += rows)
            for (int64_t c = 0; c < W; ++c) {
                const int t0 = wet_tile_row(R0, ntr), t1 = t0 + 1 < ntr ? t0 + 1 : ntr - 1, t2 = t0 + 2 < ntr ? t0 + 2 : ntr - 1;
                REQUIRE(t0 >= 0 && t0 < ntr, "wet tile row");
                const int64_t k0 = (int64_t)t0 * W + c, k1 = (int64_t)t1 * W + c, k2 = (int64_t)t2 * W + c;
                REQUIRE(k0 >= 0 && k0 < nw && k1 >= 0 && k1 < nw && k2 >= 0 && k2 < nw, "wet read");
                const uint64_t m = wet_rows64(wet[(size_t)k0], wet[(size_t)k1], rows == 64 ? wet[(size_t)k2] : 0ull, R0, H, ntr);
                const bool inner_col = c > 0 && c < W - 1;
                for (int i = 0; i < rows; ++i) {
                    const int64_t R = R0 + i;
                    const bool got = inner_col && ((m >> i) & 1ull);
                    const bool want = R > 0 && R < H - 1 && inner_col && wet_pattern(R, c);
                    REQUIRE(got == want, "%lldx%lld: %d rows from %lld, cell %lld,%lld: bit %d, stored %d", (long long)H, (long long)W, rows, (long long)R0,
                            (long long)R, (long long)c, (int)got, (int)want);
                }
            }
}

static void walk(int64_t H, int64_t W)
{
    const int ntr = (int)((H - 2 + TI - 1) / TI), ntc = (int)((W - 2 + TI - 1) / TI);      // GeoRun::begin and PfRun::begin alike
    const int64_t n = H * W, ntab = (int64_t)ntr * ntc * NBMAX;
    std::vector<int> stored((size_t)n, 0);
    std::vector<float> dem((size_t)n, 0.0f);            // (the arrays the indices go into: the sanitizer sees every access)
    std::vector<uint32_t> tab((size_t)ntab, 0u);
    const uint32_t slots[] = {0u, 1u, (uint32_t)NBMAX - 1u, (uint32_t)NBMAX, 0xa5a5u, 0xffffu};
    for (int ti = 0; ti < ntr; ++ti)
        for (int tj = 0; tj < ntc; ++tj) {
            const Win w = window(H, W, ntr, ntc, ti, tj);
            REQUIRE(w.last_row >= 2 && w.last_row <= WN - 1, "%lldx%lld tile %d,%d last_row %d", (long long)H, (long long)W, ti, tj, w.last_row);
            REQUIRE(tab_origin(w) >= 0 && tab_words_behind_origin(w) > 0, "table origin");
            for (int r = 0; r < WN; ++r)
                for (int lane = 0; lane < WN; ++lane) {
                    const int64_t i = cell_index(w, r, lane);
                    REQUIRE(i >= 0 && i < n, "%lldx%lld tile %d,%d cell %d,%d reads %lld", (long long)H, (long long)W, ti, tj, r, lane, (long long)i);
                    (void)dem[(size_t)i];
                    const int64_t rr = i / W, cc = i % W;
                    const bool is_border = rr == 0 || rr == H - 1 || cc == 0 || cc == W - 1;
                    const bool border = border_row(w, r) || border_col(w, lane);
                    REQUIRE(border == is_border, "%lldx%lld tile %d,%d cell %d,%d (raster %lld,%lld): border %d, is %d", (long long)H, (long long)W, ti, tj,
                            r, lane, (long long)rr, (long long)cc, (int)border, (int)is_border);
                    for (uint32_t s : slots) {
                        const int64_t k = tab_index(w, r, lane, s, border);
                        REQUIRE(k >= 0 && k < ntab, "%lldx%lld tile %d,%d cell %d,%d slot %u: table index %lld of %lld", (long long)H, (long long)W, ti, tj, r,
                                lane, s, (long long)k, (long long)ntab);
                        REQUIRE(k - tab_origin(w) < tab_words_behind_origin(w), "behind the buffer's records");
                        (void)tab[(size_t)k];
                        if (!border && s < (uint32_t)NBMAX) {      // pf_row_finish: the tile of interior cell (rr, cc)
                            const int64_t want = ((int64_t)((rr - 1) / TI) * ntc + (cc - 1) / TI) * NBMAX + s;
                            REQUIRE(k == want, "%lldx%lld tile %d,%d cell %d,%d: table index %lld, the flood's %lld", (long long)H, (long long)W, ti, tj, r, lane,
                                    (long long)k, (long long)want);
                        }
                    }
                    if (own_row(w, r) && own_col(w, lane)) {
                        const int64_t o = store_index(w, r, lane);
                        REQUIRE(o >= 0 && o < n, "store index");
                        REQUIRE(o == i, "%lldx%lld tile %d,%d cell %d,%d: stores %lld, read %lld", (long long)H, (long long)W, ti, tj, r, lane, (long long)o,
                                (long long)i);
                        ++stored[(size_t)o];
                    }
                }
        }
    walk_wet(H, W, ntr, ntc);
    for (int64_t i = 0; i < n; ++i)
        REQUIRE(stored[(size_t)i] == 1, "%lldx%lld: cell %lld,%lld stored %d times", (long long)H, (long long)W, (long long)(i / W), (long long)(i % W), stored[(size_t)i]);
}

int main()
{
    // the shapes of tests/test_gpu_fill_handover.py ...
    const int64_t shapes[][2] = {{3, 3}, {3, 200}, {200, 3}, {64, 64}, {65, 65}, {126, 126}, {127, 190}, {131, 67}, {188, 250}, {200, 264}, {130, 512},
                                 {420, 380}, {192, 192}, {400, 300},
                                 // ... those of tests/test_gpu_wetbits.py ...
                                 {63, 125}, {126, 190}, {130, 200},
                                 // ... a labelling tile row that starts on the last row of a tile row of the transform (row 1984 = 31 * 64 = 32 * 62: three words) ...
                                 {2100, 6},
                                 // ... and every ragged remainder of the tile grid in both directions
                                 {4, 4}, {63, 66}, {66, 63}, {125, 129}, {129, 125}, {187, 189}, {189, 187}, {250, 188}, {1026, 70}};
    for (const auto &s : shapes) walk(s[0], s[1]);
    for (int64_t h = 3; h <= 132; ++h) walk(h, 260 - h);
    std::printf("handover address check: %lld assertions hold\n", g_checks);
    return 0;
}
