// Pins the tile list of the conv and filter-gradient kernels (annonet_amd/csrc/tilewalk.h) on the host: the walks of a grid's
// workgroups partition the list, the incremental cursor agrees with the division decode, and the band walk and the host tile
// counts equal lists written out by hand from the expressions the kernels carried before the header existed.  A change to the
// walk has to edit those lists knowingly.
#include <cstdio>
#include <vector>

#include "tilewalk.h"

using namespace anh;

static int failures = 0;
#define CHECK(cond, ...) \
    do { if (!(cond)) { if (++failures <= 20) { std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static std::vector<int> tiles_of(int wg, int n_wgs, int n_tiles, int bands) {
    const TileWalk w = tile_walk(wg, n_wgs, n_tiles, bands);
    std::vector<int> v;
    for (int tile = w.first; tile < w.end; tile += w.step) v.push_back(tile);
    return v;
}

// partition + cursor against decode, exhaustive over small grids
static long check_grids() {
    const int wgs[] = {1, 2, 3, 7, 8, 16, 24, 40};
    long walks = 0;
    for (int tiles_x = 1; tiles_x <= 5; ++tiles_x)
        for (int tiles_y = 1; tiles_y <= 5; ++tiles_y)
            for (int n = 1; n <= 3; ++n)
                for (int n_wgs : wgs)
                    for (int bands = 0; bands <= (tile_bands_ok(n_wgs) ? 1 : 0); ++bands) {
                        const int n_tiles = tiles_x * tiles_y * n;
                        std::vector<int> seen(n_tiles, 0);
                        for (int wg = 0; wg < n_wgs; ++wg, ++walks) {
                            const TileWalk w = tile_walk(wg, n_wgs, n_tiles, bands);
                            CHECK(w.step >= 1, "x %d y %d n %d wgs %d bands %d wg %d: step %d", tiles_x, tiles_y, n, n_wgs, bands, wg, w.step);
                            if (w.step < 1) return walks;
                            TileCursor c(w.first, w.step, tiles_x, tiles_y);
                            for (int tile = w.first; tile < w.end; tile += w.step, c.advance()) {
                                CHECK(tile >= 0 && tile < n_tiles, "x %d y %d n %d wgs %d bands %d wg %d: tile %d outside the list", tiles_x, tiles_y, n, n_wgs, bands, wg, tile);
                                if (tile >= 0 && tile < n_tiles) ++seen[tile];
                                const TilePos p = tile_pos(tile, tiles_x, tiles_y);
                                CHECK(p.tx >= 0 && p.tx < tiles_x && p.ty >= 0 && p.ty < tiles_y && p.n >= 0 && p.n < n && (p.n * tiles_y + p.ty) * tiles_x + p.tx == tile,
                                      "x %d y %d tile %d: decode (%d, %d, %d)", tiles_x, tiles_y, tile, p.tx, p.ty, p.n);
                                CHECK(c.tile == tile && c.pos.tx == p.tx && c.pos.ty == p.ty && c.pos.n == p.n,
                                      "x %d y %d n %d wgs %d bands %d wg %d tile %d: cursor at %d (%d, %d, %d), decode (%d, %d, %d)", tiles_x, tiles_y, n, n_wgs, bands, wg, tile,
                                      c.tile, c.pos.tx, c.pos.ty, c.pos.n, p.tx, p.ty, p.n);
                            }
                        }
                        for (int tile = 0; tile < n_tiles; ++tile)
                            CHECK(seen[tile] == 1, "x %d y %d n %d wgs %d bands %d: tile %d visited %d times", tiles_x, tiles_y, n, n_wgs, bands, tile, seen[tile]);
                    }
    return walks;
}

static void check_bands_ok() {
    for (int g = 0; g <= 64; ++g) CHECK(tile_bands_ok(g) == (g == 8 || g == 16 || g == 24 || g == 32 || g == 40 || g == 48 || g == 56 || g == 64), "tile_bands_ok(%d)", g);
}

// the band walk, worked out by hand from band_len = (n + 7) >> 3, first = (wg & 7) * band_len + (wg >> 3), step = grid >> 3,
// end = min(n, ((wg & 7) + 1) * band_len)
static void check_frozen(const char* name, int n_wgs, int n_tiles, const std::vector<std::vector<int>>& want) {
    CHECK((int)want.size() == n_wgs, "%s: the list has %d workgroups", name, (int)want.size());
    for (int wg = 0; wg < n_wgs && wg < (int)want.size(); ++wg) {
        const std::vector<int> got = tiles_of(wg, n_wgs, n_tiles, 1);
        CHECK(got == want[wg], "%s: workgroup %d walks %d tiles, first %d", name, wg, (int)got.size(), got.empty() ? -1 : got[0]);
    }
}
static void check_frozen_walks() {
    // 8 workgroups, 20 tiles: bands of 3, the last band empty, the one before ragged
    check_frozen("8 wgs, 20 tiles", 8, 20, {{0, 1, 2}, {3, 4, 5}, {6, 7, 8}, {9, 10, 11}, {12, 13, 14}, {15, 16, 17}, {18, 19}, {}});
    // 16 workgroups, 45 tiles: bands of 6 walked by two workgroups each, the last band holds 3
    check_frozen("16 wgs, 45 tiles", 16, 45,
                 {{0, 2, 4}, {6, 8, 10}, {12, 14, 16}, {18, 20, 22}, {24, 26, 28}, {30, 32, 34}, {36, 38, 40}, {42, 44},
                  {1, 3, 5}, {7, 9, 11}, {13, 15, 17}, {19, 21, 23}, {25, 27, 29}, {31, 33, 35}, {37, 39, 41}, {43}});
    // 24 workgroups, 5 tiles: fewer tiles than bands — bands of 1, workgroups 0..4 take one tile each
    check_frozen("24 wgs, 5 tiles", 24, 5, {{0}, {1}, {2}, {3}, {4}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}});
}

// host tile counts of every geometry against a hand-written table
static void check_frozen_counts() {
    const int dims[6] = {1, 31, 32, 33, 113, 227};
    const int cols[6] = {1, 1, 1, 2, 4, 8};          // 32 columns per tile
    const int rows8[6] = {1, 4, 4, 5, 15, 29};       // 8 rows per tile
    const int rows4[6] = {1, 8, 8, 9, 29, 57};       // 4 rows per tile
    const int up_cols[6] = {1, 1, 2, 2, 4, 8};       // up: w_in + 1 positions
    const int up_rows[6] = {1, 8, 9, 9, 29, 57};     // up: h_in + 1 positions, 4 rows per tile
    auto same = [](const TileCounts& c, int x, int y, int n) { return c.tiles_x == x && c.tiles_y == y && c.total == x * y * n; };
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j)
            for (int n = 1; n <= 3; n += 2) {
                const int h = dims[i], w = dims[j];
                CHECK(same(tiles_s1(h, w, n), cols[j], rows8[i], n), "tiles_s1(%d, %d, %d)", h, w, n);
                CHECK(same(tiles_down(h, w, n), cols[j], rows4[i], n), "tiles_down(%d, %d, %d)", h, w, n);
                CHECK(same(tiles_up(h, w, n), up_cols[j], up_rows[i], n), "tiles_up(%d, %d, %d)", h, w, n);
                CHECK(same(tiles_stem(h, w, n), cols[j], rows8[i], n), "tiles_stem(%d, %d, %d)", h, w, n);
                CHECK(same(tiles_wgrad(h, w, 8, n), cols[j], rows8[i], n), "tiles_wgrad(%d, %d, 8, %d)", h, w, n);
                CHECK(same(tiles_wgrad(h, w, 4, n), cols[j], rows4[i], n), "tiles_wgrad(%d, %d, 4, %d)", h, w, n);
            }
}

int main() {
    const long walks = check_grids();
    check_bands_ok();
    check_frozen_walks();
    check_frozen_counts();
    if (failures) { std::printf("tilewalk check: %d failures\n", failures); return 1; }
    std::printf("tilewalk ok: %ld walks\n", walks);
    return 0;
}
